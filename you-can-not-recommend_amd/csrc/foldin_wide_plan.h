// foldin_wide_plan.h -- how a request of ycnr_als_fold_in_implicit_wide is cut into the rows foldin_implicit_wide_kernel serves (in
// two launch classes that differ in their LDS allocation alone), the rows it does not serve and the rows without observations;
// and the sizes the kernels of foldin_wide_kernels.hip.h share with the host.  Host-only and a function of its arguments alone,
// like foldin_plan.h: no HIP, no environment, no device call (tests/cpp/foldin_wide_plan_test.cc builds it with a plain C++
// compiler).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "step_policy.h"

namespace ycnr {

constexpr int kFoldWideMaxK = 512;      // factorsCount the wide fold-in serves (the limit of ycnr_als_step_implicit_sub)
constexpr int kFoldWideMaxObs = 128;    // observations of a served row: eight groups of 16, one per wave of the row kernel
constexpr int kFoldWideShortObs = 32;   // ... of the short launch class: two groups, three tiles of the small system
constexpr int kFoldWideBlock = 64;      // block width of the factorisation of G + lambda I and of the images L and Linv
constexpr int kFoldWideThreads = 512;   // threads of foldin_implicit_wide_kernel: eight waves
constexpr int kFoldWideTLd = 68;        // doubles per row of the 64 x 64 product foldin_wide_inverse_kernel keeps in LDS

// A row is served when it has 1 .. 128 observations and D = diag(sqrt(alpha r)) is real.  There is no n <= k condition:
// I + D K D is symmetric with eigenvalues >= 1 whatever n is.
YCNR_HD constexpr bool fold_wide_row_is_served(int64_t n, bool allNonNegative) { return n >= 1 && n <= kFoldWideMaxObs && allNonNegative; }

// leading dimension (doubles) of the images M, L and Linv: factorsCount rounded up to whole 64-column blocks
YCNR_HD constexpr int fold_wide_image_ld(int k) { return (k + kFoldWideBlock - 1) / kFoldWideBlock * kFoldWideBlock; }
YCNR_HD constexpr size_t fold_wide_image_bytes(int k) { return (size_t)fold_wide_image_ld(k) * fold_wide_image_ld(k) * sizeof(double); }
// observations rounded up to whole groups of 16
YCNR_HD constexpr int fold_wide_np(int n) { return (n + 15) / 16 * 16; }
// doubles per row of a 16 x np panel of P: 16 mod 32, so that the four rows an MFMA operand reads fall on different banks
YCNR_HD constexpr int fold_wide_pld(int np) { return np % 32 == 0 ? np + 16 : np; }

// The LDS of one row of foldin_implicit_wide_kernel, in doubles from the start of its dynamic LDS.  A function of (np, kp) of
// the ROW, not of its launch class: a class only allocates what its longest row needs.
struct FoldWideLds {
  int S, panel, cv, sw, rhs, yv, vv, invd, u, t, ids, end;
};
YCNR_HD constexpr FoldWideLds fold_wide_lds(int np, int kp) {
  FoldWideLds o{};
  o.S = 0;                                          // packed upper 16 x 16 tiles of K, then of I + D K D
  o.panel = o.S + tile_count(np / 16) * 256;        // two panels [16][pld] of P, block row J in panel J & 1
  o.cv = o.panel + 2 * 16 * fold_wide_pld(np);      // c = 1 + alpha r, zero past n
  o.sw = o.cv + np;                                 // sqrt(alpha r)
  o.rhs = o.sw + np;                                // D K c, then what the elimination leaves of it
  o.yv = o.rhs + np;                                // y
  o.vv = o.yv + np;                                 // v = c - D y
  o.invd = o.vv + np;                               // 1 / pivot
  o.u = o.invd + np;                                // u = V^T v (kp)
  o.t = o.u + kp;                                   // t = Linv u (kp)
  o.ids = o.t + kp;                                 // the observations' ids: np int32
  o.end = o.ids + np / 2;
  return o;
}
// dynamic LDS of a launch class whose longest row has maxObs observations
YCNR_HD constexpr size_t fold_wide_lds_bytes(int maxObs, int k) {
  return (size_t)fold_wide_lds(fold_wide_np(maxObs), (k + 15) / 16 * 16).end * sizeof(double);
}

// The four lists partition the request's rows, each in request order.
struct FoldWideCut {
  std::vector<int32_t> shortRows, longRows, notServed, empty;
};

// rowPtr: nRows + 1 offsets from 0, not decreasing; vals: the request's values in the handle's type.  A value r with !(r >= 0)
// (negative or NaN) leaves its row unserved.  The vectors are reused, not shrunk.
template <typename T>
inline void fold_wide_cut(int64_t nRows, const int64_t *rowPtr, const T *vals, FoldWideCut &cut) {
  cut.shortRows.clear(), cut.longRows.clear(), cut.notServed.clear(), cut.empty.clear();
  for (int64_t r = 0; r < nRows; ++r) {
    const int64_t beg = rowPtr[r], end = rowPtr[r + 1], n = end - beg;
    if (n == 0) {
      cut.empty.push_back((int32_t)r);
      continue;
    }
    bool nonNegative = n <= kFoldWideMaxObs;
    for (int64_t q = beg; nonNegative && q < end; ++q) nonNegative = vals[q] >= (T)0;
    if (!fold_wide_row_is_served(n, nonNegative)) cut.notServed.push_back((int32_t)r);
    else (n <= kFoldWideShortObs ? cut.shortRows : cut.longRows).push_back((int32_t)r);
  }
}

}  // namespace ycnr
