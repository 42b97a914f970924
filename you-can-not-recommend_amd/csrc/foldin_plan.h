// foldin_plan.h -- how a request of ycnr_als_fold_in_implicit is cut into the rows foldin_implicit_dual_kernel solves in dual
// (Woodbury) form, the rows that take the exact k x k solve of implicit_unit_kernel, and the rows without observations; and the
// sizes the kernels of foldin_implicit_kernels.hip.h share with the host.  Host-only and a function of its arguments alone, like
// schedule.h and rank_plan.h: no HIP, no environment, no device call (tests/cpp/foldin_plan_test.cc builds it with a plain C++
// compiler).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "schedule.h"

#ifdef __HIPCC__
#define YCNR_FOLD_HD __host__ __device__
#else
#define YCNR_FOLD_HD
#endif

namespace ycnr {

constexpr int kFoldDualMax = 32;        // observations of a dual row: two groups of 16 = the columns of two MFMA tiles
constexpr int kFoldImplicitMaxK = 128;  // factorsCount the implicit fold-in serves (the implicit half-steps' limit)
constexpr int kFoldDualSLd = kFoldDualMax + 1;  // doubles per row of the small system: 32 columns and the right-hand side

// A row goes the dual way when the n x n system is the smaller one and D = diag(sqrt(alpha r)) is real.  From the operation and
// barrier counts (n k^2 / 2 + n^2 k + n^3 / 3 and a handful of barriers against n k^2 + k^3 / 3 and k barriers), not measured.
YCNR_FOLD_HD constexpr bool fold_row_is_dual(int64_t n, int k, bool allNonNegative) {
  return n >= 1 && n <= kFoldDualMax && n <= k && allNonNegative;
}

// doubles per row of the gathered panel [32][ld]: 16 mod 32, so that the rows two lane groups read fall on different banks
YCNR_FOLD_HD constexpr int fold_dual_ld(int kp) { return kp % 32 == 0 ? kp + 16 : kp; }
// dynamic LDS of foldin_implicit_dual_kernel: the panel V [32][ld] that P^T overwrites, the small system [32][33], c, sqrt(w), v
// and 1 / d (32 each), t (kp)
YCNR_FOLD_HD constexpr size_t fold_dual_lds_bytes(int k) {
  const int kp = (k + 15) / 16 * 16;
  return ((size_t)kFoldDualMax * fold_dual_ld(kp) + (size_t)kFoldDualMax * kFoldDualSLd + 4 * kFoldDualMax + (size_t)kp) * sizeof(double);
}
// dynamic LDS of foldin_factor_kernel: the packed upper tiles of G + lambda I, as many tiles for the inverse, 1 / pivot (kp)
YCNR_FOLD_HD constexpr size_t fold_factor_lds_bytes(int k) {
  const int nb = (k + 15) / 16;
  return ((size_t)2 * (nb * (nb + 1) / 2) * 256 + (size_t)nb * 16) * sizeof(double);
}

// The three lists partition the request's rows.  dual / empty: request rows in request order.  primal: one whole-row unit of
// implicit_unit_kernel per row (slab = -1: the unit solves its row), in request order.
struct FoldCut {
  std::vector<int32_t> dual, empty;
  std::vector<Unit> primal;
};

// rowPtr: nRows + 1 offsets from 0, not decreasing; vals: the request's values in the handle's type.  primalOnly: no dual rows.
// A value r with !(r >= 0) (negative or NaN) sends its row to the primal path.  The vectors are reused, not shrunk.
template <typename T>
inline void fold_cut(int64_t nRows, const int64_t *rowPtr, const T *vals, int k, bool primalOnly, FoldCut &cut) {
  cut.dual.clear(), cut.empty.clear(), cut.primal.clear();
  for (int64_t r = 0; r < nRows; ++r) {
    const int64_t beg = rowPtr[r], end = rowPtr[r + 1], n = end - beg;
    if (n == 0) {
      cut.empty.push_back((int32_t)r);
      continue;
    }
    bool nonNegative = !primalOnly && n <= kFoldDualMax;
    for (int64_t q = beg; nonNegative && q < end; ++q) nonNegative = vals[q] >= (T)0;
    if (!primalOnly && fold_row_is_dual(n, k, nonNegative)) cut.dual.push_back((int32_t)r);
    else cut.primal.push_back(Unit{beg, end, (int32_t)r, -1});
  }
}

}  // namespace ycnr
