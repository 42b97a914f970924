// foldin_implicit_kernels.hip.h -- fold-in for the implicit-feedback model of Hu, Koren, Volinsky: the factor rows of a REQUEST
// (new users / new items whose observations arrive in the call) against the fixed opposite matrix Y the handle holds,
// factorsCount <= 128.  One row with observations S (n of them), raw values r, w = alpha r, c = 1 + w:
//     A x = Y_S^T c,   A = M + Y_S^T W Y_S,   M = Y^T Y + lambda I        (the row of ycnr_als_step_implicit)
// A new user's row is short: n is far below k, and M is the same for every row of the call.  So M = L L^T is factorised and
// inverted ONCE per call, and a row with n <= 32 is solved in DUAL (Woodbury) form, an n x n system instead of a k x k one:
//     P = Linv Y_S^T (k x n);   K = P^T P = Y_S M^-1 Y_S^T;   D = diag(sqrt w)
//     (I + D K D) y = D K c;    v = c - D y;    x = Linv^T (P v)
// (I + D K D is symmetric with eigenvalues >= 1; nothing divides by w, so r = 0 is served.)
//
// Launched in this order on the handle's stream, behind implicit_gram_kernel / implicit_gram_reduce_kernel (G = Y^T Y):
//   foldin_factor_kernel            one workgroup: G + lambda I -> LDS, L D L^T in double, then Linv = L^-1 column by column
//                                   (two lanes per column, each column its own forward substitution) -> a zero-padded kp x kp
//                                   row-major double image in global memory (<= 128 KB: L2 resident for the row kernels)
//   foldin_implicit_dual_kernel<T>  one workgroup of four waves per dual row, five phases with a barrier between them:
//       gather   the row's <= 32 fixed rows -> LDS as double [32][ld], zero-padded; c and sqrt(w) beside them
//       P        P = Linv V^T on v_mfma_f64_16x16x4_f64, block rows of 16 factors dealt over the waves (J and 7 - J: equal work),
//                both operands as one 32-byte load per four MFMAs (the dealing of implicit_cg_dense); the tiles of Linv above the
//                diagonal are skipped.  P^T is written OVER V once every wave holds its tiles in registers.
//       K        P^T P: the <= 3 upper 16 x 16 tiles, one per wave, contraction over kp in one chain
//       solve    wave 0: S = I + D K D and D K c in LDS, L D L^T with lanes as columns and the right-hand side as column 32,
//                back substitution, v = c - D y.  Wave-level ordering only, no workgroup barrier inside.
//       back     t = P v (thread j < kp, observation order), barrier, x_j = sum_{i >= j} Linv[i][j] t_i (ascending i), one
//                rounding to T at the store
//   implicit_unit_kernel<T>         (implicit_kernels.hip.h, unchanged) the rows that are not dual: one whole-row unit each
//   foldin_implicit_finish_kernel<T> status, zeros for rows that were not solved, the copy into the handle's matrix
// ALL arithmetic is float64 for both handle types (gathered values are converted exactly); every sum's order is fixed by the row
// alone, so a row's bits do not depend on what else the request holds.
#pragma once
#include "foldin_plan.h"
#include "implicit_kernels.hip.h"

namespace ycnr {

// the LDS traffic of ONE wave in program order (lanes exchange values through LDS inside the small solve and the inverse)
__device__ __forceinline__ void foldin_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------ Linv, once per call
// flags[0]: the bad-row count of the primal units (cleared by implicit_gram_reduce_kernel); flags[1] <- 1 if a pivot p of
// G + lambda I has !(p > 0), else 0.  Linv: kp x kp, row-major, everything outside the lower triangle of the k real rows zero.
__global__ __launch_bounds__(256) void foldin_factor_kernel(const double *__restrict__ G, double lambda, int k, double *__restrict__ Linv,
                                                            int32_t *flags) {
  extern __shared__ double ffac_lds[];
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int nb = (k + 15) >> 4, kp = nb << 4, nt = tile_count(nb);
  double *img = ffac_lds;                  // packed upper tiles: A, then R (R[j][c] = d_j L'[c][j]), then L^T
  double *inv = img + (size_t)nt * 256;    // X = L^-1: X[i][m], m <= i, in tile (m / 16, i / 16) at [(i % 16) * 16 + m % 16]
  double *invd = inv + (size_t)nt * 256;   // 1 / d_j, then 1 / L[j][j]
  auto at = [&](int i, int c) -> double & { return img[(size_t)tile_index(i >> 4, c >> 4, nb) * 256 + (i & 15) * 16 + (c & 15)]; };
  auto xat = [&](int i, int m) -> double & { return inv[(size_t)tile_index(m >> 4, i >> 4, nb) * 256 + (i & 15) * 16 + (m & 15)]; };
  if (tid == 0) bad = 0;
  for (int e = tid; e < nt * 256; e += 256) {
    int bi, bj;
    implicit_tile_of(e >> 8, nb, bi, bj);
    const int gi = 16 * bi + ((e >> 4) & 15), gj = 16 * bj + (e & 15);
    img[e] = G[(size_t)gi * kp + gj] + ((gi == gj && gi < k) ? lambda : 0.0);
  }
  __syncthreads();
  // A = L' D L'^T row by row, as implicit_solve does it (two lanes per column, terms i even / odd), without a right-hand side
  if (tid == 0) {
    const double d = img[0];
    if (!(d > 0.0)) bad = 1;
    invd[0] = 1.0 / d;
  }
  __syncthreads();
  const int pair = tid >> 1, half = tid & 1;
  for (int j = 1; j < k; ++j) {
    const int c = j + pair;
    const bool live = c < k;
    double s = 0.0;
    if (live) {
      for (int bi = 0; 16 * bi < j; ++bi) {
        const int iend = j - 16 * bi;
        const double *pj = img + (size_t)tile_index(bi, j >> 4, nb) * 256 + (j & 15);
        const double *pc = img + (size_t)tile_index(bi, c >> 4, nb) * 256 + (c & 15);
        const double *pd = invd + 16 * bi;
        double va[8], vb[8], vd[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int ii = half + 2 * t;
          va[t] = pj[ii * 16];
          vd[t] = pd[ii];
          vb[t] = pc[ii * 16];
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) s = half + 2 * t < iend ? fma(va[t] * vd[t], vb[t], s) : s;
      }
    }
    s += __shfl_xor(s, 1, 64);
    if (live && half == 0) {
      const double v = at(j, c) - s;
      at(j, c) = v;
      if (c == j) {
        if (!(v > 0.0)) bad = 1;
        invd[j] = 1.0 / v;
      }
    }
    __syncthreads();
  }
  // R -> L^T: L[c][j] = R[j][c] / sqrt(d_j); row j of the image is scaled by its thread, then invd[j] = 1 / L[j][j]
  if (tid < k) {
    const int j = tid;
    const double rs = sqrt(invd[j]);
    for (int c = j; c < k; ++c) at(j, c) *= rs;
  }
  __syncthreads();
  if (tid < k) invd[tid] = 1.0 / at(tid, tid);
  __syncthreads();
  // X = L^-1: column m (lanes 2 m and 2 m + 1 of the workgroup) by its own forward substitution,
  //   X[m][m] = 1 / L[m][m],   X[i][m] = -(sum_{m <= p < i} L[i][p] X[p][m]) / L[i][i],
  // the terms p even / odd on the two lanes, a tile row of 16 at a time, added in ascending p.  The lanes of a column share X
  // through LDS inside their wave: wave-level ordering is all it needs.
  {
    const int m = pair;
    const bool mine = m < k;
    const int wave0 = (tid & ~63) >> 1;  // the first column of this wave: the loop bounds below are the wave's, not the lane's
    if (mine && half == 0) xat(m, m) = invd[m];
    foldin_wave_sync();
    for (int i = wave0 + 1; i < k; ++i) {
      double s = 0.0;
      const bool on = mine && i > m;
      for (int bp = wave0 >> 4; 16 * bp < i; ++bp) {
        const double *pl = img + (size_t)tile_index(bp, i >> 4, nb) * 256 + (i & 15);                    // L^T[16 bp + ii][i]
        const double *px = inv + (size_t)tile_index(mine ? m >> 4 : 0, bp, nb) * 256 + (mine ? m & 15 : 0);  // X[16 bp + ii][m]
        const bool tileOn = on && bp >= (m >> 4);
        double vl[8], vx[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int ii = half + 2 * t;
          vl[t] = pl[ii * 16];
          vx[t] = tileOn ? px[ii * 16] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int p = 16 * bp + half + 2 * t;
          s = (tileOn && p >= m && p < i) ? fma(vl[t], vx[t], s) : s;
        }
      }
      s += __shfl_xor(s, 1, 64);
      if (on && half == 0) xat(i, m) = -s * invd[i];
      foldin_wave_sync();
    }
  }
  __syncthreads();
  for (int e = tid; e < kp * kp; e += 256) {
    const int i = e / kp, m = e - i * kp;
    Linv[e] = (i < k && m <= i) ? xat(i, m) : 0.0;
  }
  if (tid == 0) flags[1] = bad;
}

// ------------------------------------------------------------------------------------------------ one dual row
template <typename T>
struct FoldDualArgs {
  const int32_t *rows;     // the dual rows of the request (foldin_plan.h): 1 <= n <= 32, n <= k, every value >= 0
  const int64_t *rowPtr;   // the request's, relative to it
  const int32_t *indx;     // validated on the host: every id is a row of `fixed`
  const T *vals;
  const T *fixed;          // [m x k]
  const double *Linv;      // [kp x kp]
  T *out;                  // [nRows x k]
  int32_t *status;         // nRows: 0 solved, 1 a pivot of the small system with !(p > 0)
  double alpha;
  int32_t k;
};

template <typename T>
__global__ __launch_bounds__(256) void foldin_implicit_dual_kernel(FoldDualArgs<T> a) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  typedef double d4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(32))) double fdual_lds[];  // (32-byte operand loads)
  __shared__ int failed;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l16 = lane & 15;
  const int row = a.rows[blockIdx.x];
  const int k = a.k, nb = (k + 15) >> 4, kp = nb << 4, ld = fold_dual_ld(kp);
  const int64_t q0 = a.rowPtr[row];
  const int n = (int)(a.rowPtr[row + 1] - q0);
  constexpr int SL = kFoldDualSLd;
  double *V = fdual_lds;                        // [32][ld]: the gathered rows, then P^T (observation q, factor j)
  double *S = V + (size_t)kFoldDualMax * ld;    // [32][33]: K, then I + D K D (upper part) with the right-hand side as column 32
  double *cv = S + kFoldDualMax * SL;           // c = 1 + w, zero past n
  double *sw = cv + kFoldDualMax;               // sqrt(w)
  double *vv = sw + kFoldDualMax;               // v = c - D y
  double *invd = vv + kFoldDualMax;             // 1 / pivot of the small system
  double *tv = invd + kFoldDualMax;             // t = P v, kp
  if (tid == 0) failed = 0;

  // ---- gather: thread (pr, pc) brings columns pc, pc + 16, ... of observations pr and pr + 16; all loads before the first store
  {
    const int pr = tid >> 4, pc = tid & 15;
    T gv[2][8], gr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = pr + 16 * h;
      const bool live = q < n;
      const T *src = a.fixed + (live ? (int64_t)a.indx[q0 + q] * k : 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = pc + 16 * j;
        gv[h][j] = (live && c < k) ? src[c] : (T)0;
      }
      gr[h] = live ? a.vals[q0 + q] : (T)0;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = pr + 16 * h;
      double *dst = V + (size_t)q * ld;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < nb) dst[pc + 16 * j] = (double)gv[h][j];
      if (pc == 0) {
        const double w = a.alpha * (double)gr[h];
        cv[q] = q < n ? 1.0 + w : 0.0;
        sw[q] = q < n ? sqrt(w) : 0.0;
      }
    }
  }
  __syncthreads();

  // ---- P = Linv V^T: block rows J = wave and 7 - wave (J + 1 column blocks each: nine per wave at kp = 128), both groups of 16
  // observations from one load of Linv.  Lane (l16, g) supplies columns 16 c + 4 g + t of Linv's row 16 J + l16 and of V's row
  // (observation) l16 in step t of block c; the result tile holds P[16 J + g + 4 r][observation l16].
  const bool two = n > 16;  // (the second group is all zeros otherwise, and so is its part of P^T: V's rows stay as they are)
  const int Jb[2] = {wave, 7 - wave};
  acc_t acc[2][2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    acc[jj][0] = acc[jj][1] = acc_t{0.0, 0.0, 0.0, 0.0};
    if (Jb[jj] < nb) {
      const double *lp = a.Linv + (size_t)(16 * Jb[jj] + l16) * kp + 4 * g;
      const double *v0 = V + (size_t)l16 * ld + 4 * g, *v1 = v0 + (size_t)16 * ld;
      for (int c = 0; c <= Jb[jj]; ++c) {
        const d4 la = *reinterpret_cast<const d4 *>(lp + 16 * c);
        const d4 b0 = *reinterpret_cast<const d4 *>(v0 + 16 * c);
        const d4 b1 = *reinterpret_cast<const d4 *>(v1 + 16 * c);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc[jj][0] = Tr::mma(la[t], b0[t], acc[jj][0]);
          if (two) acc[jj][1] = Tr::mma(la[t], b1[t], acc[jj][1]);
        }
      }
    }
  }
  __syncthreads();  // every wave has read what it needs of V
#pragma unroll
  for (int jj = 0; jj < 2; ++jj)
    if (Jb[jj] < nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * Jb[jj] + Tr::cd_row(lane, r);
        V[(size_t)l16 * ld + j] = acc[jj][0][r];
        if (two) V[(size_t)(16 + l16) * ld + j] = acc[jj][1][r];
      }
    }
  __syncthreads();

  // ---- K = P^T P: tile (0, 0) by wave 0 and, with a second group, (0, 1) by wave 1 and (1, 1) by wave 2.  Both operands of an
  // element and of its mirror image meet in the same order, so K is symmetric to the bit.
  if (wave == 0 || (two && wave < 3)) {
    const int ta = wave == 2 ? 16 : 0, tb = wave == 0 ? 0 : 16;
    const double *pa = V + (size_t)(ta + l16) * ld + 4 * g, *pb = V + (size_t)(tb + l16) * ld + 4 * g;
    acc_t kk = acc_t{0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nb; ++c) {
      const d4 x = *reinterpret_cast<const d4 *>(pa + 16 * c), y = *reinterpret_cast<const d4 *>(pb + 16 * c);
#pragma unroll
      for (int t = 0; t < 4; ++t) kk = Tr::mma(x[t], y[t], kk);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ta + Tr::cd_row(lane, r), j = tb + l16;
      S[i * SL + j] = kk[r];
      if (wave == 1) S[j * SL + i] = kk[r];
    }
  }
  __syncthreads();

  // ---- the small system, by wave 0: lane q < n owns column q, lane 32 the right-hand side (column 32)
  if (wave == 0) {
    const int q = lane;
    const bool col = q < n;
    if (col) {
      double gq = 0.0;
      for (int p = 0; p < n; ++p) gq = fma(S[p * SL + q], cv[p], gq);  // (K c)_q down the lane's own column (K is symmetric)
      const double sq = sw[q];
      for (int p = 0; p <= q; ++p) S[p * SL + q] = sw[p] * S[p * SL + q] * sq + (p == q ? 1.0 : 0.0);
      S[q * SL + kFoldDualMax] = sq * gq;
    }
    foldin_wave_sync();
    // R[j][c] = S[j][c] - sum_{i<j} R[i][j] R[i][c] / d_i, d_j = R[j][j]; the right-hand side rides along
    bool badPivot = false;
    for (int j = 0; j < n; ++j) {
      const bool live = (q >= j && col) || q == kFoldDualMax;
      if (live) {
        double s = 0.0;
#pragma unroll 4
        for (int i = 0; i < j; ++i) s = fma(S[i * SL + j] * invd[i], S[i * SL + q], s);
        const double v = S[j * SL + q] - s;
        S[j * SL + q] = v;
        if (q == j) {
          badPivot = !(v > 0.0);
          invd[j] = 1.0 / v;
        }
      }
      foldin_wave_sync();
    }
    // y_i = (z_i - sum_{c>i} R[i][c] y_c) / d_i, column by column: lane l keeps z_l, then y_l
    double y = col ? S[q * SL + kFoldDualMax] : 0.0;
    for (int c = n - 1; c >= 0; --c) {
      const double yc = __shfl(y, c, 64) * invd[c];
      if (q < c) y = fma(-S[q * SL + c], yc, y);
      if (q == c) y = yc;
    }
    if (q < kFoldDualMax) vv[q] = col ? cv[q] - sw[q] * y : 0.0;
    const bool anyBad = __ballot(badPivot) != 0;
    if (lane == 0) {
      failed = anyBad ? 1 : 0;
      a.status[row] = anyBad ? 1 : 0;
    }
  }
  __syncthreads();

  // ---- x = Linv^T (P v)
  if (tid < kp) {
    double t = 0.0;
    for (int q = 0; q < n; ++q) t = fma(V[(size_t)q * ld + tid], vv[q], t);
    tv[tid] = t;
  }
  __syncthreads();
  if (tid < k) {
    double x = 0.0;
    const double *lc = a.Linv + tid;
#pragma unroll 8
    for (int i = tid; i < k; ++i) x = fma(lc[(size_t)i * kp], tv[i], x);
    a.out[(int64_t)row * k + tid] = failed ? (T)0 : (T)x;
  }
}

// ------------------------------------------------------------------------------------------------ status, zeros, store
// One workgroup per request row.  status comes in as -1 except where the dual kernel has written 0 / 1.  flags: {bad-row count of
// the primal units, bad pivot of G + lambda I}.  implicit_unit_kernel zeroes a row it could not solve and counts it without
// naming it: a primal row is taken as failed when the count is non-zero and the row is all zeros.
// Status 0 solved; 1 bad pivot, the row zeroed; 2 no observations, zeros.  Rows with status 0 are copied to `store` (may be null).
template <typename T>
__global__ __launch_bounds__(256) void foldin_implicit_finish_kernel(const int64_t *rowPtr, const int32_t *flags, int k, T *rows, int32_t *status,
                                                                     T *store, const int32_t *storeIds) {
  const int64_t row = blockIdx.x;
  T *r = rows + row * k;
  const int tid = threadIdx.x;
  const T mine = tid < k ? r[tid] : (T)0;  // (k <= 128: one element per thread)
  const int anyNonZero = __syncthreads_or(mine != (T)0 ? 1 : 0);
  const int was = status[row];
  int st;
  if (rowPtr[row + 1] == rowPtr[row]) st = 2;
  else if (flags[1] != 0) st = 1;
  else if (was >= 0) st = was;
  else st = (flags[0] > 0 && !anyNonZero) ? 1 : 0;
  if (tid < k) {
    if (st != 0) r[tid] = (T)0;
    else if (store) store[(int64_t)storeIds[row] * k + tid] = mine;
  }
  __syncthreads();  // every thread has read status[row]
  if (tid == 0) status[row] = st;
}

}  // namespace ycnr
