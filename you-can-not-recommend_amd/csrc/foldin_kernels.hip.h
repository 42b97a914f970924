// foldin_kernels.hip.h -- fold-in: solve the factor rows of a REQUEST (new users / new items whose ratings arrive in the
// call) against the fixed opposite matrix the handle holds on the device.
//
// The reference has no such path: a user without a trained row gets no personal recommendations
// (YcnrController.recommendItemsForUser, lib/YcnrController.js:275-280) and its warm start gives new rows random
// factors (EmfMaster.js:347-358).  One row of a half-step is all a new row needs:
//     x = (Y^T Y + lambda n I)^-1 Y^T r,   Y = fixed[indx[0..n), :]          (EmfWorker.js:214-248)
//
// als_foldin_kernel<T>, factorsCount <= 128, T = float | double, one launch per request, no host-built plan:
//  * one workgroup of 256 threads (four waves) per request row;
//  * ALL arithmetic in double: gathered factors and ratings are converted exactly, the result is rounded to T once at
//    the store -- a float32 handle's row is the float64 solution of its float32 inputs;
//  * Gramian on v_mfma_f64_16x16x4_f64 (MfmaTraits<double>): k padded to kp = 16 nb, the nb (nb + 1) / 2 <= 36 upper
//    tiles dealt round-robin over the four waves (<= 9 tiles = 72 accumulator registers per wave); the gathered rows go
//    through LDS in panels of 16 ratings as double [16][ld], two buffers: the gather of panel p + 1 is in flight while
//    panel p is multiplied.  The contraction runs over the ratings in request order, four per MFMA;
//  * b = Y^T r: one double fma chain per column, in rating order, on the VALU (threads 0 .. kp - 1);
//  * every sum's order is fixed by the row alone: a row's bits do not depend on what else the request holds;
//  * solve: lambda n on the diagonal, the packed upper tiles in LDS (<= 72 KB, over the dead panels), an L D L^T
//    factorisation in double by the whole workgroup -- the square-root-free Cholesky: its pivots d_j are the Cholesky
//    pivots before the root -- with the right-hand side carried along as one more column (the forward substitution),
//    then the back substitution by wave 0.  Only the k real columns are factorised, so the padded columns need no
//    unit diagonal: nothing reads them;
//  * a pivot p with !(p > 0) (NaN included) sets the row's status to 1 and its output to zeros; the flag is looked at
//    after the last barrier, no thread leaves early.  A row without ratings gets status 2 and zeros (the whole
//    workgroup returns before its first barrier).
// Plain HIP + the MFMA builtin; the compiler counts the waits.
#pragma once
#include "als_kernels.hip.h"

namespace ycnr {

constexpr int kFoldMaxK = 128;
constexpr int kFoldPanel = 16;  // ratings per LDS panel = four MFMA contraction steps

// leading dimension (doubles) of a panel row: 16 mod 32, so that the two rows a half-wave reads fall on different banks
__host__ __device__ constexpr int foldin_ld(int kp) { return kp % 32 == 0 ? kp + 16 : kp; }
// dynamic LDS of the kernel: [image of packed upper tiles | two panels] (aliased), rhs, 1 / d, two panels of ratings
__host__ __device__ constexpr size_t foldin_lds_bytes(int k) {
  const int nb = (k + 15) / 16, kp = nb * 16;
  const size_t img = (size_t)tile_count(nb) * 256, pan = (size_t)2 * kFoldPanel * foldin_ld(kp);
  return ((img > pan ? img : pan) + 2 * (size_t)kp + 2 * kFoldPanel) * sizeof(double);
}

template <typename T>
struct FoldArgs {
  const int64_t *rowPtr;    // nRows + 1, relative to the request
  const int32_t *indx;      // validated on the host: every id is a row of `fixed`
  const T *vals;
  const T *fixed;           // [fixedRows x k]: the handle's matrix of the opposite side
  T *out;                   // [nRows x k]
  int32_t *status;          // nRows
  T *store;                 // the handle's matrix of the solved side, or null
  const int32_t *storeIds;  // nRows row ids of `store` (with store)
  double lambda;
  int32_t k;
};

template <typename T>
__global__ __launch_bounds__(256) void als_foldin_kernel(FoldArgs<T> a) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  extern __shared__ double fold_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const int k = a.k, nb = (k + 15) >> 4, kp = nb << 4, ld = foldin_ld(kp), nt = tile_count(nb);
  const int64_t q0 = a.rowPtr[row];
  const int64_t n = a.rowPtr[row + 1] - q0;
  T *out = a.out + row * k;
  if (n <= 0) {  // the whole workgroup: no barrier has been reached
    for (int c = tid; c < k; c += 256) out[c] = (T)0;
    if (tid == 0) a.status[row] = 2;
    return;
  }
  const size_t imgElems = (size_t)nt * 256, panElems = (size_t)2 * kFoldPanel * ld;
  double *img = fold_lds;                                          // packed upper tiles, 16 x 16 row-major each
  double *pan = fold_lds;                                          // the two panels: dead before the image is written
  double *rhs = fold_lds + (imgElems > panElems ? imgElems : panElems);  // kp
  double *invd = rhs + kp;                                         // kp
  double *rpan = invd + kp;                                        // 2 x 16 ratings
  __shared__ int bad;
  if (tid == 0) bad = 0;

  // this wave's tiles: wave, wave + 4, ... (upper triangle in row-major order of the tiles)
  int offA[9], offB[9];
  bool diag[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    int rem = wave + 4 * t, bi = 0;
    if (rem < nt) {
      while (rem >= nb - bi) {
        rem -= nb - bi;
        ++bi;
      }
    } else {
      rem = 0;
    }
    offA[t] = 16 * bi + (lane & 15);
    offB[t] = 16 * (bi + rem) + (lane & 15);
    diag[t] = rem == 0;
  }
  acc_t acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = acc_t{0.0, 0.0, 0.0, 0.0};
  double bsum = 0.0;

  // gather: thread (pr = tid / 16, pc = tid % 16) brings columns pc, pc + 16, ... of the panel's rating pr
  const int pr = tid >> 4, pc = tid & 15;
  const int64_t nPanels = (n + kFoldPanel - 1) / kFoldPanel;
  T g[8];  // as loaded: converted when staged, so that nothing waits for the loads before the products
  T gr = (T)0;
  auto gather = [&](int64_t p) {
    const int64_t q = p * kFoldPanel + pr;
    const bool live = q < n;
    const T *src = a.fixed + (live ? (int64_t)a.indx[q0 + q] * k : 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = pc + 16 * j;
      g[j] = (live && c < k) ? src[c] : (T)0;
    }
    if (pc == 0) gr = live ? a.vals[q0 + q] : (T)0;
  };
  auto stage = [&](int buf) {
    double *dst = pan + (size_t)buf * kFoldPanel * ld + (size_t)pr * ld;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nb) dst[pc + 16 * j] = (double)g[j];
    if (pc == 0) rpan[buf * kFoldPanel + pr] = (double)gr;
  };
  gather(0);
  stage(0);
  __syncthreads();
  for (int64_t p = 0; p < nPanels; ++p) {
    const int buf = (int)(p & 1);
    if (p + 1 < nPanels) gather(p + 1);  // in flight during the products below
    const double *cur = pan + (size_t)buf * kFoldPanel * ld;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const double *r4 = cur + (size_t)(4 * s + (lane >> 4)) * ld;
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if (wave + 4 * t < nt) acc[t] = Tr::mma(r4[offA[t]], r4[offB[t]], acc[t]);
    }
    if (tid < kp) {
      const double *rr = rpan + buf * kFoldPanel;
#pragma unroll
      for (int q = 0; q < kFoldPanel; ++q) bsum = fma(cur[(size_t)q * ld + tid], rr[q], bsum);
    }
    if (p + 1 < nPanels) stage(buf ^ 1);  // last read in iteration p - 1, before that iteration's barrier
    __syncthreads();
  }
  // (every read of the panels lies in front of the loop's last barrier) the image: Gramian + lambda n on the diagonal
  const double ridge = a.lambda * (double)n;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int ti = wave + 4 * t;
    if (ti < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tr = Tr::cd_row(lane, r), tc = lane & 15;
        img[(size_t)ti * 256 + tr * 16 + tc] = acc[t][r] + ((diag[t] && tr == tc) ? ridge : 0.0);
      }
    }
  }
  if (tid < kp) rhs[tid] = bsum;
  __syncthreads();

  // element (i, c), i <= c, of the packed image
  auto at = [&](int i, int c) -> double & {
    const int bi = i >> 4, bj = c >> 4;
    return img[(size_t)tile_index(bi, bj, nb) * 256 + (i & 15) * 16 + (c & 15)];
  };
  // A = L D L^T, row by row: R[j][c] = A[j][c] - sum_{i<j} R[i][j] R[i][c] / d_i, d_j = R[j][j], L[c][j] = R[j][c] / d_j.
  // Two lanes per column (terms i even / odd, added pairwise); the right-hand side is column k: z = L^-1 b.
  if (tid == 0) {
    const double d = at(0, 0);
    if (!(d > 0.0)) bad = 1;
    invd[0] = 1.0 / d;
  }
  __syncthreads();
  const int pair = tid >> 1, half = tid & 1;
  for (int j = 1; j < k; ++j) {
    const int c = j + pair;  // c == k: the right-hand side
    const bool live = c <= k;
    double s = 0.0;
    if (live) {
      // tile row by tile row: the (up to) eight terms of this lane are loaded together -- rows past j are loaded too (they lie
      // inside the tile) and left out of the sum -- then added in ascending i
      for (int bi = 0; 16 * bi < j; ++bi) {
        const int iend = j - 16 * bi;
        const double *pj = img + (size_t)tile_index(bi, j >> 4, nb) * 256 + (j & 15);
        const double *pc = c < k ? img + (size_t)tile_index(bi, c >> 4, nb) * 256 + (c & 15) : rhs + 16 * bi;
        const int sc = c < k ? 16 : 1;
        const double *pd = invd + 16 * bi;
        double va[8], vb[8], vd[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int ii = half + 2 * t;
          va[t] = pj[ii * 16];
          vd[t] = pd[ii];
          vb[t] = pc[ii * sc];
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) s = half + 2 * t < iend ? fma(va[t] * vd[t], vb[t], s) : s;
      }
    }
    s += __shfl_xor(s, 1, 64);
    if (live && half == 0) {
      if (c < k) {
        const double v = at(j, c) - s;
        at(j, c) = v;
        if (c == j) {
          if (!(v > 0.0)) bad = 1;
          invd[j] = 1.0 / v;
        }
      } else {
        rhs[j] -= s;
      }
    }
    __syncthreads();
  }
  // back substitution by wave 0: x_i = (z_i - sum_{c>i} R[i][c] x_c) / d_i; lane l keeps z_l and z_{l+64}, then x_l and x_{l+64}
  if (wave == 0) {
    // column by column: once x_c is known (one broadcast from its lane), every row above takes its term out of its own z
    double x0 = lane < k ? rhs[lane] : 0.0, x1 = lane + 64 < k ? rhs[lane + 64] : 0.0;
    for (int c = k - 1; c >= 0; --c) {
      const double xc = __shfl(c < 64 ? x0 : x1, c & 63, 64) * invd[c];
      if (lane < c) x0 = fma(-at(lane, c), xc, x0);
      if (lane + 64 < c) x1 = fma(-at(lane + 64, c), xc, x1);
      if (lane == c) x0 = xc;
      if (lane + 64 == c) x1 = xc;
    }
    const bool failed = bad != 0;
    const bool keep = a.store != nullptr && !failed;
    T *dst = keep ? a.store + (int64_t)a.storeIds[row] * k : nullptr;
    if (lane < k) {
      const T v = failed ? (T)0 : (T)x0;
      out[lane] = v;
      if (keep) dst[lane] = v;
    }
    if (lane + 64 < k) {
      const T v = failed ? (T)0 : (T)x1;
      out[lane + 64] = v;
      if (keep) dst[lane + 64] = v;
    }
    if (lane == 0) a.status[row] = failed ? 1 : 0;
  }
}

// recommend_for_ratings: users whose fold-in failed or who gave no rating get an empty list
__global__ __launch_bounds__(256) void foldin_clear_lists_kernel(const int32_t *status, int64_t nUsers, int limit, int32_t *ids, double *pred, int32_t *cnt) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nUsers * limit) return;
  const int64_t u = q / limit;
  if (status[u] == 0) return;
  ids[q] = -1;
  pred[q] = 0.0;
  if (q == u * limit) cnt[u] = 0;
}

// factorsCount > 128 (the request went through the step kernels, out of place): status and store.  Those kernels count the rows
// that were not positive definite and name one of them (ErrInfo), not all: with any such row EVERY solved row of the call gets
// status 1 and zeros.  Rows without ratings (never written by the kernels) get status 2 and zeros.
template <typename T>
__global__ __launch_bounds__(256) void foldin_finish_kernel(const int64_t *rowPtr, const ErrInfo *err, int64_t nRows, int k, T *rows, int32_t *status,
                                                            T *store, const int32_t *storeIds) {
  const int64_t row = blockIdx.x;
  const int st = rowPtr[row + 1] == rowPtr[row] ? 2 : err->count > 0 ? 1 : 0;
  T *r = rows + row * k;
  for (int c = threadIdx.x; c < k; c += 256) {
    if (st != 0) r[c] = (T)0;
    else if (store) store[(int64_t)storeIds[row] * k + c] = r[c];
  }
  if (threadIdx.x == 0) status[row] = st;
}

__global__ __launch_bounds__(256) void foldin_iota_kernel(int32_t *ids, int64_t n) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < n) ids[q] = (int32_t)q;
}

}  // namespace ycnr
