// foldin_wide_kernels.hip.h -- fold-in for the implicit-feedback model up to factorsCount = 512 (ycnr_als_fold_in_implicit_wide):
// every served row of the request in the DUAL form of foldin_implicit_kernels.hip.h, rows of up to 128 observations.
//     M = Y^T Y + lambda I = L L^T,  Linv = L^-1                             once per call
//     P = Linv Y_S^T (k x n);   K = P^T P = Y_S M^-1 Y_S^T;   D = diag(sqrt(alpha r));   c = 1 + alpha r
//     (I + D K D) y = D K c;    v = c - D y;    x = Linv^T (Linv (Y_S^T v))
// Nothing of the k <= 128 kernels' on-chip layout carries over: L and Linv would be 1 MB each in LDS at k = 512, a row's panel
// 540 KB.  Here L and Linv are images in GLOBAL memory (ld = k rounded up to 64, <= 2 MB, L2 resident), and a row streams over
// Linv's block rows without ever holding V = Y_S or P whole.
//
// Launched in this order on the handle's stream, behind the Gramian kernels (implicit_gram_kernel or implicit_gram_wide_kernel and
// their reduce, unchanged).  No workgroup waits for another inside a kernel: the stream orders the phases.
//   foldin_wide_init_kernel      M = G + lambda I as a ld x ld image, unit diagonal in the padding
//   per 64-column block j = 0 .. nb64 - 1 (a blocked right-looking factorisation):
//     foldin_wide_diag_kernel    one workgroup: M_jj -> LDS, L D L^T and the column-per-lane-pair inverse of foldin_factor_kernel
//                                restated for one block: L_jj and W_j = L_jj^-1 (W_j is Linv's diagonal block); bad pivot -> flags[1]
//     foldin_wide_panel_kernel   a workgroup per block row i > j:      L_ij = M_ij W_j^T          v_mfma_f64_16x16x4_f64
//     foldin_wide_trail_kernel   a workgroup per pair i >= l > j:      M_il -= L_ij L_lj^T        the same MFMA
//   foldin_wide_inverse_kernel   per block distance d = 1 .. nb64 - 1, a workgroup per block (i, i - d):
//                                Linv_ij = -W_i sum_{p = j .. i-1} L_ip Linv_pj, p ascending (the sum through LDS into the second product)
//   foldin_implicit_wide_kernel<T>  one workgroup of EIGHT waves per served row, twice: the rows of <= 32 observations with the
//                                LDS of three tiles, then the others with the LDS their 36 tiles need.  Same code, same order of
//                                every sum: a row's bits do not depend on its class.  np = n rounded up to 16, ng = np / 16:
//       setup    ids, c and sqrt(w) -> LDS; padded observations get c = 0, w = 0 and a zero operand
//       stream   over the 16-row block rows J of Linv: wave g < ng forms the tile P_J[:, g] = sum_{c <= J} Linv[J, c] V[g, c]^T
//                (4 (J + 1) MFMAs; Linv by 32-byte loads, V gathered by the lane that feeds it straight from the fixed matrix in
//                the handle's type; the operands of the next step are requested before this one is multiplied, across J) and
//                writes it to panel J & 1; one barrier; then the <= 36 upper tiles of K, dealt over the eight waves, take
//                K[a][b] += P_J[:, a]^T P_J[:, b] (four MFMAs each), accumulators in registers for the whole stream
//       system   K -> LDS as packed upper tiles; D K c; S = I + D K D in place; implicit_solve (unchanged) with n columns; v
//       back     u = V^T v (thread per coordinate, observation order); t = Linv u (a wave per row, lane l the columns l, l + 64,
//                ... ascending, then a butterfly); x = Linv^T t (thread j, ascending i); one rounding to T at the store
//   foldin_wide_finish_kernel<T> status (0 solved, 1 bad pivot, 2 empty, 3 not served), zeros, the copy into the handle's matrix
// ALL arithmetic is float64 for both handle types; every sum's order is fixed by (m, the row) alone.
#pragma once
#include "foldin_implicit_kernels.hip.h"
#include "foldin_wide_plan.h"

namespace ycnr {

typedef double fwide_d4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ M, L, Linv: once per call
// G: kp x kp (full, symmetric).  M: ld x ld.
__global__ __launch_bounds__(256) void foldin_wide_init_kernel(const double *__restrict__ G, double lambda, int k, double *__restrict__ M) {
  const int kp = (k + 15) / 16 * 16, ld = fold_wide_image_ld(k);
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;  // (ld * ld is a multiple of 256)
  const int r = e / ld, c = e - r * ld;
  M[e] = (r < k && c < k) ? G[(size_t)r * kp + c] + (r == c ? lambda : 0.0) : (r == c ? 1.0 : 0.0);
}

// One workgroup.  R: the block's upper triangle row by row -- A, then R[j][c] = d_j L'[c][j], then L^T -- and, strictly below the
// diagonal, X = L^-1 (its diagonal is invd).  flags[1] <- 1 on a pivot with !(p > 0) (never cleared here).
__global__ __launch_bounds__(256) void foldin_wide_diag_kernel(const double *__restrict__ M, int ld, int j, double *__restrict__ L,
                                                               double *__restrict__ Linv, int32_t *flags) {
  constexpr int B = kFoldWideBlock, RL = B + 1;
  __shared__ double R[B * RL], invd[B];
  __shared__ int bad;
  const int tid = threadIdx.x;
  const size_t j0 = (size_t)B * j;
  if (tid == 0) bad = 0;
  for (int e = tid; e < B * B; e += 256) R[(e >> 6) * RL + (e & 63)] = M[(j0 + (e >> 6)) * ld + j0 + (e & 63)];
  __syncthreads();
  if (tid == 0) {
    const double d = R[0];
    if (!(d > 0.0)) bad = 1;
    invd[0] = 1.0 / d;
  }
  __syncthreads();
  // R[jj][c] = A[jj][c] - sum_{i < jj} R[i][jj] R[i][c] / d_i: two lanes per column c >= jj, the terms i even / odd, ascending
  const int pair = tid >> 1, half = tid & 1;
  for (int jj = 1; jj < B; ++jj) {
    const int c = jj + pair;
    const bool live = c < B;
    double s = 0.0;
    if (live)
      for (int i = half; i < jj; i += 2) s = fma(R[i * RL + jj] * invd[i], R[i * RL + c], s);
    s += __shfl_xor(s, 1, 64);
    if (live && half == 0) {
      const double v = R[jj * RL + c] - s;
      R[jj * RL + c] = v;
      if (c == jj) {
        if (!(v > 0.0)) bad = 1;
        invd[jj] = 1.0 / v;
      }
    }
    __syncthreads();
  }
  if (tid < B) {
    const double rs = sqrt(invd[tid]);
    for (int c = tid; c < B; ++c) R[tid * RL + c] *= rs;  // L[c][tid]
  }
  __syncthreads();
  if (tid < B) invd[tid] = 1.0 / R[tid * RL + tid];
  __syncthreads();
  // X[m][m] = 1 / L[m][m],  X[i][m] = -(sum_{m <= p < i} L[i][p] X[p][m]) / L[i][i]: column m by lanes 2 m and 2 m + 1 (the terms
  // p - m even / odd, ascending), every column its own forward substitution.  A column is shared inside its wave only.
  if (tid < 2 * B) {
    const int m = pair, wave0 = (tid & ~63) >> 1;  // the first column of this wave: the loop bound is the wave's
    for (int i = wave0 + 1; i < B; ++i) {
      const bool on = i > m;
      double s = 0.0;
      if (on)
        for (int p = m + half; p < i; p += 2) s = fma(R[p * RL + i], p == m ? invd[m] : R[p * RL + m], s);
      s += __shfl_xor(s, 1, 64);
      if (on && half == 0) R[i * RL + m] = -s * invd[i];
      foldin_wave_sync();
    }
  }
  __syncthreads();
  for (int e = tid; e < B * B; e += 256) {
    const int r = e >> 6, c = e & 63;
    const size_t at = (j0 + r) * ld + j0 + c;
    L[at] = c <= r ? R[c * RL + r] : 0.0;
    Linv[at] = c < r ? R[r * RL + c] : (c == r ? invd[r] : 0.0);
  }
  if (tid == 0 && bad) flags[1] = 1;
}

// The 64 x 64 products below: wave w owns the four 16 x 16 tiles of tile row w.  In step t of contraction block c lane (l16, g)
// supplies column 16 c + 4 g + t of row l16 of both operands' tiles (one 32-byte load per four MFMAs, as implicit_cg_dense); the
// result tile holds element (g + 4 r, l16) in register r.

// L_ij = M_ij W_j^T, i = j + 1 + blockIdx.x.  W_j is lower triangular: the contraction blocks right of tile column tj are skipped.
__global__ __launch_bounds__(256) void foldin_wide_panel_kernel(const double *__restrict__ M, const double *__restrict__ Linv, int ld, int j,
                                                                double *__restrict__ L) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l16 = lane & 15;
  const size_t i0 = (size_t)kFoldWideBlock * (j + 1 + blockIdx.x), j0 = (size_t)kFoldWideBlock * j;
  const double *pa = M + (i0 + 16 * wave + l16) * ld + j0 + 4 * g;
  fwide_d4 xa[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) xa[c] = *reinterpret_cast<const fwide_d4 *>(pa + 16 * c);
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    const double *pw = Linv + (j0 + 16 * tj + l16) * ld + j0 + 4 * g;
    acc_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c <= tj; ++c) {
      const fwide_d4 y = *reinterpret_cast<const fwide_d4 *>(pw + 16 * c);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = Tr::mma(xa[c][t], y[t], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) L[(i0 + 16 * wave + Tr::cd_row(lane, r)) * ld + j0 + 16 * tj + l16] = acc[r];
  }
}

// M_il -= L_ij L_lj^T for the pairs i >= l > j: blockIdx.x numbers the upper triangle of (l, i) row by row.
__global__ __launch_bounds__(256) void foldin_wide_trail_kernel(const double *__restrict__ L, int ld, int j, int nb64, double *M) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l16 = lane & 15;
  int bl, bi;
  implicit_tile_of((int)blockIdx.x, nb64 - 1 - j, bl, bi);
  const size_t i0 = (size_t)kFoldWideBlock * (j + 1 + bi), l0 = (size_t)kFoldWideBlock * (j + 1 + bl), j0 = (size_t)kFoldWideBlock * j;
  const double *pa = L + (i0 + 16 * wave + l16) * ld + j0 + 4 * g;
  fwide_d4 xa[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) xa[c] = *reinterpret_cast<const fwide_d4 *>(pa + 16 * c);
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    const double *pb = L + (l0 + 16 * tj + l16) * ld + j0 + 4 * g;
    acc_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const fwide_d4 y = *reinterpret_cast<const fwide_d4 *>(pb + 16 * c);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = Tr::mma(xa[c][t], y[t], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) M[(i0 + 16 * wave + Tr::cd_row(lane, r)) * ld + l0 + 16 * tj + l16] -= acc[r];
  }
}

// Linv_ij = -W_i sum_{p = j .. i-1} L_ip Linv_pj for i = d + blockIdx.x, j = i - d.  Every Linv_pj read lies at a distance < d.
__global__ __launch_bounds__(256) void foldin_wide_inverse_kernel(const double *__restrict__ L, double *Linv, int ld, int d) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  constexpr int TL = kFoldWideTLd;
  __shared__ double Ts[kFoldWideBlock * TL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l16 = lane & 15;
  const int i = d + (int)blockIdx.x, j = i - d;
  const size_t i0 = (size_t)kFoldWideBlock * i, j0 = (size_t)kFoldWideBlock * j;
  acc_t acc[4];
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) acc[tj] = acc_t{0.0, 0.0, 0.0, 0.0};
  for (int p = j; p < i; ++p) {
    const size_t p0 = (size_t)kFoldWideBlock * p;
    const double *pa = L + (i0 + 16 * wave + l16) * ld + p0 + 4 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const fwide_d4 x = *reinterpret_cast<const fwide_d4 *>(pa + 16 * c);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double *pb = Linv + (p0 + 16 * c + 4 * g + t) * ld + j0 + l16;  // row 16 c + 4 g + t of Linv_pj
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[tj] = Tr::mma(x[t], pb[16 * tj], acc[tj]);
      }
    }
  }
#pragma unroll
  for (int tj = 0; tj < 4; ++tj)
#pragma unroll
    for (int r = 0; r < 4; ++r) Ts[(16 * wave + Tr::cd_row(lane, r)) * TL + 16 * tj + l16] = acc[tj][r];
  __syncthreads();
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) acc[tj] = acc_t{0.0, 0.0, 0.0, 0.0};
  const double *pw = Linv + (i0 + 16 * wave + l16) * ld + i0 + 4 * g;  // W_i: lower triangular, the blocks right of `wave` are zero
  for (int c = 0; c <= wave; ++c) {
    const fwide_d4 x = *reinterpret_cast<const fwide_d4 *>(pw + 16 * c);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double *pb = Ts + (16 * c + 4 * g + t) * TL + l16;
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) acc[tj] = Tr::mma(x[t], pb[16 * tj], acc[tj]);
    }
  }
#pragma unroll
  for (int tj = 0; tj < 4; ++tj)
#pragma unroll
    for (int r = 0; r < 4; ++r) Linv[(i0 + 16 * wave + Tr::cd_row(lane, r)) * ld + j0 + 16 * tj + l16] = -acc[tj][r];
}

// ------------------------------------------------------------------------------------------------ one served row
template <typename T>
struct FoldWideArgs {
  const int32_t *rows;     // the rows of this launch class (foldin_wide_plan.h): 1 <= n <= 128 (<= 32 in the short class), every value >= 0
  const int64_t *rowPtr;   // the request's, relative to it
  const int32_t *indx;     // validated on the host: every id is a row of `fixed`
  const T *vals;
  const T *fixed;          // [m x k]
  const double *Linv;      // [ld x ld]
  T *out;                  // [nRows x k]
  int32_t *status;         // nRows: 0 solved, 1 a pivot of the small system with !(p > 0)
  double alpha;
  int32_t k, ld;
};

constexpr int kFoldWideSlots = 5;  // upper tiles of K per wave: 36 over eight waves

template <typename T>
__global__ __launch_bounds__(kFoldWideThreads) void foldin_implicit_wide_kernel(FoldWideArgs<T> a) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  extern __shared__ __attribute__((aligned(32))) double fwide_lds[];
  __shared__ int bad;
  __shared__ int32_t badCount;  // (what implicit_solve counts into; not used)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l16 = lane & 15;
  const int row = a.rows[blockIdx.x];
  const int k = a.k, nb = (k + 15) >> 4, kp = nb << 4, ld = a.ld;
  const int64_t q0 = a.rowPtr[row];
  const int n = (int)(a.rowPtr[row + 1] - q0), np = fold_wide_np(n), ng = np >> 4, nt = tile_count(ng), pld = fold_wide_pld(np);
  const FoldWideLds o = fold_wide_lds(np, kp);
  double *S = fwide_lds + o.S, *panel = fwide_lds + o.panel, *cv = fwide_lds + o.cv, *sw = fwide_lds + o.sw, *rhs = fwide_lds + o.rhs,
         *yv = fwide_lds + o.yv, *vv = fwide_lds + o.vv, *invd = fwide_lds + o.invd, *uv = fwide_lds + o.u, *tv = fwide_lds + o.t;
  int32_t *ids = reinterpret_cast<int32_t *>(fwide_lds + o.ids);

  // ---- setup
  if (tid == 0) bad = 0, badCount = 0;
  if (tid < np) {
    const bool live = tid < n;
    const double w = live ? a.alpha * (double)a.vals[q0 + tid] : 0.0;
    cv[tid] = live ? 1.0 + w : 0.0;
    sw[tid] = live ? sqrt(w) : 0.0;
    ids[tid] = live ? a.indx[q0 + tid] : -1;
  }
  __syncthreads();

  // ---- stream over the block rows of Linv
  int offA[kFoldWideSlots], offB[kFoldWideSlots];
  acc_t kacc[kFoldWideSlots];
#pragma unroll
  for (int s = 0; s < kFoldWideSlots; ++s) {
    int ta = 0, tb = 0;
    if (wave + 8 * s < nt) implicit_tile_of(wave + 8 * s, ng, ta, tb);
    offA[s] = 16 * ta + l16;
    offB[s] = 16 * tb + l16;
    kacc[s] = acc_t{0.0, 0.0, 0.0, 0.0};
  }
  const bool forms = wave < ng;  // this wave forms the tiles of observations 16 wave .. 16 wave + 15
  const int32_t id = forms ? ids[16 * wave + l16] : -1;
  const T *src = a.fixed + (id >= 0 ? (int64_t)id * k : 0) + 4 * g;
  const double *lrow = a.Linv + (size_t)l16 * ld + 4 * g;
  // step (J, c): columns 16 c + 4 g + t of Linv's row 16 J + l16 and of the lane's observation
  auto load_l = [&](int J, int c) { return *reinterpret_cast<const fwide_d4 *>(lrow + (size_t)16 * J * ld + 16 * c); };
  auto load_v = [&](int c, T(&y)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) y[t] = (id >= 0 && 16 * c + 4 * g + t < k) ? src[16 * c + t] : (T)0;
  };
  fwide_d4 lNext = {0.0, 0.0, 0.0, 0.0};
  T yNext[4] = {(T)0, (T)0, (T)0, (T)0};
  if (forms) {
    lNext = load_l(0, 0);
    load_v(0, yNext);
  }
  for (int J = 0; J < nb; ++J) {
    double *pan = panel + (size_t)(J & 1) * 16 * pld;
    if (forms) {
      acc_t acc = {0.0, 0.0, 0.0, 0.0};
      for (int c = 0; c <= J; ++c) {
        const fwide_d4 lc = lNext;
        T y[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) y[t] = yNext[t];
        // the operands of the next step -- of the next block row behind the last one of this -- before this step is multiplied
        if (c < J) {
          lNext = load_l(J, c + 1);
          load_v(c + 1, yNext);
        } else if (J + 1 < nb) {
          lNext = load_l(J + 1, 0);
          load_v(0, yNext);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = Tr::mma(lc[t], (double)y[t], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) pan[Tr::cd_row(lane, r) * pld + 16 * wave + l16] = acc[r];
    }
    __syncthreads();  // (panel (J + 1) & 1 was last read in iteration J - 1, in front of this barrier)
#pragma unroll
    for (int s = 0; s < kFoldWideSlots; ++s)
      if (wave + 8 * s < nt) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double *r4 = pan + (4 * g + t) * pld;
          kacc[s] = Tr::mma(r4[offA[s]], r4[offB[s]], kacc[s]);
        }
      }
  }

  // ---- the small system: K as packed upper tiles, D K c, S = I + D K D, the solve, v
#pragma unroll
  for (int s = 0; s < kFoldWideSlots; ++s)
    if (wave + 8 * s < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) S[(size_t)(wave + 8 * s) * 256 + Tr::cd_row(lane, r) * 16 + l16] = kacc[s][r];
    }
  __syncthreads();
  if (tid < np) {
    // (K c)_q down column q, ascending p: K[p][q] above the diagonal, its mirror image K[q][p] below (K is symmetric to the bit)
    double gq = 0.0;
    for (int p = 0; p < n; ++p) {
      const int lo = p < tid ? p : tid, hi = p < tid ? tid : p;
      gq = fma(S[(size_t)tile_index(lo >> 4, hi >> 4, ng) * 256 + (lo & 15) * 16 + (hi & 15)], cv[p], gq);
    }
    rhs[tid] = sw[tid] * gq;
  }
  __syncthreads();
  for (int e = tid; e < nt * 256; e += kFoldWideThreads) {
    int bi, bj;
    implicit_tile_of(e >> 8, ng, bi, bj);
    const int i = 16 * bi + ((e >> 4) & 15), j = 16 * bj + (e & 15);
    S[e] = sw[i] * S[e] * sw[j] + (i == j ? 1.0 : 0.0);
  }
  __syncthreads();
  implicit_solve<double>(S, rhs, invd, &bad, n, ng, yv, &badCount);
  __syncthreads();
  if (tid < np) vv[tid] = tid < n ? cv[tid] - sw[tid] * yv[tid] : 0.0;
  __syncthreads();

  // ---- back: u = V^T v, t = Linv u, x = Linv^T t
  if (tid < kp) {
    double s = 0.0;
    if (tid < k)
      for (int q = 0; q < n; ++q) s = fma((double)a.fixed[(int64_t)ids[q] * k + tid], vv[q], s);
    uv[tid] = s;
  }
  __syncthreads();
  for (int i = wave; i < kp; i += 8) {
    const double *lr = a.Linv + (size_t)i * ld;
    double s = 0.0;
    for (int j = lane; j <= i; j += 64) s = fma(lr[j], uv[j], s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (lane == 0) tv[i] = s;
  }
  __syncthreads();
  const bool failed = bad != 0;
  if (tid < k) {
    double x = 0.0;
    const double *lc = a.Linv + tid;
#pragma unroll 8
    for (int i = tid; i < k; ++i) x = fma(lc[(size_t)i * ld], tv[i], x);
    a.out[(int64_t)row * k + tid] = failed ? (T)0 : (T)x;
  }
  if (tid == 0) a.status[row] = failed ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ status, zeros, store
// One workgroup per request row.  status comes in as -1 except where the row kernel has written 0 / 1.  flags[1]: a bad pivot of
// G + lambda I.  Status 0 solved; 1 bad pivot; 2 no observations; 3 not served.  Rows with a non-zero status become zeros, rows
// with status 0 are copied to `store` (may be null).
template <typename T>
__global__ __launch_bounds__(256) void foldin_wide_finish_kernel(const int64_t *rowPtr, const int32_t *flags, int k, T *rows, int32_t *status,
                                                                 T *store, const int32_t *storeIds) {
  const int64_t row = blockIdx.x;
  T *r = rows + row * k;
  const int was = status[row];
  int st;
  if (rowPtr[row + 1] == rowPtr[row]) st = 2;
  else if (was < 0) st = 3;
  else if (flags[1] != 0) st = 1;
  else st = was;
  for (int c = threadIdx.x; c < k; c += 256) {
    if (st != 0) r[c] = (T)0;
    else if (store) store[(int64_t)storeIds[row] * k + c] = r[c];
  }
  __syncthreads();  // every thread has read status[row]
  if (threadIdx.x == 0) status[row] = st;
}

}  // namespace ycnr
