// implicit_wide_kernels.hip.h -- the PRIMAL rows of ycnr_als_step_implicit_wide: the exact implicit-feedback half-step of
// implicit_kernels.hip.h for factorsCount up to 512, where a row's k x k image (1.03 MB at k = 512) fits neither registers nor
// LDS.  The rows of 1 .. 128 non-negative observations do not come here: foldin_implicit_wide_kernel solves them in dual form
// (foldin_wide_kernels.hip.h).  For every other non-empty row u, with G, alpha, lambda, S_u, r as in implicit_kernels.hip.h:
//     A_u = G + alpha sum_{i in S_u} r_ui y_i y_i^T + lambda I,   b_u = sum_{i in S_u} (1 + alpha r_ui) y_i,   x_u = A_u^-1 b_u
// A row's image lives in device memory as the packed upper 16 x 16 tiles of implicit_kernels.hip.h followed by b
// (wide_slab_elems doubles: a slab).  The rows go through in batches whose slabs fit one arena (implicit_wide_plan.h):
//   implicit_wide_classify_kernel<T>  once per upload: which rows have a value with !(r >= 0)
//   implicit_wide_gram_kernel<T>      a workgroup per (chunk unit, square of column groups): the tile columns are cut into groups
//                                     of 8 (128 columns); the workgroup walks the unit's observations once for its square
//                                     (gi <= gj) and forms the up to 8 x 8 tiles sum w y[gi] y[gj]^T on MfmaTraits<T>, sixteen
//                                     accumulator tiles per wave, observations staged through LDS in panels of 16 (the scaled
//                                     columns of gi, the plain ones of gj), the gathers of the next panel and the ids of the one
//                                     behind it in flight; the diagonal squares also form b in double on the VALU.  Sums in the
//                                     handle's precision, stored as double into the unit's slab.
//   implicit_wide_solve_kernel<T>     a workgroup of eight waves per row: the row's slabs added in slab order in double into
//                                     its first slab, + G + lambda I once (unit pivots and a zero right-hand side in the
//                                     padding); a right-looking blocked Cholesky A = R^T R, block width 16, in place:
//                                       per block row J: tiles (J, J .. nb - 1) and b_J -> a 16-row LDS panel (b as the first
//                                       column of one more tile); wave 0 factors the diagonal tile, a column per lane, and
//                                       inverts R_JJ; panel: P_b = R_JJ^-T A_Jb, four v_mfma_f64_16x16x4_f64 per tile, in place
//                                       in LDS and out to the image; trailing: A_ab -= P_a^T P_b for J < a <= b (and the
//                                       right-hand side) on the same MFMA, operands from the LDS panel, the tile read from and
//                                       written to the image.  A tile written by one wave is read by another only across a
//                                       workgroup barrier (four per block row).
//                                     Then R x = z block row by block row from the bottom, one rounding to T at the store.
//                                     A pivot with !(p > 0), a result that is not finite, or a bad pivot of G + lambda I
//                                     (flags[1]): the row becomes zeros and is counted.
//   implicit_wide_dual_finish_kernel<T>  the dual rows' status -> the bad-row count; flags[1] set: zeros for every one of them
// Every sum's order is fixed by (m, the row, the chunk length): which workgroup or batch a row fell into changes no bit.
#pragma once
#include "foldin_wide_kernels.hip.h"
#include "implicit_kernels.hip.h"
#include "implicit_wide_plan.h"

namespace ycnr {

template <typename T>
struct ImplicitWideArgs {
  const Unit *units;     // of this batch; rows are local to the shard, slabs count from `arena`
  const SplitRow *rows;  // the batch's primal rows: slab0, nslabs
  const int32_t *indx;   // validated at upload: every id is a row of `fixed`
  const T *vals;
  const T *fixed;        // [m x k]
  T *solved;             // the shard's first row of the side's matrix, written in place
  const double *G;       // [kp x kp]
  double *arena;
  const int32_t *flags;  // flags[1] != 0: a bad pivot of G + lambda I
  int32_t *badRows;
  double alpha, lambda;
  int32_t k;
};

// One thread per local row of 1 .. 128 observations: nonNegative[row] = every value is >= 0 (a NaN is not).
template <typename T>
__global__ __launch_bounds__(256) void implicit_wide_classify_kernel(const int64_t *__restrict__ rowPtr, const T *__restrict__ vals, int64_t nRows,
                                                                     uint8_t *__restrict__ nonNegative) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= nRows) return;
  const int64_t beg = rowPtr[row], end = rowPtr[row + 1];
  bool ok = end - beg <= kFoldWideMaxObs;
  if (ok)
    for (int64_t q = beg; q < end; ++q) ok = ok && vals[q] >= (T)0;
  nonNegative[row] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ one unit, one square
template <typename T>
__global__ __launch_bounds__(256) void implicit_wide_gram_kernel(ImplicitWideArgs<T> a) {
  using Tr = MfmaTraits<T>;
  using acc_t = typename Tr::acc_t;
  constexpr int W = kWideGroupTiles, LDP = kWideGramLd, P = kImplicitPanel * LDP;
  extern __shared__ double iwg_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l16 = lane & 15;
  const int k = a.k, nb = (k + 15) >> 4, kp = nb << 4, ng = (nb + W - 1) / W, nsq = tile_count(ng), nt = tile_count(nb);
  const int unit = (int)(blockIdx.x / (unsigned)nsq), sq = (int)(blockIdx.x - (unsigned)unit * (unsigned)nsq);
  int gi, gj;
  implicit_tile_of(sq, ng, gi, gj);
  const Unit u = a.units[unit];
  const int64_t q0 = u.beg, n = u.end - u.beg;
  const int64_t nPanels = (n + kImplicitPanel - 1) / kImplicitPanel;
  double *cpan = iwg_lds;                          // 2 x 16 weights 1 + alpha r
  T *pan = reinterpret_cast<T *>(iwg_lds + 32);    // buffer b: scaled columns of group gi at 2 b P, plain ones of gj at (2 b + 1) P
  const bool diag = gi == gj;
  const int ci0 = 16 * W * gi, cj0 = 16 * W * gj;
  // tile (ta, tb) = (W gi + 2 wave + i, W gj + lb) is this wave's accumulator [i][lb]; live: inside the matrix and not below
  // the diagonal
  unsigned live = 0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int lb = 0; lb < W; ++lb) {
      const int ta = W * gi + 2 * wave + i, tb = W * gj + lb;
      if (ta < nb && tb < nb && ta <= tb) live |= 1u << (W * i + lb);
    }
  acc_t acc[2][W];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int lb = 0; lb < W; ++lb) acc[i][lb] = acc_t{(T)0, (T)0, (T)0, (T)0};
  double bsum = 0.0;

  const int pr = tid >> 4, pc = tid & 15;
  T ga[W], gb[W];
  T gr = (T)0, rNext = (T)0;
  int32_t idNext = -1;  // id and value of observation pr of the panel gathered next (-1: past the unit's end)
  auto fetch_id = [&](int64_t p) {
    const int64_t q = p * kImplicitPanel + pr;
    const bool on = p < nPanels && q < n;
    idNext = on ? a.indx[q0 + q] : -1;
    rNext = on ? a.vals[q0 + q] : (T)0;
  };
  auto gather = [&]() {
    const bool on = idNext >= 0;
    const T *src = a.fixed + (on ? (int64_t)idNext * k : 0);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int c = ci0 + pc + 16 * j;
      ga[j] = (on && c < k) ? src[c] : (T)0;
    }
    if (!diag) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const int c = cj0 + pc + 16 * j;
        gb[j] = (on && c < k) ? src[c] : (T)0;
      }
    }
    gr = rNext;
  };
  auto stage = [&](int buf) {
    T *scaled = pan + (size_t)(2 * buf) * P + (size_t)pr * LDP, *plain = scaled + P;
    const T w = (T)(a.alpha * (double)gr);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      scaled[pc + 16 * j] = w * ga[j];
      plain[pc + 16 * j] = diag ? ga[j] : gb[j];
    }
    if (pc == 0) cpan[buf * kImplicitPanel + pr] = fma(a.alpha, (double)gr, 1.0);
  };
  fetch_id(0);
  gather();
  fetch_id(1);
  stage(0);
  __syncthreads();
  for (int64_t p = 0; p < nPanels; ++p) {
    const int buf = (int)(p & 1);
    if (p + 1 < nPanels) {
      gather();         // panel p + 1: in flight during the products below
      fetch_id(p + 2);  // ... and the ids behind it
    }
    const T *cur = pan + (size_t)(2 * buf) * P;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const T *r4 = cur + (size_t)(4 * s + g) * LDP + l16;
      T xa[2], yb[W];
#pragma unroll
      for (int i = 0; i < 2; ++i) xa[i] = r4[16 * (2 * wave + i)];
#pragma unroll
      for (int lb = 0; lb < W; ++lb) yb[lb] = r4[P + 16 * lb];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int lb = 0; lb < W; ++lb)
          if (live >> (W * i + lb) & 1) acc[i][lb] = Tr::mma(xa[i], yb[lb], acc[i][lb]);
    }
    if (diag && tid < 16 * W) {
      const double *cw = cpan + buf * kImplicitPanel;
#pragma unroll
      for (int q = 0; q < kImplicitPanel; ++q) bsum = fma((double)cur[P + (size_t)q * LDP + tid], cw[q], bsum);
    }
    if (p + 1 < nPanels) stage(buf ^ 1);  // last read in iteration p - 1, in front of that iteration's barrier
    __syncthreads();
  }
  double *slab = a.arena + (size_t)u.slab * (size_t)wide_slab_elems(k);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int lb = 0; lb < W; ++lb)
      if (live >> (W * i + lb) & 1) {
        double *tile = slab + (size_t)tile_index(W * gi + 2 * wave + i, W * gj + lb, nb) * 256;
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[Tr::cd_row(lane, r) * 16 + l16] = (double)acc[i][lb][r];
      }
  if (diag && tid < 16 * W && cj0 + tid < kp) slab[(size_t)nt * 256 + cj0 + tid] = bsum;
}

// ------------------------------------------------------------------------------------------------ one row: sum, factor, solve
template <typename T>
__global__ __launch_bounds__(kWideSolveThreads) void implicit_wide_solve_kernel(ImplicitWideArgs<T> a) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  constexpr int NW = kWideSolveThreads / 64;
  extern __shared__ double iws_lds[];
  __shared__ int bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l16 = lane & 15;
  const SplitRow sr = a.rows[blockIdx.x];
  const int k = a.k, nb = (k + 15) >> 4, kp = nb << 4, nt = tile_count(nb), pld = wide_solve_pld(kp);
  const size_t se = (size_t)wide_slab_elems(k);
  double *img = a.arena + (size_t)sr.slab0 * se, *rhs = img + (size_t)nt * 256;
  double *pan = iws_lds, *Rt = pan + (size_t)16 * pld, *Wt = Rt + 256, *zs = Wt + 256;
  if (tid == 0) bad = 0;

  // ---- the image: the slabs in slab order, + G + lambda I; unit pivots and a zero right-hand side in the padding
  {
    int bi = 0, bj = tid >> 8;  // tile tid >> 8, then every second one (nb >= 1: tile 1 is (0, 1), or (1, 1) at nb == 1 -- past nt)
    if (bj >= nb) bi = 1, bj = 1;
    for (int ti = tid >> 8; ti < nt; ti += 2) {
      const int e = tid & 255, gi = 16 * bi + (e >> 4), gj = 16 * bj + (e & 15);
      double *p = img + (size_t)ti * 256 + e;
      double s = 0.0;
      for (int q = 0; q < sr.nslabs; ++q) s += p[(size_t)q * se];
      s += a.G[(size_t)gi * kp + gj] + (gi == gj ? a.lambda : 0.0);
      *p = (gi < k && gj < k) ? s : (gi == gj ? 1.0 : 0.0);
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (++bj == nb) ++bi, bj = bi;
    }
    for (int c = tid; c < kp; c += kWideSolveThreads) {
      double s = 0.0;
      for (int q = 0; q < sr.nslabs; ++q) s += rhs[(size_t)q * se + c];
      rhs[c] = c < k ? s : 0.0;
    }
  }
  __syncthreads();

  // ---- A = R^T R, block row by block row
  for (int J = 0; J < nb; ++J) {
    const int below = nb - 1 - J;  // tile rows (and tile columns of the matrix) behind J
    double *rowJ = img + (size_t)tile_index(J, J, nb) * 256;  // tiles (J, J), (J, J + 1), ... follow each other
    for (int e = tid; e < (below + 2) * 256; e += kWideSolveThreads) {
      const int t = e >> 8, r = (e >> 4) & 15, c = e & 15;
      pan[(size_t)r * pld + 16 * (J + t) + c] = t <= below ? rowJ[e] : (c == 0 ? rhs[16 * J + r] : 0.0);
    }
    __syncthreads();
    if (wave == 0) {
      // lane c keeps column c of the diagonal tile; step j: row j of R goes to LDS and leaves every later row
      double av[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) av[i] = pan[(size_t)i * pld + 16 * J + l16];
      bool badPivot = false;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double p = __shfl(av[j], j, 64);
        badPivot = badPivot || !(p > 0.0);
        const double rj = l16 >= j ? av[j] * (1.0 / sqrt(p)) : 0.0;
        if (lane < 16) Rt[j * 16 + l16] = rj;
        foldin_wave_sync();
#pragma unroll
        for (int i = j + 1; i < 16; ++i) av[i] = fma(-Rt[j * 16 + i], rj, av[i]);
      }
      // column c of R^-1 from the bottom: X[c][c] = 1 / R[c][c], X[i][c] = -(sum_{i < p <= c} R[i][p] X[p][c]) / R[i][i]
      double wv[16];
#pragma unroll
      for (int i = 15; i >= 0; --i) {
        double s = 0.0;
#pragma unroll
        for (int p = i + 1; p < 16; ++p) s = fma(Rt[i * 16 + p], wv[p], s);
        const double di = 1.0 / Rt[i * 16 + i];
        wv[i] = i == l16 ? di : (i < l16 ? -s * di : 0.0);
      }
      if (lane < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          Wt[i * 16 + l16] = wv[i];
          rowJ[i * 16 + l16] = Rt[i * 16 + l16];
        }
      }
      if (lane == 0 && badPivot) bad = 1;
    }
    __syncthreads();
    // panel: P_b = R_JJ^-T A_Jb for the tiles behind the diagonal one and the right-hand side (t == below + 1)
    for (int t = 1 + wave; t <= below + 1; t += NW) {
      double *col = pan + 16 * (J + t) + l16;
      acc_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = Tr::mma(Wt[(4 * s + g) * 16 + l16], col[(size_t)(4 * s + g) * pld], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = Tr::cd_row(lane, r);
        col[(size_t)i * pld] = acc[r];
        if (t <= below) rowJ[(size_t)t * 256 + i * 16 + l16] = acc[r];
        else if (l16 == 0) rhs[16 * J + i] = acc[r];
      }
    }
    __syncthreads();
    // trailing: tile (a, b) -= P_a^T P_b for J < a <= b, b == nb: the right-hand side.  The pairs, row by row, are dealt
    // round-robin over the waves.
    {
      int la = 0, pos = wave;  // pair number `pos` of row la, which has below - la + 1 pairs
      for (;;) {
        while (la < below && pos >= below - la + 1) pos -= below - la + 1, ++la;
        if (la >= below) break;
        const int ta = J + 1 + la, tb = ta + pos;  // tb == nb: the right-hand side
        const double *pa = pan + 16 * ta + l16, *pb = pan + 16 * tb + l16;
        acc_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = Tr::mma(pa[(size_t)(4 * s + g) * pld], pb[(size_t)(4 * s + g) * pld], acc);
        if (tb < nb) {
          double *tile = img + (size_t)tile_index(ta, tb, nb) * 256 + l16;
#pragma unroll
          for (int r = 0; r < 4; ++r) tile[Tr::cd_row(lane, r) * 16] -= acc[r];
        } else if (l16 == 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) rhs[16 * ta + Tr::cd_row(lane, r)] -= acc[r];
        }
        pos += NW;
      }
    }
    __syncthreads();
  }

  // ---- R x = z, block row by block row from the bottom
  for (int c = tid; c < kp; c += kWideSolveThreads) zs[c] = rhs[c];
  __syncthreads();
  for (int J = nb - 1; J >= 0; --J) {
    if (wave == 0) {
      const double *R = img + (size_t)tile_index(J, J, nb) * 256;
      double rr[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) rr[c] = R[l16 * 16 + c];
      const double invd = 1.0 / R[l16 * 17];
      double x = zs[16 * J + l16];
#pragma unroll
      for (int c = 15; c >= 0; --c) {
        const double xc = __shfl(x, c, 64) * __shfl(invd, c, 64);
        if (l16 < c) x = fma(-rr[c], xc, x);
        if (l16 == c) x = xc;
      }
      if (lane < 16) zs[16 * J + l16] = x;
    }
    __syncthreads();
    for (int e = tid; e < 16 * J; e += kWideSolveThreads) {
      const double *R = img + (size_t)tile_index(e >> 4, J, nb) * 256 + (e & 15) * 16;
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 16; ++c) s = fma(R[c], zs[16 * J + c], s);
      zs[e] -= s;
    }
    __syncthreads();
  }
  T x = (T)0;
  if (tid < k) {
    x = (T)zs[tid];
    if (!isfinite((double)x)) bad = 1;
  }
  __syncthreads();
  const bool failed = bad != 0 || a.flags[1] != 0;
  if (tid < k) a.solved[(int64_t)sr.row * k + tid] = failed ? (T)0 : x;
  if (tid == 0 && failed) atomicAdd(a.badRows, 1);
}

// ------------------------------------------------------------------------------------------------ the dual rows' count
// One thread per dual row (both launch classes, `rows` lists them).  status: what foldin_implicit_wide_kernel wrote (1: a bad
// pivot of the small system, the row is zeros already).  flags[1]: G + lambda I had a bad pivot: zeros, counted.
template <typename T>
__global__ __launch_bounds__(256) void implicit_wide_dual_finish_kernel(const int32_t *__restrict__ rows, int64_t nRows, const int32_t *__restrict__ status,
                                                                        const int32_t *__restrict__ flags, int k, T *solved, int32_t *badRows) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nRows) return;
  const int32_t row = rows[q];
  if (flags[1] != 0) {
    for (int c = 0; c < k; ++c) solved[(int64_t)row * k + c] = (T)0;
    atomicAdd(badRows, 1);
  } else if (status[row] != 0) {
    atomicAdd(badRows, 1);
  }
}

}  // namespace ycnr
