// implicit_sub_kernels.hip.h -- the implicit-feedback half-step by block coordinate descent on each row's quadratic, sixteen
// coordinates at a time: the subspace solver of iALS++ (Rendle, Krichene, Zhang, Koren 2021, "iALS++: Speeding up Matrix
// Factorization with Subspace Optimization"), factorsCount <= 512.  Nothing here grows with k^2 on chip: a row's state is one
// k-vector, and the largest system solved is 16 x 16.
//
// Y = all m rows of the fixed matrix, G = Y^T Y, lambda plain.  For a row: S = its observations, r_i = raw values, w_i = alpha r_i,
// c_i = 1 + w_i.  B = ceil(k / 16) blocks, pi_b = coordinates 16 b .. min(16 b + 15, k - 1).
//     x = the row as it stands;   e_i = y_i . x   for i in S
//     repeat `sweeps` times, for b = 0 .. B-1 in order:
//         g = (G x)_pi + lambda x_pi + sum_i (w_i e_i - c_i) y_i,pi
//         H = G_pipi + lambda I + sum_i w_i y_i,pi y_i,pi^T
//         delta = H^-1 g  (L D L^T);   a pivot p with !(p > 0): the row is bad
//         x_pi -= delta;   e_i -= y_i,pi . delta   for i in S
//     store x, rounded once to T
// Per sweep a row of n observations costs about 2 n k multiply-adds for scores and gradients, 8 n k for the Hessians and k^2 for
// its share of the product with G, where the exact solve costs n k^2 + k^3 / 3.
//
// implicit_sub_kernel<T>: one workgroup of 256 threads (four waves) takes a batch of 16 whole rows through the prologue and all
// sweeps * B block steps.  x of the batch lies in LDS as double [16][ld]; the scores e lie in global memory, one double per
// rating at the rating's CSR position (written and read by this workgroup alone, with the block step's barriers in between).
// Everything is float64 for both T.  A block step has three phases:
//   sparse   a row's observations in strips of 16 = four contraction steps of v_mfma_f64_16x16x4_f64: lane (l, q) gathers
//            y_i[16 b + l] of observation i = 4 t + q of the strip in step t, A operand = w_i y, B operand = y, one accumulator
//            tile is the row's Hessian sum.  The same lane adds (w_i e_i - c_i) y to its share of the gradient (VALU; the four
//            shares are joined by a two-step butterfly at the row's end).  The score update of the PREVIOUS block step is applied
//            in the same pass: the lane also gathers y_i[16 b' + l], the group's 16 lanes sum y . delta' by a butterfly, and e_i
//            is written back once (not in the last block step: nobody reads it).  The gathers of strip s + 1 and the ids of strip
//            s + 2 are requested before strip s is multiplied.  A row of at most kSubWideRow observations is walked by one wave
//            (batch row j by wave j mod 4); a longer one by all four, strip s by wave s mod 4, the four partial H and g joined
//            through LDS in wave order.  Which of the two depends on the row alone.
//   dense    (G X)_pi for the 16 rows: one 16 x kp by kp x 16 product, the 16-column stretches of the contraction dealt over the
//            waves (stretch c to wave c mod 4), G from global memory (L2 resident, read once per 16 rows), X from LDS; the four
//            partial tiles are joined in wave order by the solve.
//   solve    16 lanes per row, four rows per wave: lane c holds column c of H in registers; right-looking L D L^T with the
//            gradient as one more row, back substitution, x_pi -= delta, delta kept in LDS for the next step's score update.
//            Padded coordinates of the last block have a unit pivot and a zero gradient.
// implicit_gram_wide_kernel<T> + implicit_gram_wide_reduce_kernel: G for k > 128 (the packed tiles of implicit_gram_kernel do not
// fit its registers there).  For k <= 128 the half-step uses implicit_gram_kernel unchanged.
// Every sum's order is fixed by (m, the row): the same request gives the same bits, whichever rows share a batch.
#pragma once
#include "implicit_cg_kernels.hip.h"

namespace ycnr {

constexpr int kImplicitSubMaxK = 512;
constexpr int kSubBatch = 16;       // rows per workgroup = columns of the dense product's B operand
constexpr int kSubMaxSweeps = 16;
constexpr int kSubWideRow = 256;    // a row of more observations is walked by all four waves (not measured: DESIGN.md 14)
constexpr int kSubPart = 272;       // doubles of one wave's partial: a 16 x 16 tile and 16 gradient sums

// x [16][ld] | the waves' partials [4][272] | H [16][256] | sparse gradient [16][16] | delta [16][16]
__host__ __device__ constexpr size_t implicit_sub_lds_bytes(int k) {
  const int kp = (k + 15) / 16 * 16;
  return ((size_t)kSubBatch * implicit_ld(kp) + 4 * kSubPart + kSubBatch * 256 + 2 * kSubBatch * 16) * sizeof(double);
}

template <typename T>
struct ImplicitSubArgs {
  const Unit *rows;      // every non-empty row of the piece, whole, longest first
  int64_t nRows;
  const int32_t *indx;   // validated at upload: every id is a row of `fixed`
  const T *vals;
  const T *fixed;        // [m x k]
  T *solved;             // [rows x k]: read for the warm start, written in place
  const double *G;       // [kp x kp], full and symmetric, padding exactly zero
  double *scores;        // one per rating of the piece
  int32_t *badRows;
  double alpha, lambda;
  int32_t k, sweeps;
};

// e_i = y_i . x for strips first, first + stride, ... of a row: 16 lanes per observation, four observations per wave at a time
template <typename T>
__device__ __forceinline__ void implicit_sub_scores(const ImplicitSubArgs<T> &a, const double *x, int64_t beg, int n, int first, int stride,
                                                    int lane) {
  const int q = lane >> 4, l = lane & 15, k = a.k, nb = (k + 15) >> 4;
  for (int o0 = 16 * first; o0 < n; o0 += 16 * stride)
    for (int t = 0; t < 4; ++t) {
      const int o = o0 + 4 * t + q;
      const bool live = o < n;
      const T *src = a.fixed + (live ? (int64_t)a.indx[beg + o] * k : 0);
      double s = 0.0;
      for (int c = 0; c < nb; ++c) {
        const int col = l + 16 * c;
        s = fma((live && col < k) ? (double)src[col] : 0.0, x[col], s);
      }
      s = implicit_cg_group_sum(s);
      if (live && l == 0) a.scores[beg + o] = s;
    }
}

// Strips first, first + stride, ... of a row for block b (col = 16 b + l of this lane): H += sum w y y^T, gsum += sum (w e - c) y
// over this lane's observations; prev (pcol = this lane's column of the previous block, dp = its delta): e -= y' . delta' first.
template <typename T>
__device__ __forceinline__ void implicit_sub_walk(const ImplicitSubArgs<T> &a, int64_t beg, int n, int first, int stride, int col, bool prev,
                                                  int pcol, double dp, bool storeE, int lane, typename MfmaTraits<double>::acc_t &H,
                                                  double &gsum) {
  using Tr = MfmaTraits<double>;
  const int q = lane >> 4, l = lane & 15, k = a.k;
  const bool colLive = col < k, pLive = prev && pcol < k;
  const int nStrips = (n + 15) >> 4;
  int32_t id0[4], id1[4];
  double w0[4], w1[4];
  T y0[4], p0[4];
  double e0[4];
  auto ids = [&](int s, int32_t(&id)[4], double(&w)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int o = 16 * s + 4 * t + q;
      const bool live = s < nStrips && o < n;
      id[t] = live ? a.indx[beg + o] : -1;
      w[t] = live ? a.alpha * (double)a.vals[beg + o] : 0.0;
    }
  };
  auto gather = [&](int s, const int32_t(&id)[4], T(&y)[4], T(&p)[4], double(&e)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bool live = id[t] >= 0;
      const T *src = a.fixed + (live ? (int64_t)id[t] * k : 0);
      y[t] = (live && colLive) ? src[col] : (T)0;
      p[t] = (live && pLive) ? src[pcol] : (T)0;
      e[t] = live ? a.scores[beg + 16 * s + 4 * t + q] : 0.0;
    }
  };
  ids(first, id0, w0);
  gather(first, id0, y0, p0, e0);
  ids(first + stride, id1, w1);
  for (int s = first; s < nStrips; s += stride) {
    // the gathers of the next strip and the ids of the one behind it are requested before this strip is multiplied
    int32_t id2[4];
    double w2[4], e1[4];
    T y1[4], p1[4];
    gather(s + stride, id1, y1, p1, e1);
    ids(s + 2 * stride, id2, w2);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double yv = (double)y0[t];
      double ev = e0[t];
      if (prev) {
        ev -= implicit_cg_group_sum((double)p0[t] * dp);
        if (storeE && id0[t] >= 0 && l == 0) a.scores[beg + 16 * s + 4 * t + q] = ev;
      }
      gsum = fma(fma(w0[t], ev, -(1.0 + w0[t])), yv, gsum);  // (a dead observation: y = 0)
      H = Tr::mma(w0[t] * yv, yv, H);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      id0[t] = id1[t], w0[t] = w1[t], y0[t] = y1[t], p0[t] = p1[t], e0[t] = e1[t];
      id1[t] = id2[t], w1[t] = w2[t];
    }
  }
  gsum += __shfl_xor(gsum, 16, 64);
  gsum += __shfl_xor(gsum, 32, 64);
}

template <typename T>
__global__ __launch_bounds__(256) void implicit_sub_kernel(ImplicitSubArgs<T> a) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  typedef double d4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(32))) double isub_lds[];  // (32-byte B fragments)
  __shared__ int64_t sBeg[kSubBatch];
  __shared__ int sN[kSubBatch], sRow[kSubBatch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 4, l16 = lane & 15;
  const int k = a.k, nb = (k + 15) >> 4, kp = nb << 4, ld = implicit_ld(kp);
  double *xs = isub_lds, *part = xs + kSubBatch * ld, *Hs = part + 4 * kSubPart, *gs = Hs + kSubBatch * 256, *dl = gs + kSubBatch * 16;
  if (tid < kSubBatch) {
    const int64_t i = (int64_t)blockIdx.x * kSubBatch + tid;
    const Unit u = i < a.nRows ? a.rows[i] : Unit{0, 0, -1, -1};  // a batch's unused places: zero vectors that never move
    sBeg[tid] = u.beg;
    sN[tid] = (int)(u.end - u.beg);
    sRow[tid] = u.row;
  }
  __syncthreads();
  // the warm start; the padded columns of x are zero from here on
  for (int e = tid; e < kSubBatch * ld; e += 256) {
    const int j = e / ld, c = e - j * ld, row = sRow[j];
    xs[e] = (row >= 0 && c < k) ? (double)a.solved[(int64_t)row * k + c] : 0.0;
  }
  __syncthreads();
  for (int j = 0; j < kSubBatch; ++j) {
    const bool wide = sN[j] > kSubWideRow;
    if (wide || (j & 3) == wave) implicit_sub_scores<T>(a, xs + j * ld, sBeg[j], sN[j], wide ? wave : 0, wide ? 4 : 1, lane);
  }
  __syncthreads();

  const int mine = 4 * wave + grp;  // the batch row of this group in the solve
  bool bad = false;
  const int steps = a.sweeps * nb;
  int b = 0;
  for (int step = 0; step < steps; ++step) {
    const bool prev = step > 0;
    const int pb = b == 0 ? nb - 1 : b - 1, col = 16 * b + l16, pcol = 16 * pb + l16;
    // ---- sparse: H and the sparse part of g for every row of the batch
    for (int j = 0; j < kSubBatch; ++j) {
      const int n = sN[j];
      const bool wide = n > kSubWideRow;
      if (!wide && (j & 3) != wave) continue;  // (uniform in a wave; `wide` is uniform in the workgroup)
      acc_t H = {0.0, 0.0, 0.0, 0.0};
      double gsum = 0.0;
      implicit_sub_walk<T>(a, sBeg[j], n, wide ? wave : 0, wide ? 4 : 1, col, prev, pcol, prev ? dl[j * 16 + l16] : 0.0, step + 1 < steps, lane, H,
                           gsum);
      double *Hd = wide ? part + wave * kSubPart : Hs + j * 256, *gd = wide ? part + wave * kSubPart + 256 : gs + j * 16;
#pragma unroll
      for (int r = 0; r < 4; ++r) Hd[Tr::cd_row(lane, r) * 16 + l16] = H[r];
      if (grp == 0) gd[l16] = gsum;
      if (wide) {
        __syncthreads();
        Hs[j * 256 + tid] = ((part[tid] + part[kSubPart + tid]) + part[2 * kSubPart + tid]) + part[3 * kSubPart + tid];
        if (tid < 16)
          gs[j * 16 + tid] = ((part[256 + tid] + part[kSubPart + 256 + tid]) + part[2 * kSubPart + 256 + tid]) + part[3 * kSubPart + 256 + tid];
        __syncthreads();
      }
    }
    // ---- dense: this wave's share of (G X)_pi, element (coordinate i, batch row j) at part[wave][j][i]
    {
      acc_t acc = {0.0, 0.0, 0.0, 0.0};
      const double *gr = a.G + (size_t)(16 * b + l16) * kp + 4 * grp, *xb = xs + l16 * ld + 4 * grp;
      for (int c = wave; c < nb; c += 4) {
        const d4 ga = *reinterpret_cast<const d4 *>(gr + 16 * c), bv = *reinterpret_cast<const d4 *>(xb + 16 * c);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = Tr::mma(ga[t], bv[t], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) part[wave * kSubPart + l16 * 16 + Tr::cd_row(lane, r)] = acc[r];
    }
    __syncthreads();
    // ---- solve: lane c of the group holds column c of H (h[i] = H[i][c]) and element c of g
    {
      const bool colLive = col < k;
      const int at = mine * 16 + l16;
      double gg = ((part[at] + part[kSubPart + at]) + part[2 * kSubPart + at]) + part[3 * kSubPart + at];
      gg = fma(a.lambda, xs[mine * ld + col], gg) + gs[at];
      if (!colLive) gg = 0.0;
      double h[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const bool liveEl = colLive && 16 * b + i < k;
        const double v = Hs[mine * 256 + i * 16 + l16] + a.G[(size_t)(16 * b + i) * kp + col] + (i == l16 ? a.lambda : 0.0);
        h[i] = liveEl ? v : (i == l16 ? 1.0 : 0.0);
      }
      double dmine = 1.0;
      bool badNow = false;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double d = __shfl(h[j], j, 16);  // the pivot, the same in the group's 16 lanes
        if (!(d > 0.0)) badNow = true;
        if (l16 == j) dmine = d;
        const double lj = h[j] / d;            // L[c][j] for the lanes c > j
        const double zj = __shfl(gg, j, 16);
        if (l16 > j) gg = fma(-lj, zj, gg);
#pragma unroll
        for (int i = j + 1; i < 16; ++i) {
          const double li = __shfl(lj, i, 16);
          // lane j keeps column j of L from here on, the lanes behind it update their column of the trailing matrix
          h[i] = l16 == j ? li : (l16 > j ? fma(-li, h[j], h[i]) : h[i]);
        }
      }
      double dv = gg / dmine;
#pragma unroll
      for (int c = 15; c > 0; --c) {
        const double dc = __shfl(dv, c, 16);
        if (l16 < c) dv = fma(-h[c], dc, dv);
      }
      bad = bad || badNow;
      if (bad) dv = 0.0;  // a bad row stops moving; it is zeroed at the store
      xs[mine * ld + col] -= dv;
      dl[at] = dv;
    }
    __syncthreads();
    b = b + 1 == nb ? 0 : b + 1;
  }
  // one rounding to T; a bad row, or one that would store a value that is not finite, becomes zeros and is counted
  const int row = sRow[mine];
  for (int e = 0; e < nb; ++e) bad = bad || !isfinite((double)(T)xs[mine * ld + l16 + 16 * e]);
  const bool rowBad = ((__ballot(bad) >> (16 * grp)) & 0xffffull) != 0;
  if (row >= 0) {
    for (int e = 0; e < nb; ++e)
      if (l16 + 16 * e < k) a.solved[(int64_t)row * k + l16 + 16 * e] = rowBad ? (T)0 : (T)xs[mine * ld + l16 + 16 * e];
    if (rowBad && l16 == 0) atomicAdd(a.badRows, 1);
  }
}

// ------------------------------------------------------------------------------------------------ G = Y^T Y, k > 128
// rows of the fixed matrix per slice: a function of m alone (<= 128 slices: the partials of k = 512 stay within 256 MB)
__host__ __device__ constexpr int64_t implicit_wide_slice_rows(int64_t m) {
  const int64_t a = (m + 127) / 128, s = a > 2048 ? a : 2048;
  return (s + 15) & ~(int64_t)15;
}
constexpr int kWideLd = 80;  // doubles per staged row of 64 columns: 16 mod 32, as implicit_ld

// One workgroup per (pair of 64-column blocks bi <= bj: blockIdx.x, slice of fixed rows: blockIdx.y): the 64 x 64 block of the
// slice's Y^T Y as 16 tiles, wave w the four tiles of tile row w.  A panel = 16 consecutive rows of the two column blocks, staged
// as double in one of two LDS buffers while the previous one is multiplied; chains of kImplicitFlush panels joined by TwoSum as
// in implicit_gram_kernel.  Columns >= k are staged as zeros.  Output: partial[(slice, pair)][64][64].
template <typename T>
__global__ __launch_bounds__(256) void implicit_gram_wide_kernel(const T *__restrict__ Y, int64_t m, int k, int64_t sliceRows, double *__restrict__ partial) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  __shared__ double wlds[2][2][kImplicitPanel * kWideLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15;
  const int nb64 = (k + 63) >> 6;
  int bi, bj;
  implicit_tile_of((int)blockIdx.x, nb64, bi, bj);
  const int64_t r0 = (int64_t)blockIdx.y * sliceRows;
  const int64_t rows = (m - r0 < sliceRows ? m - r0 : sliceRows);
  const int64_t nPanels = (rows + kImplicitPanel - 1) / kImplicitPanel;
  const int pr = tid >> 4, pc = (tid & 15) * 4;  // this thread stages row pr, columns pc .. pc + 3 of both blocks
  acc_t acc[4], tot[4], low[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = tot[t] = low[t] = acc_t{0.0, 0.0, 0.0, 0.0};
  T g[8];
  auto load = [&](int64_t p) {
    const int64_t r = p * kImplicitPanel + pr;
    const bool live = r < rows;
    const T *src = Y + (live ? (r0 + r) * k : 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ca = 64 * bi + pc + e, cb = 64 * bj + pc + e;
      g[e] = (live && ca < k) ? src[ca] : (T)0;
      g[4 + e] = (live && cb < k) ? src[cb] : (T)0;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      wlds[buf][0][pr * kWideLd + pc + e] = (double)g[e];
      wlds[buf][1][pr * kWideLd + pc + e] = (double)g[4 + e];
    }
  };
  if (nPanels > 0) {
    load(0);
    stage(0);
  }
  __syncthreads();
  for (int64_t p = 0; p < nPanels; ++p) {
    const int buf = (int)(p & 1);
    if (p + 1 < nPanels) load(p + 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ro = (4 * s + (lane >> 4)) * kWideLd;
      const double av = wlds[buf][0][ro + 16 * wave + l16];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = Tr::mma(av, wlds[buf][1][ro + 16 * t + l16], acc[t]);
    }
    if (p + 1 < nPanels) stage(buf ^ 1);  // that buffer was last read in iteration p - 1, in front of its barrier
    if ((p & (kImplicitFlush - 1)) == kImplicitFlush - 1 || p + 1 == nPanels) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double s = tot[t][r], l = low[t][r];
          implicit_two_sum(s, l, acc[t][r]);
          tot[t][r] = s, low[t][r] = l;
        }
        acc[t] = acc_t{0.0, 0.0, 0.0, 0.0};
      }
    }
    __syncthreads();
  }
  double *out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4096;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(16 * wave + Tr::cd_row(lane, r)) * 64 + 16 * t + l16] = tot[t][r] + low[t][r];
}

// 16 workgroups per pair of column blocks: element by element, the slices' partials in slice order (TwoSum) -> G, full and
// symmetric, kp x kp (what lies beyond kp is dropped; columns k .. kp - 1 are exact zeros).  Also clears the bad-row count.
__global__ __launch_bounds__(256) void implicit_gram_wide_reduce_kernel(const double *__restrict__ partial, int nSlices, int k, double *__restrict__ G,
                                                                        int32_t *badRows) {
  const int nb64 = (k + 63) >> 6, nPairs = tile_count(nb64), kp = (k + 15) / 16 * 16;
  const int pair = blockIdx.x >> 4, e = ((blockIdx.x & 15) << 8) + threadIdx.x;
  double s = 0.0, low = 0.0;
  for (int q = 0; q < nSlices; ++q) implicit_two_sum(s, low, partial[((size_t)q * nPairs + pair) * 4096 + e]);
  s += low;
  int bi, bj;
  implicit_tile_of(pair, nb64, bi, bj);
  const int r = 64 * bi + (e >> 6), c = 64 * bj + (e & 63);
  if (r < kp && c < kp) {
    G[(size_t)r * kp + c] = s;
    if (bi != bj) G[(size_t)c * kp + r] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *badRows = 0;
}

}  // namespace ycnr
