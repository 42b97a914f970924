// implicit_kernels.hip.h -- the implicit-feedback ALS half-step of Hu, Koren, Volinsky (2008, "Collaborative Filtering for
// Implicit Feedback Datasets"; the method lib/emf/Emf.js of the reference points at and does not have), factorsCount <= 128.
//
// For the side being solved, with Y = the whole fixed matrix (m rows) and r_ui the raw values of row u's observations S_u:
//     G   = Y^T Y                                        once per half-step, shared by every row
//     A_u = G + alpha sum_{i in S_u} r_ui y_i y_i^T + lambda I
//     b_u =     sum_{i in S_u} (1 + alpha r_ui) y_i      (confidence c = 1 + alpha r, preference 1)
//     x_u = A_u^-1 b_u;   S_u empty: x_u = 0 exactly.
// lambda is used plain (the paper's), not times n as the explicit half-step does.
//
// Five kernels, launched in this order on the handle's stream; every one reads and writes the handle's matrices with leading
// dimension k (no padded copies, no bf16 planes):
//   implicit_gram_kernel<T, VEC>    partial sums of G in float64 on v_mfma_f64_16x16x4_f64, one workgroup per slice of fixed rows
//                                   (an MFMA chain per 64 rows, the chains joined by compensated additions: DESIGN.md 14)
//   implicit_gram_reduce_kernel     the partials added in slice order -> G as a full symmetric kp x kp double image
//   implicit_unit_kernel<T>         one workgroup per work unit (schedule.h): weighted Gramian on MfmaTraits<T>, b on the VALU in
//                                   double; a unit that covers its row goes on to the solve, a chunk writes a slab
//   implicit_reduce_solve_kernel<T> one workgroup per split row: its slabs added in slab order in double, then the same solve
//   implicit_zero_rows_kernel<T>    rows of the shard without observations become zeros
// The solve (implicit_solve): G and lambda are added to the row's sums once, in double; the image lies in LDS as packed upper
// 16 x 16 tiles; L D L^T by the whole workgroup in double with b as one more column, back substitution by wave 0, one rounding
// to T at the store.  Every sum's order is fixed by (m, the row, the chunk length): no result depends on the grid.
#pragma once
#include "als_kernels.hip.h"

namespace ycnr {

constexpr int kImplicitMaxK = 128;
constexpr int kImplicitPanel = 16;    // rows (ratings) per LDS panel = four MFMA contraction steps
constexpr int kImplicitChunk = 4096;  // ratings per work unit when options.chunkRatings leaves it to the library

// rows of the fixed matrix per slice of implicit_gram_kernel: a function of m alone (<= 1024 slices)
__host__ __device__ constexpr int64_t implicit_slice_rows(int64_t m) {
  const int64_t a = (m + 1023) / 1024, s = a > 2048 ? a : 2048;
  return (s + 15) & ~(int64_t)15;
}
// leading dimension (elements) of a panel row: 16 mod 32, so that the four rows an MFMA operand reads fall on different banks
__host__ __device__ constexpr int implicit_ld(int kp) { return kp % 32 == 0 ? kp + 16 : kp; }
// doubles of one slab, and of the solve's image with its right-hand side: packed upper tiles, then b
__host__ __device__ constexpr int64_t implicit_slab_elems(int k) {
  const int nb = (k + 15) / 16;
  return (int64_t)tile_count(nb) * 256 + nb * 16;
}
__host__ __device__ constexpr size_t implicit_gram_lds_bytes(int k) {
  const int kp = (k + 15) / 16 * 16;
  return (size_t)2 * kImplicitPanel * implicit_ld(kp) * sizeof(double);
}
// [image | two panels, each plain and scaled] (aliased), b, 1 / d, two panels of weights 1 + alpha r
__host__ __device__ constexpr size_t implicit_unit_lds_bytes(int k, size_t tsz) {
  const int nb = (k + 15) / 16, kp = nb * 16;
  const size_t img = (size_t)tile_count(nb) * 256 * sizeof(double), pan = (size_t)4 * kImplicitPanel * implicit_ld(kp) * tsz;
  return (img > pan ? img : pan) + (2 * (size_t)kp + 2 * kImplicitPanel) * sizeof(double);
}
__host__ __device__ constexpr size_t implicit_reduce_lds_bytes(int k) {
  const int nb = (k + 15) / 16, kp = nb * 16;
  return ((size_t)tile_count(nb) * 256 + 2 * (size_t)kp) * sizeof(double);
}

// tile number ti (row-major over the upper triangle of nb x nb tiles) -> (bi, bj)
__device__ __forceinline__ void implicit_tile_of(int ti, int nb, int &bi, int &bj) {
  int rem = ti;
  bi = 0;
  while (rem >= nb - bi) {
    rem -= nb - bi;
    ++bi;
  }
  bj = bi + rem;
}

// s + low <- s + low + v with the rounding error of the addition kept in `low` (Knuth's TwoSum; the library is built without
// fast-math, so the compiler keeps the order)
__device__ __forceinline__ void implicit_two_sum(double &s, double &low, double v) {
  const double t = s + v, bb = t - s;
  low += (s - (t - bb)) + (v - bb);
  s = t;
}
constexpr int kImplicitFlush = 4;  // panels (of 16 fixed rows) per MFMA chain of implicit_gram_kernel

// ------------------------------------------------------------------------------------------------ G = Y^T Y
// One workgroup of 256 threads per slice of `sliceRows` fixed rows.  A panel is 16 consecutive rows = 16 k CONTIGUOUS elements of
// the matrix: thread t loads elements (or 16-byte vectors, VEC) t, t + 256, ... -- coalesced, no gather -- and stages them as
// double [16][ld] in one of two LDS buffers; the loads of panel p + 1 are in flight while panel p is multiplied.  The
// nb (nb + 1) / 2 <= 36 upper tiles are dealt round-robin over the four waves (<= 9 accumulator tiles each).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void implicit_gram_kernel(const T *__restrict__ Y, int64_t m, int k, int64_t sliceRows, double *__restrict__ partial) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  constexpr int V = VEC ? (int)(16 / sizeof(T)) : 1;        // elements per load
  constexpr int NL = 16 * kImplicitMaxK / (256 * V);        // loads per thread and panel at k = 128
  typedef T vec_t __attribute__((ext_vector_type(V)));
  extern __shared__ double igram_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = (k + 15) >> 4, kp = nb << 4, ld = implicit_ld(kp), nt = tile_count(nb);
  const int64_t r0 = (int64_t)blockIdx.x * sliceRows;
  const int64_t rows = (m - r0 < sliceRows ? m - r0 : sliceRows);
  const int64_t nPanels = (rows + kImplicitPanel - 1) / kImplicitPanel;
  const T *src = Y + r0 * k;
  const int panelElems = kImplicitPanel * k;
  // the padded columns of both buffers are written here once and never again
  for (int e = tid; e < 2 * kImplicitPanel * (kp - k); e += 256) igram_lds[(size_t)(e / (kp - k)) * ld + k + e % (kp - k)] = 0.0;

  int offA[9], offB[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    int bi = 0, bj = 0;
    if (wave + 4 * t < nt) implicit_tile_of(wave + 4 * t, nb, bi, bj);
    offA[t] = 16 * bi + (lane & 15);
    offB[t] = 16 * bj + (lane & 15);
  }
  acc_t acc[9], tot[9], low[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = tot[t] = low[t] = acc_t{0.0, 0.0, 0.0, 0.0};

  vec_t g[NL];
  auto load = [&](int64_t p) {
    const int64_t left = (rows - p * kImplicitPanel) * k;  // elements of the slice from this panel on
    const T *ps = src + p * panelElems;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int e = (tid + 256 * j) * V;
      vec_t v;
#pragma unroll
      for (int c = 0; c < V; ++c) v[c] = (T)0;
      if (e < panelElems && e < left) v = *reinterpret_cast<const vec_t *>(ps + e);  // (VEC: k % V == 0, a vector is live or dead as a whole)
      g[j] = v;
    }
  };
  auto stage = [&](int buf) {
    double *dst = igram_lds + (size_t)buf * kImplicitPanel * ld;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int e = (tid + 256 * j) * V;
      if (e < panelElems) {
        const int r = e / k, c = e - r * k;  // (VEC: the V elements lie in one row)
#pragma unroll
        for (int q = 0; q < V; ++q) dst[(size_t)r * ld + c + q] = (double)g[j][q];
      }
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
    const double *cur = igram_lds + (size_t)buf * kImplicitPanel * ld;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const double *r4 = cur + (size_t)(4 * s + (lane >> 4)) * ld;
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if (wave + 4 * t < nt) acc[t] = Tr::mma(r4[offA[t]], r4[offB[t]], acc[t]);
    }
    if (p + 1 < nPanels) stage(buf ^ 1);  // that buffer was last read in iteration p - 1, in front of its barrier
    // every kImplicitFlush panels the MFMA chain ends: its sum joins the slice's total by an error-free addition whose rounding
    // error is kept in `low`, so the error of a slice's sum is that of chains of 64 rows, not of one chain over the slice
    if ((p & (kImplicitFlush - 1)) == kImplicitFlush - 1 || p + 1 == nPanels) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if (wave + 4 * t < nt) {
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
  double *out = partial + (size_t)blockIdx.x * nt * 256;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int ti = wave + 4 * t;
    if (ti < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)ti * 256 + Tr::cd_row(lane, r) * 16 + (lane & 15)] = tot[t][r] + low[t][r];
    }
  }
}

// One workgroup per upper tile: element by element, the slices' partials in slice order (compensated like the slices' own sums).  G: full symmetric kp x kp (the padded
// rows and columns are sums of products with the panels' zero columns: exactly zero).  Also clears the half-step's bad-row count.
__global__ __launch_bounds__(256) void implicit_gram_reduce_kernel(const double *__restrict__ partial, int nSlices, int k, double *__restrict__ G,
                                                                   int32_t *badRows) {
  const int nb = (k + 15) >> 4, kp = nb << 4, nt = tile_count(nb), ti = blockIdx.x, e = threadIdx.x;
  double s = 0.0, low = 0.0;
  for (int q = 0; q < nSlices; ++q) implicit_two_sum(s, low, partial[((size_t)q * nt + ti) * 256 + e]);
  s += low;
  int bi, bj;
  implicit_tile_of(ti, nb, bi, bj);
  const int r = 16 * bi + (e >> 4), c = 16 * bj + (e & 15);
  G[(size_t)r * kp + c] = s;
  if (bi != bj) G[(size_t)c * kp + r] = s;
  if (ti == 0 && e == 0) *badRows = 0;
}

// ------------------------------------------------------------------------------------------------ the solve, shared
// img: packed upper tiles of A (16 x 16 row-major each), rhs: b, both in LDS and complete (a barrier lies behind their last
// write).  A = L D L^T row by row -- R[j][c] = A[j][c] - sum_{i<j} R[i][j] R[i][c] / d_i, d_j = R[j][j] -- two lanes per column
// (terms i even / odd), the right-hand side as column k; only the k real columns.  Then x by wave 0.  A pivot with !(p > 0)
// raises *bad, which is read behind the last barrier: the row becomes zeros and is counted.
template <typename T>
__device__ __forceinline__ void implicit_solve(double *img, double *rhs, double *invd, int *bad, int k, int nb, T *out, int32_t *badRows) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto at = [&](int i, int c) -> double & { return img[(size_t)tile_index(i >> 4, c >> 4, nb) * 256 + (i & 15) * 16 + (c & 15)]; };
  if (tid == 0) {
    const double d = img[0];
    if (!(d > 0.0)) *bad = 1;
    invd[0] = 1.0 / d;
  }
  __syncthreads();
  const int pair = tid >> 1, half = tid & 1;
  for (int j = 1; j < k; ++j) {
    const int c = j + pair;  // c == k: the right-hand side
    const bool live = c <= k;
    double s = 0.0;
    if (live) {
      // tile row by tile row; a lane's (up to) eight terms of a tile row are loaded together, then added in ascending i
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
          if (!(v > 0.0)) *bad = 1;
          invd[j] = 1.0 / v;
        }
      } else {
        rhs[j] -= s;
      }
    }
    __syncthreads();
  }
  if (wave == 0) {
    // x_i = (z_i - sum_{c>i} R[i][c] x_c) / d_i, column by column; lane l keeps z_l and z_{l+64}, then x_l and x_{l+64}
    double x0 = lane < k ? rhs[lane] : 0.0, x1 = lane + 64 < k ? rhs[lane + 64] : 0.0;
    for (int c = k - 1; c >= 0; --c) {
      const double xc = __shfl(c < 64 ? x0 : x1, c & 63, 64) * invd[c];
      if (lane < c) x0 = fma(-at(lane, c), xc, x0);
      if (lane + 64 < c) x1 = fma(-at(lane + 64, c), xc, x1);
      if (lane == c) x0 = xc;
      if (lane + 64 == c) x1 = xc;
    }
    const bool failed = *bad != 0;
    if (lane < k) out[lane] = failed ? (T)0 : (T)x0;
    if (lane + 64 < k) out[lane + 64] = failed ? (T)0 : (T)x1;
    if (lane == 0 && failed) atomicAdd(badRows, 1);
  }
}

// ------------------------------------------------------------------------------------------------ one work unit
template <typename T>
struct ImplicitArgs {
  const Unit *units;
  const SplitRow *split;
  const int32_t *indx;   // validated at upload: every id is a row of `fixed`
  const T *vals;
  const T *fixed;        // [m x k]
  T *solved;             // [rows x k], written in place
  const double *G;       // [kp x kp]
  double *slabs;         // implicit_slab_elems(k) doubles each: the implicit path's own
  int32_t *badRows;
  double alpha, lambda;
  int32_t k;
};

// Ratings go through LDS in panels of 16, two buffers; thread (pr = tid / 16, pc = tid % 16) gathers columns pc, pc + 16, ... of
// the panel's rating pr.  Every staged row is kept twice, plain and scaled by w = alpha r: the scaling happens AS IT IS STAGED --
// nb multiplies per thread and panel, where scaling the A-fragment on its way out of LDS would cost one per MFMA (up to 36).
// Gramian: A-operand = the scaled copy, B-operand = the plain one, so tile (bi, bj) holds sum_q w_q y_q[16 bi + i] y_q[16 bj + j],
// contraction in rating order.  b: threads 0 .. kp - 1, one double fma chain per column with weight 1 + alpha r.
template <typename T>
__global__ __launch_bounds__(256) void implicit_unit_kernel(ImplicitArgs<T> a) {
  using Tr = MfmaTraits<T>;
  using acc_t = typename Tr::acc_t;
  extern __shared__ double iunit_lds[];
  __shared__ int bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Unit u = a.units[blockIdx.x];
  const int k = a.k, nb = (k + 15) >> 4, kp = nb << 4, ld = implicit_ld(kp), nt = tile_count(nb);
  const int64_t q0 = u.beg, n = u.end - u.beg;
  const size_t imgBytes = (size_t)nt * 256 * sizeof(double), panBytes = (size_t)4 * kImplicitPanel * ld * sizeof(T);
  double *img = iunit_lds;
  T *pan = reinterpret_cast<T *>(iunit_lds);  // buffer b: plain rows at pan + 2 b P, scaled rows at pan + (2 b + 1) P, P = 16 ld
  double *rhs = iunit_lds + (imgBytes > panBytes ? imgBytes : panBytes) / sizeof(double);
  double *invd = rhs + kp;
  double *cpan = invd + kp;  // 2 x 16 weights 1 + alpha r
  const size_t P = (size_t)kImplicitPanel * ld;
  if (tid == 0) bad = 0;

  int offA[9], offB[9], tbi[9], tbj[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    tbi[t] = tbj[t] = 0;
    if (wave + 4 * t < nt) implicit_tile_of(wave + 4 * t, nb, tbi[t], tbj[t]);
    offA[t] = 16 * tbi[t] + (lane & 15);
    offB[t] = 16 * tbj[t] + (lane & 15);
  }
  acc_t acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = acc_t{(T)0, (T)0, (T)0, (T)0};
  double bsum = 0.0;

  const int pr = tid >> 4, pc = tid & 15;
  const int64_t nPanels = (n + kImplicitPanel - 1) / kImplicitPanel;
  T g[8];
  T gr = (T)0;
  auto gather = [&](int64_t p) {
    const int64_t q = p * kImplicitPanel + pr;
    const bool live = q < n;
    const T *src = a.fixed + (live ? (int64_t)a.indx[q0 + q] * k : 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = pc + 16 * j;
      g[j] = (live && c < k) ? src[c] : (T)0;
    }
    gr = live ? a.vals[q0 + q] : (T)0;
  };
  auto stage = [&](int buf) {
    T *plain = pan + (size_t)(2 * buf) * P + (size_t)pr * ld, *scaled = plain + P;
    const T w = (T)(a.alpha * (double)gr);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nb) {
        plain[pc + 16 * j] = g[j];
        scaled[pc + 16 * j] = w * g[j];
      }
    if (pc == 0) cpan[buf * kImplicitPanel + pr] = fma(a.alpha, (double)gr, 1.0);
  };
  gather(0);
  stage(0);
  __syncthreads();
  for (int64_t p = 0; p < nPanels; ++p) {
    const int buf = (int)(p & 1);
    if (p + 1 < nPanels) gather(p + 1);  // in flight during the products below
    const T *cur = pan + (size_t)(2 * buf) * P;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const T *r4 = cur + (size_t)(4 * s + (lane >> 4)) * ld;
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if (wave + 4 * t < nt) acc[t] = Tr::mma(r4[P + offA[t]], r4[offB[t]], acc[t]);
    }
    if (tid < kp) {
      const double *cw = cpan + buf * kImplicitPanel;
#pragma unroll
      for (int q = 0; q < kImplicitPanel; ++q) bsum = fma((double)cur[(size_t)q * ld + tid], cw[q], bsum);
    }
    if (p + 1 < nPanels) stage(buf ^ 1);  // last read in iteration p - 1, in front of that iteration's barrier
    __syncthreads();
  }
  // (every read of the panels lies in front of the loop's last barrier)
  if (u.slab >= 0) {  // a chunk of a split row: the whole workgroup writes its sums and is done
    double *slab = a.slabs + (size_t)u.slab * implicit_slab_elems(k);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ti = wave + 4 * t;
      if (ti < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) slab[(size_t)ti * 256 + Tr::cd_row(lane, r) * 16 + (lane & 15)] = (double)acc[t][r];
      }
    }
    if (tid < kp) slab[(size_t)nt * 256 + tid] = bsum;
    return;
  }
  const int kpG = kp;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int ti = wave + 4 * t;
    if (ti < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tr = Tr::cd_row(lane, r), tc = lane & 15, gi = 16 * tbi[t] + tr, gj = 16 * tbj[t] + tc;
        img[(size_t)ti * 256 + tr * 16 + tc] = (double)acc[t][r] + a.G[(size_t)gi * kpG + gj] + ((gi == gj && gi < k) ? a.lambda : 0.0);
      }
    }
  }
  if (tid < kp) rhs[tid] = bsum;
  __syncthreads();
  implicit_solve<T>(img, rhs, invd, &bad, k, nb, a.solved + (int64_t)u.row * k, a.badRows);
}

// One workgroup per split row: element e of the image (tiles, then b) = the row's slabs in slab order, in double, + G + lambda.
template <typename T>
__global__ __launch_bounds__(256) void implicit_reduce_solve_kernel(ImplicitArgs<T> a) {
  extern __shared__ double ired_lds[];
  __shared__ int bad;
  const int tid = threadIdx.x;
  const SplitRow sr = a.split[blockIdx.x];
  const int k = a.k, nb = (k + 15) >> 4, kp = nb << 4, nt = tile_count(nb);
  const int64_t se = implicit_slab_elems(k);  // = nt * 256 + kp: the right-hand side follows the image in LDS as in a slab
  double *img = ired_lds, *rhs = img + (size_t)nt * 256, *invd = rhs + kp;
  if (tid == 0) bad = 0;
  const double *s0 = a.slabs + (size_t)sr.slab0 * se;
  for (int e = tid; e < (int)se; e += 256) {
    double s = 0.0;
    for (int q = 0; q < sr.nslabs; ++q) s += s0[(size_t)q * se + e];
    if (e < nt * 256) {
      int bi, bj;
      implicit_tile_of(e >> 8, nb, bi, bj);
      const int gi = 16 * bi + ((e >> 4) & 15), gj = 16 * bj + (e & 15);
      s += a.G[(size_t)gi * kp + gj] + ((gi == gj && gi < k) ? a.lambda : 0.0);
    }
    img[e] = s;
  }
  __syncthreads();
  implicit_solve<T>(img, rhs, invd, &bad, k, nb, a.solved + (int64_t)sr.row * k, a.badRows);
}

// rows of the shard without observations: x = 0 is their exact solution
template <typename T>
__global__ __launch_bounds__(256) void implicit_zero_rows_kernel(const int32_t *rows, int64_t nRows, int k, T *solved) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < nRows * k) solved[(int64_t)rows[q / k] * k + q % k] = (T)0;
}

}  // namespace ycnr
