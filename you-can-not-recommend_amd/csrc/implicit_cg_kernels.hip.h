// implicit_cg_kernels.hip.h -- the implicit-feedback half-step by a fixed number of conjugate-gradient steps per row, warm-started
// from the row as it stands (Takacs, Pilaszy, Tikk 2011, "Applications of the conjugate gradient method for implicit feedback
// collaborative filtering"), factorsCount <= 128.  The cheap standard trainer next to the exact solve of implicit_kernels.hip.h.
//
// For row u with observations S_u, raw values r_i, Y = the whole fixed matrix, G = Y^T Y, w_i = alpha r_i, c_i = 1 + w_i:
//     op(v) = G v + lambda v + sum_{i in S_u} w_i (y_i . v) y_i
//     x = the row as it stands;   r = sum_i c_i y_i - op(x);   p = r;   rho = r . r
//     cgSteps times, unless the row has stopped:
//         q = op(p);  d = p . q;  rho == 0 or !(d > 0): the row stops, x stays
//         a = rho / d;  x += a p;  r -= a q;  rho' = r . r;  p = r + (rho' / rho) p;  rho = rho'
//     store x, rounded once to T; a row that met a rho or d that is not finite (it would stop there and keep its warm start), or
//     whose stored value would not be finite, becomes zeros and is counted
// Per application of op a row of n observations costs 2 n k multiply-adds and its share of one k x k x 16 matrix product, where
// the exact solve costs an n k^2 Gramian and a k^3 / 3 factorisation.
//
// implicit_cg_kernel<T>: one workgroup of 256 threads (four waves) takes a batch of 16 whole rows through all cgSteps + 1
// applications of op.  x, r, p, q of the batch lie in LDS as double [16][ld]; everything is float64 for both T.  An application
// has three phases with a barrier behind each:
//   sparse   wave w takes batch rows 4 w .. 4 w + 3 one after another.  Ids and values are loaded 64 at a time, coalesced, and
//            handed out by lane; a group of 16 lanes works on one observation, four observations per wave at a time, four per
//            group in flight.  Lane j of a group holds elements j, j + 16, ... of y_i (gathered from the handle's matrix, leading
//            dimension k: 64 contiguous bytes per group and load for float32) and of the row's v: t = y_i . v by <= 8 fmas and
//            a four-step butterfly in the group, s = w_i t, part += s y_i.  The groups' parts are added by a two-step butterfly
//            (fixed order) and written to q.  The first application runs with s = w_i t - c_i, so that it leaves op(x) - b.
//   dense    Q += lambda V + G V for the whole batch on v_mfma_f64_16x16x4_f64: V = the batch's 16 vectors as a kp x 16 matrix,
//            the <= 8 row blocks of Q dealt over the waves (block w and w + 4: the B fragments are read once for both), the
//            accumulator started from the sparse part.  G comes from global memory (<= 128 KB, shared by every workgroup, L2
//            resident), read once per 16 rows.  The contraction index is dealt so that a lane's four values of a 16-column
//            stretch are contiguous: lane (i, g) supplies columns 16 c + 4 g + t of G's row i and of V in step t of stretch c --
//            one 32-byte load from G and one from LDS per four MFMAs.  Padding (k -> kp) contracts over zeros on both sides.
//   update   16 lanes per row, four rows per wave: all 16 rows at once; rho and the stopped flag stay in registers of the group.
// Every sum's order is fixed by the row alone (its observations in CSR order modulo 4, then the groups; the contraction order of
// the MFMAs): the same request gives the same bits, whichever rows share its batch.
#pragma once
#include "implicit_kernels.hip.h"

namespace ycnr {

constexpr int kImplicitCgBatch = 16;    // rows per workgroup = columns of the MFMA's B operand
constexpr int kImplicitCgMaxSteps = 64;
constexpr int kImplicitCgDepth = 4;     // observations per group whose gathers are in flight together

// x, r, p, q: double [16][ld].  ld = implicit_ld(kp) = 16 mod 32 doubles: batch rows j and j + 1 start 32 banks apart, so the
// 32-byte B fragments of two rows and the 128-byte row segments of two groups of the update never meet in a bank.
__host__ __device__ constexpr size_t implicit_cg_lds_bytes(int k) {
  const int kp = (k + 15) / 16 * 16;
  return (size_t)4 * kImplicitCgBatch * implicit_ld(kp) * sizeof(double);
}

template <typename T>
struct ImplicitCgArgs {
  const Unit *rows;      // the whole-row units of the plan, longest first (slab < 0)
  int64_t nRows;
  const int32_t *indx;   // validated at upload: every id is a row of `fixed`
  const T *vals;
  const T *fixed;        // [m x k]
  T *solved;             // [rows x k]: read for the warm start, written in place
  const double *G;       // [kp x kp], full and symmetric, padding exactly zero
  int32_t *badRows;
  double alpha, lambda;
  int32_t k, cgSteps;
};

// sum over the 16 lanes of a group, the same bits in every lane
__device__ __forceinline__ double implicit_cg_group_sum(double v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

// q[j] <- sum_i (w_i (y_i . v) - (first ? c_i : 0)) y_i for batch row j by the calling wave; skip: q[j] <- 0
template <typename T, int NB>
__device__ __forceinline__ void implicit_cg_sparse(const ImplicitCgArgs<T> &a, const double *v, double *q, int64_t beg, int n, bool skip,
                                                   bool first, int lane) {
  const int grp = lane >> 4, l16 = lane & 15, k = a.k;
  double vr[NB], part[NB];
#pragma unroll
  for (int e = 0; e < NB; ++e) {
    vr[e] = v[l16 + 16 * e];
    part[e] = 0.0;
  }
  for (int base = 0; base < (skip ? 0 : n); base += 64) {
    const int left = n - base;
    int32_t myId = 0;
    double myW = 0.0;
    if (lane < left) {
      myId = a.indx[beg + base + lane];
      myW = a.alpha * (double)a.vals[beg + base + lane];
    }
    const int steps = ((left < 64 ? left : 64) + 3) >> 2;  // of four observations, one per group
    for (int t0 = 0; t0 < steps; t0 += kImplicitCgDepth) {
      T y[kImplicitCgDepth][NB];
      double w[kImplicitCgDepth];
#pragma unroll
      for (int u = 0; u < kImplicitCgDepth; ++u) {
        const int o = 4 * (t0 + u) + grp;  // (<= 63: the depth divides 16)
        const bool live = o < left;        // a dead observation reads row 0 (id 0 of the lanes past the end) and counts as zeros
        const T *src = a.fixed + (int64_t)__shfl(myId, o, 64) * k;
        w[u] = __shfl(myW, o, 64);
#pragma unroll
        for (int e = 0; e < NB; ++e) {  // every lane loads (the padded columns an element of the row, then dropped): no divergent loads
          const int c = l16 + 16 * e;
          const T got = src[c < k ? c : k - 1];
          y[u][e] = (live && c < k) ? got : (T)0;
        }
      }
#pragma unroll
      for (int u = 0; u < kImplicitCgDepth; ++u) {
        double t = 0.0;
#pragma unroll
        for (int e = 0; e < NB; ++e) t = fma((double)y[u][e], vr[e], t);
        t = implicit_cg_group_sum(t);
        const double s = fma(w[u], t, first ? -(1.0 + w[u]) : 0.0);  // (a dead observation: y = 0, whatever s)
#pragma unroll
        for (int e = 0; e < NB; ++e) part[e] = fma(s, (double)y[u][e], part[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < NB; ++e) {
    double s = part[e];
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (grp == 0) q[l16 + 16 * e] = s;
  }
}

// q <- q + lambda v + G v for the batch: row blocks `wave` and `wave + 4` of the result
template <int NB>
__device__ __forceinline__ void implicit_cg_dense(const double *__restrict__ G, double lambda, const double *v, double *q, int wave, int lane) {
  using Tr = MfmaTraits<double>;
  using acc_t = typename Tr::acc_t;
  typedef double d4 __attribute__((ext_vector_type(4)));
  constexpr int kp = NB * 16, ld = implicit_ld(kp);
  if (wave >= NB) return;
  const int g = lane >> 4, l16 = lane & 15;
  const bool two = wave + 4 < NB;
  const int b0 = 16 * wave, b1 = two ? b0 + 64 : b0;
  acc_t acc0, acc1;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c0 = l16 * ld + b0 + Tr::cd_row(lane, r), c1 = l16 * ld + b1 + Tr::cd_row(lane, r);
    acc0[r] = fma(lambda, v[c0], q[c0]);
    acc1[r] = fma(lambda, v[c1], q[c1]);
  }
  const double *g0 = G + (size_t)(b0 + l16) * kp + 4 * g, *g1 = G + (size_t)(b1 + l16) * kp + 4 * g;
  const double *vb = v + l16 * ld + 4 * g;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const d4 ga = *reinterpret_cast<const d4 *>(g0 + 16 * c), gb = *reinterpret_cast<const d4 *>(g1 + 16 * c);
    const d4 bv = *reinterpret_cast<const d4 *>(vb + 16 * c);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc0 = Tr::mma(ga[t], bv[t], acc0);
      if (two) acc1 = Tr::mma(gb[t], bv[t], acc1);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    q[l16 * ld + b0 + Tr::cd_row(lane, r)] = acc0[r];
    if (two) q[l16 * ld + b1 + Tr::cd_row(lane, r)] = acc1[r];
  }
}

template <typename T, int NB>
__global__ __launch_bounds__(256) void implicit_cg_kernel(ImplicitCgArgs<T> a) {
  extern __shared__ __attribute__((aligned(32))) double icg_lds[];  // (32-byte B fragments)
  __shared__ int64_t sBeg[kImplicitCgBatch];
  __shared__ int sN[kImplicitCgBatch], sRow[kImplicitCgBatch], sStop[kImplicitCgBatch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 4, l16 = lane & 15;
  constexpr int kp = NB * 16, ld = implicit_ld(kp);  // NB = ceil(k / 16)
  const int k = a.k;
  double *xs = icg_lds, *rs = xs + kImplicitCgBatch * ld, *ps = rs + kImplicitCgBatch * ld, *qs = ps + kImplicitCgBatch * ld;
  if (tid < kImplicitCgBatch) {
    const int64_t i = (int64_t)blockIdx.x * kImplicitCgBatch + tid;
    const bool live = i < a.nRows;
    const Unit u = live ? a.rows[i] : Unit{0, 0, -1, -1};
    sBeg[tid] = u.beg;
    sN[tid] = (int)(u.end - u.beg);
    sRow[tid] = u.row;
    sStop[tid] = live ? 0 : 1;  // a batch's unused places: zero vectors that never move
  }
  __syncthreads();
  // the warm start; the padded columns of all four arrays are zero from here on (no phase writes a non-zero there)
  for (int e = tid; e < kImplicitCgBatch * ld; e += 256) {
    const int j = e / ld, c = e - j * ld, row = sRow[j];
    xs[e] = (row >= 0 && c < k) ? (double)a.solved[(int64_t)row * k + c] : 0.0;
    rs[e] = ps[e] = qs[e] = 0.0;
  }
  __syncthreads();

  const int mine = 4 * wave + grp;  // the batch row of this group in the update
  double *xm = xs + mine * ld, *rm = rs + mine * ld, *pm = ps + mine * ld, *qm = qs + mine * ld;
  double rho = 0.0;
  bool stopped = sStop[mine] != 0, poisoned = false;
  for (int it = 0; it <= a.cgSteps; ++it) {
    const bool first = it == 0;
    const double *v = first ? xs : ps;
#pragma unroll 1
    for (int jj = 0; jj < 4; ++jj) {
      const int j = 4 * wave + jj;
      implicit_cg_sparse<T, NB>(a, v + j * ld, qs + j * ld, sBeg[j], sN[j], sStop[j] != 0, first, lane);
    }
    __syncthreads();
    implicit_cg_dense<NB>(a.G, a.lambda, v, qs, wave, lane);
    __syncthreads();
    if (first) {  // q = op(x) - b
      double s = 0.0;
#pragma unroll
      for (int e = 0; e < NB; ++e) {
        const double rv = -qm[l16 + 16 * e];
        rm[l16 + 16 * e] = pm[l16 + 16 * e] = rv;
        s = fma(rv, rv, s);
      }
      rho = implicit_cg_group_sum(s);
    } else {
      double pv[NB], qv[NB], d = 0.0;
#pragma unroll
      for (int e = 0; e < NB; ++e) {
        pv[e] = pm[l16 + 16 * e];
        qv[e] = qm[l16 + 16 * e];
        d = fma(pv[e], qv[e], d);
      }
      d = implicit_cg_group_sum(d);
      // a rho or d that is not finite (NaN / Inf in the row's values, its warm start or G) would stop the row by the rule below
      // and leave the warm start standing as if it were a result: the row is bad instead
      if (!stopped && !(isfinite(rho) && isfinite(d))) poisoned = true;
      const bool go = !stopped && !poisoned && rho != 0.0 && d > 0.0;  // (the same in the 16 lanes of a group)
      const double al = rho / d;
      double rv[NB], s = 0.0;
#pragma unroll
      for (int e = 0; e < NB; ++e) {
        rv[e] = go ? fma(-al, qv[e], rm[l16 + 16 * e]) : 0.0;
        s = fma(rv[e], rv[e], s);
      }
      const double rho2 = implicit_cg_group_sum(s), beta = rho2 / rho;
      if (go) {
#pragma unroll
        for (int e = 0; e < NB; ++e) {
          xm[l16 + 16 * e] = fma(al, pv[e], xm[l16 + 16 * e]);
          rm[l16 + 16 * e] = rv[e];
          pm[l16 + 16 * e] = fma(beta, pv[e], rv[e]);
        }
        rho = rho2;
      } else if (!stopped) {
        stopped = true;
        if (l16 == 0) sStop[mine] = 1;
      }
    }
    __syncthreads();
  }
  // one rounding to T; a row that met a rho or d that is not finite, or would store a value that is not, becomes zeros and is counted
  const int row = sRow[mine];
  T out[NB];
  bool bad = poisoned;
#pragma unroll
  for (int e = 0; e < NB; ++e) {
    out[e] = (T)xm[l16 + 16 * e];
    bad = bad || !isfinite((double)out[e]);
  }
  const bool rowBad = ((__ballot(bad) >> (16 * grp)) & 0xffffull) != 0;
  if (row >= 0) {
#pragma unroll
    for (int e = 0; e < NB; ++e)
      if (l16 + 16 * e < k) a.solved[(int64_t)row * k + l16 + 16 * e] = rowBad ? (T)0 : out[e];
    if (rowBad && l16 == 0) atomicAdd(a.badRows, 1);
  }
}

}  // namespace ycnr
