// kernel_choice.h -- which instantiation of the four kernels of a half-step at k <= 128 runs (chunk Gramian, fused row kernel,
// reduce, band reduce).  Host-only and a function of its arguments alone, like schedule.h: no HIP, no environment.
// ycnr_als.hip maps a choice to function pointers (row_kernels) and launches them (launch_rows, step_banded_t).
#pragma once

#ifndef YCNR_EDGE4_SOLVE  // (als_kernels.hip.h: 0 builds the solvers without the edge-first elimination)
#define YCNR_EDGE4_SOLVE 1
#endif

namespace ycnr {

// Gramian of the chunk kernel and of the row kernel.  kGramMfma: exact float32 (float64) MFMA chains, the only form of float64.
// kGramX6: bf16x6 (exact 3-way split, six products), gathered through registers -- chunks only.  kGramX6D: the same with the
// gather staged through LDS by LDS-DMA, k % 4 == 0 (two waves per SIMD up to k = 112, one from 116 to 128).  kGramPlanes: bf16x6 on the pre-split planes of the fixed matrix -- rows only.
enum GramForm { kGramMfma, kGramX6, kGramX6D, kGramPlanes };

// Every field is a template argument of one kernel; a field that its kernel's form does not have stays false.
struct KernelChoice {
  int nb;          // blocks of 16 columns: ceil(k / 16), 1 ... 8
  bool ldsSolver;  // YCNR_FLAG_LDS_SOLVER (float64 without it: its own register solver)
  // chunk kernel: als_gram_slab_kernel<T, nb, chunkEdge> | als_gram_slab_x6_kernel<nb> | als_gram_slab_x6d_kernel<nb, chunkPadRhs, chunkPk3>
  GramForm chunk;
  bool chunkEdge, chunkPadRhs, chunkPk3;
  // row kernel: als_gram_solve_kernel<T, nb, ldsSolver, rowEdge, rowE4> | als_gram_solve_x6d_kernel<nb, rowPadRhs, ldsSolver, rowE4, rowPk3>
  // | als_gram_solve_x6p_kernel<nb, rowPack, rowE4>
  GramForm row;
  bool rowEdge, rowE4, rowPadRhs, rowPk3, rowPack;
  // als_reduce_solve_kernel<T, nb, ldsSolver, reduceEdge, reduceE4, reduceFew>, als_band_reduce_solve_kernel<T, nb, ldsSolver, reduceEdge, bandE4>
  bool reduceEdge, reduceE4, reduceFew, bandE4;
  bool rowLdsImage;  // dynamic LDS of the row kernel: the solver's image, or none (the planes kernel solves in the slots of its Gramian)
};

// f64: the dtype.  edge: the last 4 columns of a k = 16 m + 4 Gramian on the VALU (use_valu_edge).  x6: split chunks on the bf16
// pipe, the fixed matrix within a 32-bit buffer offset (use_slab_x6).  hasPlanes: the half-step split the fixed matrix into
// planes.  fewSlabs: no split row of the piece has more than kFewSlabs slabs.  noX6d, noFusedX6d, noPk3: the A/B toggles
// YCNR_NO_X6D, YCNR_NO_FUSED_X6D, YCNR_NO_PK3.
inline KernelChoice choose_kernels(bool f64, int k, bool ldsSolver, bool edge, bool x6, bool hasPlanes, bool fewSlabs, bool noX6d,
                                   bool noFusedX6d, bool noPk3) {
  const int nb = (k + 15) / 16;
  KernelChoice c = {};
  c.nb = nb, c.ldsSolver = ldsSolver, c.rowLdsImage = true;
  if (f64) return c;  // float64: the MFMA kernels, nothing else
  edge = edge && nb >= 2;  // (the VALU-edge Gramian exists from two blocks on)
  const bool first4 = k == 16 * (nb - 1) + 4;  // four columns in the last block
  const bool padRhs = k < 16 * nb;             // x6d: the right-hand side rides in a padding column of the Gramian
  const bool e4 = YCNR_EDGE4_SOLVE && nb >= 2 && !ldsSolver && first4;  // the solve eliminates the four edge columns first
  const bool x6d = x6 && k % 4 == 0 && !noX6d;
  const bool pk3 = padRhs && first4 && !noPk3;  // the last block's planes packed into one operand (GramX6D's PK3)
  // Split chunks that go through a bf16x6 kernel leave plain slabs, so the reduce reads plain slabs whatever the row kernel uses:
  // the VALU-edge layout of chunk and reduce holds only without x6.
  c.chunk = x6d ? kGramX6D : x6 ? kGramX6 : kGramMfma;
  c.chunkEdge = c.reduceEdge = edge && !x6;
  c.chunkPadRhs = x6d && padRhs;
  c.chunkPk3 = x6d && pk3;
  c.reduceE4 = c.bandE4 = e4;
  c.reduceFew = fewSlabs && !ldsSolver;
  // the row kernel: planes before x6d before MFMA.  There is no x6d row kernel for eight blocks with the LDS solver (it keeps
  // the float32-MFMA kernel), and the planes kernel has the register solver only and does not look at noX6d.
  if (x6 && hasPlanes && !ldsSolver && k % 4 == 0 && padRhs) {
    c.row = kGramPlanes;
    c.rowPack = c.rowE4 = nb >= 2 && first4;
    c.rowLdsImage = false;
  } else if (x6d && !noFusedX6d && !(ldsSolver && nb == 8)) {
    c.row = kGramX6D;
    c.rowPadRhs = padRhs;
    c.rowE4 = e4;  // (four columns in the last block: padRhs holds)
    c.rowPk3 = pk3;
  } else {
    c.row = kGramMfma;
    c.rowEdge = edge;
    c.rowE4 = e4;
  }
  return c;
}

}  // namespace ycnr
