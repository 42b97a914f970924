// implicit_wide_plan.h -- how a shard is cut for ycnr_als_step_implicit_wide: the rows foldin_implicit_wide_kernel solves in
// dual form (its two launch classes), the rows without observations, and the PRIMAL rows -- every other row -- with their chunk
// units and the batches whose slabs fit the arena; and the sizes the kernels of implicit_wide_kernels.hip.h share with the host.
// Host-only and a function of its arguments alone, like foldin_wide_plan.h: no HIP, no environment, no device call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "foldin_wide_plan.h"
#include "schedule.h"

namespace ycnr {

constexpr int kImplicitWideMaxK = kFoldWideMaxK;  // 512: what the factorisation of G + lambda I and the dual row kernel serve
constexpr int kWideGroupTiles = 8;                // 16-column tiles per column group of the Gramian kernel: a square is 8 x 8 tiles
constexpr int kWideGramLd = 16 * kWideGroupTiles + 16;  // elements per staged observation: 16 mod 32, as implicit_ld
constexpr int kWideSolveThreads = 512;            // eight waves factor one row image
// The arena of slabs: a constant, whatever the shard.  At k = 512 a slab is 1.09 MB, so a batch is about 350 slabs: more row
// images than the chip has CUs, and what the solve of a batch rereads is of the size of the last-level cache.
constexpr int64_t kImplicitWideArenaBytes = (int64_t)384 << 20;

YCNR_HD constexpr int wide_groups(int k) { return ((k + 15) / 16 + kWideGroupTiles - 1) / kWideGroupTiles; }
YCNR_HD constexpr int wide_squares(int k) { return tile_count(wide_groups(k)); }
// doubles of a slab, and of a row's image with its right-hand side: the packed upper 16 x 16 tiles, then b
YCNR_HD constexpr int64_t wide_slab_elems(int k) { return (int64_t)tile_count((k + 15) / 16) * 256 + (k + 15) / 16 * 16; }
// [2 x 16 weights 1 + alpha r | two buffers, each 16 scaled and 16 plain observations of kWideGramLd elements]
YCNR_HD constexpr size_t wide_gram_lds_bytes(size_t tsz) { return 32 * sizeof(double) + (size_t)4 * 16 * kWideGramLd * tsz; }
// doubles per row of the solve's 16-row panel: the kp columns, then the tile of the right-hand side; 16 mod 32
YCNR_HD constexpr int wide_solve_pld(int kp) { return (kp + 16) % 32 == 0 ? kp + 32 : kp + 16; }
// [panel | R_JJ | R_JJ^-1 | z]
YCNR_HD constexpr size_t wide_solve_lds_bytes(int k) {
  const int kp = (k + 15) / 16 * 16;
  return ((size_t)16 * wide_solve_pld(kp) + 512 + kp) * sizeof(double);
}
YCNR_HD constexpr int64_t wide_arena_slabs(int k, int64_t arenaBytes) {
  const int64_t n = arenaBytes / (wide_slab_elems(k) * (int64_t)sizeof(double));
  return n < 1 ? 1 : n;
}

// primal rows [row0, row0 + nRows) of the list with their units [unit0, unit0 + nUnits): slabs 0 .. nUnits - 1 of the arena
struct ImplicitWideBatch {
  int64_t unit0, nUnits, row0, nRows;
};
// Rows are LOCAL (0 = the shard's first).  The dual lists and `empty` are in row order; so are the primal rows, and a row's
// units follow each other in chunk order.  A unit's slab and a row's slab0 count from the start of the batch's arena.
struct ImplicitWideCut {
  std::vector<int32_t> dualShort, dualLong, empty;
  std::vector<Unit> units;
  std::vector<SplitRow> rows;
  std::vector<ImplicitWideBatch> batches;
};

// rowPtr: nRows + 1 offsets, any base; nonNegative[r] != 0: every value of row r is >= 0 (read only for rows of 1 .. 128
// observations).  A row's chunks are those build_schedule gives it with `chunk`, so they depend on the row alone; a batch takes
// rows while their slabs fit arenaSlabs (at least one row).
inline void implicit_wide_cut(const int64_t *rowPtr, int64_t nRows, const uint8_t *nonNegative, int chunk, int64_t arenaSlabs,
                              ImplicitWideCut &cut) {
  cut = ImplicitWideCut{};
  std::vector<Unit> units;
  std::vector<SplitRow> split;
  ImplicitWideBatch cur{0, 0, 0, 0};
  for (int64_t r = 0; r < nRows; ++r) {
    const int64_t n = rowPtr[r + 1] - rowPtr[r];
    if (n <= 0) {
      cut.empty.push_back((int32_t)r);
      continue;
    }
    if (fold_wide_row_is_served(n, n <= kFoldWideMaxObs && nonNegative[r] != 0)) {
      (n <= kFoldWideShortObs ? cut.dualShort : cut.dualLong).push_back((int32_t)r);
      continue;
    }
    const int64_t two[2] = {rowPtr[r], rowPtr[r + 1]}, at = rowPtr[r] - rowPtr[0];
    int64_t nSlabs = 0, solved = 0;
    build_schedule(two, r, 1, chunk, units, split, nSlabs, solved, 0, 0, kMaxSlabsPerRow);  // every row through slabs
    if (cur.nRows && cur.nUnits + nSlabs > arenaSlabs) {
      cut.batches.push_back(cur);
      cur = ImplicitWideBatch{cur.unit0 + cur.nUnits, 0, cur.row0 + cur.nRows, 0};
    }
    for (Unit u : units) {
      u.beg += at, u.end += at, u.slab += (int32_t)cur.nUnits;
      cut.units.push_back(u);
    }
    cut.rows.push_back(SplitRow{n, (int32_t)r, (int32_t)cur.nUnits, (int32_t)nSlabs, 0});
    cur.nUnits += nSlabs, ++cur.nRows;
  }
  if (cur.nRows) cut.batches.push_back(cur);
}

}  // namespace ycnr
