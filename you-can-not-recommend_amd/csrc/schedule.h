// schedule.h -- how a rating upload is cut into work units.  Where a split row is cut decides the order in which its float32
// partial sums are added, so everything here is host-only index arithmetic, a function of its arguments alone: no HIP, no
// environment, no device pointer.  ycnr_als.hip uploads, calls these planners, allocates and copies.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace ycnr {

// A wave-level work unit: ratings [beg, end) of the local CSR belong to `row`.  slab < 0: the unit covers the whole row and
// solves it; else it writes partial sums to slab number `slab`.
struct Unit {
  int64_t beg, end;
  int32_t row, slab;
};
// A row whose Gramian was split over nslabs units (slab0 .. slab0+nslabs-1); n: ratings of the row (for lambda * n)
struct SplitRow {
  int64_t n;
  int32_t row, slab0, nslabs, pad;
};
// Rows of at most this many slabs are summed as one short float32 chain (the FEW form of als_reduce_solve_kernel, the band
// slabs of a banded side); beyond it the sum is taken in double and rounded once.
constexpr int kFewSlabs = 8;
// dst slab <- sum of n consecutive source slabs, in order (element offsets into one arena)
struct SlabSum {
  int64_t dst, src0;
  int32_t n, pad;
};
// a batch of the any-k path: split rows [firstSplit, +nSplit) with their units = slabs [slabBase, +nSlabs)
struct GenBatch {
  int32_t firstSplit, nSplit, slabBase, nSlabs;
};

constexpr int kGenChunk = 4096;      // ratings per unit of the any-k path (als_gen_kernels.hip.h): every row goes through slabs there
constexpr int kWgChunk = 8192;       // ratings per chunk of a row that is split over workgroups (k > 128)
#ifndef YCNR_WG_FUSED_MAX
#define YCNR_WG_FUSED_MAX 8192
#endif
constexpr int kWgFusedMax = YCNR_WG_FUSED_MAX;  // longest row one workgroup takes whole (k > 128).  16384 until round 5: a row's Gramian is ONE float32 chain over
                                     // its ratings / 32 steps, and the item rows of the full C5 that missed the flat 1e-5 against float64 (2 of 54 sampled,
                                     // 1.09e-5) were whole rows of 8 - 16 K ratings; at 8192: every sampled row within 7.2e-6, item half-step + 1 %
constexpr int kDefaultChunk = 1024;  // ratings per split unit (and the largest fused row)
constexpr int kMaxSlabsPerRow = 64;  // heavier rows get proportionally longer chunks
constexpr int kMaxSlabsPerRowBig = 4096;  // k > 128 (chunks of kWgChunk ratings): an item of the full C5 has 10 M ratings; with 64 slabs its
                                          // chunks were float32 sums over 156 K ratings each (backward error 0.86 of its gate in round 3);
                                          // 8192-rating chunks keep every accumulation chain short, the workgroup reduce adds the slabs in order
constexpr int kMaxDualBlocks = 12;       // dual-form kernels exist for 1..12 blocks of 16 ratings (12: 340 bytes of scratch per lane, still 1.0 ms per C5-shard iteration cheaper than the primal form for rows of 177..192 ratings; 13: 936 bytes and no gain)
// Launch order of the whole rows in primal form (k <= 128: one wave per row).  Sorted by descending length, the waves that
// share a SIMD at any moment work on rows of the same length that started together and go through their Gramian phase (matrix
// pipe) and their solve phase (vector ALU) side by side.  A large launch (this many primal rows) therefore takes its rows in a
// fixed pseudo-random order -- neighbours in launch order differ in length and drift apart -- with the shortest rows kept,
// sorted, for the tail: MAL-scale user half-step 12.18 -> 11.95 ms (interleaved A/B, two runs each; profiles/r05_ab.sh).  Every
// row is solved by its own wave: the order cannot change a result.  Riffles of the sorted list (position q i + j takes row
// i + j N / q) were measured much SLOWER for q = 2 ... 32 (12.5 ... 19.4 ms): the dispatcher deals workgroups to the XCDs
// round-robin, so part j of the list -- and all the long rows -- landed on XCD j mod 8.
constexpr int64_t kShuffleMinRows = 16384;

// Ratings per split unit when the caller leaves it to the library: every chunk costs a 30 KB
// slab written and read again (k = 100), so chunks should be long -- but a launch wants >= 16
// units per resident wave (2048 on a 256-CU part at two waves per SIMD) to keep its tail short.
// MAL item side: 121.5 M ratings on one GPU -> 3072; an eighth of it on each of 8 GPUs -> 1024.
// Small uploads (below 2 M ratings: the ML-1M shape) are bound by their longest wave, not by slab traffic:
// there the chunk shrinks, down to 256, so that one round of waves covers the half-step (ML-1M shape, k = 100:
// 0.62 -> 0.54 ms per iteration with 512; 200 K x 20 K with 20 M ratings is fastest at 1024).
// nnz: ratings of the whole side; splitNnz: those of its rows above kDefaultChunk ratings (the rows that are split at all).
// Both describe the side, not the shard: the cuts of a split row must not depend on how the rows are dealt to GPUs.
inline int auto_chunk(int64_t nnz, int64_t splitNnz) {
  if (nnz < (int64_t)2048 * kDefaultChunk)
    return (int)((std::min<int64_t>(kDefaultChunk, std::max<int64_t>(256, nnz / 2048)) + 3) & ~(int64_t)3);
  const int64_t c = splitNnz / (2048 * 16);
  return (int)((std::min<int64_t>(3072, std::max<int64_t>(kDefaultChunk, c)) + 3) & ~(int64_t)3);
}

// The two arguments of auto_chunk for a side whose rows are described by rowPtr (length nRows + 1): the row pointer of an
// upload, or the prefix sums of the row totals a banded upload has agreed on.  scale: one rank of an emulated world sees only
// its own share of every row and sizes the chunks for a side `scale` times that, as the real run would.
struct SideNnz {
  int64_t nnz = 0, splitNnz = 0;
};
inline SideNnz side_nnz(const int64_t *rowPtr, int64_t nRows, int64_t scale = 1) {
  SideNnz s;
  for (int64_t r = 0; r < nRows; ++r) {
    const int64_t n = (rowPtr[r + 1] - rowPtr[r]) * scale;
    s.nnz += n > 0 ? n : 0;
    if (n > kDefaultChunk) s.splitNnz += n;
  }
  return s;
}

// Split rows into wave-level units (the counterpart of EmfLord.splitToPortions,
// lib/emf/EmfLord.js:510-612, at wave instead of worker-process granularity).
// rowPtr: local (length nRows + 1, any base).  Units index ratings relative to rowPtr[0].
inline void build_schedule(const int64_t *rowPtr, int64_t rowBegin, int64_t nRows, int chunk,
                           std::vector<Unit> &units, std::vector<SplitRow> &split, int64_t &nSlabs,
                           int64_t &solvedRows, int64_t splitAbove = -1, int fusedMax = 0, int maxSlabs = kMaxSlabsPerRow) {
  // fusedMax: longest row that stays one unit (default: chunk)
  if (fusedMax <= 0) fusedMax = chunk;
  // splitAbove >= 0 (big path): every row longer than splitAbove goes through slabs, in row
  // order (no longest-first sort, so that batches are contiguous)
  // on return units = [split chunks (nSlabs of them) | whole rows]
  const int64_t base = rowPtr[0];
  units.clear();
  split.clear();
  nSlabs = 0;
  solvedRows = 0;
  std::vector<Unit> fused;
  fused.reserve((size_t)nRows);
  for (int64_t r = 0; r < nRows; ++r) {
    const int64_t b = rowPtr[r] - base, e = rowPtr[r + 1] - base, n = e - b;
    if (n <= 0) continue;  // rows without ratings are never written
    ++solvedRows;
    const int32_t row = (int32_t)(rowBegin + r);
    if (splitAbove >= 0 ? n <= splitAbove : n <= fusedMax) {
      fused.push_back(Unit{b, e, row, -1});
      continue;
    }
    int64_t ch = chunk;
    if ((n + ch - 1) / ch > maxSlabs) ch = (n + maxSlabs - 1) / maxSlabs;
    ch = (ch + 3) & ~(int64_t)3;
    const int64_t parts = (n + ch - 1) / ch;
    split.push_back(SplitRow{n, row, (int32_t)nSlabs, (int32_t)parts, 0});
    for (int64_t p = 0; p < parts; ++p) {
      const int64_t ub = b + p * ch, ue = std::min(e, ub + ch);
      units.push_back(Unit{ub, ue, row, (int32_t)(nSlabs + p)});
    }
    nSlabs += parts;
  }
  // longest first: split chunks (all ~chunk long, longest chunks first), then fused rows by
  // descending length, so the tail of the launch is made of the cheapest units
  if (splitAbove < 0)
    std::stable_sort(units.begin(), units.end(),
                     [](const Unit &a, const Unit &b) { return (a.end - a.beg) > (b.end - b.beg); });
  std::stable_sort(fused.begin(), fused.end(),
                   [](const Unit &a, const Unit &b) { return (a.end - a.beg) > (b.end - b.beg); });
  units.insert(units.end(), fused.begin(), fused.end());
}

// Batches of consecutive split rows whose slabs fit `arenaSlabs` (at least one row per batch).
inline std::vector<GenBatch> gen_batches(const std::vector<SplitRow> &split, int64_t arenaSlabs) {
  std::vector<GenBatch> out;
  size_t i = 0;
  while (i < split.size()) {
    GenBatch b{(int32_t)i, 0, split[i].slab0, 0};
    while (i < split.size() && (b.nSplit == 0 || b.nSlabs + split[i].nslabs <= arenaSlabs)) {
      b.nSlabs += split[i].nslabs;
      ++b.nSplit;
      ++i;
    }
    out.push_back(b);
  }
  return out;
}

// Ratings [b, e) of `row` as even pieces of at most ~ch ratings, multiples of 4 long (all but the last), appended to `out`
// with slabs slab0, slab0 + 1, ...  Returns the number of pieces.  (build_schedule cuts at a fixed chunk length instead.)
inline int64_t cut_even(int64_t b, int64_t e, int64_t ch, int32_t row, int64_t slab0, std::vector<Unit> &out) {
  const int64_t len = e - b, np = (len + ch - 1) / ch;
  const int64_t pl = (((len + np - 1) / np) + 3) & ~(int64_t)3;
  int64_t made = 0;
  for (int64_t q = 0; q < np; ++q) {
    const int64_t ub = b + q * pl, ue = std::min(e, ub + pl);
    if (ue <= ub) break;
    out.push_back(Unit{ub, ue, row, (int32_t)(slab0 + made)});
    ++made;
  }
  return made;
}

// ------------------------------------------------------------------------------------------------ one piece of a row shard

enum PathKind {
  kOneWave,    // k <= 128: a wave per unit (als_kernels.hip.h)
  kWorkgroup,  // 128 < k <= 256, float32: a workgroup per unit (als_wg_kernels.hip.h)
  kAnyK        // beyond: every primal row through slabs, in row order, in batches that fit an arena (als_gen_kernels.hip.h)
};

struct PlanParams {
  PathKind kind = kOneWave;
  int chunk = kDefaultChunk;        // ratings per split unit
  int fusedMax = 0;                 // longest row that stays one unit (0: chunk); kAnyK: rows above dualMax are split
  int maxSlabs = kMaxSlabsPerRow;   // rows with more chunks than this get longer chunks
  int dualMax = 0;                  // longest row solved in dual form (0: none)
  int k = 0;                        // factors, for dualFlops
  bool shuffle = true;              // kOneWave: the launch-order shuffle of kShuffleMinRows and more primal rows
  bool sortSplit = true;            // kOneWave: the reduce takes the rows with the most slabs first (else: row order)
  int64_t arenaSlabs = 0;           // kAnyK: slabs the arena holds
};

// what a plan says in numbers (ycnr_als.hip's Schedule keeps these next to the device copies of the lists)
struct PlanCounts {
  int64_t nSlabs = 0, arenaSlabs = 0, solvedRows = 0, fusedRatings = 0;
  int32_t maxRowSlabs = 0;  // most slabs any split row has
  // whole-row units: [nSlabs, nSlabs + nPrimal) primal form, then dual classes m = kMaxDualBlocks..1
  int64_t nPrimal = 0, dualFirst[kMaxDualBlocks + 1] = {}, dualCount[kMaxDualBlocks + 1] = {};
  int64_t dualRows = 0, dualRatings = 0;
  double dualFlops = 0;  // flops the dual form executes for those rows: G = Y Y^T (symmetric), Cholesky, x = Y^T w
};

struct PiecePlan : PlanCounts {
  std::vector<Unit> units;      // [split chunks (nSlabs of them) | primal rows | dual rows by block count]
  std::vector<SplitRow> split;  // in the order the reduce takes them
  std::vector<GenBatch> genBatches;
};

// maxRowSlabs, and the order of the reduce: one wave per row, rows with the most slabs first, so that the 64-slab rows of
// the most popular items do not start when everything else has finished
inline void order_split(PiecePlan &p, const PlanParams &P) {
  p.maxRowSlabs = 0;
  for (const SplitRow &sr : p.split) p.maxRowSlabs = std::max(p.maxRowSlabs, sr.nslabs);
  if (P.kind == kOneWave && P.sortSplit)
    std::stable_sort(p.split.begin(), p.split.end(), [](const SplitRow &x, const SplitRow &y) { return x.nslabs > y.nslabs; });
}

// The schedule of rows [rowBegin, rowBegin + nRows); rowPtr: local (length nRows + 1, any base).
inline PiecePlan plan_piece(const int64_t *rowPtr, int64_t rowBegin, int64_t nRows, const PlanParams &P) {
  PiecePlan p;
  if (P.kind == kAnyK)
    build_schedule(rowPtr, rowBegin, nRows, P.chunk, p.units, p.split, p.nSlabs, p.solvedRows, P.dualMax, 0, P.maxSlabs);
  else
    build_schedule(rowPtr, rowBegin, nRows, P.chunk, p.units, p.split, p.nSlabs, p.solvedRows, -1, P.fusedMax, P.maxSlabs);
  std::vector<Unit> &units = p.units;
  const int64_t nSlabs = p.nSlabs;
  // whole rows are sorted by descending length: rows short enough for the dual form are the
  // tail of the list, grouped by their number of 16-rating blocks
  for (size_t i = (size_t)nSlabs; i < units.size(); ++i) {
    const int64_t n = units[i].end - units[i].beg;
    p.fusedRatings += n;
    if (n > P.dualMax) {
      ++p.nPrimal;
      continue;
    }
    const int m = (int)((n + 15) / 16);
    if (p.dualCount[m] == 0) p.dualFirst[m] = (int64_t)i;
    ++p.dualCount[m];
    ++p.dualRows;
    p.dualRatings += n;
    const double nd = (double)n, kd = (double)P.k;
    p.dualFlops += nd * (nd + 1) * kd + nd * nd * nd / 3.0 + 2.0 * nd * nd + 2.0 * nd * kd;
  }
  if (P.kind == kOneWave && P.shuffle && p.nPrimal >= kShuffleMinRows) {
    const int64_t tail = std::min<int64_t>(p.nPrimal / 8, 8192);  // the shortest rows stay where they are
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int64_t i = p.nPrimal - tail - 1; i > 0; --i) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      std::swap(units[(size_t)(nSlabs + i)], units[(size_t)(nSlabs + (int64_t)(x % (uint64_t)(i + 1)))]);
    }
  }
  order_split(p, P);
  p.arenaSlabs = nSlabs;
  if (P.kind == kAnyK) {
    // rows are solved in batches whose slabs fit the arena (a k = 512 float32 image is 541 KB)
    p.genBatches = gen_batches(p.split, P.arenaSlabs);
    p.arenaSlabs = 0;
    for (const GenBatch &b : p.genBatches) p.arenaSlabs = std::max<int64_t>(p.arenaSlabs, b.nSlabs);
  }
  return p;
}

// ------------------------------------------------------------------------------------------------ band-major chunks
// When the fixed matrix is far larger than the last-level cache, every split row of a kOneWave plan is cut at the same
// column-id boundaries ("bands" of W rows of the fixed matrix) instead of every `chunk` ratings, and the chunks run band by
// band.  All waves in flight then gather from one band, which stays cache-resident while each of its rows is used once per
// rating that refers to it.  Rows are assumed sorted by column id (they are when they come from a CSR transpose); unsorted
// rows only lose locality.  The column ids may live on the device only, so the re-cut comes in two halves around the one
// lookup it needs: band_queries, the caller's lower bounds (`cuts`, one per query), band_recut.

// out[q] wanted: first position p in [beg[q], end[q]) whose column id is >= key[q] (end[q] if none)
struct BoundQueries {
  std::vector<int64_t> beg, end;
  std::vector<int32_t> key;
};

// one query per listed row (index into the local rowPtr) and key, row-major
inline BoundQueries bound_queries(const int64_t *rowPtr, const std::vector<int64_t> &rows, const std::vector<int32_t> &keys) {
  BoundQueries q;
  const int64_t base = rowPtr[0];
  for (int64_t r : rows)
    for (int32_t key : keys) {
      q.beg.push_back(rowPtr[r] - base);
      q.end.push_back(rowPtr[r + 1] - base);
      q.key.push_back(key);
    }
  return q;
}

// First half: the band boundaries j W (0 < j < nBands) in every split row.  Puts the split rows back into row order, in
// which band_recut numbers the slabs.
inline BoundQueries band_queries(PiecePlan &p, const int64_t *rowPtr, int64_t rowBegin, int64_t W, int nBands) {
  std::sort(p.split.begin(), p.split.end(), [](const SplitRow &x, const SplitRow &y) { return x.row < y.row; });
  std::vector<int64_t> rows;
  std::vector<int32_t> keys;
  for (const SplitRow &sr : p.split) rows.push_back(sr.row - rowBegin);
  for (int j = 1; j < nBands; ++j) keys.push_back((int32_t)(j * W));
  return bound_queries(rowPtr, rows, keys);
}

// a row that would need more than kMaxSlabsPerRow chunks (parts == 0: none, the plan is rewritten)
struct BandCutError {
  int32_t parts = 0, row = 0;
};

// Second half: the split chunks of `p` replaced by band-major ones, ordered by band, then by descending length.
inline BandCutError band_recut(PiecePlan &p, const int64_t *rowPtr, int64_t rowBegin, const PlanParams &P, int nBands,
                               const std::vector<int64_t> &cuts) {
  const int64_t base = rowPtr[0], chunk = P.chunk, minSeg = std::max<int64_t>(64, chunk / 4);
  std::vector<Unit> bu;
  std::vector<int> band;  // of bu[i]
  int64_t slabs = 0;
  for (size_t r = 0; r < p.split.size(); ++r) {
    SplitRow &sr = p.split[r];
    const int64_t b = rowPtr[sr.row - rowBegin] - base, e = rowPtr[sr.row - rowBegin + 1] - base;
    // band segments, short ones merged into their successor (the last into its predecessor)
    std::vector<std::pair<int64_t, int>> seg;  // (start, band); ends at the next start / e
    int64_t s = b;
    for (int j = 0; j < nBands; ++j) {
      const int64_t q = j + 1 < nBands ? std::min(e, std::max(s, cuts[r * (size_t)(nBands - 1) + j])) : e;
      if (q - s >= minSeg) {
        seg.push_back({s, j});
        s = q;
      }
    }
    if (seg.empty()) seg.push_back({b, 0});
    seg[0].first = b;  // ratings left over before the first kept boundary join the first segment
    int64_t ch = chunk;
    const int64_t room = kMaxSlabsPerRow - (int64_t)seg.size();
    if (room < 1 || (sr.n + ch - 1) / ch > room) ch = std::max(ch, (sr.n + std::max<int64_t>(1, room) - 1) / std::max<int64_t>(1, room));
    sr.slab0 = (int32_t)slabs;
    int64_t parts = 0;
    for (size_t i = 0; i < seg.size(); ++i) {
      parts += cut_even(seg[i].first, i + 1 < seg.size() ? seg[i + 1].first : e, ch, sr.row, slabs + parts, bu);
      band.resize(bu.size(), seg[i].second);
    }
    if (parts > kMaxSlabsPerRow) return BandCutError{(int32_t)parts, sr.row};
    sr.nslabs = (int32_t)parts;
    slabs += parts;
  }
  std::vector<size_t> order(bu.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
    return band[x] != band[y] ? band[x] < band[y] : (bu[x].end - bu[x].beg) > (bu[y].end - bu[y].beg);
  });
  std::vector<Unit> all;
  all.reserve(bu.size() + p.units.size() - (size_t)p.nSlabs);
  for (size_t i : order) all.push_back(bu[i]);
  all.insert(all.end(), p.units.begin() + p.nSlabs, p.units.end());
  p.units.swap(all);
  for (int m = 0; m <= kMaxDualBlocks; ++m)
    if (p.dualCount[m]) p.dualFirst[m] += slabs - p.nSlabs;
  p.nSlabs = slabs;
  p.arenaSlabs = slabs;
  order_split(p, P);
  return BandCutError{};
}

// ------------------------------------------------------------------------------------------------ a side sharded by bands of columns
// ycnr_als_set_ratings_banded: every rank holds, for EVERY row of the side, the ratings of its own bands [rankBands[rank],
// rankBands[rank + 1]) and accumulates one slab per (row, band); the slabs travel to the row's owner (rows [ownerBounds[g],
// ownerBounds[g + 1]) belong to rank g), which adds a row's band slabs in band order and solves.

// where an owner finds a band slab: slab number `slab` of what rank `src` computed -- in the owner's own arena for
// src == rank, else in its receive buffer (numbered from recvSlab0[src]).  src < 0: no rating of the row in that band
struct SlabRef {
  int32_t src;
  int64_t slab;
};

// where things are in the lists and arenas of a banded side (ycnr_als.hip's BandedSide keeps these)
struct BandedLayout {
  std::vector<int64_t> groupUnit0, groupUnits;  // per owner group: its chunk units [unit0, +n) of the unit list
  std::vector<int64_t> groupSum0, groupSums;    // ... and its multi-chunk (row, band) segments [sum0, +n) of the sums
  std::vector<int64_t> groupSlab0;              // first band slab of group g in the arena (rows of g x local bands)
  std::vector<int64_t> recvSlab0;               // first slab of source rank r in the receive buffer (owned rows x bands of r; own rank: unused)
  int64_t bandSlabs = 0, tmpSlabs = 0;          // the arena: band slabs, then the chunks of the multi-chunk segments
};

struct BandedPlan : BandedLayout {
  const char *error = nullptr;  // set: the upload is too large for 32-bit slab numbers, the plan is not to be used
  std::vector<Unit> units;      // chunk units, owner group by owner group
  std::vector<SlabSum> sums;    // the (row, band) segments that were cut into several chunks
  std::vector<SplitRow> owned;  // the rows this rank solves: nBands slabs each, through `table`
  std::vector<SlabRef> table;   // owned rows (empty ones included) x nBands
};

// hp: this rank's row pointer over all rows of the side; counts[row * nBands + band]: ratings of every (row, band) on every
// rank; slabElems: elements of one slab (SlabSum counts in elements).
inline BandedPlan plan_banded(const int64_t *hp, const double *counts, int nBands, const int64_t *rankBands, const int64_t *ownerBounds,
                              int rank, int world, int64_t chunk, int64_t slabElems) {
  BandedPlan B;
  const int64_t own0 = ownerBounds[rank], ownN = ownerBounds[rank + 1] - own0;
  if (ownN > 0x7fffffffLL / std::max(nBands, 1)) {  // (an owned row's slab0 is its index x nBands)
    B.error = "too many owned rows";
    return B;
  }
  const int bl = (int)rankBands[rank], bpr = (int)rankBands[rank + 1] - bl;
  B.groupSlab0.assign((size_t)world + 1, 0);
  for (int g = 0; g < world; ++g) B.groupSlab0[(size_t)g + 1] = B.groupSlab0[(size_t)g] + (ownerBounds[g + 1] - ownerBounds[g]) * bpr;
  B.bandSlabs = B.groupSlab0[(size_t)world];
  // units: group by group (the order they are computed and sent in), longest first inside a group
  const int64_t base = hp[0];
  B.groupUnit0.assign((size_t)world, 0);
  B.groupUnits.assign((size_t)world, 0);
  B.groupSum0.assign((size_t)world, 0);
  B.groupSums.assign((size_t)world, 0);
  int64_t tmp = 0;
  for (int st = 1; st <= world; ++st) {  // in the order the groups are computed and sent: consecutive stages are contiguous
    const int g = (rank + st) % world;
    B.groupUnit0[(size_t)g] = (int64_t)B.units.size();
    B.groupSum0[(size_t)g] = (int64_t)B.sums.size();
    const size_t u0 = B.units.size();
    for (int64_t r = ownerBounds[g]; r < ownerBounds[g + 1]; ++r) {
      if (hp[r + 1] == hp[r]) continue;
      int64_t p = hp[r] - base;
      for (int j = 0; j < bpr; ++j) {
        const int64_t len = (int64_t)counts[(size_t)r * nBands + (size_t)(bl + j)];
        if (len <= 0) continue;
        const int64_t bandSlab = B.groupSlab0[(size_t)g] + (r - ownerBounds[g]) * bpr + j;
        if (len <= chunk) {
          cut_even(p, p + len, chunk, (int32_t)r, bandSlab, B.units);
        } else {
          const int64_t made = cut_even(p, p + len, chunk, (int32_t)r, B.bandSlabs + tmp, B.units);
          B.sums.push_back(SlabSum{bandSlab * slabElems, (B.bandSlabs + tmp) * slabElems, (int32_t)made, 0});
          tmp += made;
        }
        p += len;
      }
    }
    std::stable_sort(B.units.begin() + (ptrdiff_t)u0, B.units.end(), [](const Unit &x, const Unit &y) { return (x.end - x.beg) > (y.end - y.beg); });
    B.groupUnits[(size_t)g] = (int64_t)B.units.size() - B.groupUnit0[(size_t)g];
    B.groupSums[(size_t)g] = (int64_t)B.sums.size() - B.groupSum0[(size_t)g];
  }
  B.tmpSlabs = tmp;
  if (B.bandSlabs + B.tmpSlabs > 0x7fffffffLL) {
    B.error = "too many slabs";
    return B;
  }
  // what this rank owns: its rows' band slabs from every rank, and the rows to solve
  B.recvSlab0.assign((size_t)world + 1, 0);
  for (int r = 0; r < world; ++r)
    B.recvSlab0[(size_t)r + 1] = B.recvSlab0[(size_t)r] + (r == rank ? 0 : ownN * (rankBands[r + 1] - rankBands[r]));
  B.table.assign((size_t)ownN * (size_t)nBands, SlabRef{-1, 0});
  for (int64_t i = 0; i < ownN; ++i) {
    const int64_t r = own0 + i;
    int64_t total = 0;
    for (int b = 0; b < nBands; ++b) total += (int64_t)counts[(size_t)r * nBands + b];
    if (total <= 0) continue;
    B.owned.push_back(SplitRow{total, (int32_t)r, (int32_t)(i * nBands), (int32_t)nBands, 0});
    for (int b = 0; b < nBands; ++b) {
      if (counts[(size_t)r * nBands + b] <= 0) continue;
      int src = 0;
      while (src + 1 < world && b >= rankBands[src + 1]) ++src;
      B.table[(size_t)i * nBands + b] =
          SlabRef{src, src == rank ? B.groupSlab0[(size_t)rank] + i * bpr + (b - bl)
                                   : B.recvSlab0[(size_t)src] + i * (rankBands[src + 1] - rankBands[src]) + (b - rankBands[src])};
    }
  }
  return B;
}

}  // namespace ycnr
