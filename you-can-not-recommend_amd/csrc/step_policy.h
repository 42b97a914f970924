// step_policy.h -- which of the three paths a solve takes and with which sizes: the path and its slab size, the parameters of
// a piece's plan (schedule.h), the predicates every half-step consults, whether the dual classes go to side streams, and the
// launch geometry of the any-k path (choose_gen).  Host-only and a function of its arguments alone, like schedule.h and
// kernel_choice.h: no HIP, no environment, no device call.  The toggles of the environment come in as the plain fields of
// Toggles; ycnr_als.hip fills them, evaluates the policy per upload and launches what it says.  The sizing functions the
// kernels share with the host live here too, behind YCNR_HD.
#pragma once
#include "../../include/ycnr_als.h"
#include "schedule.h"

// the one host/device marker: a plain C++ compiler builds this header for the CPU tests
#ifdef __HIPCC__
#define YCNR_HD __host__ __device__
#else
#define YCNR_HD
#endif

namespace ycnr {

constexpr int kMaxFactors = 128;     // float64, and the one-wave-per-row float32 kernels
constexpr int kMaxFactorsBig = 256;  // float32 through the workgroup-per-row kernels of als_wg_kernels.hip.h
constexpr int kMaxFactorsAny = 4096; // beyond kMaxFactorsBig (float64: kMaxFactors): the any-k path of als_gen_kernels.hip.h
constexpr int kMaxDualBlocksSmallK = 5;  // k <= 128: beyond 80 ratings the row kernel (k x k) is cheaper (MAL scale, k = 100: 6 -> 5 blocks took 0.2 ms off the user half-step once the solve had lost its readlanes and transposes; 4 was slower)
constexpr int64_t kPlanesMaxBytes = (int64_t)64 << 20;  // largest plane matrix that stays cache-resident (use_planes)
constexpr int64_t kGraphMaxRatings = 2 * 1024 * 1024;  // uploads below this replay their half-step as a captured hipGraph ...
constexpr int64_t kGraphMinRatings = 256 * 1024;       // ... unless they are so small that the graph launch itself costs more than four
                                                        // kernel launches (ML-100k shape: 0.124 ms per iteration launch by launch, 0.174 as graphs)
constexpr int64_t kMinOverlapDualRows = 1024;  // fewer dual-form rows than this: everything in stream order

// ---------------------------------------------------------------------------------- sizes the kernels share with the host

YCNR_HD constexpr int tile_count(int nb) { return nb * (nb + 1) / 2; }
// elements of T one split unit writes: NT tiles x 4 regs x 64 lanes + NB b-partials x 64 lanes
YCNR_HD constexpr int64_t slab_elems(int nb) { return (int64_t)(tile_count(nb) * 4 + nb) * 64; }
// bytes of a row of the plane matrix (GramX6P): 96 per 16-column block, 32 for a packed last block of four columns
YCNR_HD constexpr int planes_row_bytes(int nb, bool pack) { return pack ? (nb - 1) * 96 + 32 : nb * 96; }
YCNR_HD constexpr bool planes_pack(int k) { return k > 16 && k % 16 == 4; }
// floats of a slab of the workgroup-per-row path: NT tiles of 256 + the right-hand side
YCNR_HD constexpr int64_t wg_slab_floats(int nb) { return (int64_t)tile_count(nb) * 256 + nb * 16; }

// the any-k path (als_gen_kernels.hip.h)
YCNR_HD constexpr int64_t gen_slab_elems(int nb) { return (int64_t)tile_count(nb) * 256 + (int64_t)nb * 16; }
constexpr int kGenSq = 4;
constexpr int kGenGramMaxWaves = 8;
// rectangles of sr x cw tiles over a matrix of nb block columns: block rows sr at a time, from the diagonal to the right in steps of cw
YCNR_HD constexpr int gen_items(int nb, int sr, int cw) {
  int n = 0;
  for (int x = 0; x < nb; x += sr) n += (nb - x + cw - 1) / cw;
  return n;
}
// block rows of a wave's rectangle: float64 tiles take twice the registers, and 2 x 4 tiles leave room for two waves per SIMD
// of an eight-wave workgroup (k = 256: 20 rectangles, three passes of seven waves; 4 x 4 ran five waves on four SIMDs)
template <typename T>
constexpr int gen_rect_rows() { return sizeof(T) == 4 ? 4 : 2; }
#ifndef YCNR_GEN_SQW_F32
#define YCNR_GEN_SQW_F32 1  // (2 -- 4 x 8 tiles, three passes of seven waves at k = 512 -- measured slower: 269 against 241 ms per iteration)
#endif
template <typename T>
constexpr int gen_sqw() { return sizeof(T) == 4 ? YCNR_GEN_SQW_F32 : 1; }
// row pitch of a panel in elements: a multiple of 16, P * sizeof(T) = 64 bytes modulo 256 (float32) / 128 modulo 256 (float64)
YCNR_HD constexpr int gen_panel_pitch(int nb, size_t ts) {
  const int mod = (int)(256 / ts);
  return nb * 16 + ((16 - (nb * 16) % mod) + mod) % mod;
}
template <typename T, int V>
constexpr int gen_loader_slots() { return V == 1 ? 8 : 4; }
YCNR_HD constexpr size_t gen_gram_lds_bytes(int R, int P, size_t ts) { return (size_t)2 * R * ((size_t)P + 1) * ts; }
YCNR_HD constexpr size_t gen_solve_left_lds_bytes(int nb, size_t ts, int pw) {
  return (2 * 16 * (ts == 8 ? 18 : 20) + 3 * (size_t)nb * 16 + 16 + (size_t)pw * pw * 256) * ts + 64;
}
YCNR_HD constexpr size_t gen_solve_lds_bytes(int nb, size_t ts, bool panelLds) {
  return (2 * 16 * (ts == 8 ? 18 : 20) + 3 * (size_t)nb * 16 + 16 + (panelLds ? (size_t)nb * 256 : 0)) * ts + 64;
}
constexpr size_t kGenPanelLdsMax = 36 * 1024;  // panels up to this size live in LDS (k = 512 float32, k = 256 float64: four workgroups per CU)

// ------------------------------------------------------------------------------------------------------------ the inputs

// What the policy reads of a handle's options for one side: the dtype, k AS THE KERNELS SEE IT, the option flags, and the
// rows of the fixed (opposite) matrix.
struct StepShape {
  bool f64;
  int k;
  uint32_t flags;     // YCNR_FLAG_*
  int64_t fixedRows;
};

// A/B toggles of the environment, as ycnr_als.hip read them
struct Toggles {
  bool noOverlap = false, noGraph = false;  // YCNR_NO_OVERLAP, YCNR_NO_GRAPH
  bool noX6p = false;                       // YCNR_NO_X6P
  bool genRightLooking = false;             // YCNR_GEN_RIGHT_LOOKING: the right-looking any-k solve everywhere
  bool noGenX6 = false;                     // YCNR_NO_GEN_X6
  int dualMaxBlocks = -1;                   // YCNR_DUAL_MAX_BLOCKS (>= 0; < 0: not set)
};

// --------------------------------------------------------------------------------------------------------------- the path

inline int slab_nb(int k) { return (k + 15) / 16; }

// The path of a solve.  k is the k the kernels see: the resident trainer pads float32 rows to a multiple of 4 first (kPad), so
// it never takes the any-k path for k % 4 != 0 up to 256; the out-of-place callers (fold-in, the portion op) do not pad, and
// their float32 rows that are not 16-byte multiples take the any-k path above 128 factors.
inline PathKind step_path(bool f64, int k) {
  if (k <= kMaxFactors) return kOneWave;
  if (!f64 && k <= kMaxFactorsBig && k % 4 == 0) return kWorkgroup;
  return kAnyK;
}

// float32, k = 16 m + 4 (m >= 1), k <= 128: the last 4 columns of the Gramian go to the VALU
inline bool use_valu_edge(const StepShape &s) {
  return !s.f64 && !(s.flags & YCNR_FLAG_NO_VALU_EDGE) && s.k >= 20 && s.k <= kMaxFactors && s.k % 16 == 4;
}

// split chunks on the bf16 matrix pipe (exact 3-way split, six products): float32, one-wave
// kernels, fixed matrix addressable by a 32-bit buffer offset
inline bool use_slab_x6(const StepShape &s) {
  return !s.f64 && !(s.flags & YCNR_FLAG_NO_BF16X6) && s.k <= kMaxFactors && s.fixedRows * s.k * 4 < ((int64_t)1 << 31);
}

// The fused row kernel on pre-split planes (GramX6P): float32 bf16x6 path, k % 4 == 0, k <= 124 with a padded column for
// the right-hand side (k % 16 != 0), and a plane matrix (96 bytes per 16-column block and row) that stays cache-resident.
inline bool use_planes(const StepShape &s, const Toggles &t) {
  return !t.noX6p && use_slab_x6(s) && !(s.flags & YCNR_FLAG_LDS_SOLVER) && s.k % 4 == 0 && s.k <= 124 && s.k % 16 != 0 &&
         s.fixedRows * planes_row_bytes(slab_nb(s.k), planes_pack(s.k)) <= kPlanesMaxBytes;
}

// registers (x 64 lanes x sizeof(T)) one split unit of the one-wave kernels writes
inline int64_t slab_regs(const StepShape &s) {
  const int nb = slab_nb(s.k);
  if (use_valu_edge(s) && !use_slab_x6(s)) {
    const int nbm = nb - 1;
    return tile_count(nbm) * 4 + nbm + nbm * 4 + 8;
  }
  return tile_count(nb) * 4 + nb;
}

// elements of a slab on a path; the one-wave kernels of the resident trainer write theirs in the layout of slab_regs
inline int64_t step_slab_elems(PathKind path, int k) {
  return path == kAnyK ? gen_slab_elems(slab_nb(k)) : path == kWorkgroup ? wg_slab_floats(slab_nb(k)) : slab_elems(slab_nb(k));
}
inline int64_t resident_slab_elems(const StepShape &s) {
  const PathKind path = step_path(s.f64, s.k);
  return path == kOneWave ? slab_regs(s) * 64 : step_slab_elems(path, s.k);
}

// Longest row solved in dual form (0 = never): float32 MFMA solver only, rows of 16-byte
// multiples, and strictly fewer 16-blocks than the primal form would use.
inline int dual_max_ratings(const StepShape &s, const Toggles &t) {
  // (k > 128 with k % 4 != 0 runs on rows padded to a multiple of 4: see kPad)
  if (s.f64 || (s.flags & (YCNR_FLAG_LDS_SOLVER | YCNR_FLAG_NO_DUAL)) || (s.k % 4 != 0 && s.k <= kMaxFactors)) return 0;
  // k > 128: every row that is not dual goes through slabs and the 4-wave LDS solve, whose cost
  // grows with k^3; an n x n problem with n <= 176 still fits one wave's registers
  int most = s.k > kMaxFactors ? kMaxDualBlocks : kMaxDualBlocksSmallK;
  if (t.dualMaxBlocks >= 0) most = std::min(t.dualMaxBlocks, most);  // experiments
  return 16 * std::min(most, slab_nb(s.k) - 1);
}

// Small uploads (the ML-100k / ML-1M shapes) capture their half-step once and replay it as a hipGraph: one piece without
// an exchange on the handle's own stream, the one-wave path, between kGraphMinRatings and kGraphMaxRatings ratings.
inline bool graphable(const StepShape &s, const Toggles &t, bool exchange, size_t nParts, int64_t ratings, bool ownStream) {
  return !exchange && nParts == 1 && step_path(s.f64, s.k) == kOneWave && ratings < kGraphMaxRatings && ratings >= kGraphMinRatings &&
         ownStream && !(s.flags & (YCNR_FLAG_NO_OVERLAP | YCNR_FLAG_NO_GRAPH)) && !t.noOverlap && !t.noGraph;
}

// Whether the dual classes of a piece go to side streams, next to the row kernel: enough dual rows to pay for the fork and the
// joins (any, in the captured form of a small half-step), unless the piece runs in stream order (inOrder: one of several pieces
// in flight) or overlap is switched off.  The any-k path takes its dual classes in stream order.  launch_part launches by this;
// the step info's dualOverlapped reports it with captured = inOrder = false.
inline bool duals_on_side_streams(const StepShape &s, const Toggles &t, int64_t dualRows, bool captured, bool inOrder) {
  return step_path(s.f64, s.k) != kAnyK && (dualRows >= kMinOverlapDualRows || (captured && dualRows > 0)) && !inOrder &&
         !(s.flags & YCNR_FLAG_NO_OVERLAP) && !t.noOverlap;
}

// ------------------------------------------------------------------------------------------------------ the plan parameters

// slabs the arena of the any-k path holds: rows are solved in batches that fit it (a k = 512 float32 image is 541 KB and
// several MB beyond 1024 factors: a portion of 10 K short rows would ask for gigabytes)
inline int64_t gen_arena_slabs(int64_t arenaBytes, int64_t slabBytes) { return std::max<int64_t>(1, arenaBytes / slabBytes); }

// A piece of the resident trainer.  kReal: the caller's factorsCount (s.k is the padded one); autoChunk: options.chunkRatings
// was 0; side: the ratings of the WHOLE side; genArenaBytes: the arena of the any-k path.
inline PlanParams resident_plan_params(const StepShape &s, const Toggles &t, int kReal, bool autoChunk, int chunkRatings, SideNnz side,
                                       bool shuffle, int64_t genArenaBytes) {
  PlanParams P;
  P.kind = step_path(s.f64, s.k);
  const bool gen = P.kind == kAnyK, big = P.kind == kWorkgroup;
  // k > 128: a unit is a whole workgroup's work, so chunks are long (a slab is 140 KB at k = 256)
  // (an explicit options.chunkRatings is honoured there too: tests cut short rows into chunks with it)
  // The automatic chunk length follows the split rows of the WHOLE side (side: their ratings), not of this piece: where a
  // split row is cut decides the order its partial sums are added in, so a length that depended on the piece would make the
  // factors depend on how the rows are cut into shards and pieces (and a feedback re-cut would change them: round-3 review).
  P.chunk = autoChunk ? (gen ? kGenChunk : big ? kWgChunk : auto_chunk(side.nnz, side.splitNnz)) : chunkRatings;
  P.fusedMax = big && autoChunk ? kWgFusedMax : std::min(P.chunk, chunkRatings);
  P.maxSlabs = big ? kMaxSlabsPerRowBig : kMaxSlabsPerRow;
  P.dualMax = dual_max_ratings(s, t);
  P.k = kReal;
  P.shuffle = shuffle;
  if (gen) P.arenaSlabs = gen_arena_slabs(genArenaBytes, step_slab_elems(kAnyK, s.k) * (s.f64 ? 8 : 4));
  return P;
}

// The out-of-place callers (fold-in beyond 128 factors, the level-1 portion op): the plan of a piece of the resident trainer
// with every row in primal form, no shuffle, and the split rows in row order.
inline PlanParams out_of_place_plan_params(bool f64, int k, int64_t genArenaBytes) {
  PlanParams P;
  P.kind = step_path(f64, k);
  const bool gen = P.kind == kAnyK, big = P.kind == kWorkgroup;
  P.chunk = gen ? kGenChunk : big ? kWgChunk : kDefaultChunk;
  P.fusedMax = big ? kWgFusedMax : 0;
  P.k = k;
  P.shuffle = P.sortSplit = false;
  if (gen) P.arenaSlabs = gen_arena_slabs(genArenaBytes, step_slab_elems(kAnyK, k) * (f64 ? 8 : 4));
  return P;
}

// ------------------------------------------------------------------------------------------- the geometry of the any-k path

enum GenStatus {
  kGenOk,
  kGenRhsTooLarge,   // the right-hand side does not fit a CU's LDS
  kGenPanelTooLarge  // a panel of four ratings does not fit a CU's LDS
};

struct GenChoice {
  GenStatus status;
  int nb;
  // solve: als_gen_solve_left_kernel<T, leftMaxc, leftPw, leftWaves, ...> where `left`, else als_gen_solve_kernel<T, panelLds>
  bool panelLds, left;
  int leftMaxc, leftPw, leftWaves;
  // Gramian: als_gen_gram_kernel<T, vec ? 16 / sizeof(T) : 1, x6>, panels of R ratings at pitch P, `threads` per workgroup,
  // `slots` loader slots per thread
  bool vec, x6;
  int R, P, slots, threads;
  size_t panelBytes, solveLds, leftLds, gramLds;  // the solve's panel; dynamic LDS of the right-looking solve, the left-looking one, the Gramian
};

// ts: sizeof(T); fixedAligned: the fixed matrix starts on a 16-byte boundary
inline GenChoice choose_gen(size_t ts, int k, bool fixedAligned, const Toggles &t) {
  GenChoice c = {};
  c.nb = slab_nb(k);
  c.panelBytes = (size_t)c.nb * 256 * ts;
  c.panelLds = c.panelBytes <= kGenPanelLdsMax;
  c.solveLds = gen_solve_lds_bytes(c.nb, ts, c.panelLds);
  if (c.solveLds > 160 * 1024) {
    c.status = kGenRhsTooLarge;
    return c;
  }
  // the left-looking solve where a block of four rows fits the registers of eight waves: float32 up to k = 512, float64 up to 256 (beyond: the right-looking kernel)
  // (YCNR_GEN_RIGHT_LOOKING: the right-looking kernel everywhere, for A/B runs)
  c.leftWaves = 8, c.leftPw = 4;
  if (!t.genRightLooking) {
    if (ts == 4) {
      const int maxc = (c.nb + 7) / 8;
      c.left = maxc <= 4;
      c.leftMaxc = maxc <= 2 ? 2 : 4;
    } else if (c.nb <= 16) {
      // (k = 256, 200 K x 20 K, per iteration: right-looking 301 ms; 4 rows x 8 waves as in float32, one workgroup per CU: 347;
      // 2 rows x 8 waves, two per CU: 277; 2 rows x 4 waves, three per CU: 253)
      c.left = true;
      c.leftMaxc = 4, c.leftWaves = 4, c.leftPw = 2;
    }
  }
  c.leftLds = gen_solve_left_lds_bytes(c.nb, ts, c.leftPw);
  // Gramian: 16-byte loads when every row of the fixed matrix starts on a 16-byte boundary, single elements otherwise;
  // the waves of a workgroup share the rectangles of a pass evenly; R ratings per panel: as many as two buffers of <= 72 KB
  // (two workgroups per CU) and the loader's slots allow, at least 4
  const int V = 16 / (int)ts;
  c.vec = k % V == 0 && fixedAligned;
  const int nSq = ts == 4 ? gen_items(c.nb, gen_rect_rows<float>(), gen_sqw<float>() * kGenSq) : gen_items(c.nb, gen_rect_rows<double>(), gen_sqw<double>() * kGenSq);
  const int passes = (nSq + kGenGramMaxWaves - 1) / kGenGramMaxWaves;
  c.threads = 64 * std::max(2, (nSq + passes - 1) / passes);
  c.P = gen_panel_pitch(c.nb, ts);
  c.slots = c.vec ? gen_loader_slots<float, 4>() : gen_loader_slots<float, 1>();  // (the same in both precisions)
  c.R = 32;
  const int64_t loads = k / (c.vec ? V : 1);  // loads per rating of a panel
  // float32 with 16-byte rows whose panel of 32 ratings fits one workgroup's LDS AND its loader slots (8 per thread of at most
  // eight waves: 32 (k / 4) <= 8 * 512, i.e. k <= 512): the products on the bf16 pipe (X6); 516 <= k keeps float32 MFMAs
  c.x6 = ts == 4 && c.vec && !t.noGenX6 && gen_gram_lds_bytes(32, c.P, ts) <= 150 * 1024 && 32 * loads <= (int64_t)8 * c.threads;
  if (c.x6) c.slots = 8;
  else
    while (c.R > 4 && (gen_gram_lds_bytes(c.R, c.P, ts) > 72 * 1024 || c.R * loads > (int64_t)c.slots * c.threads)) c.R >>= 1;
  c.gramLds = gen_gram_lds_bytes(c.R, c.P, ts);
  if (c.gramLds > 150 * 1024 || c.R * loads > (int64_t)c.slots * c.threads) c.status = kGenPanelTooLarge;
  return c;
}

}  // namespace ycnr
