// CPU test of csrc/step_policy.h, the host-only rules that say which path a solve takes and with which sizes
// (tests/test_step_policy.py builds this with the host sanitizers and runs it).  Every expectation below is written out from
// the rules and the kernels' limits as independent statements, none is captured from the code under test.
#include "step_policy.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace ycnr;

#define CHECK(...)                                                               \
  do {                                                                           \
    if (!(__VA_ARGS__)) {                                                        \
      printf("FAIL %s:%d (%s): %s\n", __FILE__, __LINE__, g_case, #__VA_ARGS__); \
      exit(1);                                                                   \
    }                                                                            \
  } while (0)
static char g_case[200] = "";

// ------------------------------------------------------------------------------------------------------------------ path

// The three derivations of the parent commit, literally: the record of what step_path unified.
static bool old_is_gen(bool f64, int k) { return k > (f64 ? 128 : 256); }
static PathKind old_build_part(bool f64, int k) {  // resident trainer
  const bool gen = old_is_gen(f64, k);
  const bool big = !gen && k > 128;
  return gen ? kAnyK : big ? kWorkgroup : kOneWave;
}
static PathKind old_fold_launch_steps(bool f64, int k) {  // fold-in beyond 128 factors
  const bool gen = old_is_gen(f64, k) || k % 4 != 0;
  return gen ? kAnyK : kWorkgroup;
}
static PathKind old_als_calc_portion(bool f64, int k) {  // level-1 portion op
  const bool gen = old_is_gen(f64, k) || (k > 128 && k % 4 != 0);
  const bool big = !gen && k > 128;
  return gen ? kAnyK : big ? kWorkgroup : kOneWave;
}

static long test_path() {
  long n = 0;
  CHECK(kMaxFactorsAny == 4096);
  for (int f64 = 0; f64 < 2; ++f64)
    for (int k = 1; k <= kMaxFactorsAny; ++k) {
      snprintf(g_case, sizeof g_case, "path f64=%d k=%d", f64, k);
      ++n;
      const PathKind p = step_path(f64 != 0, k);
      // the rule
      const PathKind want = k <= 128 ? kOneWave : (!f64 && k <= 256 && k % 4 == 0) ? kWorkgroup : kAnyK;
      CHECK(p == want);
      // what each caller can reach: the trainer pads float32 rows to a multiple of 4 (every k above 128), fold-in comes
      // here only beyond 128 factors, the portion op with every k
      if (f64 || k <= 128 || k % 4 == 0) CHECK(p == old_build_part(f64 != 0, k));
      if (k > 128) CHECK(p == old_fold_launch_steps(f64 != 0, k));
      CHECK(p == old_als_calc_portion(f64 != 0, k));
      // slab sizes: tiles of the upper triangle of nb x nb blocks; 256 elements per tile + 16 per block of the right-hand
      // side (workgroup and any-k), 4 registers x 64 lanes per tile + 64 per block (one wave)
      const int64_t nb = (k + 15) / 16, nt = nb * (nb + 1) / 2;
      CHECK(slab_nb(k) == nb);
      CHECK(step_slab_elems(kAnyK, k) == nt * 256 + nb * 16);
      CHECK(step_slab_elems(kWorkgroup, k) == nt * 256 + nb * 16);
      CHECK(step_slab_elems(kOneWave, k) == (nt * 4 + nb) * 64);
    }
  // literal
  snprintf(g_case, sizeof g_case, "path literal");
  CHECK(step_path(false, 128) == kOneWave && step_path(true, 128) == kOneWave);
  CHECK(step_path(false, 129) == kAnyK && step_path(false, 130) == kAnyK && step_path(false, 132) == kWorkgroup);
  CHECK(step_path(true, 129) == kAnyK && step_path(true, 132) == kAnyK && step_path(true, 136) == kAnyK);
  CHECK(step_path(false, 256) == kWorkgroup && step_path(false, 257) == kAnyK && step_path(false, 260) == kAnyK);
  CHECK(step_slab_elems(kWorkgroup, 256) * 4 == 140288);  // "a slab is 140 KB at k = 256"
  CHECK(step_slab_elems(kOneWave, 100) == (28 * 4 + 7) * 64);
  return n;
}

// ------------------------------------------------------------------------------------------------------------ predicates

static const uint32_t kFlagBits[6] = {YCNR_FLAG_LDS_SOLVER, YCNR_FLAG_NO_DUAL, YCNR_FLAG_NO_VALU_EDGE, YCNR_FLAG_NO_BF16X6, YCNR_FLAG_NO_OVERLAP,
                                      YCNR_FLAG_NO_GRAPH};

static int64_t want_plane_row_bytes(int k) {
  const int nb = (k + 15) / 16;
  return k > 16 && k % 16 == 4 ? (nb - 1) * 96 + 32 : nb * 96;  // a last block of four columns is packed into 32 bytes
}

static long test_predicates() {
  long n = 0;
  CHECK(YCNR_FLAG_LDS_SOLVER == 1 && YCNR_FLAG_NO_DUAL == 2 && YCNR_FLAG_NO_VALU_EDGE == 8 && YCNR_FLAG_NO_BF16X6 == 16 && YCNR_FLAG_NO_OVERLAP == 64 &&
        YCNR_FLAG_NO_GRAPH == 128);
  const int64_t GB2 = (int64_t)1 << 31, MB64 = (int64_t)64 << 20;
  for (int f64 = 0; f64 < 2; ++f64)
    for (int k = 1; k <= 256; ++k)
      for (int bits = 0; bits < 64; ++bits) {
        uint32_t flags = 0;
        for (int b = 0; b < 6; ++b)
          if (bits & (1 << b)) flags |= kFlagBits[b];
        const bool lds = flags & 1, noDual = flags & 2, noEdge = flags & 8, noX6 = flags & 16, noOverlap = flags & 64, noGraph = flags & 128;
        // fixed matrices on each side of the 2 GB limit of the 32-bit buffer offset (rows * k * 4 bytes) and of the 64 MB limit
        // of the plane matrix, and a few ordinary ones
        const int64_t last2g = (GB2 - 1) / (4 * (int64_t)k), last64m = MB64 / want_plane_row_bytes(k);
        const int64_t rowsList[8] = {1, 1682, 12700, last64m, last64m + 1, last2g, last2g + 1, (int64_t)0x7fffffff};
        for (int64_t rows : rowsList) {
          const StepShape s{f64 != 0, k, flags, rows};
          snprintf(g_case, sizeof g_case, "f64=%d k=%d flags=%u fixedRows=%lld", f64, k, flags, (long long)rows);
          ++n;
          const int nb = (k + 15) / 16;
          // the VALU edge: float32, k = 16 m + 4 with m >= 1, one-wave kernels
          const bool edge = !f64 && !noEdge && k % 16 == 4 && k >= 20 && k <= 128;
          CHECK(use_valu_edge(s) == edge);
          // bf16x6 chunks: float32, one-wave kernels, the fixed matrix below 2 GB
          const bool x6 = !f64 && !noX6 && k <= 128 && rows * k * 4 < GB2;
          CHECK(use_slab_x6(s) == x6);
          // planes
          for (int off = 0; off < 2; ++off) {
            Toggles t;
            t.noX6p = off != 0;
            const bool planes = !off && x6 && !lds && k % 4 == 0 && k % 16 != 0 && k <= 124 && rows * want_plane_row_bytes(k) <= MB64;
            CHECK(use_planes(s, t) == planes);
          }
          // registers of a slab: the VALU-edge layout only where the chunks do not go through a bf16x6 kernel
          const int nbm = nb - 1;
          const int64_t regs = edge && !x6 ? nbm * (nbm + 1) / 2 * 4 + nbm + nbm * 4 + 8 : nb * (nb + 1) / 2 * 4 + nb;
          CHECK(slab_regs(s) == regs);
          if (k <= 128) CHECK(resident_slab_elems(s) == regs * 64);
          else CHECK(resident_slab_elems(s) == (int64_t)nb * (nb + 1) / 2 * 256 + nb * 16);
          // dual classes: float32 register solver, rows of 16-byte multiples up to 128 factors (beyond: the trainer has padded
          // them), strictly fewer blocks than the primal form, at most 5 blocks up to 128 factors and 12 beyond;
          // YCNR_DUAL_MAX_BLOCKS lowers the limit and never raises it
          for (int env = -1; env <= 14; ++env) {
            Toggles t;
            t.dualMaxBlocks = env;
            int want = 0;
            if (!f64 && !lds && !noDual && !(k <= 128 && k % 4 != 0)) {
              int most = k > 128 ? 12 : 5;
              if (env >= 0 && env < most) most = env;
              want = 16 * (most < nb - 1 ? most : nb - 1);
            }
            CHECK(dual_max_ratings(s, t) == want);
          }
          // graph replay: one piece, no exchange, own stream, one-wave path, 256 K <= ratings < 2 M, nothing switched off
          for (int g = 0; g < 32; ++g) {
            Toggles t;
            t.noOverlap = g & 1, t.noGraph = g & 2;
            const bool exchange = g & 4, own = g & 8;
            const size_t nParts = g & 16 ? 2 : 1;
            const int64_t ratings[6] = {0, 256 * 1024 - 1, 256 * 1024, 1000209, 2 * 1024 * 1024 - 1, 2 * 1024 * 1024};
            for (int64_t r : ratings) {
              const bool want = !exchange && nParts == 1 && own && k <= 128 && r >= 256 * 1024 && r < 2 * 1024 * 1024 && !noOverlap && !noGraph &&
                                !t.noOverlap && !t.noGraph;
              CHECK(graphable(s, t, exchange, nParts, r, own) == want);
            }
          }
          // side streams for the dual classes: from 1024 dual rows on (any, in a captured half-step), never on the any-k path,
          // never in order, never with overlap switched off
          for (int g = 0; g < 8; ++g) {
            Toggles t;
            t.noOverlap = g & 1;
            const bool captured = g & 2, inOrder = g & 4;
            const int64_t dualRows[5] = {0, 1, 1023, 1024, 500000};
            const bool anyK = k > 128 && (f64 || k % 4 != 0);
            for (int64_t d : dualRows) {
              const bool want = !anyK && (d >= 1024 || (captured && d > 0)) && !inOrder && !noOverlap && !t.noOverlap;
              CHECK(duals_on_side_streams(s, t, d, captured, inOrder) == want);
            }
          }
        }
      }
  // one case per quirk
  snprintf(g_case, sizeof g_case, "predicates literal");
  const Toggles t0;
  // the VALU edge from k = 20: not at 4 (one block), not at 132
  CHECK(!use_valu_edge({false, 4, 0, 1000}) && use_valu_edge({false, 20, 0, 1000}) && use_valu_edge({false, 116, 0, 1000}) && !use_valu_edge({false, 132, 0, 1000}));
  CHECK(!use_valu_edge({true, 20, 0, 1000}) && !use_valu_edge({false, 20, YCNR_FLAG_NO_VALU_EDGE, 1000}));
  // k = 100, 12.7 K items: x6, planes, plain slabs; 5.4 M users of k = 100 pass 2 GB: no x6, the edge layout in the slabs
  CHECK(use_slab_x6({false, 100, 0, 12700}) && use_planes({false, 100, 0, 12700}, t0) && slab_regs({false, 100, 0, 12700}) == 28 * 4 + 7);
  CHECK(!use_slab_x6({false, 100, 0, 5400000}) && slab_regs({false, 100, 0, 5400000}) == 21 * 4 + 6 + 24 + 8);
  // planes only for k % 4 == 0, k % 16 != 0, k <= 124
  CHECK(use_planes({false, 124, 0, 1000}, t0) && !use_planes({false, 128, 0, 1000}, t0) && !use_planes({false, 112, 0, 1000}, t0) &&
        !use_planes({false, 110, 0, 1000}, t0) && use_planes({false, 4, 0, 1000}, t0));
  // k = 100 packs its last block: 6 * 96 + 32 bytes per row, 64 MB hold 110376 rows
  CHECK(use_planes({false, 100, 0, 110376}, t0) && !use_planes({false, 100, 0, 110377}, t0));
  CHECK(!use_planes({false, 100, YCNR_FLAG_LDS_SOLVER, 1000}, t0));
  // dual classes: off for k <= 128 with k % 4 != 0, on beyond (rows padded by the trainer); one block has none
  CHECK(dual_max_ratings({false, 100, 0, 1}, t0) == 80 && dual_max_ratings({false, 102, 0, 1}, t0) == 0 && dual_max_ratings({false, 130, 0, 1}, t0) == 128);
  CHECK(dual_max_ratings({false, 16, 0, 1}, t0) == 0 && dual_max_ratings({false, 20, 0, 1}, t0) == 16 && dual_max_ratings({false, 64, 0, 1}, t0) == 48);
  CHECK(dual_max_ratings({false, 256, 0, 1}, t0) == 192 && dual_max_ratings({false, 512, 0, 1}, t0) == 192 && dual_max_ratings({false, 132, 0, 1}, t0) == 128);
  {
    Toggles t;
    t.dualMaxBlocks = 3;  // clamps
    CHECK(dual_max_ratings({false, 100, 0, 1}, t) == 48 && dual_max_ratings({false, 256, 0, 1}, t) == 48 && dual_max_ratings({false, 20, 0, 1}, t) == 16);
    t.dualMaxBlocks = 99;  // ... and never raises
    CHECK(dual_max_ratings({false, 100, 0, 1}, t) == 80 && dual_max_ratings({false, 256, 0, 1}, t) == 192);
    t.dualMaxBlocks = 0;
    CHECK(dual_max_ratings({false, 100, 0, 1}, t) == 0);
  }
  // the ML-100k shape (100 K ratings) runs launch by launch, ML-1M as a graph
  CHECK(!graphable({false, 20, 0, 1682}, t0, false, 1, 100000, true) && graphable({false, 100, 0, 3706}, t0, false, 1, 1000209, true));
  return n;
}

// ------------------------------------------------------------------------------------------------------------ plan params

static void test_plan_params() {
  snprintf(g_case, sizeof g_case, "plan params");
  const Toggles t0;
  const int64_t GB2 = (int64_t)2 << 30;
  // out of place: every row primal, no shuffle, split rows in row order; the path's chunk; arena slabs on the any-k path only
  for (int f64 = 0; f64 < 2; ++f64)
    for (int k = 1; k <= kMaxFactorsAny; ++k) {
      snprintf(g_case, sizeof g_case, "out of place f64=%d k=%d", f64, k);
      const PlanParams P = out_of_place_plan_params(f64 != 0, k, GB2);
      const int64_t nb = (k + 15) / 16;
      CHECK(P.dualMax == 0 && !P.shuffle && !P.sortSplit && P.k == k && P.maxSlabs == 64);
      if (k <= 128) CHECK(P.kind == kOneWave && P.chunk == 1024 && P.fusedMax == 0 && P.arenaSlabs == 0);
      else if (!f64 && k <= 256 && k % 4 == 0) CHECK(P.kind == kWorkgroup && P.chunk == 8192 && P.fusedMax == kWgFusedMax && P.arenaSlabs == 0);
      else {
        const int64_t slabBytes = (nb * (nb + 1) / 2 * 256 + nb * 16) * (f64 ? 8 : 4);
        CHECK(P.kind == kAnyK && P.chunk == 4096 && P.fusedMax == 0 && P.arenaSlabs == (GB2 / slabBytes > 1 ? GB2 / slabBytes : 1));
      }
    }
  snprintf(g_case, sizeof g_case, "resident plan params");
  // an arena smaller than a slab still holds one
  CHECK(out_of_place_plan_params(false, 4096, 1 << 20).arenaSlabs == 1);
  // resident, k = 100 float32, chunk left to the library: sized for the side; dual rows up to 80 ratings; kReal for the flops
  SideNnz mal;
  mal.nnz = 121500000, mal.splitNnz = 121000000;
  PlanParams P = resident_plan_params({false, 100, 0, 12700}, t0, 100, true, 1024, mal, true, GB2);
  CHECK(P.kind == kOneWave && P.chunk == 3072 && P.fusedMax == 1024 && P.maxSlabs == 64 && P.dualMax == 80 && P.k == 100 && P.shuffle && P.sortSplit &&
        P.arenaSlabs == 0);
  // ... an explicit chunk is the fused limit too
  P = resident_plan_params({false, 100, 0, 12700}, t0, 100, false, 32, mal, false, GB2);
  CHECK(P.chunk == 32 && P.fusedMax == 32 && !P.shuffle);
  // workgroup path, k = 130 padded to 132: long chunks, rows up to kWgFusedMax whole, 4096 slabs per row, k of the caller
  P = resident_plan_params({false, 132, 0, 12700}, t0, 130, true, 1024, mal, true, GB2);
  CHECK(P.kind == kWorkgroup && P.chunk == 8192 && P.fusedMax == kWgFusedMax && P.maxSlabs == 4096 && P.dualMax == 128 && P.k == 130 && P.arenaSlabs == 0);
  // ... with an explicit chunk (tests cut short rows with it)
  P = resident_plan_params({false, 132, 0, 12700}, t0, 130, false, 32, mal, true, GB2);
  CHECK(P.chunk == 32 && P.fusedMax == 32 && P.maxSlabs == 4096);
  // any-k path, float32 k = 512: a 541 KB image, the dual classes up to 192 ratings
  P = resident_plan_params({false, 512, 0, 12700}, t0, 512, true, 1024, mal, true, GB2);
  CHECK(P.kind == kAnyK && P.chunk == 4096 && P.fusedMax == 1024 && P.maxSlabs == 64 && P.dualMax == 192 && P.arenaSlabs == GB2 / ((528 * 256 + 512) * 4));
  // float64 k = 200: any-k, no dual classes
  P = resident_plan_params({true, 200, 0, 12700}, t0, 200, true, 1024, mal, true, (int64_t)8 << 20);
  CHECK(P.kind == kAnyK && P.dualMax == 0 && P.arenaSlabs == ((int64_t)8 << 20) / ((91 * 256 + 13 * 16) * 8));
  // YCNR_DUAL_MAX_BLOCKS reaches the plan
  Toggles t;
  t.dualMaxBlocks = 2;
  CHECK(resident_plan_params({false, 100, 0, 12700}, t, 100, true, 1024, mal, true, GB2).dualMax == 32);
}

// ------------------------------------------------------------------------------------------------------------- choose_gen

static bool pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

static long test_choose_gen() {
  long n = 0, refused = 0;
  for (int f64 = 0; f64 < 2; ++f64)
    for (int k = 129; k <= kMaxFactorsAny; ++k)
      for (int bits = 0; bits < 8; ++bits) {
        const size_t ts = f64 ? 8 : 4;
        const bool aligned = bits & 1;
        Toggles t;
        t.genRightLooking = bits & 2, t.noGenX6 = bits & 4;
        snprintf(g_case, sizeof g_case, "choose_gen ts=%zu k=%d aligned=%d right=%d noX6=%d", ts, k, aligned, t.genRightLooking, t.noGenX6);
        const GenChoice c = choose_gen(ts, k, aligned, t);
        ++n;
        const int nb = (k + 15) / 16, V = 16 / (int)ts;
        if (c.status != kGenOk) {
          // a refusal must be one: the loader of the Gramian has `slots` registers per thread of at most eight waves for the
          // loads of a panel, and the smallest panel has four ratings; the right-hand side of the solve fits up to k = 4096
          ++refused;
          const bool vec = aligned && k % V == 0;
          const int64_t loads4 = (int64_t)4 * (k / (vec ? V : 1));
          CHECK(c.status == kGenPanelTooLarge && (loads4 > (int64_t)(vec ? 4 : 8) * 64 * 8 || (size_t)2 * 4 * (nb * 16 + 64 + 1) * ts > 150 * 1024));
          continue;
        }
        CHECK(c.nb == nb);
        // 16-byte loads need rows of 16-byte multiples that start aligned
        CHECK(c.vec == (aligned && k % V == 0));
        // the panel: R ratings, a power of two in 4 ... 32, every load of it in a slot of some thread
        CHECK(pow2(c.R) && c.R >= 4 && c.R <= 32);
        CHECK((int64_t)c.R * (k / (c.vec ? V : 1)) <= (int64_t)c.slots * c.threads);
        CHECK(c.slots == (c.x6 || !c.vec ? 8 : 4));  // the loader's registers (als_gen_gram_kernel's MAXI)
        CHECK(c.P >= nb * 16 && c.P < nb * 16 + 64 && c.P % 16 == 0 && (c.P * (int)ts) % 256 == (ts == 4 ? 64 : 128));
        // two panel buffers of R rows of P + 1 elements
        CHECK(c.gramLds == (size_t)2 * c.R * (c.P + 1) * ts);
        CHECK(c.gramLds <= 150 * 1024);
        if (!c.x6 && c.R != 4) CHECK(c.gramLds <= 72 * 1024);
        // the workgroup: two to kGenGramMaxWaves waves
        CHECK(c.threads % 64 == 0 && c.threads >= 128 && c.threads <= 64 * kGenGramMaxWaves && kGenGramMaxWaves == 8);
        // bf16x6: float32 with 16-byte loads only, panels of 32 ratings, never when switched off
        if (c.x6) CHECK(ts == 4 && c.vec && c.R == 32 && !t.noGenX6);
        if (ts == 4 && c.vec && !t.noGenX6 && k <= 512) CHECK(c.x6);
        if (k > 512) CHECK(!c.x6);
        // the solves: the right-looking one keeps its panel in LDS up to 36 KB; the left-looking one float32 up to k = 512 in
        // two widths, float64 up to 256, never under YCNR_GEN_RIGHT_LOOKING
        CHECK(c.panelBytes == (size_t)nb * 256 * ts && c.panelLds == (c.panelBytes <= 36 * 1024));
        CHECK(c.solveLds <= 160 * 1024 && c.leftLds <= 160 * 1024);
        CHECK(c.left == (!t.genRightLooking && k <= (f64 ? 256 : 512)));
        if (c.left) {
          if (f64) CHECK(c.leftMaxc == 4 && c.leftPw == 2 && c.leftWaves == 4);
          else CHECK(c.leftMaxc == (k <= 256 ? 2 : 4) && c.leftPw == 4 && c.leftWaves == 8);
          CHECK(c.leftMaxc * c.leftWaves >= nb);  // MAXC column tiles per wave cover the row
        }
        // both solves: two 16 x 16 tile images (pitch 18 / 20), three vectors of 16 nb, 16 pivots, a 64-byte flag area;
        // + the panel (right-looking, in LDS) / PW x PW tiles (left-looking)
        const size_t common = (size_t)2 * 16 * (ts == 8 ? 18 : 20) + 3 * (size_t)nb * 16 + 16;
        CHECK(c.solveLds == (common + (c.panelLds ? (size_t)nb * 256 : 0)) * ts + 64);
        CHECK(c.leftLds == (common + (size_t)c.leftPw * c.leftPw * 256) * ts + 64);
      }
  // The refusals.  Four ratings of k factors in the loader's slots: 16-byte loads serve float32 up to k = 2048 and float64 up to
  // 1024, element loads up to 1024; a right-hand side beyond a CU's LDS only far beyond kMaxFactorsAny.
  snprintf(g_case, sizeof g_case, "choose_gen refusals");
  CHECK(refused > 0);
  CHECK(choose_gen(4, 2048, true, Toggles()).status == kGenOk && choose_gen(4, 2052, true, Toggles()).status == kGenPanelTooLarge);
  CHECK(choose_gen(4, 1024, false, Toggles()).status == kGenOk && choose_gen(4, 1025, false, Toggles()).status == kGenPanelTooLarge);
  CHECK(choose_gen(4, 2047, true, Toggles()).status == kGenPanelTooLarge);  // (not a 16-byte multiple: element loads)
  CHECK(choose_gen(8, 1024, true, Toggles()).status == kGenOk && choose_gen(8, 1026, true, Toggles()).status == kGenPanelTooLarge);
  CHECK(choose_gen(8, 16 * 430, true, Toggles()).status == kGenRhsTooLarge);
  // the edges the comments name
  snprintf(g_case, sizeof g_case, "choose_gen literal");
  const Toggles t0;
  GenChoice c = choose_gen(4, 512, true, t0);  // bf16x6: panels of 32 ratings, eight waves, the wide left-looking solve
  CHECK(c.status == kGenOk && c.x6 && c.vec && c.R == 32 && c.slots == 8 && c.threads == 512 && c.P == 528 && c.gramLds == 2 * 32 * 529 * 4);
  CHECK(c.left && c.leftMaxc == 4 && c.leftPw == 4 && c.leftWaves == 8 && c.panelLds && c.panelBytes == 32768);
  c = choose_gen(4, 516, true, t0);  // float32 MFMA, the right-looking solve with its panel in LDS
  CHECK(c.status == kGenOk && !c.x6 && c.vec && c.slots == 4 && !c.left && c.panelLds && c.R == 8 && c.threads == 512);
  c = choose_gen(4, 513, true, t0);  // not vectorised: element loads, eight slots
  CHECK(c.status == kGenOk && !c.x6 && !c.vec && c.slots == 8 && !c.left && c.R == 4);
  c = choose_gen(4, 512, false, t0);  // a fixed matrix that is not 16-byte aligned: element loads too
  CHECK(c.status == kGenOk && !c.x6 && !c.vec && c.left);
  c = choose_gen(4, 260, true, t0);  // the narrow left-looking solve ends at 256
  CHECK(c.left && c.leftMaxc == 4 && c.x6);
  c = choose_gen(8, 256, true, t0);  // float64: 2 x 4 tiles per wave, 20 rectangles in three passes of seven waves
  CHECK(c.status == kGenOk && c.left && c.leftMaxc == 4 && c.leftPw == 2 && c.leftWaves == 4 && c.threads == 7 * 64 && !c.x6 && c.vec && c.panelLds);
  c = choose_gen(8, 272, true, t0);  // ... beyond: right-looking, its panel (17 x 2 KB) still in LDS; from 18 blocks on in global memory
  CHECK(c.status == kGenOk && !c.left && c.panelLds && !choose_gen(8, 304, true, t0).panelLds);
  c = choose_gen(4, kMaxFactorsAny, true, t0);  // the largest k: refused by the loader's slots, not by LDS
  CHECK(c.status == kGenPanelTooLarge && (size_t)2 * 4 * (c.P + 1) * 4 <= 150 * 1024 && c.solveLds <= 160 * 1024 && !c.panelLds && !c.left);
  CHECK(choose_gen(8, kMaxFactorsAny, true, t0).status == kGenPanelTooLarge);
  c = choose_gen(4, 2048, true, t0);  // the largest float32 k served: panels of four ratings in 64 KB, the solve's panel in global memory
  CHECK(c.status == kGenOk && c.R == 4 && c.vec && !c.x6 && c.threads == 512 && !c.panelLds && !c.left && c.gramLds == 2 * 4 * 2065 * 4);
  {
    Toggles t;
    t.genRightLooking = true;
    CHECK(!choose_gen(4, 512, true, t).left && !choose_gen(8, 200, true, t).left);
    Toggles u;
    u.noGenX6 = true;
    c = choose_gen(4, 512, true, u);
    CHECK(!c.x6 && c.vec && c.slots == 4 && c.R == 16);
  }
  return n;
}

int main() {
  const long np = test_path();
  CHECK(np == 2 * 4096);
  const long nq = test_predicates();
  CHECK(nq == 2L * 256 * 64 * 8);
  test_plan_params();
  const long ng = test_choose_gen();
  CHECK(ng == 2L * (4096 - 128) * 8);
  printf("step_policy_test: ok (%ld paths, %ld shapes, %ld any-k launches)\n", np, nq, ng);
  return 0;
}
