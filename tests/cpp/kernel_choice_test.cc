// CPU test of csrc/kernel_choice.h, the host-only rules that pick the kernels of a half-step at k <= 128
// (tests/test_kernel_choice.py builds this with the host sanitizers and runs it).  Every expectation below is written out from
// the rules as independent statements, none is captured from the code under test.
#include "kernel_choice.h"

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
static char g_case[160] = "";

struct In {
  bool f64;
  int k;
  bool ldsSolver, edge, x6, hasPlanes, fewSlabs, noX6d, noFusedX6d, noPk3;
};
static KernelChoice choose(const In &i) {
  snprintf(g_case, sizeof g_case, "f64=%d k=%d lds=%d edge=%d x6=%d planes=%d few=%d noX6d=%d noFusedX6d=%d noPk3=%d", i.f64, i.k, i.ldsSolver,
           i.edge, i.x6, i.hasPlanes, i.fewSlabs, i.noX6d, i.noFusedX6d, i.noPk3);
  return choose_kernels(i.f64, i.k, i.ldsSolver, i.edge, i.x6, i.hasPlanes, i.fewSlabs, i.noX6d, i.noFusedX6d, i.noPk3);
}
static bool same(const KernelChoice &a, const KernelChoice &b) {
  return a.nb == b.nb && a.ldsSolver == b.ldsSolver && a.chunk == b.chunk && a.chunkEdge == b.chunkEdge && a.chunkPadRhs == b.chunkPadRhs &&
         a.chunkPk3 == b.chunkPk3 && a.row == b.row && a.rowEdge == b.rowEdge && a.rowE4 == b.rowE4 && a.rowPadRhs == b.rowPadRhs &&
         a.rowPk3 == b.rowPk3 && a.rowPack == b.rowPack && a.reduceEdge == b.reduceEdge && a.reduceE4 == b.reduceE4 &&
         a.reduceFew == b.reduceFew && a.bandE4 == b.bandE4 && a.rowLdsImage == b.rowLdsImage;
}

// the rules, over every input
static long test_rules() {
  long n = 0;
  for (int k = 1; k <= 128; ++k)
    for (int bits = 0; bits < 512; ++bits) {
      const In i = {(bits & 1) != 0, k, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0,
                    (bits & 128) != 0, (bits & 256) != 0};
      const KernelChoice c = choose(i);
      ++n;
      const int nb = (k + 15) / 16;
      const bool first4 = k == 16 * (nb - 1) + 4;
      CHECK(c.nb == nb && c.ldsSolver == i.ldsSolver);
      // a field belongs to one form of its kernel
      if (c.chunk != kGramMfma) CHECK(!c.chunkEdge);
      if (c.chunk != kGramX6D) CHECK(!c.chunkPadRhs && !c.chunkPk3);
      if (c.row != kGramMfma) CHECK(!c.rowEdge);
      if (c.row != kGramX6D) CHECK(!c.rowPadRhs && !c.rowPk3);
      if (c.row != kGramPlanes) CHECK(!c.rowPack);
      CHECK(c.chunk != kGramPlanes && c.row != kGramX6);
      CHECK(c.rowLdsImage == (c.row != kGramPlanes));  // the planes kernel has no dynamic LDS
      // float64: the MFMA kernels alone
      if (i.f64) {
        CHECK(c.chunk == kGramMfma && c.row == kGramMfma);
        CHECK(!c.chunkEdge && !c.rowEdge && !c.reduceEdge && !c.rowE4 && !c.reduceE4 && !c.bandE4 && !c.reduceFew);
        continue;
      }
      // rows that are not 16 bytes long: neither x6d nor planes, but still the plain x6 chunk kernel
      if (k % 4 != 0) {
        CHECK(c.chunk != kGramX6D && c.row == kGramMfma);
        CHECK((c.chunk == kGramX6) == i.x6);
      }
      CHECK((c.chunk != kGramMfma) == i.x6);
      if (k % 16 == 0) CHECK(!c.chunkPadRhs && !c.rowPadRhs && !c.chunkPk3 && !c.rowPk3 && !c.rowE4 && !c.reduceE4 && !c.bandE4 && c.row != kGramPlanes);
      if (c.chunk == kGramX6D) CHECK(c.chunkPadRhs == (k % 16 != 0));
      if (c.row == kGramX6D) CHECK(c.rowPadRhs == (k % 16 != 0));
      // e4: float32, register solver, two blocks or more, four columns in the last one -- in all three solving kernels
      const bool e4 = !i.ldsSolver && nb >= 2 && first4;
      CHECK(c.rowE4 == e4 && c.reduceE4 == e4 && c.bandE4 == e4);
      // pk3: x6d at k = 16 (nb - 1) + 4 (one block included) unless switched off
      CHECK(c.chunkPk3 == (c.chunk == kGramX6D && first4 && !i.noPk3));
      CHECK(c.rowPk3 == (c.row == kGramX6D && first4 && !i.noPk3));
      // planes
      const bool planes = i.x6 && i.hasPlanes && !i.ldsSolver && k % 4 == 0 && 16 * (nb - 1) < k && k < 16 * nb;
      CHECK((c.row == kGramPlanes) == planes);
      if (planes) CHECK(c.rowPack == (nb >= 2 && first4));
      // x6d and its toggles: noX6d takes it from both kernels, noFusedX6d from the row kernel only; no x6d row kernel for
      // eight blocks with the LDS solver
      CHECK((c.chunk == kGramX6D) == (i.x6 && k % 4 == 0 && !i.noX6d));
      if (!planes) CHECK((c.row == kGramX6D) == (i.x6 && k % 4 == 0 && !i.noX6d && !i.noFusedX6d && !(i.ldsSolver && nb == 8)));
      if (i.ldsSolver && nb == 8) CHECK(c.row == kGramMfma);
      // the VALU edge: from two blocks on, in the MFMA row kernel whatever x6 says, in chunk, reduce and band reduce only without x6
      const bool edge = i.edge && nb >= 2;
      if (c.row == kGramMfma) CHECK(c.rowEdge == edge);
      CHECK(c.reduceEdge == (edge && !i.x6) && c.chunkEdge == (edge && !i.x6));
      CHECK(c.reduceFew == (i.fewSlabs && !i.ldsSolver));
    }
  return n;
}

// one case per quirk, the expected choice written out
static void test_literal() {
  KernelChoice w;
  // eight blocks, LDS solver, x6: the chunks go through x6d, the row kernel stays float32-MFMA
  w = KernelChoice{};
  w.nb = 8, w.ldsSolver = true, w.chunk = kGramX6D, w.row = kGramMfma, w.rowLdsImage = true;
  CHECK(same(choose({false, 128, true, false, true, false, false, false, false, false}), w));
  // ... and k = 116 likewise, with the padded right-hand side and PK3 in the chunk kernel
  w.chunkPadRhs = w.chunkPk3 = true;
  CHECK(same(choose({false, 116, true, false, true, false, false, false, false, false}), w));
  // edge and x6 together (k = 20): x6d everywhere, the reduce is NOT the edge form
  w = KernelChoice{};
  w.nb = 2, w.chunk = kGramX6D, w.chunkPadRhs = w.chunkPk3 = true, w.row = kGramX6D, w.rowPadRhs = w.rowPk3 = w.rowE4 = true;
  w.reduceE4 = w.bandE4 = true, w.reduceFew = true, w.rowLdsImage = true;
  CHECK(same(choose({false, 20, false, true, true, false, true, false, false, false}), w));
  // ... with YCNR_NO_FUSED_X6D the row kernel is the MFMA one WITH the edge, the reduce still without
  w.row = kGramMfma, w.rowPadRhs = w.rowPk3 = false, w.rowEdge = true;
  CHECK(same(choose({false, 20, false, true, true, false, true, false, true, false}), w));
  // edge without x6 (k = 36): the edge form in all four
  w = KernelChoice{};
  w.nb = 3, w.chunk = kGramMfma, w.chunkEdge = true, w.row = kGramMfma, w.rowEdge = w.rowE4 = true;
  w.reduceEdge = w.reduceE4 = w.bandE4 = true, w.rowLdsImage = true;
  CHECK(same(choose({false, 36, false, true, false, false, false, false, false, false}), w));
  // the planes row kernel at k = 100 = 16 * 6 + 4: packed, edge-first solve, no dynamic LDS; chunks x6d
  w = KernelChoice{};
  w.nb = 7, w.chunk = kGramX6D, w.chunkPadRhs = w.chunkPk3 = true, w.row = kGramPlanes, w.rowPack = w.rowE4 = true;
  w.reduceE4 = w.bandE4 = true, w.rowLdsImage = false;
  CHECK(same(choose({false, 100, false, false, true, true, false, false, false, false}), w));
  // ... the planes kernel does not look at YCNR_NO_X6D; the chunks fall to plain x6
  w.chunk = kGramX6, w.chunkPadRhs = w.chunkPk3 = false;
  CHECK(same(choose({false, 100, false, false, true, true, false, true, false, false}), w));
  // one block, k = 4: PK3 without the edge-first solve
  w = KernelChoice{};
  w.nb = 1, w.chunk = kGramX6D, w.chunkPadRhs = w.chunkPk3 = true, w.row = kGramX6D, w.rowPadRhs = w.rowPk3 = true, w.rowLdsImage = true;
  CHECK(same(choose({false, 4, false, false, true, false, false, false, false, false}), w));
  // k % 4 != 0 with x6: the plain x6 chunk kernel, MFMA rows
  w = KernelChoice{};
  w.nb = 1, w.chunk = kGramX6, w.row = kGramMfma, w.rowLdsImage = true;
  CHECK(same(choose({false, 10, false, false, true, true, false, false, false, false}), w));
  // what a caller without flags gets (the portion API) at k = 36: float32-MFMA, no edge, but the edge-first solve
  w = KernelChoice{};
  w.nb = 3, w.chunk = kGramMfma, w.row = kGramMfma, w.rowE4 = w.reduceE4 = w.bandE4 = true, w.rowLdsImage = true;
  CHECK(same(choose({false, 36, false, false, false, false, false, false, false, false}), w));
  // float64 with everything asked for
  w = KernelChoice{};
  w.nb = 7, w.ldsSolver = true, w.chunk = kGramMfma, w.row = kGramMfma, w.rowLdsImage = true;
  CHECK(same(choose({true, 100, true, true, true, true, true, false, false, false}), w));
}

int main() {
  const long n = test_rules();
  CHECK(n == 128 * 512);
  test_literal();
  printf("kernel_choice_test: ok (%ld inputs)\n", n);
  return 0;
}
