// CPU test of csrc/rank_plan.h (tests/test_rank_plan.py builds this with the host sanitizers and runs it): how the held-out
// lists of a ranking request are cut into slots, and the sizes the kernel shares with the host.
#undef NDEBUG
#include "rank_plan.h"

#include <cassert>
#include <cstdio>

using namespace ycnr;

int main() {
  // users with 0, 1, 64, 65, 130 and 0 held-out items: 0 + 1 + 1 + 2 + 3 + 0 slots
  const int64_t ptr[] = {0, 0, 1, 65, 130, 260, 260};
  const std::vector<RankSlot> s = rank_cut_slots(6, ptr);
  const int32_t user[] = {1, 2, 3, 3, 4, 4, 4}, count[] = {1, 64, 64, 1, 64, 64, 2};
  assert(s.size() == 7);
  int64_t next = 0;  // every target exactly once, in order
  for (size_t i = 0; i < s.size(); ++i) {
    assert(s[i].begin == next && s[i].user == user[i] && s[i].count == count[i]);
    assert(s[i].begin >= ptr[s[i].user] && s[i].begin + s[i].count <= ptr[s[i].user + 1]);
    next += s[i].count;
  }
  assert(next == 260);
  assert(rank_cut_slots(0, ptr).empty());
  // factorsCount <= 256 is served in both precisions; the bounds the header states
  assert(rank_lds_bytes(100, 4) == 16 * 112 * 4 + 20544 && rank_lds_bytes(256, 8) == 16 * 256 * 8 + 28736);
  assert(rank_supported(256, 4) && rank_supported(256, 8));
  assert(rank_supported(688, 4) && !rank_supported(689, 4) && rank_supported(272, 8) && !rank_supported(273, 8));
  // parts: few slots spread the catalogue over the chip (at least 16 tiles each), many slots need no split
  assert(rank_parts(3, 1234, 256) == 5 && rank_parts(16 * 4096, 1234, 256) == 1 && rank_parts(16 * 512, 100000, 256) == 2);
  assert(rank_parts(1, 5, 256) == 1);
  printf("rank_plan_test: ok\n");
  return 0;
}
