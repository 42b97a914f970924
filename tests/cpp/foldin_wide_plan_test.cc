// CPU test of csrc/foldin_wide_plan.h (tests/test_foldin_wide_plan.py builds this with the host sanitizers and runs it): the cut
// of a request of ycnr_als_fold_in_implicit_wide into its four lists, and the LDS sizes DESIGN.md 16 states.
#undef NDEBUG
#include "foldin_wide_plan.h"

#include <cassert>
#include <cstdio>

using namespace ycnr;

int main() {
  // the lengths of tests/test_gpu_fold_in_implicit_wide.py; the last row has a negative value, the one before it a NaN
  const int64_t lens[] = {0, 1, 15, 16, 17, 32, 33, 64, 100, 127, 128, 129, 5, 3};
  std::vector<int64_t> ptr{0};
  std::vector<double> vals;
  for (int64_t n : lens) {
    for (int64_t q = 0; q < n; ++q) vals.push_back((double)(q % 5));  // (zeros are served)
    ptr.push_back(ptr.back() + n);
  }
  vals[ptr[12] + 2] = -0.25;
  vals[ptr[13] + 1] = __builtin_nan("");
  FoldWideCut cut;
  for (int pass = 0; pass < 2; ++pass) {  // the vectors are reused
    fold_wide_cut<double>(14, ptr.data(), vals.data(), cut);
    assert((cut.empty == std::vector<int32_t>{0}));
    assert((cut.shortRows == std::vector<int32_t>{1, 2, 3, 4, 5}));
    assert((cut.longRows == std::vector<int32_t>{6, 7, 8, 9, 10}));
    assert((cut.notServed == std::vector<int32_t>{11, 12, 13}));
  }
  assert(fold_wide_row_is_served(128, true) && !fold_wide_row_is_served(129, true) && !fold_wide_row_is_served(0, true) &&
         !fold_wide_row_is_served(5, false));
  // the sizes DESIGN.md 16 states
  assert(fold_wide_image_ld(129) == 192 && fold_wide_image_ld(512) == 512 && fold_wide_image_bytes(512) == 2097152);
  assert(fold_wide_np(17) == 32 && fold_wide_pld(32) == 48 && fold_wide_pld(128) == 144 && fold_wide_pld(16) == 16);
  assert(fold_wide_lds_bytes(32, 128) == 22144 && fold_wide_lds_bytes(32, 256) == 24192 && fold_wide_lds_bytes(32, 512) == 28288);
  assert(fold_wide_lds_bytes(128, 128) == 119296 && fold_wide_lds_bytes(128, 256) == 121344 && fold_wide_lds_bytes(128, 512) == 125440);
  assert(fold_wide_lds(128, 512).panel == 36 * 256 && fold_wide_lds(32, 512).panel == 3 * 256);
  printf("foldin_wide_plan_test: ok\n");
  return 0;
}
