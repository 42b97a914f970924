// CPU test of csrc/foldin_plan.h (tests/test_foldin_plan.py builds this with the host sanitizers and runs it): which rows of an
// implicit fold-in request go the dual way, that the three lists partition the request, and the LDS sizes DESIGN.md 16 states.
#undef NDEBUG
#include "foldin_plan.h"

#include <cassert>
#include <cstdio>

using namespace ycnr;

int main() {
  for (int k : {7, 20, 100, 128}) {
    // n = 0, 1, 32, 33, k, k + 1, each once with values 1.. and once with one negative value
    const int64_t lens[] = {0, 1, 32, 33, k, k + 1};
    std::vector<int64_t> ptr{0};
    std::vector<float> vals;
    for (int neg = 0; neg < 2; ++neg)
      for (int64_t n : lens) {
        for (int64_t q = 0; q < n; ++q) vals.push_back(neg && q == n / 2 ? -0.25f : (float)(q % 5));  // (zeros are served)
        ptr.push_back(ptr.back() + n);
      }
    const int64_t nRows = (int64_t)ptr.size() - 1;
    FoldCut cut;
    fold_cut<float>(nRows, ptr.data(), vals.data(), k, false, cut);
    std::vector<int> seen(nRows, 0);
    for (int32_t r : cut.dual) {
      const int64_t n = ptr[r + 1] - ptr[r];
      assert(r < 6 && n >= 1 && n <= 32 && n <= k);  // never a row with a negative value
      ++seen[r];
    }
    for (int32_t r : cut.empty) assert(ptr[r + 1] == ptr[r]), ++seen[r];
    for (const Unit &u : cut.primal) {
      const int64_t n = u.end - u.beg;
      assert(u.beg == ptr[u.row] && u.end == ptr[u.row + 1] && u.slab == -1 && n > 0);
      assert(u.row >= 6 || n > 32 || n > k);
      ++seen[u.row];
    }
    for (int64_t r = 0; r < nRows; ++r) assert(seen[r] == 1);
    assert(cut.empty.size() == 2 && cut.dual.size() + cut.primal.size() == (size_t)nRows - 2);
    for (int neg = 0; neg < 2; ++neg)
      for (int64_t n : lens) assert(fold_row_is_dual(n, k, !neg) == (!neg && n >= 1 && n <= 32 && n <= k));
    // primal only: the same units, no dual row; the vectors are reused
    fold_cut<float>(nRows, ptr.data(), vals.data(), k, true, cut);
    assert(cut.dual.empty() && cut.empty.size() == 2 && cut.primal.size() == (size_t)nRows - 2);
  }
  const double nan = __builtin_nan("");
  const int64_t one[] = {0, 1};
  FoldCut cut;
  fold_cut<double>(1, one, &nan, 20, false, cut);  // !(r >= 0): primal
  assert(cut.dual.empty() && cut.primal.size() == 1);
  // the sizes DESIGN.md 16 states
  assert(fold_dual_lds_bytes(128) == 47360 && fold_dual_lds_bytes(100) == 39040 && fold_dual_lds_bytes(64) == 30464 && fold_dual_lds_bytes(7) == 13696);
  assert(fold_factor_lds_bytes(128) == 148480 && fold_factor_lds_bytes(100) == 115584);
  assert(fold_dual_ld(128) == 144 && fold_dual_ld(112) == 112);
  printf("foldin_plan_test: ok\n");
  return 0;
}
