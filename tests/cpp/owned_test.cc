// CPU test of csrc/owned.h, the move-only owner and the grow-only buffer that hold every device buffer, event and stream of
// ycnr_als.hip (tests/test_owned.py builds this with the host sanitizers and runs it).  The policies here count: every handle
// is a heap cell with its id, Free logs the id and deletes the cell, so a handle freed twice or never is caught both by the
// counts below and by the address sanitizer.
#include "owned.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

using namespace ycnr;

#define CHECK(...)                                                  \
  do {                                                              \
    if (!(__VA_ARGS__)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

// ------------------------------------------------------------------------------------------------------------------ Owned

static std::vector<int> g_freed;  // ids in the order Free saw them
static int g_made = 0;
static int *make() { return new int(g_made++); }
struct CountingFree {
  void operator()(int *p) const {
    CHECK(p != nullptr);  // an empty owner never calls Free
    g_freed.push_back(*p);
    delete p;
  }
};
using Own = Owned<int *, CountingFree>;

static int times_freed(int id) {
  int n = 0;
  for (int f : g_freed) n += f == id;
  return n;
}
// every handle made so far has been freed exactly once
static void check_all_freed_once() {
  CHECK((int)g_freed.size() == g_made);
  for (int id = 0; id < g_made; ++id) CHECK(times_freed(id) == 1);
}

struct PartLike {  // a stand-in for Part: several owners and plain data, no special member of its own
  Own a, b, c[3];
  int tag = 0;
  void fill() {
    a.reset(make()), b.reset(make());
    for (Own &o : c) *o.put() = make();
  }
};

static_assert(!std::is_copy_constructible<Own>::value && !std::is_copy_assignable<Own>::value, "Owned must not copy");
static_assert(std::is_nothrow_move_constructible<Own>::value && std::is_nothrow_move_assignable<Own>::value, "Owned moves, nothrow");
static_assert(!std::is_copy_constructible<PartLike>::value && !std::is_copy_assignable<PartLike>::value, "a struct of owners must not copy");
static_assert(std::is_nothrow_move_constructible<PartLike>::value, "a struct of owners moves, nothrow (std::vector relies on it)");

static void test_owned() {
  {  // empty owners: Free is never called (CountingFree fails on null), whatever is done to them
    Own e, f;
    CHECK(!e && e.get() == nullptr);
    e.reset();
    CHECK(e.put() != nullptr && e.release() == nullptr);
    f = std::move(e);
    Own g(std::move(f));
    CHECK(!g);
  }
  CHECK(g_freed.empty());
  {  // destructor
    Own a(make());
    CHECK(a && *a.get() == 0 && g_freed.empty());
  }
  check_all_freed_once();
  {  // move construction: the source is left empty, one free at the end
    Own a(make());
    const int *was = a.get();
    Own b(std::move(a));
    CHECK(!a && b.get() == was && times_freed(1) == 0);
  }
  check_all_freed_once();
  {  // move assignment onto an occupied owner: the old handle is freed at that moment, the new one later
    Own a(make()), b(make());  // ids 2, 3
    b = std::move(a);
    CHECK(times_freed(3) == 1 && times_freed(2) == 0 && !a && *b.get() == 2);
  }
  check_all_freed_once();
  {  // self-move-assignment keeps the handle
    Own a(make());  // id 4
    Own &same = a;
    a = std::move(same);
    CHECK(a && *a.get() == 4 && times_freed(4) == 0);
  }
  check_all_freed_once();
  {  // put() on an occupied owner frees what was held and hands out the slot
    Own a(make());  // id 5
    int **slot = a.put();
    CHECK(times_freed(5) == 1 && *slot == nullptr && !a);
    *slot = make();  // id 6, as an out-parameter would
    CHECK(a && *a.get() == 6);
  }
  check_all_freed_once();
  {  // reset(): to another handle, then to empty
    Own a(make());  // id 7
    a.reset(make());  // id 8
    CHECK(times_freed(7) == 1 && times_freed(8) == 0 && *a.get() == 8);
    a.reset();
    CHECK(times_freed(8) == 1 && !a);
  }
  check_all_freed_once();
  {  // release() frees nothing: the handle is the caller's again
    Own a(make());  // id 9
    int *raw = a.release();
    CHECK(!a && times_freed(9) == 0);
    { Own gone(std::move(a)); }
    CHECK(times_freed(9) == 0);
    CountingFree{}(raw);
  }
  check_all_freed_once();
}

static void test_vector_of_owners() {
  const int first = g_made;
  {
    std::vector<PartLike> v(2);
    for (PartLike &p : v) p.fill();  // 5 handles each
    CHECK(g_made == first + 10);
    const size_t cap0 = v.capacity();
    while (v.capacity() == cap0) {  // growth that reallocates: the elements move, nothing is freed
      v.emplace_back();
      v.back().fill();
    }
    const int afterGrowth = g_made;
    CHECK((int)g_freed.size() == first);
    v.resize(v.size() + 3);  // up: empty elements
    CHECK((int)g_freed.size() == first && g_made == afterGrowth);
    v.resize(v.size() - 3);  // down over the empty ones: still nothing
    CHECK((int)g_freed.size() == first);
    const int lastA = *v.back().a.get();
    v.resize(v.size() - 1);  // down over a filled one: its five handles, now
    CHECK((int)g_freed.size() == first + 5 && times_freed(lastA) == 1);
    {
      std::vector<PartLike> w(1);  // a staged upload swapped in: the previous one is freed where `w` ends, not before
      w[0].fill();
      const int staged = *w[0].a.get();
      const size_t before = g_freed.size();
      v.swap(w);
      CHECK(g_freed.size() == before && v.size() == 1 && *v[0].a.get() == staged);
    }
    CHECK((int)g_freed.size() == g_made - 5);  // everything but the one swapped in
    v.clear();
    check_all_freed_once();
  }
  check_all_freed_once();
}

// ------------------------------------------------------------------------------------------------------------------ GrowBuf

struct Op {
  char what;  // 'a' alloc, 'f' free
  size_t size;
  void *p;
};
static std::vector<Op> g_ops;
static int g_failNext = 0;  // the next alloc returns this code (once)
struct CountingAlloc {
  static int alloc(size_t n, void **p) {
    if (g_failNext) {
      const int e = g_failNext;
      g_failNext = 0;
      *p = reinterpret_cast<void *>(0x10);  // what a failed allocator may leave behind: must not be kept or freed
      g_ops.push_back(Op{'a', n, nullptr});
      return e;
    }
    *p = malloc(n ? n : 1);
    g_ops.push_back(Op{'a', n, *p});
    return 0;
  }
  static void free(void *p) {
    g_ops.push_back(Op{'f', 0, p});
    ::free(p);
  }
};
// the three growth rules of ycnr_als.hip, as the issue states them
struct ArenaRule : CountingAlloc {
  static size_t grow(size_t b) { return b + b / 2 > 4096 ? b + b / 2 : 4096; }
};
struct PinnedRule : CountingAlloc {
  static size_t grow(size_t b) { return b + b / 2; }
};
struct ExactRule : CountingAlloc {
  static size_t grow(size_t b) { return b; }
};

template <typename Rule>
static size_t cap_after(size_t bytes) {
  GrowBuf<Rule> g;
  CHECK(g.reserve(bytes) == 0);
  return g.cap();
}

static void test_growbuf() {
  static_assert(!std::is_copy_constructible<GrowBuf<ExactRule>>::value, "GrowBuf must not copy");
  static_assert(std::is_nothrow_move_constructible<GrowBuf<ExactRule>>::value, "GrowBuf moves, nothrow");
  {
    GrowBuf<ExactRule> g;
    CHECK(g.get() == nullptr && g.cap() == 0);
    CHECK(g.reserve(0) == 0 && g_ops.empty());  // nothing asked, nothing done
    CHECK(g.reserve(100) == 0 && g.cap() == 100 && g.get() != nullptr);
    CHECK(g_ops.size() == 1 && g_ops[0].what == 'a' && g_ops[0].size == 100);
    void *first = g.get();
    CHECK(g.reserve(100) == 0 && g.reserve(1) == 0 && g.reserve(99) == 0);  // within the capacity: no call
    CHECK(g_ops.size() == 1 && g.get() == first);
    CHECK(g.reserve(101) == 0 && g.cap() == 101);  // growth: the old block is freed BEFORE the new one is allocated
    CHECK(g_ops.size() == 3 && g_ops[1].what == 'f' && g_ops[1].p == first && g_ops[2].what == 'a' && g_ops[2].size == 101);
    // a failing alloc: the code comes back unchanged, the buffer is empty, and the old block was freed once
    void *second = g.get();
    g_failNext = 2;
    CHECK(g.reserve(500) == 2);
    CHECK(g.get() == nullptr && g.cap() == 0);
    CHECK(g_ops.size() == 5 && g_ops[3].what == 'f' && g_ops[3].p == second && g_ops[4].what == 'a' && g_ops[4].size == 500);
    g_failNext = 7;
    CHECK(g.reserve(8) == 7 && g_ops.size() == 6 && g.cap() == 0);  // (nothing to free this time)
    // ... and a later reserve works
    CHECK(g.reserve(8) == 0 && g.cap() == 8 && g.get() != nullptr && g_ops.size() == 7);
    GrowBuf<ExactRule> h(std::move(g));  // a move carries block and capacity
    CHECK(g.get() == nullptr && g.cap() == 0 && h.cap() == 8 && g_ops.size() == 7);
    g = std::move(h);
    CHECK(g.cap() == 8 && h.get() == nullptr && g_ops.size() == 7);
  }
  CHECK(g_ops.size() == 8 && g_ops[7].what == 'f');  // the destructor frees the last block; the sanitizer sees any other
  int allocs = 0, frees = 0;
  for (const Op &o : g_ops) allocs += o.what == 'a' && o.p, frees += o.what == 'f';
  CHECK(allocs == 3 && frees == 3);
  // the three rules, literal requests
  CHECK(cap_after<ArenaRule>(1) == 4096 && cap_after<ArenaRule>(2730) == 4096 && cap_after<ArenaRule>(2731) == 4096);
  CHECK(cap_after<ArenaRule>(2732) == 4098 && cap_after<ArenaRule>(4096) == 6144 && cap_after<ArenaRule>(32832) == 49248);
  CHECK(cap_after<ArenaRule>(1000001) == 1500001);
  CHECK(cap_after<PinnedRule>(1) == 1 && cap_after<PinnedRule>(2) == 3 && cap_after<PinnedRule>(4096) == 6144 && cap_after<PinnedRule>(1000001) == 1500001);
  CHECK(cap_after<ExactRule>(1) == 1 && cap_after<ExactRule>(4096) == 4096 && cap_after<ExactRule>(1000001) == 1000001);
}

int main() {
  test_owned();
  test_vector_of_owners();
  test_growbuf();
  printf("owned_test: ok (%d handles, %zu buffer calls)\n", g_made, g_ops.size());
  return 0;
}
