// CPU test of csrc/schedule.h, the host-only work-unit scheduler (tests/test_schedule.py builds this with the host sanitizers
// and runs it).  Every expectation below is written out from the scheduling rules, none is captured from the code under test.
#include "schedule.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>

using namespace ycnr;

#define CHECK(...)                                                              \
  do {                                                                          \
    if (!(__VA_ARGS__)) {                                                       \
      printf("FAIL %s:%d (%s): %s\n", __FILE__, __LINE__, g_case, #__VA_ARGS__); \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)
static const char *g_case = "";

struct Rng {
  uint64_t x;
  explicit Rng(uint64_t seed) : x(seed * 0x9E3779B97F4A7C15ull + 1) {}
  uint64_t next() {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return x;
  }
  int64_t below(int64_t n) { return (int64_t)(next() % (uint64_t)n); }
};

struct Side {
  std::vector<int64_t> ptr{0};
  std::vector<int32_t> indx;  // ascending in every row (ids may repeat: only their order matters to the scheduler)
  int64_t rows() const { return (int64_t)ptr.size() - 1; }
  int64_t len(int64_t r) const { return ptr[r + 1] - ptr[r]; }
  // a row of n ratings spread evenly over the columns [lo, hi)
  void add_row(int64_t n, int64_t lo, int64_t hi) {
    for (int64_t i = 0; i < n; ++i) indx.push_back((int32_t)(lo + (hi - lo) * i / std::max<int64_t>(n, 1)));
    ptr.push_back(ptr.back() + n);
  }
  // a row with counts[j] ratings in band j (columns [j W, (j + 1) W))
  void add_banded_row(const std::vector<int64_t> &counts, int64_t W) {
    int64_t n = 0;
    for (size_t j = 0; j < counts.size(); ++j) {
      for (int64_t i = 0; i < counts[j]; ++i) indx.push_back((int32_t)(j * W + W * i / counts[j]));
      n += counts[j];
    }
    ptr.push_back(ptr.back() + n);
  }
};

// row lengths that straddle every threshold of a chunk length: the fused limit, the 4-alignment, the slab limit
static Side random_side(uint64_t seed, int64_t nRows, int chunk, int64_t cols) {
  Rng g(seed);
  Side s;
  const int64_t edges[] = {0, 1, 3, 4, 5, 15, 16, 17, 80, 81, chunk - 1, chunk, chunk + 1, chunk + 4, 2 * chunk, 2 * chunk + 1, 3 * chunk - 3,
                           63 * (int64_t)chunk, 64 * (int64_t)chunk, 64 * (int64_t)chunk + 1, 65 * (int64_t)chunk + 7};
  for (int64_t r = 0; r < nRows; ++r) {
    const int u = (int)g.below(10);
    int64_t n = u < 1 ? 0 : u < 5 ? g.below(2 * chunk + 2) : u < 8 ? edges[g.below((int64_t)(sizeof edges / sizeof edges[0]))] : g.below(12 * (int64_t)chunk);
    if (n > 70000) n = 70000 - g.below(100);
    s.add_row(n, 0, cols);
  }
  return s;
}

static std::vector<int64_t> answer(const BoundQueries &q, const Side &s, int64_t base) {
  std::vector<int64_t> out;
  const int32_t *indx = s.indx.data() + base;
  for (size_t i = 0; i < q.key.size(); ++i) out.push_back(std::lower_bound(indx + q.beg[i], indx + q.end[i], q.key[i]) - indx);
  return out;
}

// The properties every plan of rows [rowBegin, rowBegin + nRows) has.  aligned: unit bounds are multiples of 4 away from the
// row start, except at the row end (band-major plans cut at the band boundaries too: checked there).
static void check_plan(const PiecePlan &p, const Side &s, int64_t rowBegin, int64_t nRows, const PlanParams &P, bool aligned) {
  const int64_t base = s.ptr[rowBegin], nnz = s.ptr[rowBegin + nRows] - base;
  std::vector<char> seen((size_t)nnz, 0), slabUsed((size_t)p.nSlabs, 0);
  std::map<int32_t, std::vector<int32_t>> slabsOfRow;
  CHECK((int64_t)p.units.size() >= p.nSlabs);
  for (size_t i = 0; i < p.units.size(); ++i) {
    const Unit &u = p.units[i];
    CHECK(u.row >= rowBegin && u.row < rowBegin + nRows);
    const int64_t rb = s.ptr[u.row] - base, re = s.ptr[u.row + 1] - base;
    CHECK(u.beg < u.end && u.beg >= rb && u.end <= re);  // inside its row and not empty: empty rows are in no unit
    for (int64_t j = u.beg; j < u.end; ++j) {
      CHECK(!seen[(size_t)j]);
      seen[(size_t)j] = 1;
    }
    if ((int64_t)i < p.nSlabs) {  // a split chunk
      CHECK(u.slab >= 0 && u.slab < p.nSlabs && !slabUsed[(size_t)u.slab]);
      slabUsed[(size_t)u.slab] = 1;
      slabsOfRow[u.row].push_back(u.slab);
      if (aligned) CHECK((u.beg - rb) % 4 == 0 && ((u.end - rb) % 4 == 0 || u.end == re));
    } else {  // a whole row
      CHECK(u.slab < 0 && u.beg == rb && u.end == re);
    }
  }
  for (int64_t j = 0; j < nnz; ++j) CHECK(seen[(size_t)j]);  // every rating of every non-empty row is in exactly one unit
  int64_t solved = 0, fused = 0;
  for (int64_t r = rowBegin; r < rowBegin + nRows; ++r) solved += s.len(r) > 0;
  for (size_t i = (size_t)p.nSlabs; i < p.units.size(); ++i) fused += p.units[i].end - p.units[i].beg;
  CHECK(p.solvedRows == solved && p.fusedRatings == fused);
  CHECK(p.split.size() == slabsOfRow.size());
  int32_t most = 0;
  for (const SplitRow &sr : p.split) {
    std::vector<int32_t> &sl = slabsOfRow[sr.row];
    std::sort(sl.begin(), sl.end());
    CHECK(sr.n == s.len(sr.row) && sr.nslabs == (int32_t)sl.size() && sr.nslabs <= P.maxSlabs);
    for (int32_t i = 0; i < sr.nslabs; ++i) CHECK(sl[(size_t)i] == sr.slab0 + i);
    most = std::max(most, sr.nslabs);
  }
  CHECK(p.maxRowSlabs == most);
  // the dual classes
  int64_t rows = 0, ratings = 0, at = p.nSlabs + p.nPrimal;
  double flops = 0;
  for (int64_t i = p.nSlabs; i < (int64_t)p.units.size(); ++i) {
    const int64_t n = p.units[(size_t)i].end - p.units[(size_t)i].beg;
    CHECK((i < p.nSlabs + p.nPrimal) == (n > P.dualMax));  // the whole rows after nPrimal are exactly those with n <= dualMax
    if (n <= P.dualMax) {
      ++rows;
      ratings += n;
      // G = Y Y^T (symmetric): n (n + 1) k; Cholesky: n^3 / 3; the two triangular solves: 2 n^2; x = Y^T w: 2 n k
      flops += (double)n * (n + 1) * P.k + (double)n * n * n / 3.0 + 2.0 * n * n + 2.0 * n * P.k;
    }
  }
  CHECK(p.dualRows == rows && p.dualRatings == ratings && std::fabs(p.dualFlops - flops) <= 1e-12 * flops);
  for (int m = kMaxDualBlocks; m >= 0; --m) {  // contiguous runs in descending m = ceil(n / 16)
    if (!p.dualCount[m]) continue;
    CHECK(m >= 1 && m <= P.dualMax / 16 && p.dualFirst[m] == at);
    for (int64_t i = at; i < at + p.dualCount[m]; ++i) CHECK((p.units[(size_t)i].end - p.units[(size_t)i].beg + 15) / 16 == m);
    at += p.dualCount[m];
  }
  CHECK(at == (int64_t)p.units.size());
}

static PlanParams params(PathKind kind, int chunk) {
  PlanParams P;
  P.kind = kind;
  P.chunk = chunk;
  P.fusedMax = chunk;
  P.maxSlabs = kind == kWorkgroup ? kMaxSlabsPerRowBig : kMaxSlabsPerRow;
  P.dualMax = kind == kOneWave ? 80 : kind == kWorkgroup ? 192 : 176;
  P.k = 100;
  P.arenaSlabs = 40;
  return P;
}

static void test_coverage() {
  g_case = "coverage";
  for (int chunk : {8, 64, 1024})
    for (PathKind kind : {kOneWave, kWorkgroup, kAnyK})
      for (uint64_t seed = 1; seed <= (chunk == 1024 ? 1 : 3); ++seed) {  // (one side of 2 M ratings is enough)
        const Side s = random_side(seed * 100 + (uint64_t)chunk, 300, chunk, 5000);
        const PlanParams P = params(kind, chunk);
        check_plan(plan_piece(s.ptr.data(), 0, s.rows(), P), s, 0, s.rows(), P, true);
        check_plan(plan_piece(s.ptr.data() + 100, 100, 150, P), s, 100, 150, P, true);  // a piece: global row ids, local ratings
      }
}

static void test_literal() {
  g_case = "literal";
  {
    const int64_t ptr[] = {0, 0, 5, 2105, 3129, 4154};  // rows of 0, 5, 2100, 1024, 1025 ratings
    std::vector<Unit> u;
    std::vector<SplitRow> sp;
    int64_t nSlabs = 0, solved = 0;
    build_schedule(ptr, 0, 5, 1024, u, sp, nSlabs, solved);
    CHECK(solved == 4 && nSlabs == 5 && u.size() == 7 && sp.size() == 2);
    CHECK(sp[0].row == 2 && sp[0].n == 2100 && sp[0].slab0 == 0 && sp[0].nslabs == 3);
    CHECK(sp[1].row == 4 && sp[1].n == 1025 && sp[1].slab0 == 3 && sp[1].nslabs == 2);
    // the chunks, longest first (equal lengths keep row order), with the slab each one writes
    const Unit want[7] = {{5, 1029, 2, 0}, {1029, 2053, 2, 1}, {3129, 4153, 4, 3}, {2053, 2105, 2, 2}, {4153, 4154, 4, 4},
                          {2105, 3129, 3, -1}, {0, 5, 1, -1}};  // then the whole rows: 1024, 5
    for (int i = 0; i < 7; ++i) CHECK(u[i].beg == want[i].beg && u[i].end == want[i].end && u[i].row == want[i].row && u[i].slab == want[i].slab);
  }
  {
    const int64_t ptr[] = {10, 10 + 65537};  // 65537 / 1024 > 64 chunks: ceil(65537 / 64) = 1025 -> 1028 ratings a chunk
    std::vector<Unit> u;
    std::vector<SplitRow> sp;
    int64_t nSlabs = 0, solved = 0;
    build_schedule(ptr, 7, 1, 1024, u, sp, nSlabs, solved, -1, 0, 64);
    CHECK(solved == 1 && nSlabs == 64 && u.size() == 64 && sp.size() == 1 && sp[0].row == 7 && sp[0].nslabs == 64);
    for (int i = 0; i < 64; ++i) CHECK(u[i].row == 7 && u[i].beg == 1028 * (int64_t)u[i].slab && u[i].end == std::min<int64_t>(65537, u[i].beg + 1028));
  }
}

static void test_auto_chunk() {
  g_case = "auto_chunk";
  const int64_t sw = (int64_t)2048 * 1024;
  CHECK(auto_chunk(0, 0) == 256 && auto_chunk(2048 * 256, 0) == 256 && auto_chunk(2048 * 260, 1 << 30) == 260);
  CHECK(auto_chunk(sw - 1, 0) == 1024);                        // 1023 rounded up to a multiple of 4: the lower branch's upper clamp
  CHECK(auto_chunk(sw, 0) == 1024 && auto_chunk(sw, sw) == 1024);  // from here on the split rows decide, from 1024 ...
  CHECK(auto_chunk(sw, (int64_t)32768 * 2000) == 2000);
  CHECK(auto_chunk((int64_t)1 << 40, (int64_t)1 << 40) == 3072);   // ... to 3072
  CHECK(auto_chunk(1000209, 0) == 488 && auto_chunk(1000209, 1000209) == 488);
  CHECK(auto_chunk(121500000, 120000000) == 3072 && auto_chunk(121500000, 4000000) == 1024);
  Rng g(5);
  for (int i = 0; i < 2000; ++i) {
    const int64_t nnz = g.below((int64_t)1 << (10 + i % 20)), c = auto_chunk(nnz, g.below(nnz + 1));
    CHECK(c % 4 == 0 && c >= 256 && c <= 3072);
  }
  // the side's totals: rows above kDefaultChunk ratings count as split; an emulated world scales every row first
  const int64_t ptr[] = {0, 1024, 1024, 2049, 2649};
  const SideNnz a = side_nnz(ptr, 4), b = side_nnz(ptr, 4, 2);
  CHECK(a.nnz == 2649 && a.splitNnz == 1025 && b.nnz == 5298 && b.splitNnz == 2048 + 2050 + 1200);
}

// (beg, end) of every split row's chunks relative to the row start, in slab order
static std::map<int32_t, std::vector<std::pair<int64_t, int64_t>>> cuts_of(const PiecePlan &p, const Side &s, int64_t rowBegin) {
  std::map<int32_t, std::map<int32_t, std::pair<int64_t, int64_t>>> bySlab;
  for (int64_t i = 0; i < p.nSlabs; ++i) {
    const Unit &u = p.units[(size_t)i];
    const int64_t rb = s.ptr[u.row] - s.ptr[rowBegin];
    bySlab[u.row][u.slab] = {u.beg - rb, u.end - rb};
  }
  std::map<int32_t, std::vector<std::pair<int64_t, int64_t>>> out;
  for (auto &r : bySlab)
    for (auto &c : r.second) out[r.first].push_back(c.second);
  return out;
}

static PiecePlan plan_banded_piece(const Side &s, int64_t rowBegin, int64_t nRows, const PlanParams &P, int64_t W, int nBands, BandCutError *err = nullptr) {
  PiecePlan p = plan_piece(s.ptr.data() + rowBegin, rowBegin, nRows, P);
  const BoundQueries q = band_queries(p, s.ptr.data() + rowBegin, rowBegin, W, nBands);
  CHECK(q.key.size() == p.split.size() * (size_t)(nBands - 1) && q.beg.size() == q.key.size() && q.end.size() == q.key.size());
  const BandCutError e = band_recut(p, s.ptr.data() + rowBegin, rowBegin, P, nBands, answer(q, s, s.ptr[rowBegin]));
  if (err) *err = e;
  else CHECK(e.parts == 0);
  return p;
}

static void test_shard_invariance() {
  g_case = "shard invariance";
  Side s = random_side(77, 400, 1024, 6000);
  s.add_row(70000, 0, 6000);
  const SideNnz t = side_nnz(s.ptr.data(), s.rows());
  for (int banded = 0; banded < 2; ++banded) {
    PlanParams P = params(kOneWave, auto_chunk(t.nnz, t.splitNnz));
    P.fusedMax = std::min(P.chunk, kDefaultChunk);
    auto plan = [&](int64_t b, int64_t e) {
      return cuts_of(banded ? plan_banded_piece(s, b, e - b, P, 1000, 6) : plan_piece(s.ptr.data() + b, b, e - b, P), s, b);
    };
    const auto whole = plan(0, s.rows());
    CHECK(!whole.empty());
    for (int shards : {2, 3}) {
      std::map<int32_t, std::vector<std::pair<int64_t, int64_t>>> joined;
      for (int i = 0; i < shards; ++i)
        for (auto &r : plan(s.rows() * i / shards, s.rows() * (i + 1) / shards)) joined.insert(r);
      CHECK(joined == whole);
    }
  }
}

static void test_dual_classes() {
  g_case = "dual classes";
  const Side s = random_side(9, 600, 256, 5000);
  PlanParams P = params(kOneWave, 256);
  P.dualMax = 80;
  P.k = 100;
  const PiecePlan p = plan_piece(s.ptr.data(), 0, s.rows(), P);
  check_plan(p, s, 0, s.rows(), P, true);
  CHECK(p.dualRows > 100);
}

static void test_shuffle() {
  g_case = "shuffle";
  auto ids = [](const PiecePlan &p) {
    std::vector<int32_t> v;
    for (const Unit &u : p.units) v.push_back(u.row);
    return v;
  };
  for (int64_t nRows : {(int64_t)20000, kShuffleMinRows - 1}) {
    Rng g(3);
    Side s;
    for (int64_t r = 0; r < nRows; ++r) s.ptr.push_back(s.ptr.back() + 1 + g.below(1000));  // (the scheduler reads no column id)
    PlanParams P = params(kOneWave, 1024);
    P.dualMax = 0;
    PlanParams off = P;
    off.shuffle = false;
    const PiecePlan a = plan_piece(s.ptr.data(), 0, nRows, P), b = plan_piece(s.ptr.data(), 0, nRows, P), sorted = plan_piece(s.ptr.data(), 0, nRows, off);
    CHECK(a.nPrimal == nRows && a.nSlabs == 0 && sorted.nPrimal == nRows);
    for (int64_t i = 1; i < nRows; ++i)  // shuffle off: longest first
      CHECK(sorted.units[(size_t)i - 1].end - sorted.units[(size_t)i - 1].beg >= sorted.units[(size_t)i].end - sorted.units[(size_t)i].beg);
    const std::vector<int32_t> ia = ids(a), ib = ids(b), is = ids(sorted);
    CHECK(ia == ib);  // two calls agree
    if (nRows < kShuffleMinRows) {
      CHECK(ia == is);  // below kShuffleMinRows nothing moves
      continue;
    }
    CHECK(ia != is);
    std::vector<int32_t> pa = ia, ps = is;
    std::sort(pa.begin(), pa.end());
    std::sort(ps.begin(), ps.end());
    CHECK(pa == ps);  // a permutation of the sorted list
    const int64_t tail = std::min<int64_t>(nRows / 8, 8192);
    for (int64_t i = nRows - tail; i < nRows; ++i) CHECK(ia[(size_t)i] == is[(size_t)i]);  // the shortest rows stay, sorted, for the tail
    check_plan(a, s, 0, nRows, P, true);
  }
}

static void test_band_recut() {
  g_case = "band-major re-cut";
  const int64_t W = 1000;
  const int nBands = 5, chunk = 256;
  const int64_t minSeg = std::max<int64_t>(64, chunk / 4);
  PlanParams P = params(kOneWave, chunk);
  // 4 000 rows whose every band holds either no rating or at least minSeg: no segment is merged, every chunk lies in one band
  Rng g(11);
  Side s;
  for (int r = 0; r < 4000; ++r) {
    std::vector<int64_t> c((size_t)nBands, 0);
    if (g.below(4) == 0)
      for (int j = 0; j < nBands; ++j) c[(size_t)j] = g.below(3) ? minSeg + g.below(600) : 0;
    else
      c[(size_t)g.below(nBands)] = g.below(300);
    s.add_banded_row(c, W);
  }
  s.add_banded_row({0, 2048, 0, 0, 0}, W);           // one band only: chunk-length pieces
  s.add_banded_row({3200, 3200, 3200, 3200, 3200}, W);  // every band, n / chunk = 62.5
  const int32_t oneBand = 4000, everyBand = 4001;
  const PiecePlan p = plan_banded_piece(s, 0, s.rows(), P, W, nBands);
  check_plan(p, s, 0, s.rows(), P, false);
  CHECK(p.nSlabs > 1000 && p.arenaSlabs == p.nSlabs);
  int prevBand = -1;
  int64_t prevLen = 0, nOne = 0;
  for (int64_t i = 0; i < p.nSlabs; ++i) {
    const Unit &u = p.units[(size_t)i];
    const int band = s.indx[(size_t)u.beg] / (int32_t)W;
    const int64_t len = u.end - u.beg, rb = s.ptr[u.row], re = s.ptr[u.row + 1];
    CHECK(s.indx[(size_t)u.end - 1] / (int32_t)W == band);  // inside one band
    CHECK(band > prevBand || (band == prevBand && len <= prevLen));  // by band, then by descending length
    prevBand = band;
    prevLen = len;
    // pieces are multiples of 4 long, except where a band's ratings (or the row) end
    CHECK(len % 4 == 0 || u.end == re || s.indx[(size_t)u.end] / (int32_t)W != band);
    // ... and start a multiple of 4 behind the start of their band's ratings
    int64_t first = u.beg;
    while (first > rb && s.indx[(size_t)first - 1] / (int32_t)W == band) --first;
    CHECK((u.beg - first) % 4 == 0);
    if (u.row == oneBand) {
      CHECK(len == chunk);
      ++nOne;
    }
  }
  CHECK(nOne == 2048 / chunk);
  for (const SplitRow &sr : p.split)
    if (sr.row == everyBand) CHECK(sr.n == 16000 && sr.nslabs <= kMaxSlabsPerRow && sr.nslabs >= nBands);
  for (size_t i = 1; i < p.split.size(); ++i) CHECK(p.split[i - 1].nslabs >= p.split[i].nslabs);  // reduce order: most slabs first

  // short segments join a neighbour: the successor, the last one its predecessor
  {
    Side t;
    t.add_banded_row({1000, 10, 1000, 0, 0}, W);  // the 10 ratings of band 1 go with band 2
    t.add_banded_row({1000, 0, 0, 0, 10}, W);     // the 10 ratings of band 4 go with band 0
    t.add_banded_row({10, 1000, 0, 0, 0}, W);     // the 10 ratings of band 0 go with band 1
    PlanParams Q = P;
    Q.fusedMax = 8;  // (every row is split)
    const PiecePlan q = plan_banded_piece(t, 0, 3, Q, W, nBands);
    check_plan(q, t, 0, 3, Q, false);
    std::set<std::pair<int32_t, int64_t>> starts;
    for (int64_t i = 0; i < q.nSlabs; ++i) starts.insert({q.units[(size_t)i].row, q.units[(size_t)i].beg - t.ptr[q.units[(size_t)i].row]});
    CHECK(starts.count({0, 1000}) && !starts.count({0, 1010}));
    CHECK(!starts.count({1, 1000}));
    CHECK(!starts.count({2, 10}));
    for (int64_t i = 0; i < q.nSlabs; ++i) CHECK(q.units[(size_t)i].end - q.units[(size_t)i].beg >= minSeg);
  }
  // more band segments than a row may have slabs: reported, not cut
  {
    Side t;
    t.add_banded_row(std::vector<int64_t>(100, 64), 50);
    BandCutError e;
    PlanParams Q = P;
    plan_banded_piece(t, 0, 1, Q, 50, 100, &e);
    CHECK(e.parts == 100 && e.row == 0);
  }
}

static void test_gen_batches() {
  g_case = "gen_batches";
  Rng g(21);
  std::vector<SplitRow> split;
  int32_t slab = 0;
  for (int i = 0; i < 500; ++i) {
    const int32_t n = 1 + (int32_t)g.below(i % 50 == 0 ? 40 : 9);
    split.push_back(SplitRow{n * 100, i, slab, n, 0});
    slab += n;
  }
  const int64_t arena = 16;
  const std::vector<GenBatch> b = gen_batches(split, arena);
  int32_t next = 0;
  for (const GenBatch &x : b) {
    CHECK(x.firstSplit == next && x.nSplit >= 1 && x.slabBase == split[(size_t)x.firstSplit].slab0);
    int32_t n = 0;
    for (int32_t i = 0; i < x.nSplit; ++i) n += split[(size_t)(x.firstSplit + i)].nslabs;
    CHECK(x.nSlabs == n && (n <= arena || x.nSplit == 1));
    next += x.nSplit;
  }
  CHECK(next == (int32_t)split.size() && gen_batches({}, arena).empty());
  // through the planner: rows in row order, the arena as large as the largest batch
  const Side s = random_side(4, 300, 64, 5000);
  PlanParams P = params(kAnyK, 64);
  const PiecePlan p = plan_piece(s.ptr.data(), 0, s.rows(), P);
  int64_t most = 0, rows = 0;
  for (const GenBatch &x : p.genBatches) {
    most = std::max<int64_t>(most, x.nSlabs);
    rows += x.nSplit;
    CHECK(x.nSlabs <= P.arenaSlabs || x.nSplit == 1);
  }
  CHECK(p.genBatches.size() > 3 && rows == (int64_t)p.split.size() && p.arenaSlabs == most);
  for (size_t i = 1; i < p.split.size(); ++i) CHECK(p.split[i - 1].row < p.split[i].row && p.split[i].slab0 == p.split[i - 1].slab0 + p.split[i - 1].nslabs);
}

static void test_banded_plan() {
  g_case = "banded plan";
  const int nBands = 8;
  const int64_t W = 100, chunk = 64, slabElems = 1000;
  Rng g(31);
  Side s;  // the whole side
  for (int r = 0; r < 300; ++r) {
    std::vector<int64_t> c((size_t)nBands, 0);
    if (g.below(8))
      for (int j = 0; j < nBands; ++j) c[(size_t)j] = g.below(3) == 0 ? 0 : g.below(5) == 0 ? g.below(400) : g.below(70);
    s.add_banded_row(c, W);
  }
  const int64_t rows = s.rows();
  std::vector<double> counts((size_t)rows * nBands, 0.0);
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t i = s.ptr[r]; i < s.ptr[r + 1]; ++i) counts[(size_t)r * nBands + (size_t)(s.indx[(size_t)i] / W)] += 1;
  for (int world : {1, 2, 4}) {
    std::vector<int64_t> rankBands, ownerBounds;
    for (int r = 0; r <= world; ++r) {
      rankBands.push_back(r == world ? nBands : r == 0 ? 0 : nBands * r / world + (world == 4 && r == 1 ? 1 : 0));  // (uneven for 4 ranks)
      ownerBounds.push_back(rows * r / world);
    }
    int64_t covered = 0;
    std::vector<BandedPlan> plans;
    for (int rank = 0; rank < world; ++rank) {
      const int bl = (int)rankBands[(size_t)rank], bh = (int)rankBands[(size_t)rank + 1], bpr = bh - bl;
      std::vector<int64_t> hp(1, 0);  // this rank's ratings: its bands of every row
      for (int64_t r = 0; r < rows; ++r) {
        int64_t n = 0;
        for (int b = bl; b < bh; ++b) n += (int64_t)counts[(size_t)r * nBands + (size_t)b];
        hp.push_back(hp.back() + n);
      }
      const BandedPlan B = plan_banded(hp.data(), counts.data(), nBands, rankBands.data(), ownerBounds.data(), rank, world, chunk, slabElems);
      CHECK(!B.error);
      std::vector<char> seen((size_t)hp.back(), 0);
      for (const Unit &u : B.units) {
        CHECK(u.beg < u.end && u.beg >= hp[(size_t)u.row] && u.end <= hp[(size_t)u.row + 1]);
        for (int64_t j = u.beg; j < u.end; ++j) {
          CHECK(!seen[(size_t)j]);
          seen[(size_t)j] = 1;
          ++covered;
        }
      }
      // groups in stage order (rank + 1) % world, ...: their units and sums follow each other
      int64_t u0 = 0, s0 = 0;
      CHECK((int)B.groupUnit0.size() == world && (int)B.groupSlab0.size() == world + 1 && B.groupSlab0[0] == 0);
      for (int st = 1; st <= world; ++st) {
        const size_t gi = (size_t)((rank + st) % world);
        CHECK(B.groupUnit0[gi] == u0 && B.groupSum0[gi] == s0);
        for (int64_t i = u0; i < u0 + B.groupUnits[gi]; ++i) {
          CHECK(B.units[(size_t)i].row >= ownerBounds[gi] && B.units[(size_t)i].row < ownerBounds[gi + 1]);
          if (i > u0) CHECK(B.units[(size_t)i - 1].end - B.units[(size_t)i - 1].beg >= B.units[(size_t)i].end - B.units[(size_t)i].beg);
        }
        u0 += B.groupUnits[gi];
        s0 += B.groupSums[gi];
        CHECK(B.groupSlab0[gi + 1] - B.groupSlab0[gi] == (ownerBounds[gi + 1] - ownerBounds[gi]) * bpr);
      }
      CHECK(u0 == (int64_t)B.units.size() && s0 == (int64_t)B.sums.size() && B.bandSlabs == B.groupSlab0[(size_t)world]);
      // every (row, band) with ratings: one band slab in its owner group's range, written by its only chunk or by a SlabSum
      // over that segment's chunks, whose temporary slabs no other segment uses
      std::map<int64_t, const SlabSum *> sumOf;
      std::vector<char> tmpUsed((size_t)B.tmpSlabs, 0);
      for (const SlabSum &x : B.sums) {
        CHECK(x.dst % slabElems == 0 && x.src0 % slabElems == 0 && x.n >= 2 && !sumOf.count(x.dst / slabElems));
        sumOf[x.dst / slabElems] = &x;
        for (int32_t i = 0; i < x.n; ++i) {
          const int64_t t = x.src0 / slabElems + i - B.bandSlabs;
          CHECK(t >= 0 && t < B.tmpSlabs && !tmpUsed[(size_t)t]);
          tmpUsed[(size_t)t] = 1;
        }
      }
      std::map<int64_t, std::vector<const Unit *>> bySlab;
      for (const Unit &u : B.units) bySlab[u.slab].push_back(&u);
      size_t sumsSeen = 0;
      for (int gi = 0; gi < world; ++gi)
        for (int64_t r = ownerBounds[(size_t)gi]; r < ownerBounds[(size_t)gi + 1]; ++r) {
          int64_t pos = hp[(size_t)r];
          for (int j = 0; j < bpr; ++j) {
            const int64_t len = (int64_t)counts[(size_t)r * nBands + (size_t)(bl + j)];
            const int64_t slab = B.groupSlab0[(size_t)gi] + (r - ownerBounds[(size_t)gi]) * bpr + j;
            if (len == 0) {
              CHECK(!bySlab.count(slab) && !sumOf.count(slab));
              continue;
            }
            if (len <= chunk) {  // one chunk
              CHECK(bySlab[slab].size() == 1 && bySlab[slab][0]->row == r && bySlab[slab][0]->beg == pos && bySlab[slab][0]->end == pos + len && !sumOf.count(slab));
            } else {
              CHECK(sumOf.count(slab) && !bySlab.count(slab));
              const SlabSum &x = *sumOf[slab];
              ++sumsSeen;
              int64_t at = pos;
              CHECK(x.n == (len + chunk - 1) / chunk);
              for (int32_t i = 0; i < x.n; ++i) {  // the chunks in slab order tile the segment
                const std::vector<const Unit *> &v = bySlab[x.src0 / slabElems + i];
                CHECK(v.size() == 1 && v[0]->row == r && v[0]->beg == at && v[0]->end - v[0]->beg <= chunk + 3);
                at = v[0]->end;
              }
              CHECK(at == pos + len);
            }
            pos += len;
          }
        }
      CHECK(sumsSeen == B.sums.size());
      plans.push_back(B);
    }
    CHECK(covered == s.ptr[(size_t)rows]);  // over all ranks, every rating is in exactly one unit
    // the owners' tables
    for (int rank = 0; rank < world; ++rank) {
      const BandedPlan &B = plans[(size_t)rank];
      const int64_t own0 = ownerBounds[(size_t)rank], ownN = ownerBounds[(size_t)rank + 1] - own0;
      CHECK((int64_t)B.table.size() == ownN * nBands && (int)B.recvSlab0.size() == world + 1 && B.recvSlab0[0] == 0);
      for (int r = 0; r < world; ++r) CHECK(B.recvSlab0[(size_t)r + 1] - B.recvSlab0[(size_t)r] == (r == rank ? 0 : ownN * (rankBands[(size_t)r + 1] - rankBands[(size_t)r])));
      std::set<std::pair<int32_t, int64_t>> used;
      size_t nOwned = 0;
      for (int64_t i = 0; i < ownN; ++i) {
        int64_t total = 0;
        for (int b = 0; b < nBands; ++b) {
          const int64_t c = (int64_t)counts[(size_t)(own0 + i) * nBands + (size_t)b];
          const SlabRef ref = B.table[(size_t)i * nBands + (size_t)b];
          total += c;
          if (c == 0) {
            CHECK(ref.src < 0);
            continue;
          }
          CHECK(ref.src >= 0 && ref.src < world && b >= rankBands[(size_t)ref.src] && b < rankBands[(size_t)ref.src + 1]);
          if (ref.src == rank) {
            CHECK(ref.slab >= B.groupSlab0[(size_t)rank] && ref.slab < B.groupSlab0[(size_t)rank + 1]);
          } else {
            CHECK(ref.slab >= B.recvSlab0[(size_t)ref.src] && ref.slab < B.recvSlab0[(size_t)ref.src + 1]);
            // the source numbers the slabs of this owner's group as rows x its bands: the same offset on both sides
            const BandedPlan &S = plans[(size_t)ref.src];
            CHECK(ref.slab - B.recvSlab0[(size_t)ref.src] == i * (rankBands[(size_t)ref.src + 1] - rankBands[(size_t)ref.src]) + (b - rankBands[(size_t)ref.src]));
            CHECK(S.groupSlab0[(size_t)rank + 1] - S.groupSlab0[(size_t)rank] == B.recvSlab0[(size_t)ref.src + 1] - B.recvSlab0[(size_t)ref.src]);
          }
          CHECK(used.insert({ref.src, ref.slab}).second);
        }
        if (total == 0) continue;
        CHECK(nOwned < B.owned.size());
        const SplitRow &sr = B.owned[nOwned++];
        CHECK(sr.row == own0 + i && sr.n == total && sr.slab0 == i * nBands && sr.nslabs == nBands);
      }
      CHECK(nOwned == B.owned.size());
    }
  }
  // an owned row's slab0 is its index x nBands in 32 bits: the guard reads the bounds alone
  const int64_t rankBands[] = {0, 8}, tooMany[] = {0, ((int64_t)1 << 28)};
  const BandedPlan bad = plan_banded(nullptr, nullptr, 8, rankBands, tooMany, 0, 1, chunk, slabElems);
  CHECK(bad.error && std::string(bad.error) == "too many owned rows");
}

int main() {
  test_coverage();
  test_literal();
  test_auto_chunk();
  test_shard_invariance();
  test_dual_classes();
  test_shuffle();
  test_band_recut();
  test_gen_batches();
  test_banded_plan();
  printf("schedule_test: ok\n");
  return 0;
}
