// rank_plan.h -- how a request of ycnr_als_rank_eval is cut into the slots rank_count_kernel (rank_kernels.hip.h) works on, and
// the sizes the kernel shares with the host: its LDS image, the factorsCount it serves, its grid.  Host-only and a function of its
// arguments alone, like schedule.h and step_policy.h: no HIP, no environment, no device call (tests/cpp/rank_plan_test.cc builds
// it with a plain C++ compiler).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#ifdef __HIPCC__
#define YCNR_RANK_HD __host__ __device__
#else
#define YCNR_RANK_HD
#endif

namespace ycnr {

constexpr int kRankSlotTargets = 64;              // held-out items of one slot: one per lane of the wave that finishes it
constexpr int kRankBins = kRankSlotTargets + 1;   // an item is beaten by 0 .. 64 of a slot's targets
constexpr int kRankSlotsPerGroup = 16;            // slots of a workgroup: the rows of an MFMA tile
constexpr size_t kRankLdsBudget = 64 * 1024;      // dynamic LDS a workgroup of rank_count_kernel may ask for
constexpr int64_t kRankBatchSlots = 65536;        // slots per launch (bounds the histogram image: 17 MB)

// `count` consecutive held-out items of request user `user`, the first at position `begin` of testIds / outRank
struct RankSlot {
  int64_t begin;
  int32_t user;
  int32_t count;
};

// Every request user's held-out list [testPtr[u], testPtr[u + 1]) in pieces of at most kRankSlotTargets, in request order.  The
// ranks of different targets are independent and the targets of a user's other slots compete like any item, so the cut is exact.
// A user without held-out items gets no slot.  testPtr must not decrease.
inline std::vector<RankSlot> rank_cut_slots(int64_t nUsers, const int64_t *testPtr) {
  std::vector<RankSlot> slots;
  for (int64_t u = 0; u < nUsers; ++u)
    for (int64_t b = testPtr[u]; b < testPtr[u + 1]; b += kRankSlotTargets)
      slots.push_back(RankSlot{b, (int32_t)u, (int32_t)std::min<int64_t>(kRankSlotTargets, testPtr[u + 1] - b)});
  return slots;
}

// The LDS image of a workgroup, in this order: 16 user rows zero-padded to kp = factorsCount rounded up to 16 (elements of ts
// bytes), then the slot tables: the targets' scores and ids as scored, the same ordered best first, the histograms.
YCNR_RANK_HD constexpr size_t rank_tables_bytes(size_t ts) {
  return (size_t)kRankSlotsPerGroup * (2 * kRankSlotTargets * (ts + 4) + kRankBins * 4);
}
YCNR_RANK_HD constexpr size_t rank_lds_bytes(int k, size_t ts) {
  return (size_t)kRankSlotsPerGroup * (size_t)((k + 15) & ~15) * ts + rank_tables_bytes(ts);
}
constexpr size_t kRankStaticLds = kRankSlotsPerGroup * 24;  // the slots' descriptors (begin, count, skip list), static in the kernel
// float32: factorsCount <= 688, float64: factorsCount <= 272
YCNR_RANK_HD constexpr bool rank_supported(int k, size_t ts) { return rank_lds_bytes(k, ts) + kRankStaticLds <= kRankLdsBudget; }

// gridDim.y for nSlots slots of one launch, chosen as the fused recommend path chooses its parts: the item range of a slot group
// over enough workgroups to fill the chip four times, at least 16 item tiles (4 per wave) each
inline int64_t rank_parts(int64_t nSlots, int64_t totalItems, int64_t cus) {
  const int64_t groups = (nSlots + kRankSlotsPerGroup - 1) / kRankSlotsPerGroup, ntiles = (totalItems + 15) / 16;
  return std::max<int64_t>(1, std::min<int64_t>((ntiles + 15) / 16, (4 * cus + groups - 1) / std::max<int64_t>(groups, 1)));
}

}  // namespace ycnr
