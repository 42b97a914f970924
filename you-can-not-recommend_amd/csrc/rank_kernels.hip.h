// Ranks of held-out items from device-resident factors (ycnr_als_rank_eval): scores and counting in one kernel.
//
// Hu, Koren and Volinsky evaluate an implicit model by the rank of every held-out observation (u, i) in u's ranking of the
// whole catalogue; hit rate, MRR and AUC need the same integer: how many competing items j the model places ahead of i under
// the total order of the recommend kernels (higher score first, equal scores by lower item id).  recommend_topn_kernel is a
// fused score-and-select; this is a fused score-and-count with the same scores: the 16 user rows of a workgroup in LDS,
// zero-padded to kp, MFMA (c0, t) in the same order, so every score has the bits it has there.
//
// A slot (rank_plan.h) is at most 64 held-out items ("targets") of one request user.  With a slot's targets ordered best
// first, t_0 > t_1 > ..., an item j falls into bin p = the number of targets that beat it, and j beats t_q exactly if p <= q.
// So one histogram of 65 bins per slot holds every rank of the slot: rank(t_q) = sum_{p <= q} hist[p] - 1 (t_q is in bin q).
// Skipped items must not compete; instead of looking every score of the stream up in a skip list, the skipped items are
// scored on their own and taken out of their bins again.
//
// Needs als_kernels.hip.h's MfmaTraits and recommend_kernels.hip.h (top_better, cd_group_of, cd_reg_of) in front of this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rank_plan.h"

namespace ycnr {

// One 16 x 16 tile of scores: the workgroup's 16 user rows (LDS, urow = u + j * kp + 4 * g of this lane) against the item of
// this lane (row = its factors + 4 * g, valid = it exists).  The loop of recommend_topn_kernel, operand for operand.
template <typename T>
__device__ __forceinline__ typename MfmaTraits<T>::acc_t rank_score_tile(const T *urow, const T *row, bool valid, int k, int kp, int g) {
  using Tr = MfmaTraits<T>;
  typename Tr::acc_t acc = {T(0), T(0), T(0), T(0)};
  for (int c0 = 0; c0 < kp; c0 += 16) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int c = c0 + 4 * g + t;
      const T b = (valid && c < k) ? row[c0 + t] : T(0);
      acc = Tr::mma(urow[c0 + t], b, acc);
    }
  }
  return acc;
}

// accumulator register `reg` of this lane, reg not known at compile time (a select chain: indexing would go through scratch)
template <typename A>
__device__ __forceinline__ auto rank_pick(const A &acc, int reg) -> decltype(acc[0] + acc[0]) {
  return reg == 0 ? acc[0] : reg == 1 ? acc[1] : reg == 2 ? acc[2] : acc[3];
}

// The bins of up to four (score, item id) of this lane at once: bin[t] = how many of the n[t] keys at keyS / keyI + base[t]
// (ordered best first) beat (s[t], id[t]).  The searches advance together, as the skip search of recommend_topn_kernel does, so
// the lane pays ONE chain of at most 7 dependent LDS reads, not four.  n[t] == 0 leaves bin[t] = 0 and reads nothing.
template <typename T, int N>
__device__ __forceinline__ void rank_bins(const T *keyS, const int32_t *keyI, const int (&base)[N], const int (&n)[N], const T (&s)[N], const int32_t (&id)[N],
                                          int (&bin)[N]) {
  int lo[N], hi[N];
  bool any = false;
#pragma unroll
  for (int t = 0; t < N; ++t) {
    lo[t] = 0;
    hi[t] = n[t];
    any |= n[t] > 0;
  }
  while (any) {
    int mid[N];
    T ks[N];
    int32_t ki[N];
#pragma unroll
    for (int t = 0; t < N; ++t) {
      const bool open = lo[t] < hi[t];
      mid[t] = (lo[t] + hi[t]) >> 1;
      const int at = open ? base[t] + mid[t] : 0;  // (a closed search reads entry 0 and ignores it)
      ks[t] = keyS[at];
      ki[t] = keyI[at];
    }
    any = false;
#pragma unroll
    for (int t = 0; t < N; ++t) {
      if (lo[t] < hi[t]) {
        if (top_better((double)ks[t], ki[t], (double)s[t], id[t])) lo[t] = mid[t] + 1;
        else hi[t] = mid[t];
      }
      any |= lo[t] < hi[t];
    }
  }
#pragma unroll
  for (int t = 0; t < N; ++t) bin[t] = lo[t];
}

// gridDim = (ceil(nSlots / 16), nParts), 256 threads.  Workgroup (x, y) serves slots 16 x .. 16 x + 15 of `slots` (user rows
// userIds[slot.user] of `users`): it scores and orders their targets, streams the item tiles y * 4 + wave, + 4 nParts, ... into
// the slots' histograms, takes the skip tiles y, y + nParts, ... of every slot out again and adds the result into
// hist[slot][65] (cleared before the launch; integer sums, so the image does not depend on nParts).  Part 0 also writes
// order[slot][q] = the position in testIds of the slot's q-th best target; mark[slot][q] (cleared before) becomes 1 where that
// target is in the user's skip list.  skipPtr is indexed by request user (absolute offsets into skipIds, lists shorter than 2^31).
// Dynamic LDS: rank_lds_bytes(k, sizeof(T)).
template <typename T>
__global__ __launch_bounds__(256) void rank_count_kernel(const T *users, const int32_t *userIds, const RankSlot *slots, int64_t nSlots, const int32_t *testIds,
                                                        const T *items, int64_t totalItems, int k, const int64_t *skipPtr, const int32_t *skipIds,
                                                        int32_t *hist, int32_t *order, int32_t *mark) {
  using Tr = MfmaTraits<T>;
  using acc_t = typename Tr::acc_t;
  constexpr int S = kRankSlotsPerGroup, TG = kRankSlotTargets, NB = kRankBins;
  extern __shared__ __attribute__((aligned(16))) unsigned char smemRank[];
  const int kp = (k + 15) & ~15;
  T *u = reinterpret_cast<T *>(smemRank);                   // [16][kp]
  T *rawS = u + S * kp;                                     // [16][64] target scores, in request order
  T *keyS = rawS + S * TG;                                  // [16][64] the same, best first
  int32_t *rawI = reinterpret_cast<int32_t *>(keyS + S * TG);  // their item ids
  int32_t *keyI = rawI + S * TG;
  int32_t *bins = keyI + S * TG;                            // [16][65]
  __shared__ int64_t sBegin[S], sSkipB[S];
  __shared__ int32_t sCount[S], sSkipN[S];

  const int64_t slot0 = (int64_t)blockIdx.x * S;
  const int ns = (int)(nSlots - slot0 < S ? nSlots - slot0 : S);
  if (threadIdx.x < S) {
    const int i = threadIdx.x;
    const bool live = i < ns;
    const RankSlot sl = live ? slots[slot0 + i] : RankSlot{0, 0, 0};
    sBegin[i] = sl.begin;
    sCount[i] = sl.count;
    sSkipB[i] = live ? skipPtr[sl.user] : 0;
    sSkipN[i] = live ? (int32_t)(skipPtr[sl.user + 1] - skipPtr[sl.user]) : 0;
  }
  for (int f = threadIdx.x; f < S * kp; f += 256) {
    const int i = f / kp, c = f - i * kp;
    u[f] = (i < ns && c < k) ? users[(int64_t)userIds[slots[slot0 + i].user] * k + c] : T(0);
  }
  for (int f = threadIdx.x; f < S * NB; f += 256) bins[f] = 0;
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const T *urow = u + j * kp + 4 * g;

  // 1. target scores: tiles of 16 targets of one slot, the B rows gathered by item id; only the slot's own row of the tile is
  // kept.  16 times the MFMA work a dot product needs, on a set that is small next to the catalogue: what it buys is that a
  // target's score has the bits it gets again in the stream.  Tile w is (slot w & 15, targets 16 (w >> 4) ..).
  for (int w = wave; w < S * (TG / 16); w += 4) {
    const int s = w & 15, e = (w >> 4) * 16 + j, cnt = sCount[s];
    if ((w >> 4) * 16 >= cnt) continue;
    const bool valid = e < cnt;
    const int32_t id = valid ? testIds[sBegin[s] + e] : 0;
    const acc_t acc = rank_score_tile<T>(urow, items + (int64_t)id * k + 4 * g, valid, k, kp, g);
    if (valid && g == cd_group_of<T>(s)) {
      rawS[s * TG + e] = rank_pick(acc, cd_reg_of<T>(s));
      rawI[s * TG + e] = id;
    }
  }
  __syncthreads();

  // 2. order: a rank sort, at most 64 x 64 comparisons per slot.  The ids of a slot differ, so the order is strict.
  for (int f = threadIdx.x; f < S * TG; f += 256) {
    const int s = f >> 6, e = f & 63, cnt = sCount[s];
    if (e >= cnt) continue;
    const T mine = rawS[f];
    const int32_t id = rawI[f];
    int r = 0;
    for (int o = 0; o < cnt; ++o) r += top_better((double)rawS[s * TG + o], rawI[s * TG + o], (double)mine, id) ? 1 : 0;
    keyS[s * TG + r] = mine;
    keyI[s * TG + r] = id;
    if (blockIdx.y == 0) order[(slot0 + s) * TG + r] = (int32_t)(sBegin[s] + e);
  }
  __syncthreads();

  // 3. stream: every item of this part's tiles into the bin of each of the lane's four slots
  {
    int base[4], n[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int r = Tr::cd_row(lane, t);
      base[t] = r * TG;
      n[t] = sCount[r];  // (0 for a slot past the request: it counts nothing)
    }
    const int64_t ntiles = (totalItems + 15) >> 4;
    for (int64_t tile = (int64_t)blockIdx.y * 4 + wave; tile < ntiles; tile += 4 * (int64_t)gridDim.y) {
      const int64_t item = tile * 16 + j;
      const bool valid = item < totalItems;
      const acc_t acc = rank_score_tile<T>(urow, items + (valid ? item : 0) * (int64_t)k + 4 * g, valid, k, kp, g);
      const T s[4] = {acc[0], acc[1], acc[2], acc[3]};
      const int32_t id[4] = {(int32_t)item, (int32_t)item, (int32_t)item, (int32_t)item};
      int nv[4], bin[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) nv[t] = valid ? n[t] : 0;
      rank_bins<T, 4>(keyS, keyI, base, nv, s, id, bin);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (nv[t] > 0) atomicAdd(&bins[Tr::cd_row(lane, t) * NB + bin[t]], 1);
    }
  }

  // 4. skips, by subtraction: the skipped items of every slot's user, scored like the targets, leave their bins again.  An id
  // outside the catalogue matches nothing.  A skipped item that is one of the slot's targets is found AS that key.
  for (int s = 0; s < ns; ++s) {
    const int cnt = sCount[s], len = sSkipN[s];
    const int64_t sb = sSkipB[s];
    for (int64_t tl = (int64_t)blockIdx.y + (int64_t)gridDim.y * wave; tl * 16 < len; tl += 4 * (int64_t)gridDim.y) {
      const int64_t e = tl * 16 + j;
      const int32_t id = e < len ? skipIds[sb + e] : -1;
      const bool valid = id >= 0 && id < totalItems;
      const acc_t acc = rank_score_tile<T>(urow, items + (int64_t)(valid ? id : 0) * k + 4 * g, valid, k, kp, g);
      if (valid && g == cd_group_of<T>(s)) {
        const int base[1] = {s * TG}, n[1] = {cnt};
        const T sc[1] = {rank_pick(acc, cd_reg_of<T>(s))};
        const int32_t ids[1] = {id};
        int bin[1];
        rank_bins<T, 1>(keyS, keyI, base, n, sc, ids, bin);
        atomicAdd(&bins[s * NB + bin[0]], -1);
        if (bin[0] < cnt && keyI[s * TG + bin[0]] == id) mark[(slot0 + s) * TG + bin[0]] = 1;
      }
    }
  }
  __syncthreads();

  // 5. out
  for (int f = threadIdx.x; f < ns * NB; f += 256) {
    const int32_t v = bins[f];
    if (v != 0) atomicAdd(&hist[slot0 * NB + f], v);
  }
}

// the histogram image and the marks of nSlots slots to zero, their order to "nowhere" (on the stream, in front of rank_count_kernel)
__global__ __launch_bounds__(256) void rank_clear_kernel(int32_t *hist, int32_t *order, int32_t *mark, int64_t nSlots) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < nSlots * kRankBins) hist[q] = 0;
  if (q < nSlots * kRankSlotTargets) {
    order[q] = -1;
    mark[q] = 0;
  }
}

// One slot per wave: lane q takes the slot's q-th best target, rank = (bins 0 .. q summed) - 1, or -1 where the target is
// marked as skipped, written at the target's position in the request (NaN scores have no order: two of them can claim one place
// in phase 2 and leave another at "nowhere", which writes nothing).  gridDim.x = ceil(nSlots / 4).
__global__ __launch_bounds__(256) void rank_finish_kernel(const RankSlot *slots, int64_t nSlots, const int32_t *hist, const int32_t *order, const int32_t *mark,
                                                         int32_t *outRank, int64_t nTest) {
  const int lane = threadIdx.x & 63;
  const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= nSlots) return;
  int32_t sum = hist[slot * kRankBins + lane];
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t up = __shfl_up(sum, d, 64);
    if (lane >= d) sum += up;
  }
  const int32_t at = order[slot * kRankSlotTargets + lane];
  if (lane < slots[slot].count && at >= 0 && at < nTest) outRank[at] = mark[slot * kRankSlotTargets + lane] ? -1 : sum - 1;
}

// outCandidates[u] = totalItems - the ids of u's ascending skip list that lie in the catalogue; one thread per request user
__global__ __launch_bounds__(256) void rank_candidates_kernel(const int64_t *skipPtr, const int32_t *skipIds, int64_t nUsers, int64_t totalItems,
                                                             int32_t *outCandidates) {
  const int64_t uq = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (uq >= nUsers) return;
  const int64_t b = skipPtr[uq], e = skipPtr[uq + 1];
  // first id >= 0 and first id >= totalItems
  int64_t lo0 = b, hi0 = e, lo1 = b, hi1 = e;
  while (lo0 < hi0) {
    const int64_t mid = (lo0 + hi0) >> 1;
    if (skipIds[mid] < 0) lo0 = mid + 1;
    else hi0 = mid;
  }
  while (lo1 < hi1) {
    const int64_t mid = (lo1 + hi1) >> 1;
    if (skipIds[mid] < totalItems) lo1 = mid + 1;
    else hi1 = mid;
  }
  outCandidates[uq] = (int32_t)(totalItems - (lo1 - lo0));
}

}  // namespace ycnr
