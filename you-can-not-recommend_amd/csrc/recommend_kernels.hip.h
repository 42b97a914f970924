// Top-N recommend from device-resident factors (ycnr_als_recommend): scores and selection in one kernel.
//
// Reference: after train() the reference keeps the factors (EmfManager._saveCalcResultsToRecommender) and answers
// recommendItemsForUser per request (lib/YcnrController.js:227-284): predict = u . v + globalAvgShift
// (EmfBase._alsPredict, EmfBase.js:825-827) for every item that is not in the user's skip list, items at or above
// minRecommendRating compete, at most limit - 1 come back, best first.
//
// recommend_scores_mfma_kernel (prep_kernels.hip.h) writes an nUsers x totalItems matrix of double scores that two more
// kernels walk again.  Here the scores never leave the registers: the operand assignment of that kernel is kept (16 users'
// factors of the workgroup in LDS, zero-padded to kp; MFMA (c0, t) in the same order), so every predict has the same bits,
// and each wave keeps, per user of its tile, the best `take` (predict, id) pairs found so far as a sorted list with one
// entry per lane.  The order is total -- higher predict first, equal predicts by lower item id -- so the result does not
// depend on which wave or workgroup saw which item tile.
//
// Needs als_kernels.hip.h's MfmaTraits in front of this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ycnr {

constexpr int32_t kTopEmpty = 0x7fffffff;  // id of an unused list entry; its predict is -inf, so every candidate beats it
constexpr int kTopMaxTake = 63;            // a list is one wave wide, and the reference returns limit - 1 items

// Lane l receives lane l - 1's value (lane 0 keeps its own): the shift that makes room for an inserted entry.
// DPP wave_shr:1 moves across the whole wave inside the vector ALU; __shfl_up is a ds_bpermute_b32 per dword -- an LDS
// instruction with its round trip (and a v_lshlrev for the byte address), on the pipe the user factors are read through.
// The compiler places the wait states in front of its own DPP moves (devtest/isa_lint.py checks them).
__device__ __forceinline__ int lane_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ double readlane_f64(double v, int srcLane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), srcLane), __builtin_amdgcn_readlane(__double2loint(v), srcLane));
}
__device__ __forceinline__ double readfirstlane_f64(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// the total order of the lists
__device__ __forceinline__ bool top_better(double v, int32_t id, double cv, int32_t cid) { return v > cv || (v == cv && id < cid); }

// Inserts the wave-uniform candidate (cv, cid) into the sorted list (lv, li) of the wave: its rank is the number of entries
// that are better (a prefix, the list being sorted), the lanes behind the rank take their left neighbour's entry, lane 63's
// entry drops out.
__device__ __forceinline__ void top_insert(double &lv, int32_t &li, double cv, int32_t cid, int lane) {
  const int rank = __popcll(__ballot(top_better(lv, li, cv, cid)));
  const int sHi = lane_shr1(__double2hiint(lv)), sLo = lane_shr1(__double2loint(lv)), sId = lane_shr1(li);
  if (lane > rank) {
    lv = __hiloint2double(sHi, sLo);
    li = sId;
  } else if (lane == rank) {
    lv = cv;
    li = cid;
  }
}

// Merges `nLists` sorted lists of `take` entries each (uniform addresses: every lane reads the same entry) into the list
// (mv, mi).  A source list is sorted, so its first entry that does not beat the worst kept one ends it -- an empty entry
// (-inf, kTopEmpty) never does.
template <typename PV, typename PI>
__device__ __forceinline__ void top_merge(double &mv, int32_t &mi, PV srcV, PI srcI, int nLists, int64_t listStride, int take, int lane) {
  for (int l = 0; l < nLists; ++l) {
    for (int e = 0; e < take; ++e) {
      const double cv = readfirstlane_f64(srcV[l * listStride + e]);
      const int32_t cid = __builtin_amdgcn_readfirstlane(srcI[l * listStride + e]);
      const double wv = readlane_f64(mv, take - 1);
      const int32_t wi = __builtin_amdgcn_readlane(mi, take - 1);
      if (!top_better(cv, cid, wv, wi)) break;
      top_insert(mv, mi, cv, cid, lane);
    }
  }
}

// row of the 16 x 16 C/D tile -> (16-lane group, register) that hold it (MfmaTraits<T>::cd_row inverted)
template <typename T>
__device__ constexpr int cd_group_of(int row) { return sizeof(T) == 4 ? row >> 2 : row & 3; }
template <typename T>
__device__ constexpr int cd_reg_of(int row) { return sizeof(T) == 4 ? row & 3 : row >> 2; }

// gridDim = (ceil(nUsers / 16), nParts): workgroup (x, y) scores users 16 x .. 16 x + 15 (rows userIds[.] of `users`)
// against the item tiles y * 4 + wave, + 4 nParts, ... and writes one list of `take` entries per user to
// partV / partI[(user * nParts + y) * take + .]; recommend_topn_merge_kernel makes the final lists of them.
// minRating must be >= -DBL_MAX (the host clamps it), so neither -inf nor NaN competes -- as in the score-matrix path, where -inf
// marks an item that is out.  skipPtr is indexed by request position (absolute offsets into skipIds, lists shorter than 2^31).
// Dynamic LDS: max(16 * kp * sizeof(T), 64 * take * 12) bytes.
template <typename T>
__global__ __launch_bounds__(256) void recommend_topn_kernel(const T *users, const int32_t *userIds, int64_t nUsers, const T *items, int64_t totalItems, int k,
                                                            double shift, double minRating, const int64_t *skipPtr, const int32_t *skipIds, int take,
                                                            double *partV, int32_t *partI) {
  using Tr = MfmaTraits<T>;
  using acc_t = typename Tr::acc_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char smemTop[];
  T *u = reinterpret_cast<T *>(smemTop);  // [16][kp]
  const int kp = (k + 15) & ~15;
  const int64_t user0 = (int64_t)blockIdx.x * 16;
  const int nu = (int)(nUsers - user0 < 16 ? nUsers - user0 : 16);
  for (int f = threadIdx.x; f < 16 * kp; f += 256) {
    const int i = f / kp, c = f - i * kp;
    u[f] = (i < nu && c < k) ? users[(int64_t)userIds[user0 + i] * k + c] : T(0);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int64_t ntiles = (totalItems + 15) >> 4;
  const T *urow = u + j * kp + 4 * g;
  double lv[16];   // the wave's list of user i of the tile: entry `lane`
  int32_t li[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    lv[i] = -INFINITY;
    li[i] = kTopEmpty;
  }
  // what a predict in accumulator register t of this lane has to beat: the worst kept entry (lane take - 1) of the user that
  // register belongs to.  A user slot past the request can never be beaten.
  double wv[4];
  int32_t wi[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const bool live = Tr::cd_row(lane, t) < nu;
    wv[t] = live ? -INFINITY : INFINITY;
    wi[t] = live ? kTopEmpty : -1;
  }
  // the skip lists of the same four users: where they begin in skipIds and how long they are
  int64_t sb[4];
  int32_t sn[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int r = Tr::cd_row(lane, t);
    sb[t] = r < nu ? skipPtr[user0 + r] : 0;
    sn[t] = r < nu ? (int32_t)(skipPtr[user0 + r + 1] - sb[t]) : 0;
  }
  for (int64_t tile = (int64_t)blockIdx.y * 4 + wave; tile < ntiles; tile += 4 * (int64_t)gridDim.y) {
    const int64_t item = tile * 16 + j;
    const bool valid = item < totalItems;
    const T *row = items + (valid ? item : 0) * (int64_t)k + 4 * g;
    acc_t acc = {T(0), T(0), T(0), T(0)};
    for (int c0 = 0; c0 < kp; c0 += 16) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int c = c0 + 4 * g + t;
        const T b = (valid && c < k) ? row[c0 + t] : T(0);
        acc = Tr::mma(urow[c0 + t], b, acc);
      }
    }
    // the common case once the lists have warmed up: no predict of the tile beats its user's worst kept entry
    double p[4];
    bool c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      p[t] = (double)acc[t] + shift;
      c[t] = valid && p[t] >= minRating && top_better(p[t], (int32_t)item, wv[t], wi[t]);
    }
    if (__ballot(c[0] | c[1] | c[2] | c[3]) == 0) continue;
    // The skip lists only now, for the predicts that would enter a list: every lane searches its item in the ascending lists of
    // its (up to four) users.  The four searches advance together, so a tile pays ONE chain of dependent loads (a search per
    // candidate, one after the other, was most of this kernel's time: DESIGN.md 9-12 has both measurements).
    {
      int32_t lo[4], hi[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        lo[t] = 0;
        hi[t] = c[t] ? sn[t] : 0;
      }
      while ((lo[0] < hi[0]) | (lo[1] < hi[1]) | (lo[2] < hi[2]) | (lo[3] < hi[3])) {
        int32_t mid[4], v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          mid[t] = (lo[t] + hi[t]) >> 1;
          v[t] = lo[t] < hi[t] ? skipIds[sb[t] + mid[t]] : 0;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (lo[t] < hi[t]) {
            if (v[t] == (int32_t)item) {
              c[t] = false;  // skipped
              hi[t] = lo[t];
            } else if (v[t] < (int32_t)item) {
              lo[t] = mid[t] + 1;
            } else {
              hi[t] = mid[t];
            }
          }
        }
      }
    }
    uint64_t pass[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) pass[t] = __ballot(c[t]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int gi = cd_group_of<T>(i), ti = cd_reg_of<T>(i);  // (constants of the unrolled loop: lists and thresholds stay in registers)
      uint64_t m = (pass[ti] >> (16 * gi)) & 0xffffu;
      if (m == 0) continue;
      do {
        const int jj = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)m) - 1);
        m &= m - 1;
        top_insert(lv[i], li[i], readlane_f64(p[ti], 16 * gi + jj), (int32_t)(tile * 16) + jj, lane);
      } while (m != 0);
      const double nwv = readlane_f64(lv[i], take - 1);
      const int32_t nwi = __builtin_amdgcn_readlane(li[i], take - 1);
      if (g == gi) {
        wv[ti] = nwv;
        wi[ti] = nwi;
      }
    }
  }
  // the four waves' lists of a user into one: through LDS (the user factors are done with), wave w merges users 4 w .. 4 w + 3
  __syncthreads();
  double *mV = reinterpret_cast<double *>(smemTop);                          // [4 waves][16 users][take]
  int32_t *mI = reinterpret_cast<int32_t *>(smemTop + (size_t)64 * take * 8);  // the same shape
  if (lane < take) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      mV[(wave * 16 + i) * take + lane] = lv[i];
      mI[(wave * 16 + i) * take + lane] = li[i];
    }
  }
  __syncthreads();
  for (int q = 0; q < 4; ++q) {
    const int i = wave * 4 + q;
    if (i >= nu) break;
    double mv = lane < take ? mV[i * take + lane] : -INFINITY;
    int32_t mi = lane < take ? mI[i * take + lane] : kTopEmpty;
    top_merge(mv, mi, mV + (16 + i) * take, mI + (16 + i) * take, 3, (int64_t)16 * take, take, lane);
    if (lane < take) {
      const int64_t o = ((user0 + i) * gridDim.y + blockIdx.y) * take + lane;
      partV[o] = mv;
      partI[o] = mi;
    }
  }
}

// One wave per user: the user's nParts partial lists into the final one, written in the layout of recommend_select_kernel
// (stride = limit entries per user, unused slots -1 / 0, the count).  stride <= 64.
__global__ __launch_bounds__(256) void recommend_topn_merge_kernel(const double *partV, const int32_t *partI, int64_t nUsers, int nParts, int take, int stride,
                                                                  int32_t *outIds, double *outPredict, int32_t *outCount) {
  const int lane = threadIdx.x & 63;
  const int64_t user = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (user >= nUsers) return;
  const int64_t base = user * nParts * take;
  double mv = lane < take ? partV[base + lane] : -INFINITY;
  int32_t mi = lane < take ? partI[base + lane] : kTopEmpty;
  top_merge(mv, mi, partV + base + take, partI + base + take, nParts - 1, (int64_t)take, take, lane);
  const bool got = lane < take && mi != kTopEmpty;
  if (lane < stride) {
    outIds[user * stride + lane] = got ? mi : -1;
    outPredict[user * stride + lane] = got ? mv : 0.0;
  }
  const int found = __popcll(__ballot(got));
  if (lane == 0) outCount[user] = found;
}

// the requested rows of the user matrix, contiguous (the score-matrix path of ycnr_als_recommend)
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(const T *src, const int32_t *rowIds, int64_t n, int k, T *dst) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n * k) return;
  const int64_t r = q / k;
  dst[q] = src[(int64_t)rowIds[r] * k + (q - r * k)];
}

}  // namespace ycnr
