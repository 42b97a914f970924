// ycnr_als.hip -- host side of libycnr_als.so: the C ABI declared in include/ycnr_als.h.
//
// Owns device memory (CSR shards, factor matrices, work-unit tables, partial slabs),
// builds the work-unit schedule once per rating upload, and launches the kernels of
// als_kernels.hip.h.  There is deliberately no CPU fallback anywhere in this file: without
// a HIP device every entry point fails with YCNR_ERR_HIP.
#include "../../include/ycnr_als.h"
#include "als_kernels.hip.h"
#include "kernel_choice.h"
#include "owned.h"
#include "als_wg_kernels.hip.h"
#include "als_pair_kernels.hip.h"
#ifdef YCNR_WITH_G32  // devtest build only (make EXTRA=-DYCNR_WITH_G32): the 32 x 32 Gramian kernel of round 3, measured equal
#include "devtest/als_gram32_kernels.hip.h"
#endif
#include "als_gen_kernels.hip.h"
#include "prep_kernels.hip.h"
#include <hipcub/hipcub.hpp>
#include "recommend_kernels.hip.h"
#include "foldin_kernels.hip.h"

#include <algorithm>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

using namespace ycnr;

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define HIP_TRY(expr)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail(e_ == hipErrorOutOfMemory ? YCNR_ERR_NOMEM : YCNR_ERR_HIP, "%s failed: %s (%s:%d)", \
                  #expr, hipGetErrorString(e_), __FILE__, __LINE__);                            \
  } while (0)

// kMaxFactors (128), kMaxFactorsBig (256), kMaxFactorsAny (4096) and which path a k takes: step_policy.h
constexpr int64_t kGenArenaBytes = (int64_t)2 << 30;  // slab arena of the any-k path: rows are solved in batches that fit it
constexpr int kPairNB = 16;           // block count whose whole rows go Gramian -> slab -> two-wave solve (als_pair_kernels.hip.h): 240 < k <= 256
constexpr int64_t kPairBatchRows = 4096;   // rows per batch of that path (a slab is 140 KB: 0.57 GB of arena).  One GPU's eighth of C5, ms per
                                           // iteration at 512 / 1024 / 2048 / 3072 / 4096 / 6144 / 8192 / 12288 / 24576 / 98304 rows: 141.6 / 138.0 / 136.7 /
                                           // 136.3 / 136.2 / 136.5 / 137.3 / 139.7 / 138.6 / 137.6 -- short batches leave more of a batch's slabs in the
                                           // last-level cache for its solve, shorter ones pay two kernel tails per batch (YCNR_PAIR_BATCH_ROWS overrides)
constexpr int64_t kBandBytes = (int64_t)96 << 20;  // slice of the fixed matrix one band of chunks gathers from (cache-sized)
constexpr size_t kErrBytes = 65536;
constexpr size_t kZeroRowBytes = 32768 + 64;  // >= kMaxFactorsAny doubles: the "row" the dual kernels gather for ratings past a row's end

size_t tsize(int dtype) { return dtype == YCNR_F64 ? 8 : 4; }

// Who frees what (owned.h): every device buffer, page-locked host buffer, event and stream of this file is a member or a local
// of one of these types, and these deleters are the only calls that free one.  Kernel arguments and the other views
// (DualPlan, StepArgs, RmseArgs) stay raw and are filled from get().
struct FreeDev {
  void operator()(void *p) const { (void)hipFree(p); }
};
struct FreeHost {
  void operator()(void *p) const { (void)hipHostFree(p); }
};
struct FreeEvent {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
struct FreeStream {  // what is still queued on the stream may read buffers that are freed next
  void operator()(hipStream_t s) const {
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
};
template <typename T>
using DevPtr = Owned<T *, FreeDev>;
template <typename T>
using HostPtr = Owned<T *, FreeHost>;
using Event = Owned<hipEvent_t, FreeEvent>;
using Stream = Owned<hipStream_t, FreeStream>;

// The grow-only buffers (GrowBuf): level-1 device arenas, their page-locked host image, the per-call buffers of recommend / fold-in
struct DevAlloc {
  static hipError_t alloc(size_t n, void **p) { return hipMalloc(p, n); }
  static void free(void *p) { FreeDev{}(p); }
};
struct ArenaAlloc : DevAlloc {
  static size_t grow(size_t bytes) { return std::max<size_t>(bytes + bytes / 2, 4096); }
};
struct ExactAlloc : DevAlloc {
  static size_t grow(size_t bytes) { return bytes; }
};
struct PinnedAlloc {
  static hipError_t alloc(size_t n, void **p) { return hipHostMalloc(p, n, hipHostMallocDefault); }
  static void free(void *p) { FreeHost{}(p); }
  static size_t grow(size_t bytes) { return bytes + bytes / 2; }
};

hipError_t new_event(Event &e, bool timing) { return timing ? hipEventCreate(e.put()) : hipEventCreateWithFlags(e.put(), hipEventDisableTiming); }

struct Ratings {
  int64_t rowBegin = 0, rowEnd = 0, nnz = 0;
  DevPtr<int64_t> dRowPtr;  // local, rebased to 0 (RMSE only)
  DevPtr<int32_t> dIndx;
  DevPtr<void> dVals;
  bool loaded = false;
};

// A piece's plan (schedule.h) on the device: the counters of the plan, and the owner of the lists' device copies and the slabs
struct Schedule : PlanCounts {
  std::vector<GenBatch> genBatches;
  DevPtr<Unit> dUnits;
  DevPtr<SplitRow> dSplit;
  DevPtr<void> dSlabs;
  DevPtr<float> dRowSlabs;  // k > 240: the images of a batch of whole rows between their Gramian and their two-wave solve
  int64_t rowSlabRows = 0;
  int64_t nUnits = 0, nSplit = 0;
  int dualMax = 0;  // dual_max_ratings as the plan was built with it (YCNR_DUAL_MAX_BLOCKS is read per upload)
};

// environment toggles for A/B experiments from unmodified hosts, read once per process; the ones step_policy.h decides by
// are its Toggles (all but YCNR_DUAL_MAX_BLOCKS, which is read per upload: upload_toggles)
struct EnvFlags : Toggles {
  bool noDualX6, noX6d, noFusedX6d, ignoreNumeric, noDualQuad, noPair, g32, noPk3;
  size_t k1LdsPad;
};
const EnvFlags &env_flags() {
  static const EnvFlags f = [] {
    EnvFlags e{};
    e.noOverlap = getenv("YCNR_NO_OVERLAP") != nullptr, e.noGraph = getenv("YCNR_NO_GRAPH") != nullptr, e.noX6p = getenv("YCNR_NO_X6P") != nullptr;
    e.genRightLooking = getenv("YCNR_GEN_RIGHT_LOOKING") != nullptr, e.noGenX6 = getenv("YCNR_NO_GEN_X6") != nullptr;
    e.noDualX6 = getenv("YCNR_NO_DUAL_X6") != nullptr, e.noX6d = getenv("YCNR_NO_X6D") != nullptr, e.noFusedX6d = getenv("YCNR_NO_FUSED_X6D") != nullptr;
    e.ignoreNumeric = getenv("YCNR_IGNORE_NUMERIC") != nullptr, e.noDualQuad = getenv("YCNR_NO_DUAL_QUAD") != nullptr;
    e.noPair = getenv("YCNR_NO_PAIR") != nullptr, e.g32 = getenv("YCNR_G32") != nullptr, e.noPk3 = getenv("YCNR_NO_PK3") != nullptr;
    e.k1LdsPad = getenv("YCNR_K1_LDSPAD") ? (size_t)atoi(getenv("YCNR_K1_LDSPAD")) : 0;
    return e;
  }();
  return f;
}
// the toggles of an upload: YCNR_DUAL_MAX_BLOCKS as it is now (experiments set it between uploads)
Toggles upload_toggles() {
  Toggles t = env_flags();
  if (const char *e = getenv("YCNR_DUAL_MAX_BLOCKS")) t.dualMaxBlocks = std::max(0, atoi(e));
  return t;
}
// bytes of the slab arena of the any-k path (YCNR_GEN_ARENA_MB, read per upload and per out-of-place call: tests force several batches)
int64_t gen_arena_bytes() {
  if (const char *e = getenv("YCNR_GEN_ARENA_MB")) return (int64_t)std::max(1, atoi(e)) << 20;
  return kGenArenaBytes;
}

// hipFuncAttributeMaxDynamicSharedMemorySize, set once per (kernel, device, size) instead of per half-step
int set_max_lds(const void *fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void *, int>, size_t> done;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto it = done.find({fn, dev});
  if (it != done.end() && it->second == bytes) return YCNR_OK;
  HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  done[{fn, dev}] = bytes;
  return YCNR_OK;
}

constexpr int kSideStreams = 6;  // most side streams a handle can have; side_streams() of them are in use
// Side streams in use (YCNR_SIDE_STREAMS, read once; experiments).  The runtime maps a process's streams onto
// GPU_MAX_HW_QUEUES hardware queues (4 unless that variable says otherwise, read when the runtime starts): kernels on two
// streams that share a hardware queue run one after the other.
// The runtime reads GPU_MAX_HW_QUEUES once, when it starts.  The library does not touch the environment (a setenv from a dlopen
// constructor races with getenv in the host's other threads, and it cannot know whether the runtime has started already): the
// HOSTS set GPU_MAX_HW_QUEUES=8 before their first HIP call (bench.py, python/ycnr_als/_lib.py -- only while torch has not
// initialised HIP --, lib/ycnr_als.js).  What the variable said when this library was LOADED is what counts
// here: a value that appears later cannot have reached the runtime through one of those hosts.
int g_hw_queues_at_load = 0;
__attribute__((constructor)) void ycnr_note_hw_queues() {
  const char *q = getenv("GPU_MAX_HW_QUEUES");
  g_hw_queues_at_load = q ? atoi(q) : 0;
}
int side_streams() {
  static const int n = [] {
    const char *e = getenv("YCNR_SIDE_STREAMS");
    if (e) return std::max(1, std::min(kSideStreams, atoi(e)));
    // one stream per dual class when every stream gets a hardware queue of its own (the row kernel's stream + five), else two:
    // MAL scale, user half-step, same box: 13.20 ms with 4 queues / 2 side streams, 13.14 with 8 / 2, 12.84 with 8 / 5
    // (five streams on four queues -- streams sharing a queue wait behind each other's event waits -- is the one to avoid)
    return g_hw_queues_at_load >= 8 ? 5 : 2;
  }();
  return n;
}

struct DualPlan {
  bool noX6 = false;     // YCNR_FLAG_NO_BF16X6: float32-MFMA Gramian in the dual kernels too
  bool fewSlabs = false; // no split row of the piece has more than kFewSlabs slabs (als_reduce_solve_kernel<..., FEW>)
  int64_t nPrimal = -1;  // < 0: no dual classes, every whole row goes through the primal kernel
  const int64_t *first = nullptr, *count = nullptr;
  // Side streams (unless YCNR_FLAG_NO_OVERLAP): the dual classes are independent of the row
  // kernel and of each other (different rows of the solved matrix), so they are launched next
  // to it, alternating over kSideStreams streams that fork from and join the step's stream:
  // their waves fill what the row kernel's two waves per SIMD leave idle, and no kernel waits
  // for the last waves of the one before it (15.5 -> 15.1 ms per MAL-scale user half-step).
  int nSide = 0;
  hipStream_t side[kSideStreams] = {};
  hipEvent_t fork = nullptr, join[kSideStreams] = {};
  mutable int nextSide = 0;
  // Small uploads (a half-step of a few kernels that each fill a fraction of the chip): the chunk Gramians and the
  // reduce that consumes their slabs go to a branch of their own, next to the row kernel and the dual classes
  // -- only the reduce depends on the chunks.  The whole half-step is then captured once into a hipGraph and
  // replayed (ycnr_als_step_async), so the forks and joins cost nothing per half-step.
  hipStream_t slabStream = nullptr;
  hipEvent_t slabJoin = nullptr;
};

template <int M>
int launch_dual(StepArgs<float> args, const DualPlan &dp, hipStream_t stream) {
  if (dp.count[M] > 0) {
    if (dp.nSide > 0) stream = dp.side[dp.nextSide++ % dp.nSide];
    args.firstDual = (int32_t)dp.first[M];
    if constexpr (M == 1) {
      // rows of at most 16 ratings: four to a wave (needs 32-bit offsets into a fixed matrix below 4 GB, k <= 128)
      if (!dp.noX6 && !env_flags().noDualX6 && !env_flags().noDualQuad && args.k <= 128 && args.k % 4 == 0 && args.fixedBytes != 0) {
        hipLaunchKernelGGL(als_dual_quad_kernel, dim3((unsigned)((dp.count[M] + 3) / 4)), dim3(64), 0, stream, args, (int32_t)dp.count[M]);
        HIP_TRY(hipGetLastError());
        return YCNR_OK;
      }
    }
    // bf16x6 form unless switched off; NBN = 1 has a single tile and too little to gain
    const bool x6 = !dp.noX6 && !env_flags().noDualX6;
    void (*kd)(StepArgs<float>) = als_dual_solve_kernel<M, false>;
    if (x6) kd = als_dual_solve_kernel<M, true>;
    // (YCNR_DUAL_LDSPAD: occupancy experiments -- extra dynamic LDS per workgroup limits the workgroups a CU holds)
    static const size_t ldsPad = getenv("YCNR_DUAL_LDSPAD") ? (size_t)atoi(getenv("YCNR_DUAL_LDSPAD")) : 0;
    if (ldsPad)
      if (int rcl = set_max_lds(reinterpret_cast<const void *>(kd), SolveMfmaF32<M>::lds_bytes() + ldsPad)) return rcl;
    hipLaunchKernelGGL(kd, dim3((unsigned)dp.count[M]), dim3(64), SolveMfmaF32<M>::lds_bytes() + ldsPad, stream, args);
    HIP_TRY(hipGetLastError());
  }
  return YCNR_OK;
}

// the RMSE kernel for this k: chunks of four values per lane of a 16-lane group (als_rmse_kernel)
template <typename T>
void launch_rmse(const RmseArgs<T> &a, int nPieces, hipStream_t stream) {
  const bool vec = ((size_t)a.k * sizeof(T)) % 16 == 0 && a.k <= 512;
  void (*kr)(RmseArgs<T>) = als_rmse_kernel<T, 0>;
  if (vec) kr = a.k <= 64 ? als_rmse_kernel<T, 1> : a.k <= 128 ? als_rmse_kernel<T, 2> : a.k <= 256 ? als_rmse_kernel<T, 4> : als_rmse_kernel<T, 8>;
  hipLaunchKernelGGL(kr, dim3((unsigned)nPieces), dim3(256), 0, stream, a);
}

// the dual classes M, M - 1, ..., 1, in this order (the round-robin over the side streams depends on it); float32 only
template <typename T, int M = kMaxDualBlocks>
int launch_duals(const StepArgs<T> &args, const DualPlan &dp, hipStream_t stream) {
  if constexpr (std::is_same<T, float>::value && M > 0) {
    if (int rc = launch_dual<M>(args, dp, stream)) return rc;
    return launch_duals<T, M - 1>(args, dp, stream);
  }
  return YCNR_OK;
}

// the dual classes on `stream` itself, one after the other, whatever side streams the plan has
template <typename T>
int launch_duals_in_order(const StepArgs<T> &args, const DualPlan &dp, hipStream_t stream) {
  DualPlan serial = dp;
  serial.nSide = 0;
  return launch_duals<T>(args, serial, stream);
}

// The dual classes next to the row kernel: the side streams wait for dp.fork (which the caller has recorded), take the classes
// in turn and record their joins; join_duals makes `stream` wait for them.
template <typename T>
int fork_duals(const StepArgs<T> &args, const DualPlan &dp, hipStream_t stream) {
  for (int i = 0; i < dp.nSide; ++i) HIP_TRY(hipStreamWaitEvent(dp.side[i], dp.fork, 0));
  dp.nextSide = 0;
  if (int rc = launch_duals<T>(args, dp, stream)) return rc;
  for (int i = 0; i < dp.nSide; ++i) HIP_TRY(hipEventRecord(dp.join[i], dp.side[i]));
  return YCNR_OK;
}
int join_duals(const DualPlan &dp, hipStream_t stream) {
  for (int i = 0; i < dp.nSide; ++i) HIP_TRY(hipStreamWaitEvent(stream, dp.join[i], 0));
  return YCNR_OK;
}

// a runtime bool as a template argument: f(std::true_type()) or f(std::false_type()); CAN = false: there is no true form
template <bool CAN, typename F>
auto with_bool(bool b, F f) {
  if constexpr (CAN)
    if (b) return f(std::true_type());
  return f(std::false_type());
}
// f(std::integral_constant<int, nb>()) for LO <= nb <= HI; false: nb is outside
template <int LO, int HI, typename F>
bool dispatch_nb(int nb, F &&f) {
  if constexpr (LO <= HI) return nb == LO ? (f(std::integral_constant<int, LO>()), true) : dispatch_nb<LO + 1, HI>(nb, f);
  else return false;
}

// The kernels of a half-step at k <= 128 and their dynamic LDS.  kernel_choice.h states which instantiations run.
template <typename T>
struct RowKernels {
  void (*chunk)(StepArgs<T>), (*row)(StepArgs<T>), (*reduce)(StepArgs<T>);
  void (*band)(StepArgs<T>, const T *const *, int32_t);
  size_t ldsRow, ldsReduce;
};

// A choice to its instantiations.  Only forms that choose_kernels can return exist: the bf16x6 kernels are float32, the VALU
// edge needs two blocks, the edge-first solve (E4) also the register solver, FEW float32 and the register solver, and there is
// no x6d row kernel for eight blocks with the LDS solver.  A pointer stays null where the form does not exist.
template <typename T, int NB, bool LDSV>
void row_kernels_nb(const KernelChoice &c, RowKernels<T> &r) {
  constexpr bool F32 = std::is_same<T, float>::value, EDGE = F32 && NB >= 2, E4 = EDGE && !LDSV;
  using Fn = void (*)(StepArgs<T>);
  r.ldsReduce = SolverFor<T, NB, LDSV>::type::lds_bytes();
  r.ldsRow = c.rowLdsImage ? r.ldsReduce : 0;
  if (c.chunk == kGramMfma) r.chunk = with_bool<EDGE>(c.chunkEdge, [](auto e) -> Fn { return als_gram_slab_kernel<T, NB, decltype(e)::value>; });
  if (c.row == kGramMfma)
    r.row = with_bool<EDGE>(c.rowEdge, [&](auto e) { return with_bool<E4>(c.rowE4, [](auto e4) -> Fn { return als_gram_solve_kernel<T, NB, LDSV, decltype(e)::value, decltype(e4)::value>; }); });
  if constexpr (F32) {
    if (c.chunk == kGramX6) r.chunk = als_gram_slab_x6_kernel<NB>;
    if (c.chunk == kGramX6D)
      r.chunk = !c.chunkPadRhs ? als_gram_slab_x6d_kernel<NB, false> : c.chunkPk3 ? als_gram_slab_x6d_kernel<NB, true, true> : als_gram_slab_x6d_kernel<NB, true, false>;
    if constexpr (!(LDSV && NB == 8))
      if (c.row == kGramX6D)
        r.row = !c.rowPadRhs ? als_gram_solve_x6d_kernel<NB, false, LDSV, false> : with_bool<E4>(c.rowE4, [&](auto e4) -> Fn {
          return c.rowPk3 ? als_gram_solve_x6d_kernel<NB, true, LDSV, decltype(e4)::value, true> : als_gram_solve_x6d_kernel<NB, true, LDSV, decltype(e4)::value, false>;
        });
    if constexpr (!LDSV)
      if (c.row == kGramPlanes) r.row = with_bool<EDGE>(c.rowPack, [](auto p) -> Fn { return als_gram_solve_x6p_kernel<NB, decltype(p)::value, decltype(p)::value>; });
  }
  r.reduce = with_bool<EDGE>(c.reduceEdge, [&](auto e) { return with_bool<E4>(c.reduceE4, [&](auto e4) {
    return with_bool<F32 && !LDSV>(c.reduceFew, [](auto few) -> Fn { return als_reduce_solve_kernel<T, NB, LDSV, decltype(e)::value, decltype(e4)::value, decltype(few)::value>; });
  }); });
  r.band = with_bool<EDGE>(c.reduceEdge, [&](auto e) { return with_bool<E4>(c.bandE4, [](auto e4) -> decltype(r.band) { return als_band_reduce_solve_kernel<T, NB, LDSV, decltype(e)::value, decltype(e4)::value>; }); });
}

// The kernels of this half-step: the choice from the arguments and the environment toggles, then the table
template <typename T>
int row_kernels(const StepArgs<T> &args, bool ldsSolver, bool edge, bool x6, bool fewSlabs, RowKernels<T> &r) {
  const KernelChoice c = choose_kernels(std::is_same<T, double>::value, args.k, ldsSolver, edge, x6, args.planes != nullptr, fewSlabs,
                                        env_flags().noX6d, env_flags().noFusedX6d, env_flags().noPk3);
  r = RowKernels<T>{};
  if (!dispatch_nb<1, 8>(c.nb, [&](auto nb) { ldsSolver ? row_kernels_nb<T, decltype(nb)::value, true>(c, r) : row_kernels_nb<T, decltype(nb)::value, false>(c, r); }))
    return fail(YCNR_ERR_UNSUPPORTED, "factorsCount %d > %d is not supported by this build", args.k, kMaxFactors);
  if (!r.chunk || !r.row || !r.reduce || !r.band) return fail(YCNR_ERR_UNSUPPORTED, "factorsCount %d: no kernel of the chosen form in this build", args.k);
  return YCNR_OK;
}

// One half-step at k <= 128: [chunks of split rows -> slabs] [whole rows: Gramian + solve] [dual classes] [slabs -> solve]
template <typename T>
int launch_rows(const RowKernels<T> &rk, StepArgs<T> args, int64_t nUnits, int64_t nSplitUnits, int64_t nSplit, hipStream_t stream,
                hipEvent_t *ev /* 5 events or null */, const DualPlan &dp) {
  const size_t lds = rk.ldsReduce, ldsRow = rk.ldsRow + env_flags().k1LdsPad;  // (the pad: experiments, limits blocks per CU)
  if (int rcl = set_max_lds(reinterpret_cast<const void *>(rk.row), ldsRow)) return rcl;
  if (int rcl = set_max_lds(reinterpret_cast<const void *>(rk.reduce), lds)) return rcl;
  args.firstFused = (int32_t)nSplitUnits;
  if (ev) HIP_TRY(hipEventRecord(ev[0], stream));
  const bool branch = dp.slabStream != nullptr && nSplitUnits > 0;  // chunks -> reduce on their own branch
  const int64_t nPrimal = dp.nPrimal >= 0 ? dp.nPrimal : nUnits - nSplitUnits;
  const bool overlap = dp.nPrimal >= 0 && dp.nSide > 0;
  if (branch || overlap) HIP_TRY(hipEventRecord(dp.fork, stream));
  if (branch) {
    HIP_TRY(hipStreamWaitEvent(dp.slabStream, dp.fork, 0));
    hipLaunchKernelGGL(rk.chunk, dim3((unsigned)nSplitUnits), dim3(64), 0, dp.slabStream, args);
    HIP_TRY(hipGetLastError());
    if (nSplit > 0) {
      hipLaunchKernelGGL(rk.reduce, dim3((unsigned)nSplit), dim3(64), lds, dp.slabStream, args);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(dp.slabJoin, dp.slabStream));
  } else if (nSplitUnits > 0) {
    hipLaunchKernelGGL(rk.chunk, dim3((unsigned)nSplitUnits), dim3(64), 0, stream, args);
    HIP_TRY(hipGetLastError());
  }
  if (ev) HIP_TRY(hipEventRecord(ev[1], stream));
  if (overlap)  // dual classes first, on the side streams; then the row kernel on this one
    if (int rc = fork_duals<T>(args, dp, stream)) return rc;
  if (nPrimal > 0) {
    hipLaunchKernelGGL(rk.row, dim3((unsigned)nPrimal), dim3(64), ldsRow, stream, args);
    HIP_TRY(hipGetLastError());
  }
  if (ev) HIP_TRY(hipEventRecord(ev[2], stream));
  if (int rc = overlap ? join_duals(dp, stream) : dp.nPrimal >= 0 ? launch_duals<T>(args, dp, stream) : YCNR_OK) return rc;  // (or the classes here, in stream order)
  if (ev) HIP_TRY(hipEventRecord(ev[3], stream));
  if (branch) {
    HIP_TRY(hipStreamWaitEvent(stream, dp.slabJoin, 0));
  } else if (nSplit > 0) {
    hipLaunchKernelGGL(rk.reduce, dim3((unsigned)nSplit), dim3(64), lds, stream, args);
    HIP_TRY(hipGetLastError());
  }
  if (ev) HIP_TRY(hipEventRecord(ev[4], stream));
  return YCNR_OK;
}

// k > 128 with k % 4 != 0: the kernels of that path need 16-byte rows, so the half-step runs on copies of
// both matrices with the rows padded to kp = 4 ceil(k / 4) zero columns.  A zero column adds nothing
// to the Gramian or to b, its diagonal entry is lambda n and its solution component exactly 0.
__global__ void pad_rows_kernel(const float *src, float *dst, int64_t rowBegin, int64_t rows, int k, int kp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * kp) return;
  const int64_t r = rowBegin + i / kp;
  const int c = (int)(i % kp);
  dst[r * kp + c] = c < k ? src[r * k + c] : 0.0f;
}
__global__ void unpad_rows_kernel(const float *src, float *dst, int64_t rowBegin, int64_t rows, int k, int kp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * k) return;
  const int64_t r = rowBegin + i / k;
  const int c = (int)(i % k);
  dst[r * k + c] = src[r * kp + c];
}

int device_cus() {
  static std::mutex mu;
  static std::map<int, int> cus;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cus.find(dev);
  if (it != cus.end()) return it->second;
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
  cus[dev] = n;
  return n;
}

// 128 < k <= 256, float32 (als_wg_kernels.hip.h): one 512-thread workgroup per row or chunk, one
// workgroup per CU, persistent over its share of the units:
//   [chunks of heavy rows -> slabs] [whole rows: Gramian + solve] [dual classes] [slabs -> solve]
template <int NB>
int launch_wg_nb(StepArgs<float> args, int64_t nSplitUnits, int64_t nPrimal, int64_t nSplit, hipStream_t stream, hipEvent_t *ev,
                 const DualPlan &dp, float *rowSlabs, int64_t rowSlabRows) {
  auto k0 = als_wg_gram_slab_kernel<NB>;
  auto k1 = als_wg_gram_solve_kernel<NB>;
  auto k2 = als_wg_reduce_solve_kernel<NB>;
  const size_t lds = WgCfg<NB>::LDS_BYTES;
  if (int rc = set_max_lds(reinterpret_cast<const void *>(k0), lds)) return rc;
  if (int rc = set_max_lds(reinterpret_cast<const void *>(k1), lds)) return rc;
  if (int rc = set_max_lds(reinterpret_cast<const void *>(k2), lds)) return rc;
  const int64_t cus = device_cus();
  args.firstFused = (int32_t)nSplitUnits;
  if (ev) HIP_TRY(hipEventRecord(ev[0], stream));
  // The dual classes go to the side streams, in front of the Gramian / solve batches (round 3).  A Gramian or solve workgroup
  // fills a CU's register file, so the two kinds never share a CU -- but the one-wave dual kernels take the CUs that a
  // batch kernel's tail has already left: the user half-step of one GPU's eighth of C5 76.5 -> 73.5 ms (interleaved A/B,
  // YCNR_NO_OVERLAP=1).  (Tried on top and dropped: the solve of batch i on a second stream beside the Gramians of batch
  // i + 1 on fewer CUs -- 224 / 192 / 160 / 128 CUs for the Gramians: +3.7 / +10 / +20 / +40 ms per iteration.)
  const bool sideDuals = dp.nPrimal >= 0 && dp.nSide > 0 && dp.fork;
  if (sideDuals) {
    HIP_TRY(hipEventRecord(dp.fork, stream));
    if (int rc = fork_duals<float>(args, dp, stream)) return rc;
  }
  // NB = 16, YCNR_G32=1: the Gramians on 32 x 32 MFMAs, one wave per SIMD (als_gram32_kernels.hip.h) -- measured equal to
  // WgGram on one GPU's eighth of C5 (both are bound by the power the bf16 pipe + the split draw), so off
#ifdef YCNR_WITH_G32
  const bool g32 = NB == kPairNB && env_flags().g32;
  if (g32) {
    if (int rc = set_max_lds(reinterpret_cast<const void *>(als_g32_slab_kernel), (size_t)G32Cfg::LDS_BYTES)) return rc;
    if (int rc = set_max_lds(reinterpret_cast<const void *>(als_g32_rowslab_kernel), (size_t)G32Cfg::LDS_BYTES)) return rc;
  }
#endif
  if (nSplitUnits > 0) {
#ifdef YCNR_WITH_G32
    if (g32)
      hipLaunchKernelGGL(als_g32_slab_kernel, dim3((unsigned)std::min(nSplitUnits, cus)), dim3(kG32Threads), (size_t)G32Cfg::LDS_BYTES, stream, args,
                         (int32_t)nSplitUnits);
    else
#endif
      hipLaunchKernelGGL(k0, dim3((unsigned)std::min(nSplitUnits, cus)), dim3(kWgThreads), lds, stream, args, (int32_t)nSplitUnits);
    HIP_TRY(hipGetLastError());
  }
  if (ev) HIP_TRY(hipEventRecord(ev[1], stream));
  bool pairDone = false;
  if constexpr (NB == kPairNB) {
    // whole rows: Gramian -> slab by the workgroup kernel, then the solve by two waves per row, batch by batch
    // (als_pair_kernels.hip.h); YCNR_NO_PAIR=1 keeps the fused workgroup kernel for A/B runs
    if (nPrimal > 0 && rowSlabs && rowSlabRows > 0 && !env_flags().noPair) {
      auto kg = als_wg_gram_rowslab_kernel<NB>;
      auto ks = als_slab_solve2_kernel<NB>;
      if (int rc = set_max_lds(reinterpret_cast<const void *>(kg), lds)) return rc;
      if (int rc = set_max_lds(reinterpret_cast<const void *>(ks), (size_t)PairCfg<NB>::LDS_BYTES)) return rc;
      for (int64_t b0 = 0; b0 < nPrimal; b0 += rowSlabRows) {
        const int64_t cnt = std::min(rowSlabRows, nPrimal - b0);
        const int32_t first = (int32_t)(nSplitUnits + b0);
#ifdef YCNR_WITH_G32
        if (g32)
          hipLaunchKernelGGL(als_g32_rowslab_kernel, dim3((unsigned)std::min(cnt, cus)), dim3(kG32Threads), (size_t)G32Cfg::LDS_BYTES, stream, args,
                             rowSlabs, first, (int32_t)cnt);
        else
#endif
          hipLaunchKernelGGL(kg, dim3((unsigned)std::min(cnt, cus)), dim3(kWgThreads), lds, stream, args, rowSlabs, first, (int32_t)cnt);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ks, dim3((unsigned)cnt), dim3(kPairThreads), (size_t)PairCfg<NB>::LDS_BYTES, stream, args, (const float *)rowSlabs, first);
        HIP_TRY(hipGetLastError());
      }
      pairDone = true;
    }
  }
  if (nPrimal > 0 && !pairDone) {
    hipLaunchKernelGGL(k1, dim3((unsigned)std::min(nPrimal, cus)), dim3(kWgThreads), lds, stream, args, (int32_t)nPrimal);
    HIP_TRY(hipGetLastError());
  }
  if (ev) HIP_TRY(hipEventRecord(ev[2], stream));
  if (dp.nPrimal >= 0 && !sideDuals)  // (YCNR_FLAG_NO_OVERLAP, or too few rows to pay for the fork and the joins)
    if (int rc = launch_duals_in_order<float>(args, dp, stream)) return rc;
  if (sideDuals)
    if (int rc = join_duals(dp, stream)) return rc;
  if (ev) HIP_TRY(hipEventRecord(ev[3], stream));
  if (nSplit > 0) {
    hipLaunchKernelGGL(k2, dim3((unsigned)std::min(nSplit, cus)), dim3(kWgThreads), lds, stream, args, (int32_t)nSplit);
    HIP_TRY(hipGetLastError());
  }
  if (ev) HIP_TRY(hipEventRecord(ev[4], stream));
  return YCNR_OK;
}

int launch_step_big(const StepArgs<float> &args, int64_t nUnits, int64_t nSplitUnits, int64_t nSplit, hipStream_t stream,
                    hipEvent_t *ev, const DualPlan &dp, float *rowSlabs = nullptr, int64_t rowSlabRows = 0) {
  if (nUnits > 0x7fffffffLL) return fail(YCNR_ERR_UNSUPPORTED, "too many work units for one launch (%lld)", (long long)nUnits);
  const int64_t nPrimal = dp.nPrimal >= 0 ? dp.nPrimal : nUnits - nSplitUnits;
  int rc = YCNR_OK;
  if (!dispatch_nb<9, 16>((args.k + 15) / 16, [&](auto nb) { rc = launch_wg_nb<decltype(nb)::value>(args, nSplitUnits, nPrimal, nSplit, stream, ev, dp, rowSlabs, rowSlabRows); }))
    return fail(YCNR_ERR_UNSUPPORTED, "factorsCount %d is outside the workgroup-per-row path", args.k);
  return rc;
}

// any factorsCount (als_gen_kernels.hip.h): batches of [Gramians -> slabs] [slabs -> solve], then the dual classes
// (float32: rows of at most 176 ratings, whose n x n form does not depend on k)
template <typename T>
int launch_step_gen(const StepArgs<T> &args, const std::vector<GenBatch> &batches, hipStream_t stream, hipEvent_t *ev, const DualPlan &dp) {
  const GenChoice c = choose_gen(sizeof(T), args.k, (reinterpret_cast<uintptr_t>(args.fixed) & 15) == 0, env_flags());
  if (c.status == kGenRhsTooLarge) return fail(YCNR_ERR_UNSUPPORTED, "factorsCount %d: the right-hand side does not fit a CU's LDS", args.k);
  if (c.status == kGenPanelTooLarge) return fail(YCNR_ERR_UNSUPPORTED, "factorsCount %d: a panel of four ratings does not fit a CU's LDS", args.k);
  GenArgs<T> ga{args, c.nb, 0, 0, 0};
  const void *solveFn = c.panelLds ? reinterpret_cast<const void *>(als_gen_solve_kernel<T, true>) : reinterpret_cast<const void *>(als_gen_solve_kernel<T, false>);
  if (int rc = set_max_lds(solveFn, c.solveLds)) return rc;
  const void *leftFn = nullptr;
  if (c.left) {
    if constexpr (sizeof(T) == 4)
      leftFn = c.leftMaxc == 2 ? reinterpret_cast<const void *>(als_gen_solve_left_kernel<T, 2, 4, 8, true, 2>) : reinterpret_cast<const void *>(als_gen_solve_left_kernel<T, 4, 4, 8, true, 2>);
    else
      leftFn = reinterpret_cast<const void *>(als_gen_solve_left_kernel<T, 4, 2, 4, false, 3>);
    if (int rc = set_max_lds(leftFn, c.leftLds)) return rc;
  }
  constexpr int V = 16 / (int)sizeof(T);
  const void *gramFn = c.vec ? reinterpret_cast<const void *>(als_gen_gram_kernel<T, V>) : reinterpret_cast<const void *>(als_gen_gram_kernel<T, 1>);
  if constexpr (sizeof(T) == 4)
    if (c.x6) gramFn = reinterpret_cast<const void *>(als_gen_gram_kernel<T, V, true>);
  if (int rc = set_max_lds(gramFn, c.gramLds)) return rc;
  if (ev) HIP_TRY(hipEventRecord(ev[0], stream));
  for (const GenBatch &b : batches) {
    ga.slabBase = b.slabBase;
    ga.firstUnit = b.slabBase;  // units of split rows are numbered like their slabs
    ga.firstSplit = b.firstSplit;
    {
      int Rv = c.R, Pv = c.P;
      void *gargs[] = {(void *)&ga, (void *)&Rv, (void *)&Pv};
      HIP_TRY(hipLaunchKernel(gramFn, dim3((unsigned)b.nSlabs), dim3(c.threads), gargs, c.gramLds, stream));
    }
    HIP_TRY(hipGetLastError());
    if (leftFn) {
      void *kargs[] = {(void *)&ga};
      HIP_TRY(hipLaunchKernel(leftFn, dim3((unsigned)b.nSplit), dim3(64 * c.leftWaves), kargs, c.leftLds, stream));
    } else if (c.panelLds) {
      hipLaunchKernelGGL((als_gen_solve_kernel<T, true>), dim3((unsigned)b.nSplit), dim3(kGenThreads), c.solveLds, stream, ga);
    } else {
      hipLaunchKernelGGL((als_gen_solve_kernel<T, false>), dim3((unsigned)b.nSplit), dim3(kGenThreads), c.solveLds, stream, ga);
    }
    HIP_TRY(hipGetLastError());
  }
  if (ev) {
    HIP_TRY(hipEventRecord(ev[1], stream));
    HIP_TRY(hipEventRecord(ev[2], stream));
  }
  if constexpr (std::is_same<T, float>::value) {
    if (dp.nPrimal >= 0) {
      StepArgs<float> a2 = args;
      a2.firstFused = 0;
      if (int rc = launch_duals_in_order<float>(a2, dp, stream)) return rc;
    }
  }
  if (ev) {
    HIP_TRY(hipEventRecord(ev[3], stream));
    HIP_TRY(hipEventRecord(ev[4], stream));
  }
  return YCNR_OK;
}

template <typename T>
int launch_step(const StepArgs<T> &args, int64_t nUnits, int64_t nSplitUnits, int64_t nSplit, hipStream_t stream,
                hipEvent_t *ev, bool ldsSolver = false, const DualPlan &dp = DualPlan(), bool edge = false, bool x6 = false) {
  if (nUnits > 0x7fffffffLL || nSplit > 0x7fffffffLL)
    return fail(YCNR_ERR_UNSUPPORTED, "too many work units for one launch (%lld)", (long long)nUnits);
  RowKernels<T> rk;
  if (int rc = row_kernels<T>(args, ldsSolver, edge, x6, dp.fewSlabs, rk)) return rc;
  return launch_rows<T>(rk, args, nUnits, nSplitUnits, nSplit, stream, ev, dp);
}

// A plan of out_of_place_plan_params (fold-in beyond 128 factors, the level-1 portion op) on its path: every row in primal
// form, no timing events, everything on `stream`
template <typename T>
int launch_out_of_place(const StepArgs<T> &a, const PiecePlan &plan, hipStream_t stream) {
  const PathKind path = step_path(std::is_same<T, double>::value, a.k);
  if (path == kAnyK) return launch_step_gen<T>(a, plan.genBatches, stream, nullptr, DualPlan());
  if constexpr (std::is_same<T, float>::value)
    if (path == kWorkgroup) return launch_step_big(a, (int64_t)plan.units.size(), plan.nSlabs, (int64_t)plan.split.size(), stream, nullptr, DualPlan());
  return launch_step<T>(a, (int64_t)plan.units.size(), plan.nSlabs, (int64_t)plan.split.size(), stream, nullptr);
}

// copy `bytes` from src (host or device) to a device destination
int copy_in(void *dst, const void *src, size_t bytes, int memKind, hipStream_t stream) {
  if (bytes == 0) return YCNR_OK;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, memKind == YCNR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                         stream));
  return YCNR_OK;
}

// out[q] = first position p in [beg[q], end[q]) with indx[p] >= key[q] (end[q] if none); rows sorted by column id
__global__ void lower_bound_i32_kernel(const int32_t *indx, const int64_t *beg, const int64_t *end, const int32_t *key,
                                       int64_t *out, int64_t n) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  int64_t lo = beg[q], hi = end[q];
  const int32_t kq = key[q];
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (indx[mid] < kq) lo = mid + 1;
    else hi = mid;
  }
  out[q] = lo;
}

int lower_bound_i32(const int32_t *dIndx, const std::vector<int64_t> &beg, const std::vector<int64_t> &end,
                    const std::vector<int32_t> &key, std::vector<int64_t> &out, hipStream_t stream) {
  const size_t n = key.size();
  out.resize(n);
  if (n == 0) return YCNR_OK;
  DevPtr<char> d;
  HIP_TRY(hipMalloc(d.put(), n * 28));
  int64_t *dBeg = (int64_t *)d.get(), *dEnd = dBeg + n, *dOut = dEnd + n;
  int32_t *dKey = (int32_t *)(dOut + n);
  HIP_TRY(hipMemcpyAsync(dBeg, beg.data(), n * 8, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(dEnd, end.data(), n * 8, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(dKey, key.data(), n * 4, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(lower_bound_i32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dIndx, dBeg, dEnd, dKey, dOut, (int64_t)n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out.data(), dOut, n * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return YCNR_OK;
}

// got = {max, min} of the n > 0 column ids on the device
int index_max_min(const int32_t *dIndx, int64_t n, hipStream_t stream, int32_t got[2]) {
  got[0] = got[1] = 0;
  DevPtr<int32_t> dmm;
  HIP_TRY(hipMalloc(dmm.put(), 2 * sizeof(int32_t)));
  const int32_t init[2] = {INT32_MIN, INT32_MAX};
  HIP_TRY(hipMemcpyAsync(dmm.get(), init, sizeof init, hipMemcpyHostToDevice, stream));
  const int blocks = (int)std::min<int64_t>(2048, (n + 255) / 256);
  hipLaunchKernelGGL(max_i32_kernel, dim3(blocks), dim3(256), 0, stream, dIndx, n, dmm.get(), dmm.get() + 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(got, dmm.get(), 2 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return YCNR_OK;
}

// validate 0 <= indx[i] < limit on the device
int check_index_range(const int32_t *dIndx, int64_t n, int64_t limit, hipStream_t stream,
                      const char *what) {
  if (n == 0) return YCNR_OK;
  int32_t got[2];
  if (int rc = index_max_min(dIndx, n, stream, got)) return rc;
  if (got[1] < 0 || (int64_t)got[0] >= limit)
    return fail(YCNR_ERR_INVALID, "%s: column id out of range (min %d, max %d, rows of the opposite side %lld)",
                what, got[1], got[0], (long long)limit);
  return YCNR_OK;
}

// the column ids against a half-open range (banded uploads: only this rank's bands may appear)
int check_index_bounds(const int32_t *dIndx, int64_t n, int64_t lo, int64_t hi, hipStream_t stream, const char *what) {
  if (n == 0) return YCNR_OK;
  int32_t got[2];
  if (int rc = index_max_min(dIndx, n, stream, got)) return rc;
  if ((int64_t)got[1] < lo || (int64_t)got[0] >= hi)
    return fail(YCNR_ERR_INVALID, "%s: column id outside this rank's bands (min %d, max %d, bands cover [%lld, %lld))", what, got[1], got[0],
                (long long)lo, (long long)hi);
  return YCNR_OK;
}

#include "comm_impl.hip.h"

// one pipelined piece of a side's row shard: its ratings, its work-unit schedule and the events
// that time its kernels and its exchange
struct Part {
  Ratings R;
  Schedule S;
  Event ev[5], ready, x0, x1;
  // fork / join of the piece's dual-class launches on the handle's side streams, and "all kernels of the piece done":
  // per piece, because two pieces are in flight at a time (on the handle's two piece streams)
  Event fork, join[kSideStreams], done, slabJoin;
  hipError_t create_events() {  // (only the parts of an upload get events: a Part is also a plain value)
    hipError_t e = hipSuccess;
    for (int i = 0; i < 5 && e == hipSuccess; ++i) e = new_event(ev[i], true);
    if (e == hipSuccess) e = new_event(fork, false);
    for (int i = 0; i < kSideStreams && e == hipSuccess; ++i) e = new_event(join[i], false);
    if (e == hipSuccess) e = new_event(done, false);
    if (e == hipSuccess) e = new_event(slabJoin, false);
    if (e == hipSuccess) e = new_event(ready, false);
    if (e == hipSuccess) e = new_event(x0, true);
    if (e == hipSuccess) e = new_event(x1, true);
    return e;
  }
};

// A side whose half-step is sharded by BANDS OF COLUMNS (ycnr_als_set_ratings_banded): what the upload leaves besides the
// side's single Part (local ratings, chunk units, the arena of band + temporary slabs, the owned rows as SplitRow list)
struct BandedSide : BandedLayout {
  bool on = false;
  int nBands = 0, world = 1, rank = 0;
  std::vector<int64_t> rankBands, ownerBounds;    // world + 1 band indices / row ids
  DevPtr<SlabSum> dSums;
  DevPtr<void> dRecv;
  DevPtr<const void *> dTable;                     // owned rows x nBands slab pointers (null: no rating of the row in that band)
  int64_t recvSlabs = 0, ownedSolved = 0, nSums = 0;
  int64_t slabElems = 0;
  Event evRecv, evStage[kFewSlabs];  // stage s: the group computed in it is complete (on its piece stream)
};

}  // namespace

struct ycnr_als {
  ycnr_als_options opt{};
  // The streams stand in front of every buffer and event: members are destroyed in reverse order of declaration, so the
  // streams outlive everything their work may touch (ycnr_als_destroy: side streams, piece streams, the handle's own last).
  Stream ownStream;
  // A sharded side is solved in pieces (the exchange of one travels while the next is solved).  The pieces are
  // independent (different rows of the solved matrix), so they alternate over two streams that fork from and join the
  // step's stream: the kernels of piece c + 1 fill the tails of piece c's (one GPU's eighth of the MAL-scale user side,
  // 4 pieces in stream order: 2.5 ms against 2.0 ms in one piece).
  Stream pieceStream[2];
  Stream sideStream[kSideStreams];  // dual classes next to the row kernel (DualPlan)
  hipStream_t stream = nullptr;     // the one half-steps run on: ownStream.get() or the caller's (ycnr_als_set_stream)
  Event evStepStart;
  // Small uploads: the launches of a half-step captured once and replayed (hipGraph).  state: 0 = not run yet (the
  // first half-step runs launch by launch: it sets function attributes), 1 = capture at the next one, 2 = exec is
  // valid, -1 = capture failed once, stay with launches.  Dropped whenever something a kernel argument points
  // at changes (upload, bound matrix, stream).
  struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    int state = 0;
  } graph[2];
  bool graphRun = false;  // the half-step in flight was a graph launch: only ev[0] / ev[4] of its piece are recorded
  void drop_graphs() {
    for (GraphSlot &g : graph) {
      if (g.exec) (void)hipGraphExecDestroy(g.exec);
      g.exec = nullptr;
      g.state = 0;
    }
  }
  void *factors[2] = {nullptr, nullptr};  // what the kernels and ycnr_als_factors_ptr read: the handle's own matrix or a bound one
  DevPtr<void> factorsMem[2];             // the handle's own (empty once the caller has bound theirs: ycnr_als_bind_factors)
  // GramX6P: the fixed matrix of a half-step split into bf16 planes once (als_split_planes_kernel), where it is small
  // enough to stay cache-resident (the user half-step: the item matrix); planes[s] belongs to factors[s]
  DevPtr<unsigned short> planes[2];
  bool planesValid[2] = {false, false};  // the half-step in flight split factors[s] into planes[s]
  int kPad = 0;                          // != 0: float32, factorsCount % 4 != 0: the kernels work on copies padded to a multiple of 4
  ycnr_als_options copt{};               // opt as the kernels see it: factorsCount = kPad when padded (schedules, kernel choice, slab sizes)
  DevPtr<float> padded[2];               // [rows x kPad] copies the kernels of that case work on
  bool autoChunk = false;  // options.chunkRatings was 0: sized per upload (auto_chunk)
  std::vector<Part> parts[2];      // the side's local row shard, cut into pipelined pieces (usually one)
  BandedSide banded[2];            // ycnr_als_set_ratings_banded: the side's half-step is sharded by bands of columns
  bool deferExchange[2] = {false, false};  // ycnr_als_defer_exchange: the side's half-steps leave the solved rows where they are
  std::vector<int64_t> bounds[2];   // sharded upload: row bounds of every rank's pieces, world x (nParts + 1)
  Comm comm;                        // exchange step of the multi-GPU path (comm_impl.hip.h)
  Event evComputeEnd;
  bool exchangedInStep = false;
  Ratings rmse[2];
  double lastRmseMs = -1.0;  // device time of the last ycnr_als_rmse (its kernel, HIP events on the handle's stream)
  // ycnr_als_recommend: its device buffers grow on demand and stay (a second call of the same size allocates nothing)
  enum { REC_USER_IDS, REC_SKIP_PTR, REC_SKIP, REC_PART_V, REC_PART_I, REC_IDS, REC_PRED, REC_CNT, REC_ROWS, REC_SCORES,
         // ycnr_als_fold_in / ycnr_als_recommend_for_ratings: the request's CSR, the solved rows and their status, the ids to store at;
         // factorsCount > 128: the plan of the step kernels (units, split rows, slabs) and their error record
         FOLD_PTR, FOLD_INDX, FOLD_VALS, FOLD_ROWS, FOLD_STATUS, FOLD_STORE, FOLD_UNITS, FOLD_SPLIT, FOLD_SLABS, FOLD_ERR, FOLD_PAD, REC_NBUF };
  GrowBuf<ExactAlloc> rec[REC_NBUF];
  Event recEv[2];
  PiecePlan foldPlan;  // ycnr_als_fold_in beyond 128 factors: the plan whose lists are being copied to the device
  DevPtr<ErrInfo> dErr;
  // The error record is never reset on the device: its count only grows, the host remembers what it has seen
  // (errSeen) and gets the record through an 8-byte copy into page-locked memory at the end of every half-step
  // (before: a memset kernel in front of every half-step and a synchronous copy behind it -- 30 us of a 90 us
  // half-step at the ML-100k shape).
  HostPtr<ErrInfo> hErr;
  int32_t errSeen = 0;
  DevPtr<void> dZeros;  // the zero "factor row" read for ratings past a unit's end
  ycnr_als_step_info info{};  // of the half-step being enqueued / completed
  bool infoPending = false;   // some half-step has been enqueued and not completed by ycnr_als_sync
  int infoSide = 0;           // side of the last half-step enqueued
  // Half-steps of BOTH sides may be in flight (ycnr_als_step_async twice, then ycnr_als_sync: a whole iteration without the
  // host in between).  What ycnr_als_sync needs of each, in the order they were enqueued:
  struct Pending {
    ycnr_als_step_info info{};
    bool graphRun = false, exchanged = false;
  } pend[2];
  int pendOrder[2] = {0, 0}, nPend = 0;
  ycnr_als_step_info infoOf[2] = {};  // the last completed half-step of each side

  int64_t rows(int side) const { return side == YCNR_BY_USER ? opt.totalUsersCount : opt.totalItemsCount; }
  size_t ts() const { return tsize(opt.dtype); }
  // what step_policy.h decides by for a half-step of `side`: the options as the kernels see them (copt)
  StepShape shape(int side) const { return StepShape{copt.dtype == YCNR_F64, copt.factorsCount, (uint32_t)copt.flags, rows(1 - side)}; }
};

// the kernels' arguments for one piece of a side: its schedule and ratings, the two factor matrices (or their padded copies)
template <typename T>
static StepArgs<T> step_args(const ycnr_als *h, int side, const Part &part, const void *fixed, void *solved) {
  const double lambda = side == YCNR_BY_USER ? h->copt.userFactReg : h->copt.itemFactReg;
  return StepArgs<T>{part.S.dUnits.get(), part.S.dSplit.get(), part.R.dIndx.get(), (const T *)part.R.dVals.get(), (const T *)fixed, (const T *)h->dZeros.get(), (T *)solved,
                     (T *)part.S.dSlabs.get(), h->dErr.get(), lambda, h->copt.factorsCount, 0, 0,
                     use_slab_x6(h->shape(side)) ? (uint32_t)(h->rows(1 - side) * h->copt.factorsCount * 4) : 0u};
}

extern "C" {

const char *ycnr_last_error(void) { return g_last_error.c_str(); }

int ycnr_version(void) { return YCNR_ALS_ABI_VERSION; }

int ycnr_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(YCNR_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
  return n;
}

// ---- N1: split + stats (prep_kernels.hip.h) ----
namespace {
int timed(hipEvent_t e0, hipEvent_t e1, double *ms) {
  HIP_TRY(hipEventRecord(e1, nullptr));
  HIP_TRY(hipEventSynchronize(e1));
  float f = 0;
  HIP_TRY(hipEventElapsedTime(&f, e0, e1));
  if (ms) *ms = f;
  return YCNR_OK;
}
}  // namespace

int ycnr_split_to_sets(int64_t rows, const int64_t *rowPtr, int8_t *types, const int32_t pcts[3], uint32_t seed,
                       double *deviceMs) {
  if (rows < 0 || !rowPtr || !pcts) return fail(YCNR_ERR_INVALID, "ycnr_split_to_sets: null argument");
  if (pcts[0] < 0 || pcts[1] < 0 || pcts[2] < 0 || pcts[0] + pcts[1] + pcts[2] != 100)
    return fail(YCNR_ERR_INVALID, "ycnr_split_to_sets: dataSetDistr %d/%d/%d does not sum to 100", pcts[0], pcts[1], pcts[2]);
  if (rows == 0) return YCNR_OK;
  if (rowPtr[0] != 0) return fail(YCNR_ERR_INVALID, "ycnr_split_to_sets: rowPtr[0] != 0");
  const int64_t nnz = rowPtr[rows];
  if (nnz < 0 || (nnz > 0 && !types)) return fail(YCNR_ERR_INVALID, "ycnr_split_to_sets: bad nnz / null types");
  if (rows >= ((int64_t)1 << 31)) return fail(YCNR_ERR_UNSUPPORTED, "ycnr_split_to_sets: more than 2^31 rows");
  for (int64_t r = 0; r < rows; ++r) {
    if (rowPtr[r + 1] < rowPtr[r]) return fail(YCNR_ERR_INVALID, "ycnr_split_to_sets: rowPtr decreases at row %lld", (long long)r);
    if (rowPtr[r + 1] - rowPtr[r] >= ((int64_t)1 << 31)) return fail(YCNR_ERR_UNSUPPORTED, "row %lld too long", (long long)r);
  }
  if (nnz == 0) return YCNR_OK;
  DevPtr<void> dPtr, dTypes;
  HIP_TRY(hipMalloc(dPtr.put(), (size_t)(rows + 1) * 8));
  HIP_TRY(hipMalloc(dTypes.put(), (size_t)nnz));
  HIP_TRY(hipMemcpy(dPtr.get(), rowPtr, (size_t)(rows + 1) * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dTypes.get(), types, (size_t)nnz, hipMemcpyHostToDevice));
  Event ev0, ev1;
  HIP_TRY(hipEventCreate(ev0.put()));
  HIP_TRY(hipEventCreate(ev1.put()));
  const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
  HIP_TRY(hipEventRecord(e0, nullptr));
  // three classes of rows: up to kSplitRankRow ratings one wave ranks every rating (O(n^2 / 64), cheapest for short rows);
  // longer ones find the two thresholds by bisection instead -- one wave up to kSplitShortRow ratings, a 1024-thread
  // workgroup beyond (whose 60 KB of LDS would leave two waves per CU for everybody, hence the separate launch)
  std::vector<int32_t> lists[3];
  for (int64_t r = 0; r < rows; ++r) {
    const int64_t n = rowPtr[r + 1] - rowPtr[r];
    if (n > 0) lists[n > kSplitShortRow ? 1 : n > kSplitRankRow ? 2 : 0].push_back((int32_t)r);
  }
  // longest first within the long classes (they set the tail)
  for (int q = 1; q < 3; ++q)
    std::stable_sort(lists[q].begin(), lists[q].end(),
                     [&](int32_t x, int32_t y) { return rowPtr[x + 1] - rowPtr[x] > rowPtr[y + 1] - rowPtr[y]; });
  DevPtr<void> dList[3];
  for (int q = 0; q < 3; ++q) {
    if (lists[q].empty()) continue;
    HIP_TRY(hipMalloc(dList[q].put(), lists[q].size() * 4));
    HIP_TRY(hipMemcpy(dList[q].get(), lists[q].data(), lists[q].size() * 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipEventRecord(e0, nullptr));  // the kernels only (lists are part of the upload)
  if (!lists[1].empty())
    hipLaunchKernelGGL((split_to_sets_select_kernel<kSplitLdsKeys, 1024>), dim3((unsigned)lists[1].size()), dim3(1024), 0, nullptr, (const int64_t *)dPtr.get(),
                       (const int32_t *)dList[1].get(), (int64_t)lists[1].size(), (int8_t *)dTypes.get(), (int)pcts[0], (int)pcts[1], seed);
  if (!lists[2].empty())
    hipLaunchKernelGGL((split_to_sets_select_kernel<kSplitShortRow, 64>), dim3((unsigned)std::min<size_t>(lists[2].size(), (size_t)1 << 20)), dim3(64), 0,
                       nullptr, (const int64_t *)dPtr.get(), (const int32_t *)dList[2].get(), (int64_t)lists[2].size(), (int8_t *)dTypes.get(),
                       (int)pcts[0], (int)pcts[1], seed);
  if (!lists[0].empty())
    hipLaunchKernelGGL((split_to_sets_kernel<kSplitRankRow, 64>), dim3((unsigned)std::min<size_t>(lists[0].size(), (size_t)1 << 20)), dim3(64), 0,
                       nullptr, (const int64_t *)dPtr.get(), (const int32_t *)dList[0].get(), (int64_t)lists[0].size(), (int8_t *)dTypes.get(),
                       (int)pcts[0], (int)pcts[1], seed);
  hipError_t le = hipGetLastError();
  int rc = le == hipSuccess ? timed(e0, e1, deviceMs) : fail(YCNR_ERR_HIP, "split_to_sets launch: %s", hipGetErrorString(le));
  if (rc) return rc;
  HIP_TRY(hipMemcpy(types, dTypes.get(), (size_t)nnz, hipMemcpyDeviceToHost));
  return YCNR_OK;
}

int ycnr_rating_stats(int dtype, int64_t rows, const int64_t *rowPtr, const void *vals, const int8_t *types,
                      int32_t *cnt, double *sum, double *deviceMs) {
  if (rows < 0 || !rowPtr || !cnt || !sum) return fail(YCNR_ERR_INVALID, "ycnr_rating_stats: null argument");
  if (dtype != YCNR_F32 && dtype != YCNR_F64) return fail(YCNR_ERR_INVALID, "bad dtype %d", dtype);
  if (rows == 0) return YCNR_OK;
  if (rowPtr[0] != 0) return fail(YCNR_ERR_INVALID, "ycnr_rating_stats: rowPtr[0] != 0");
  const int64_t nnz = rowPtr[rows];
  if (nnz < 0 || (nnz > 0 && !vals)) return fail(YCNR_ERR_INVALID, "ycnr_rating_stats: bad nnz / null vals");
  const size_t ts = tsize(dtype);
  DevPtr<void> dPtr, dVals, dTypes, dCnt, dSum;
  HIP_TRY(hipMalloc(dPtr.put(), (size_t)(rows + 1) * 8));
  HIP_TRY(hipMalloc(dVals.put(), std::max<size_t>((size_t)nnz * ts, 8)));
  HIP_TRY(hipMalloc(dCnt.put(), (size_t)rows * 4));
  HIP_TRY(hipMalloc(dSum.put(), (size_t)rows * 8));
  HIP_TRY(hipMemcpy(dPtr.get(), rowPtr, (size_t)(rows + 1) * 8, hipMemcpyHostToDevice));
  if (nnz) HIP_TRY(hipMemcpy(dVals.get(), vals, (size_t)nnz * ts, hipMemcpyHostToDevice));
  if (types && nnz) {
    HIP_TRY(hipMalloc(dTypes.put(), (size_t)nnz));
    HIP_TRY(hipMemcpy(dTypes.get(), types, (size_t)nnz, hipMemcpyHostToDevice));
  }
  Event ev0, ev1;
  HIP_TRY(hipEventCreate(ev0.put()));
  HIP_TRY(hipEventCreate(ev1.put()));
  const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
  HIP_TRY(hipEventRecord(e0, nullptr));
  constexpr int64_t kLongRow = 2048;  // longer rows: a workgroup per segment of kStatsSegment ratings, then the segments in order
  std::vector<int32_t> longRows, segRow;
  std::vector<int64_t> segBeg, firstSeg;
  for (int64_t r = 0; r < rows; ++r) {
    const int64_t n = rowPtr[r + 1] - rowPtr[r];
    if (n <= kLongRow) continue;
    longRows.push_back((int32_t)r);
    firstSeg.push_back((int64_t)segRow.size());
    for (int64_t b = rowPtr[r]; b < rowPtr[r + 1]; b += kStatsSegment) {
      segRow.push_back((int32_t)r);
      segBeg.push_back(b);
    }
  }
  firstSeg.push_back((int64_t)segRow.size());
  DevPtr<void> dLong, dSegRow, dSegBeg, dFirst, dPartCnt, dPartSum;
  if (!longRows.empty()) {
    HIP_TRY(hipMalloc(dLong.put(), longRows.size() * 4));
    HIP_TRY(hipMalloc(dSegRow.put(), segRow.size() * 4));
    HIP_TRY(hipMalloc(dSegBeg.put(), segBeg.size() * 8));
    HIP_TRY(hipMalloc(dFirst.put(), firstSeg.size() * 8));
    HIP_TRY(hipMalloc(dPartCnt.put(), segRow.size() * 4));
    HIP_TRY(hipMalloc(dPartSum.put(), segRow.size() * 8));
    HIP_TRY(hipMemcpy(dLong.get(), longRows.data(), longRows.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dSegRow.get(), segRow.data(), segRow.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dSegBeg.get(), segBeg.data(), segBeg.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dFirst.get(), firstSeg.data(), firstSeg.size() * 8, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipEventRecord(e0, nullptr));
  const unsigned blocks = (unsigned)((rows * 16 + 255) / 256);
  const unsigned nSeg = (unsigned)segRow.size(), nLong = (unsigned)longRows.size();
  if (dtype == YCNR_F32) {
    if (nLong)  // (first: its workgroups are the long ones)
      hipLaunchKernelGGL(rating_stats_long_kernel<float>, dim3(nSeg), dim3(256), 0, nullptr, (const int64_t *)dPtr.get(), (const int32_t *)dSegRow.get(),
                         (const int64_t *)dSegBeg.get(), (const float *)dVals.get(), (const int8_t *)dTypes.get(), (int32_t *)dPartCnt.get(), (double *)dPartSum.get());
    hipLaunchKernelGGL(rating_stats_kernel<float>, dim3(blocks), dim3(256), 0, nullptr, (const int64_t *)dPtr.get(), rows,
                       (const float *)dVals.get(), (const int8_t *)dTypes.get(), (int32_t *)dCnt.get(), (double *)dSum.get(), kLongRow);
  } else {
    if (nLong)
      hipLaunchKernelGGL(rating_stats_long_kernel<double>, dim3(nSeg), dim3(256), 0, nullptr, (const int64_t *)dPtr.get(), (const int32_t *)dSegRow.get(),
                         (const int64_t *)dSegBeg.get(), (const double *)dVals.get(), (const int8_t *)dTypes.get(), (int32_t *)dPartCnt.get(), (double *)dPartSum.get());
    hipLaunchKernelGGL(rating_stats_kernel<double>, dim3(blocks), dim3(256), 0, nullptr, (const int64_t *)dPtr.get(), rows,
                       (const double *)dVals.get(), (const int8_t *)dTypes.get(), (int32_t *)dCnt.get(), (double *)dSum.get(), kLongRow);
  }
  if (nLong)
    hipLaunchKernelGGL(rating_stats_combine_kernel, dim3((nLong + 255) / 256), dim3(256), 0, nullptr, (const int32_t *)dLong.get(), (const int64_t *)dFirst.get(),
                       (int64_t)nLong, (const int32_t *)dPartCnt.get(), (const double *)dPartSum.get(), (int32_t *)dCnt.get(), (double *)dSum.get());
  hipError_t le = hipGetLastError();
  int rc = le == hipSuccess ? timed(e0, e1, deviceMs) : fail(YCNR_ERR_HIP, "rating_stats launch: %s", hipGetErrorString(le));
  if (rc) return rc;
  HIP_TRY(hipMemcpy(cnt, dCnt.get(), (size_t)rows * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sum, dSum.get(), (size_t)rows * 8, hipMemcpyDeviceToHost));
  return YCNR_OK;
}

// ---- N2: CSR from triplets / transpose ----
namespace {
int bits_for(int64_t n) {
  int b = 1;
  while (b < 32 && ((int64_t)1 << b) < n) ++b;
  return b;
}
// makeKeys launches the kernel that writes keys / pos on the device; then sorts and unpacks into host arrays.  Every
// buffer is allocated BEFORE the first timing event: the events bracket kernels only.  (Round 3 allocated six buffers
// between the two events; the host time of those hipMalloc calls -- 10 ... 110 ms depending on the box -- was reported as
// device time of the sort.)
int sort_and_unpack(int dtype, int64_t n, int64_t outRows, int64_t outCols, uint64_t *dKeys, uint32_t *dPos, const void *dVals,
                    int64_t *rowPtr, int32_t *indx, void *outVals, const std::function<void()> &makeKeys, double *deviceMs) {
  const size_t ts = tsize(dtype);
  DevPtr<void> dKeys2, dPos2, dTmp, dIndx, dOutVals, dPtr;
  HIP_TRY(hipMalloc(dKeys2.put(), (size_t)n * 8));
  HIP_TRY(hipMalloc(dPos2.put(), (size_t)n * 4));
  HIP_TRY(hipMalloc(dIndx.put(), (size_t)n * 4));
  HIP_TRY(hipMalloc(dOutVals.put(), (size_t)n * ts));
  HIP_TRY(hipMalloc(dPtr.put(), (size_t)(outRows + 1) * 8));
  size_t tmpBytes = 0;
  const int colBits = bits_for(outCols), endBit = colBits + bits_for(outRows);
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmpBytes, dKeys, (uint64_t *)dKeys2.get(), dPos, (uint32_t *)dPos2.get(), (int)n, 0, endBit));
  HIP_TRY(hipMalloc(dTmp.put(), std::max<size_t>(tmpBytes, 8)));
  Event ev0, ev1;
  HIP_TRY(hipEventCreate(ev0.put()));
  HIP_TRY(hipEventCreate(ev1.put()));
  const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipEventRecord(e0, nullptr));
  makeKeys();
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(dTmp.get(), tmpBytes, dKeys, (uint64_t *)dKeys2.get(), dPos, (uint32_t *)dPos2.get(), (int)n, 0, endBit));
  const unsigned b256 = (unsigned)((n + 255) / 256);
  if (dtype == YCNR_F32)
    hipLaunchKernelGGL(unpack_sorted_kernel<float>, dim3(b256), dim3(256), 0, nullptr, (const uint64_t *)dKeys2.get(), (const uint32_t *)dPos2.get(),
                       (const float *)dVals, n, colBits, (int32_t *)dIndx.get(), (float *)dOutVals.get());
  else
    hipLaunchKernelGGL(unpack_sorted_kernel<double>, dim3(b256), dim3(256), 0, nullptr, (const uint64_t *)dKeys2.get(), (const uint32_t *)dPos2.get(),
                       (const double *)dVals, n, colBits, (int32_t *)dIndx.get(), (double *)dOutVals.get());
  hipLaunchKernelGGL(row_ptr_kernel, dim3((unsigned)((outRows + 1 + 255) / 256)), dim3(256), 0, nullptr, (const uint64_t *)dKeys2.get(), n, outRows, colBits,
                     (int64_t *)dPtr.get());
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(YCNR_ERR_HIP, "csr build: %s", hipGetErrorString(le));
  int rc = timed(e0, e1, deviceMs);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(rowPtr, dPtr.get(), (size_t)(outRows + 1) * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(indx, dIndx.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(outVals, dOutVals.get(), (size_t)n * ts, hipMemcpyDeviceToHost));
  return YCNR_OK;
}
}  // namespace

int ycnr_csr_from_triplets(int dtype, int64_t n, const int32_t *rowIdx, const int32_t *colIdx, const void *vals,
                           int64_t rows, int64_t cols, int64_t *rowPtr, int32_t *indx, void *outVals, double *deviceMs) {
  if (dtype != YCNR_F32 && dtype != YCNR_F64) return fail(YCNR_ERR_INVALID, "bad dtype %d", dtype);
  if (n < 0 || rows < 0 || cols < 0 || !rowPtr) return fail(YCNR_ERR_INVALID, "ycnr_csr_from_triplets: bad sizes / null rowPtr");
  if (rows >= ((int64_t)1 << 31) || cols >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31))
    return fail(YCNR_ERR_UNSUPPORTED, "ycnr_csr_from_triplets: more than 2^31 rows, columns or ratings");
  if (n == 0) {
    for (int64_t r = 0; r <= rows; ++r) rowPtr[r] = 0;
    return YCNR_OK;
  }
  if (!rowIdx || !colIdx || !vals || !indx || !outVals) return fail(YCNR_ERR_INVALID, "ycnr_csr_from_triplets: null array");
  for (int64_t q = 0; q < n; ++q)
    if (rowIdx[q] < 0 || rowIdx[q] >= rows || colIdx[q] < 0 || colIdx[q] >= cols)
      return fail(YCNR_ERR_INVALID, "triplet %lld: (%d, %d) outside %lld x %lld", (long long)q, rowIdx[q], colIdx[q], (long long)rows,
                  (long long)cols);
  const size_t ts = tsize(dtype);
  DevPtr<void> dR, dC, dV, dKeys, dPos;
  HIP_TRY(hipMalloc(dR.put(), (size_t)n * 4));
  HIP_TRY(hipMalloc(dC.put(), (size_t)n * 4));
  HIP_TRY(hipMalloc(dV.put(), (size_t)n * ts));
  HIP_TRY(hipMalloc(dKeys.put(), (size_t)n * 8));
  HIP_TRY(hipMalloc(dPos.put(), (size_t)n * 4));
  HIP_TRY(hipMemcpy(dR.get(), rowIdx, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dC.get(), colIdx, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dV.get(), vals, (size_t)n * ts, hipMemcpyHostToDevice));
  auto makeKeys = [&] {
    hipLaunchKernelGGL(make_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, (const int32_t *)dR.get(), (const int32_t *)dC.get(), n,
                       bits_for(cols), (uint64_t *)dKeys.get(), (uint32_t *)dPos.get());
  };
  return sort_and_unpack(dtype, n, rows, cols, (uint64_t *)dKeys.get(), (uint32_t *)dPos.get(), dV.get(), rowPtr, indx, outVals, makeKeys, deviceMs);
}

int ycnr_csr_transpose(int dtype, int64_t rows, int64_t cols, const int64_t *rowPtr, const int32_t *indx, const void *vals,
                       int64_t *outPtr, int32_t *outIndx, void *outVals, double *deviceMs) {
  if (dtype != YCNR_F32 && dtype != YCNR_F64) return fail(YCNR_ERR_INVALID, "bad dtype %d", dtype);
  if (rows < 0 || cols < 0 || !rowPtr || !outPtr) return fail(YCNR_ERR_INVALID, "ycnr_csr_transpose: bad sizes / null rowPtr");
  if (rowPtr[0] != 0) return fail(YCNR_ERR_INVALID, "ycnr_csr_transpose: rowPtr[0] != 0");
  const int64_t n = rowPtr[rows];
  if (rows >= ((int64_t)1 << 31) || cols >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31))
    return fail(YCNR_ERR_UNSUPPORTED, "ycnr_csr_transpose: more than 2^31 rows, columns or ratings");
  for (int64_t r = 0; r < rows; ++r)
    if (rowPtr[r + 1] < rowPtr[r]) return fail(YCNR_ERR_INVALID, "ycnr_csr_transpose: rowPtr decreases at row %lld", (long long)r);
  if (n == 0) {
    for (int64_t c = 0; c <= cols; ++c) outPtr[c] = 0;
    return YCNR_OK;
  }
  if (!indx || !vals || !outIndx || !outVals) return fail(YCNR_ERR_INVALID, "ycnr_csr_transpose: null array");
  for (int64_t q = 0; q < n; ++q)
    if (indx[q] < 0 || indx[q] >= cols) return fail(YCNR_ERR_INVALID, "entry %lld: column %d outside %lld", (long long)q, indx[q], (long long)cols);
  const size_t ts = tsize(dtype);
  DevPtr<void> dP, dI, dV, dPos, dRowOf, dKeys2, dPos2, dTmp, dIndx, dOutVals, dPtr;
  HIP_TRY(hipMalloc(dP.put(), (size_t)(rows + 1) * 8));
  HIP_TRY(hipMalloc(dI.put(), (size_t)n * 4));
  HIP_TRY(hipMalloc(dV.put(), (size_t)n * ts));
  HIP_TRY(hipMalloc(dPos.put(), (size_t)n * 4));
  HIP_TRY(hipMalloc(dRowOf.put(), (size_t)n * 4));
  HIP_TRY(hipMalloc(dKeys2.put(), (size_t)n * 4));
  HIP_TRY(hipMalloc(dPos2.put(), (size_t)n * 4));
  HIP_TRY(hipMalloc(dIndx.put(), (size_t)n * 4));
  HIP_TRY(hipMalloc(dOutVals.put(), (size_t)n * ts));
  HIP_TRY(hipMalloc(dPtr.put(), (size_t)(cols + 1) * 8));
  HIP_TRY(hipMemcpy(dP.get(), rowPtr, (size_t)(rows + 1) * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dI.get(), indx, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dV.get(), vals, (size_t)n * ts, hipMemcpyHostToDevice));
  // a stable sort of the positions by column id alone (prep_kernels.hip.h): the ids are non-negative, so they sort as uint32
  size_t tmpBytes = 0;
  const int endBit = bits_for(cols);
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmpBytes, (const uint32_t *)dI.get(), (uint32_t *)dKeys2.get(), (const uint32_t *)dPos.get(),
                                             (uint32_t *)dPos2.get(), (int)n, 0, endBit));
  HIP_TRY(hipMalloc(dTmp.put(), std::max<size_t>(tmpBytes, 8)));
  Event ev0, ev1;
  HIP_TRY(hipEventCreate(ev0.put()));
  HIP_TRY(hipEventCreate(ev1.put()));
  const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
  HIP_TRY(hipEventRecord(e0, nullptr));
  const unsigned b256 = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(iota_rows_kernel, dim3(b256), dim3(256), 0, nullptr, (const int64_t *)dP.get(), rows, n, (uint32_t *)dPos.get(), (int32_t *)dRowOf.get());
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(dTmp.get(), tmpBytes, (const uint32_t *)dI.get(), (uint32_t *)dKeys2.get(), (const uint32_t *)dPos.get(),
                                             (uint32_t *)dPos2.get(), (int)n, 0, endBit));
  if (dtype == YCNR_F32)
    hipLaunchKernelGGL(unpack_transposed_kernel<float>, dim3(b256), dim3(256), 0, nullptr, (const uint32_t *)dPos2.get(), (const int32_t *)dRowOf.get(),
                       (const float *)dV.get(), n, (int32_t *)dIndx.get(), (float *)dOutVals.get());
  else
    hipLaunchKernelGGL(unpack_transposed_kernel<double>, dim3(b256), dim3(256), 0, nullptr, (const uint32_t *)dPos2.get(), (const int32_t *)dRowOf.get(),
                       (const double *)dV.get(), n, (int32_t *)dIndx.get(), (double *)dOutVals.get());
  hipLaunchKernelGGL(row_ptr32_kernel, dim3((unsigned)((cols + 1 + 255) / 256)), dim3(256), 0, nullptr, (const uint32_t *)dKeys2.get(), n, cols,
                     (int64_t *)dPtr.get());
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(YCNR_ERR_HIP, "csr transpose: %s", hipGetErrorString(le));
  int rc = timed(e0, e1, deviceMs);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(outPtr, dPtr.get(), (size_t)(cols + 1) * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(outIndx, dIndx.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(outVals, dOutVals.get(), (size_t)n * ts, hipMemcpyDeviceToHost));
  return YCNR_OK;
}

// ---- N3: top-N recommend ----
int ycnr_recommend_items(int dtype, int32_t k, int64_t nUsers, const void *userRows, int64_t totalItems, const void *itemFactors,
                         const int64_t *skipPtr, const int32_t *skipIds, double globalAvgShift, double minRecommendRating,
                         int32_t limit, int32_t *outIds, double *outPredict, int32_t *outCount, double *deviceMs) {
  if (dtype != YCNR_F32 && dtype != YCNR_F64) return fail(YCNR_ERR_INVALID, "bad dtype %d", dtype);
  if (k < 1 || k > 4096 || nUsers < 0 || totalItems < 0 || limit < 1 || limit > 4096)
    return fail(YCNR_ERR_INVALID, "ycnr_recommend_items: bad k / sizes / limit");
  if (totalItems >= ((int64_t)1 << 31)) return fail(YCNR_ERR_UNSUPPORTED, "ycnr_recommend_items: more than 2^31 items");
  if (nUsers == 0) return YCNR_OK;
  if (!userRows || !skipPtr || !outIds || !outPredict || !outCount || (totalItems > 0 && !itemFactors))
    return fail(YCNR_ERR_INVALID, "ycnr_recommend_items: null argument");
  if (skipPtr[0] != 0) return fail(YCNR_ERR_INVALID, "ycnr_recommend_items: skipPtr[0] != 0");
  for (int64_t u = 0; u < nUsers; ++u) {
    if (skipPtr[u + 1] > skipPtr[u] && !skipIds) return fail(YCNR_ERR_INVALID, "ycnr_recommend_items: null skipIds");
    if (skipPtr[u + 1] < skipPtr[u]) return fail(YCNR_ERR_INVALID, "ycnr_recommend_items: skipPtr decreases at user %lld", (long long)u);
    for (int64_t q = skipPtr[u]; q < skipPtr[u + 1]; ++q)
      if (q > skipPtr[u] && skipIds[q] <= skipIds[q - 1])
        return fail(YCNR_ERR_INVALID, "ycnr_recommend_items: skip ids of user %lld are not strictly ascending", (long long)u);
  }
  const int64_t nSkip = skipPtr[nUsers];
  if (nSkip > 0 && !skipIds) return fail(YCNR_ERR_INVALID, "ycnr_recommend_items: null skipIds");
  const size_t ts = tsize(dtype);
  const int take = limit - 1;  // lib/YcnrController.js:268-269
  // users in batches whose score matrix stays below 1 GB
  const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(nUsers, ((int64_t)1 << 27) / std::max<int64_t>(1, totalItems)));
  DevPtr<void> dItems, dUsers, dSkipPtr, dSkip, dScores, dIds, dPred, dCnt;
  HIP_TRY(hipMalloc(dItems.put(), std::max<size_t>((size_t)totalItems * k * ts, 8)));
  HIP_TRY(hipMalloc(dUsers.put(), (size_t)batch * k * ts));
  HIP_TRY(hipMalloc(dSkipPtr.put(), (size_t)(batch + 1) * 8));
  HIP_TRY(hipMalloc(dSkip.put(), std::max<size_t>((size_t)nSkip * 4, 8)));
  HIP_TRY(hipMalloc(dScores.put(), std::max<size_t>((size_t)batch * totalItems * 8, 8)));
  HIP_TRY(hipMalloc(dIds.put(), (size_t)batch * limit * 4));
  HIP_TRY(hipMalloc(dPred.put(), (size_t)batch * limit * 8));
  HIP_TRY(hipMalloc(dCnt.put(), (size_t)batch * 4));
  if (totalItems) HIP_TRY(hipMemcpy(dItems.get(), itemFactors, (size_t)totalItems * k * ts, hipMemcpyHostToDevice));
  if (nSkip) HIP_TRY(hipMemcpy(dSkip.get(), skipIds, (size_t)nSkip * 4, hipMemcpyHostToDevice));
  Event ev0, ev1;
  HIP_TRY(hipEventCreate(ev0.put()));
  HIP_TRY(hipEventCreate(ev1.put()));
  const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
  double total = 0.0;
  int rc = YCNR_OK;
  std::vector<int64_t> localPtr;
  for (int64_t u0 = 0; u0 < nUsers && !rc; u0 += batch) {
    const int64_t nb = std::min(batch, nUsers - u0);
    localPtr.assign(skipPtr + u0, skipPtr + u0 + nb + 1);  // absolute offsets into dSkip
    HIP_TRY(hipMemcpy(dUsers.get(), (const char *)userRows + (size_t)u0 * k * ts, (size_t)nb * k * ts, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dSkipPtr.get(), localPtr.data(), (size_t)(nb + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipEventRecord(e0, nullptr));
    // scores on the matrix cores: 16 users per workgroup, the item tiles dealt over the waves of gridDim.y workgroups
    // (YCNR_RECOMMEND_VALU=1: the 16-lane-group kernel, one user per workgroup, for A/B runs)
    const size_t kp = (size_t)((k + 15) & ~15);
    const unsigned ublk = (unsigned)((nb + 15) / 16);
    const unsigned yblk = (unsigned)std::max<int64_t>(1, std::min<int64_t>((totalItems + 63) / 64, (8 * device_cus() + ublk - 1) / ublk));
    const bool valu = getenv("YCNR_RECOMMEND_VALU") != nullptr || 16 * kp * ts > 48 * 1024;  // (16 users' factors must fit the default LDS limit)
    if (dtype == YCNR_F32) {
      if (valu)
        hipLaunchKernelGGL((recommend_scores_kernel<float, 1>), dim3((unsigned)nb), dim3(256), (size_t)k * ts, nullptr, (const float *)dUsers.get(), nb,
                           (const float *)dItems.get(), totalItems, (int)k, globalAvgShift, minRecommendRating, (double *)dScores.get());
      else
        hipLaunchKernelGGL(recommend_scores_mfma_kernel<float>, dim3(ublk, yblk), dim3(256), 16 * kp * ts, nullptr, (const float *)dUsers.get(), nb,
                           (const float *)dItems.get(), totalItems, (int)k, globalAvgShift, minRecommendRating, (double *)dScores.get());
    } else {
      if (valu)
        hipLaunchKernelGGL((recommend_scores_kernel<double, 1>), dim3((unsigned)nb), dim3(256), (size_t)k * ts, nullptr, (const double *)dUsers.get(), nb,
                           (const double *)dItems.get(), totalItems, (int)k, globalAvgShift, minRecommendRating, (double *)dScores.get());
      else
        hipLaunchKernelGGL(recommend_scores_mfma_kernel<double>, dim3(ublk, yblk), dim3(256), 16 * kp * ts, nullptr, (const double *)dUsers.get(), nb,
                           (const double *)dItems.get(), totalItems, (int)k, globalAvgShift, minRecommendRating, (double *)dScores.get());
    }
    if (nSkip)
      hipLaunchKernelGGL(recommend_skip_kernel, dim3((unsigned)nb), dim3(256), 0, nullptr, (const int64_t *)dSkipPtr.get(), (const int32_t *)dSkip.get(), totalItems,
                         (double *)dScores.get());
    hipLaunchKernelGGL(recommend_select_kernel, dim3((unsigned)nb), dim3(256), 0, nullptr, (double *)dScores.get(), totalItems, take, (int)limit,
                       (int32_t *)dIds.get(), (double *)dPred.get(), (int32_t *)dCnt.get());
    hipError_t le = hipGetLastError();
    double ms = 0.0;
    rc = le == hipSuccess ? timed(e0, e1, &ms) : fail(YCNR_ERR_HIP, "recommend launch: %s", hipGetErrorString(le));
    total += ms;
    if (rc) break;
    HIP_TRY(hipMemcpy(outIds + u0 * limit, dIds.get(), (size_t)nb * limit * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(outPredict + u0 * limit, dPred.get(), (size_t)nb * limit * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(outCount + u0, dCnt.get(), (size_t)nb * 4, hipMemcpyDeviceToHost));
  }
  if (deviceMs) *deviceMs = total;
  return rc;
}

int ycnr_als_create(const ycnr_als_options *o, ycnr_als **out) {
  if (!o || !out) return fail(YCNR_ERR_INVALID, "ycnr_als_create: null argument");
  if (o->struct_size != (int32_t)sizeof(ycnr_als_options))
    return fail(YCNR_ERR_INVALID, "ycnr_als_create: options.struct_size %d != %zu", o->struct_size,
                sizeof(ycnr_als_options));
  if (o->dtype != YCNR_F32 && o->dtype != YCNR_F64) return fail(YCNR_ERR_INVALID, "bad dtype %d", o->dtype);
  if (o->factorsCount < 1) return fail(YCNR_ERR_INVALID, "factorsCount must be >= 1");
  if (o->factorsCount > kMaxFactorsAny)
    return fail(YCNR_ERR_UNSUPPORTED, "factorsCount %d > %d is not supported by this build", o->factorsCount, kMaxFactorsAny);
  if (o->totalUsersCount < 1 || o->totalItemsCount < 1 || o->totalUsersCount > 0x7fffffffLL ||
      o->totalItemsCount > 0x7fffffffLL)
    return fail(YCNR_ERR_INVALID, "totalUsersCount / totalItemsCount must be in [1, 2^31)");
  if (!(o->userFactReg >= 0) || !(o->itemFactReg >= 0)) return fail(YCNR_ERR_INVALID, "negative regularisation");
  if (o->chunkRatings < 0) return fail(YCNR_ERR_INVALID, "chunkRatings < 0");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (o->device < 0 || o->device >= ndev)
    return fail(YCNR_ERR_INVALID, "device %d out of range (%d visible)", o->device, ndev);
  HIP_TRY(hipSetDevice(o->device));
  ycnr_als *h = new (std::nothrow) ycnr_als();
  if (!h) return fail(YCNR_ERR_NOMEM, "out of host memory");
  h->opt = *o;
  if (const char *e = getenv("YCNR_EXTRA_FLAGS")) h->opt.flags |= (uint32_t)atoi(e);  // experiments from unmodified hosts
  h->autoChunk = h->opt.chunkRatings == 0;
  if (h->opt.chunkRatings == 0) h->opt.chunkRatings = kDefaultChunk;
  h->opt.chunkRatings = (h->opt.chunkRatings + 3) & ~3;
  hipError_t e = hipStreamCreateWithFlags(h->ownStream.put(), hipStreamNonBlocking);
  if (e == hipSuccess) e = new_event(h->evComputeEnd, true);
  if (e == hipSuccess) e = new_event(h->evStepStart, false);
  // (the side streams of the one-piece half-step are created when a half-step first needs them: every stream a process creates
  // takes a share of the runtime's 4 or 8 hardware queues, and a sharded run -- step's stream, two piece streams, the
  // communicator's stream -- must not find one of its streams behind another's event waits on a shared queue)
  for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(h->pieceStream[i].put(), hipStreamNonBlocking);
  for (int s = 0; s < 2 && e == hipSuccess; ++s) {
    e = hipMalloc(h->factorsMem[s].put(), (size_t)h->rows(s) * o->factorsCount * h->ts());
    h->factors[s] = h->factorsMem[s].get();
    if (e == hipSuccess) e = hipMemsetAsync(h->factors[s], 0, (size_t)h->rows(s) * o->factorsCount * h->ts(), h->ownStream.get());
  }
  // float32 with factorsCount % 4 != 0: the kernels run on copies of the matrices padded to a multiple of 4 columns (zero columns:
  // lambda n on their diagonal, x = 0 there, the other columns' arithmetic unchanged) -- rows are then 16-byte aligned and every
  // such size takes the bf16x6 / LDS-DMA / dual-form kernels of its padded size instead of the plain float32-MFMA ones
  // (round 3: k > 128 only; round 4: every k).  Costs a pad of the fixed side and an unpad of the solved rows per half-step.
  if (o->dtype == YCNR_F32 && o->factorsCount % 4 != 0 && (o->factorsCount > kMaxFactors || !getenv("YCNR_NO_KPAD_SMALL"))) {  // (the variable: A/B runs)
    h->kPad = (o->factorsCount + 3) & ~3;
    for (int s = 0; s < 2 && e == hipSuccess; ++s) e = hipMalloc(h->padded[s].put(), (size_t)h->rows(s) * h->kPad * sizeof(float));
  }
  h->copt = h->opt;
  if (h->kPad) h->copt.factorsCount = h->kPad;
  if (e == hipSuccess) e = hipMalloc((void **)h->dErr.put(), kErrBytes);  // ErrInfo + room for in-kernel stamps of diagnostic builds
  if (e == hipSuccess) e = hipMemsetAsync(h->dErr.get(), 0, kErrBytes, h->ownStream.get());
  if (e == hipSuccess) e = hipHostMalloc((void **)h->hErr.put(), sizeof(ErrInfo), hipHostMallocDefault);
  if (e == hipSuccess) memset(h->hErr.get(), 0, sizeof(ErrInfo));
  if (e == hipSuccess) e = hipMalloc(h->dZeros.put(), kZeroRowBytes);
  if (e == hipSuccess) e = hipMemsetAsync(h->dZeros.get(), 0, kZeroRowBytes, h->ownStream.get());
  if (e == hipSuccess) e = hipStreamSynchronize(h->ownStream.get());
  if (e != hipSuccess) {
    int code = fail(e == hipErrorOutOfMemory ? YCNR_ERR_NOMEM : YCNR_ERR_HIP, "ycnr_als_create: %s",
                    hipGetErrorString(e));
    ycnr_als_destroy(h);
    return code;
  }
  h->stream = h->ownStream.get();
  *out = h;
  return YCNR_OK;
}

int ycnr_als_destroy(ycnr_als *h) {
  if (!h) return YCNR_OK;
  (void)hipSetDevice(h->opt.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->drop_graphs();
  comm_release(h->comm);
  delete h;  // the members free what they own; the streams go last (their place in the struct)
  return YCNR_OK;
}

int ycnr_als_set_stream(ycnr_als *h, void *s) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->opt.device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->drop_graphs();
  h->stream = s == YCNR_OWN_STREAM ? h->ownStream.get() : (hipStream_t)s;  // NULL = the null (default) stream
  return YCNR_OK;
}

static int upload_ratings(ycnr_als *h, Ratings &R, int64_t totalRows, int64_t oppositeRows,
                          const int64_t *rowPtr, const int32_t *indx, const void *vals, int64_t rowBegin,
                          int64_t rowEnd, int memKind, std::vector<int64_t> &hostPtr, const char *what) {
  if (!rowPtr || !indx || !vals) return fail(YCNR_ERR_INVALID, "%s: null array", what);
  if (rowBegin < 0 || rowEnd < rowBegin || rowEnd > totalRows)
    return fail(YCNR_ERR_INVALID, "%s: shard [%lld, %lld) outside [0, %lld)", what, (long long)rowBegin,
                (long long)rowEnd, (long long)totalRows);
  if (memKind != YCNR_MEM_HOST && memKind != YCNR_MEM_DEVICE) return fail(YCNR_ERR_INVALID, "bad memKind");
  HIP_TRY(hipSetDevice(h->opt.device));
  const int64_t nRows = rowEnd - rowBegin;
  hostPtr.resize((size_t)nRows + 1);
  if (memKind == YCNR_MEM_HOST) {
    memcpy(hostPtr.data(), rowPtr + rowBegin, sizeof(int64_t) * ((size_t)nRows + 1));
  } else {
    HIP_TRY(hipMemcpy(hostPtr.data(), rowPtr + rowBegin, sizeof(int64_t) * ((size_t)nRows + 1),
                      hipMemcpyDeviceToHost));
  }
  for (int64_t r = 0; r < nRows; ++r)
    if (hostPtr[r + 1] < hostPtr[r]) return fail(YCNR_ERR_INVALID, "%s: rowPtr not ascending at row %lld", what,
                                                 (long long)(rowBegin + r));
  if (hostPtr[0] < 0) return fail(YCNR_ERR_INVALID, "%s: negative rowPtr", what);
  const int64_t base = hostPtr[0], nnz = hostPtr[nRows] - base;
  R = Ratings();  // what the destination held goes before the new arrays are allocated; a failure below leaves it unloaded
  Ratings N;      // (an early return frees what has been built)
  N.rowBegin = rowBegin;
  N.rowEnd = rowEnd;
  N.nnz = nnz;
  const size_t ts = h->ts();
  // 64 bytes of slack: the bf16x6 kernel reads ids and ratings with 16-byte vector loads
  HIP_TRY(hipMalloc(N.dIndx.put(), (size_t)nnz * 4 + 64));
  HIP_TRY(hipMalloc(N.dVals.put(), (size_t)nnz * ts + 64));
  int rc = copy_in(N.dIndx.get(), indx + base, (size_t)nnz * 4, memKind, h->stream);
  if (rc) return rc;
  rc = copy_in(N.dVals.get(), (const char *)vals + (size_t)base * ts, (size_t)nnz * ts, memKind, h->stream);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  rc = check_index_range(N.dIndx.get(), nnz, oppositeRows, h->stream, what);
  if (rc) return rc;
  N.loaded = true;
  R = std::move(N);
  return YCNR_OK;
}

// Upload + schedule (schedule.h) of one piece [rowBegin, rowEnd) of a side's rows into part.R / part.S, which
// are written only when everything is built (an early return frees what it has made so far).
static int build_part(ycnr_als *h, int side, const int64_t *rowPtr, const int32_t *indx, const void *vals, int64_t rowBegin,
                      int64_t rowEnd, int memKind, Part &part, SideNnz sideNnz) {
  Ratings newR;
  Schedule S;
  std::vector<int64_t> hp;
  int rc = upload_ratings(h, newR, h->rows(side), h->rows(1 - side), rowPtr, indx, vals, rowBegin,
                          rowEnd, memKind, hp, side == YCNR_BY_USER ? "set_ratings(byUser)" : "set_ratings(byItem)");
  if (rc) return rc;
  const StepShape shape = h->shape(side);
  const size_t slabElems = (size_t)resident_slab_elems(shape);
  static const int order = getenv("YCNR_ROW_ORDER") ? atoi(getenv("YCNR_ROW_ORDER")) : -1;  // 0: whole rows stay sorted (A/B)
  const PlanParams P = resident_plan_params(shape, upload_toggles(), h->opt.factorsCount, h->autoChunk, h->copt.chunkRatings, sideNnz, order < 0,
                                            gen_arena_bytes());
  const bool big = P.kind == kWorkgroup;
  S.dualMax = P.dualMax;
  PiecePlan plan = plan_piece(hp.data(), rowBegin, rowEnd - rowBegin, P);
  // Band-major chunks (schedule.h), unless YCNR_FLAG_NO_BANDS: when the fixed matrix is far larger than the last-level
  // cache, in bands of kBandBytes of it
  {
    const int64_t fixedRows = h->rows(1 - side);
    const int64_t rowBytes = (int64_t)h->copt.factorsCount * (int64_t)h->ts();
    int64_t bandBytes = kBandBytes;
    if (const char *e = getenv("YCNR_BAND_MB")) bandBytes = (int64_t)atoi(e) << 20;  // per upload, not per half-step: read live (tests set it)
    if (P.kind == kOneWave && plan.nSlabs > 1 && !(h->copt.flags & YCNR_FLAG_NO_BANDS) && bandBytes > 0 && fixedRows * rowBytes > 2 * bandBytes) {
      // at most kMaxSlabsPerRow / 2 bands, so that a row present in every band still has chunks to
      // spare (very large fixed matrices get wider bands instead of a failed upload)
      const int64_t W = std::max<int64_t>(std::max<int64_t>(1, bandBytes / rowBytes), (fixedRows + kMaxSlabsPerRow / 2 - 1) / (kMaxSlabsPerRow / 2));
      const int nBands = (int)((fixedRows + W - 1) / W);
      const BoundQueries q = band_queries(plan, hp.data(), rowBegin, W, nBands);
      std::vector<int64_t> cuts;
      if (int rc2 = lower_bound_i32(newR.dIndx.get(), q.beg, q.end, q.key, cuts, h->stream)) return rc2;
      const BandCutError bad = band_recut(plan, hp.data(), rowBegin, P, nBands, cuts);
      if (bad.parts) return fail(YCNR_ERR_STATE, "band schedule: %d chunks for row %d", bad.parts, bad.row);
    }
  }
  static_cast<PlanCounts &>(S) = plan;
  S.nUnits = (int64_t)plan.units.size();
  S.nSplit = (int64_t)plan.split.size();
  S.genBatches.swap(plan.genBatches);
  if (big && slab_nb(h->copt.factorsCount) == kPairNB && S.nPrimal > 0 && !env_flags().noPair) {
    int64_t batchRows = kPairBatchRows;
    if (const char *e = getenv("YCNR_PAIR_BATCH_ROWS")) batchRows = std::max(256, atoi(e));  // read per upload
    S.rowSlabRows = std::min<int64_t>(S.nPrimal, batchRows);
    HIP_TRY(hipMalloc(S.dRowSlabs.put(), (size_t)S.rowSlabRows * (size_t)wg_slab_floats(kPairNB) * sizeof(float)));
  }
  if (S.nUnits) {
    HIP_TRY(hipMalloc(S.dUnits.put(), sizeof(Unit) * plan.units.size()));
    HIP_TRY(hipMemcpy(S.dUnits.get(), plan.units.data(), sizeof(Unit) * plan.units.size(), hipMemcpyHostToDevice));
  }
  if (S.nSplit) {
    HIP_TRY(hipMalloc(S.dSplit.put(), sizeof(SplitRow) * plan.split.size()));
    HIP_TRY(hipMemcpy(S.dSplit.get(), plan.split.data(), sizeof(SplitRow) * plan.split.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(S.dSlabs.put(), (size_t)S.arenaSlabs * slabElems * h->ts()));
  }
  part.R = std::move(newR);
  part.S = std::move(S);
  return YCNR_OK;
}


// nParts pieces [b[i], b[i + 1]) of this rank's rows.  Everything is built in locals and committed
// together at the end: a failure on the way leaves the handle's previous upload (or none) intact,
// never new ratings with an old schedule.
static int set_ratings_parts(ycnr_als *h, int side, const int64_t *rowPtr, const int32_t *indx, const void *vals, int memKind,
                             int nParts, const int64_t *b) {
  std::vector<Part> parts((size_t)nParts);
  // The ratings of the WHOLE side that sit in rows long enough to be split (rowPtr describes every row of the side, whatever
  // shard this handle solves): what the automatic chunk length is sized for.  MAL scale: nearly all of the item side's 121 M
  // ratings (-> 3072), a few per cent of the user side's (-> 1024: its chunk kernel is a few hundred waves whose length is
  // the kernel's; with the item side's 3072 it was a 300 us chain in front of every piece's row kernel).
  if (!rowPtr) return fail(YCNR_ERR_INVALID, "set_ratings: null rowPtr");
  SideNnz sideNnz;
  if (h->autoChunk) {
    const int64_t nr = h->rows(side);
    std::vector<int64_t> whole;
    const int64_t *rp = rowPtr;
    if (memKind == YCNR_MEM_DEVICE) {
      whole.resize((size_t)nr + 1);
      HIP_TRY(hipMemcpy(whole.data(), rowPtr, sizeof(int64_t) * ((size_t)nr + 1), hipMemcpyDeviceToHost));
      rp = whole.data();
    }
    sideNnz = side_nnz(rp, nr);
  }
  for (int i = 0; i < nParts; ++i) {
    Part &p = parts[(size_t)i];
    hipError_t e = p.create_events();
    if (e != hipSuccess) return fail(YCNR_ERR_HIP, "set_ratings: hipEventCreate: %s", hipGetErrorString(e));
    int rc = build_part(h, side, rowPtr, indx, vals, b[i], b[i + 1], memKind, p, sideNnz);
    if (rc) return rc;
  }
  HIP_TRY(hipStreamSynchronize(h->stream));  // nothing in flight still reads the previous upload
  h->banded[side] = BandedSide();
  h->deferExchange[side] = false;  // (a new upload exchanges after every half-step again until the host says otherwise)
  h->drop_graphs();
  h->parts[side].swap(parts);  // the previous upload is freed as `parts` goes out of scope
  return YCNR_OK;
}

int ycnr_als_set_ratings(ycnr_als *h, int side, const int64_t *rowPtr, const int32_t *indx, const void *vals,
                         int64_t rowBegin, int64_t rowEnd, int memKind) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (side != YCNR_BY_USER && side != YCNR_BY_ITEM) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  const int64_t b[2] = {rowBegin, rowEnd};
  int rc = set_ratings_parts(h, side, rowPtr, indx, vals, memKind, 1, b);
  if (rc) return rc;
  h->bounds[side].clear();  // no exchange ranges: a plain shard (or the whole matrix)
  return YCNR_OK;
}

int ycnr_als_set_ratings_sharded(ycnr_als *h, int side, const int64_t *rowPtr, const int32_t *indx, const void *vals, int memKind,
                                 int nChunks, int boundsWorld, const int64_t *bounds) {
  if (!h || !bounds) return fail(YCNR_ERR_INVALID, "null argument");
  if (side != YCNR_BY_USER && side != YCNR_BY_ITEM) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  if (nChunks < 1 || nChunks > 64) return fail(YCNR_ERR_INVALID, "set_ratings_sharded: nChunks %d outside [1, 64]", nChunks);
  const int world = h->comm.world, rank = h->comm.rank;
  if (boundsWorld != world)
    return fail(YCNR_ERR_INVALID, "set_ratings_sharded: bounds describe %d rank(s), the handle's communicator has %d", boundsWorld, world);
  const size_t n = (size_t)world * (size_t)(nChunks + 1);
  if (bounds[0] != 0 || bounds[n - 1] != h->rows(side))
    return fail(YCNR_ERR_INVALID, "set_ratings_sharded: the shards must tile rows [0, %lld) (got [%lld, %lld))", (long long)h->rows(side),
                (long long)bounds[0], (long long)bounds[n - 1]);
  int64_t prev = 0;
  for (size_t i = 0; i < n; ++i) {
    if (bounds[i] < prev || bounds[i] > h->rows(side))
      return fail(YCNR_ERR_INVALID, "set_ratings_sharded: bounds must ascend within [0, %lld]", (long long)h->rows(side));
    prev = bounds[i];
  }
  for (int r = 0; r + 1 < world; ++r)
    if (bounds[(size_t)r * (nChunks + 1) + nChunks] != bounds[(size_t)(r + 1) * (nChunks + 1)])
      return fail(YCNR_ERR_INVALID, "set_ratings_sharded: the shards of ranks %d and %d do not meet", r, r + 1);
  int rc = set_ratings_parts(h, side, rowPtr, indx, vals, memKind, nChunks, bounds + (size_t)rank * (nChunks + 1));
  if (!rc) h->bounds[side].assign(bounds, bounds + n);
  // IPC: the peers map this rank's matrices; a matrix bound (ycnr_als_bind_factors) since the communicator was made is
  // published here -- this call is collective, every rank passes through, also one whose upload has just failed
  // (it says so in its slot: the peers return an error instead of waiting for it at the barrier)
  if (h->comm.transport == YCNR_COMM_IPC && h->comm.world > 1) {
    const std::string uploadError = g_last_error;
    bool failed = rc != YCNR_OK;
    if (!failed && hipStreamSynchronize(h->stream) != hipSuccess) {
      (void)hipGetLastError();
      failed = true;
    }
    const int rcp = ipc_publish(h->comm, h->factors, failed);
    if (rc) g_last_error = uploadError;  // this rank's own failure is the message to keep
    else rc = rcp;
  }
  return rc;
}

int ycnr_als_set_ratings_banded(ycnr_als *h, int side, const int64_t *rowPtr, const int32_t *indx, const void *vals, int memKind,
                                int nBands, const int64_t *bandBounds, const int64_t *rankBands, const int64_t *ownerBounds) {
  if (!h || !bandBounds || !rankBands || !ownerBounds) return fail(YCNR_ERR_INVALID, "null argument");
  if (side != YCNR_BY_USER && side != YCNR_BY_ITEM) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  if (nBands < 1 || nBands > kFewSlabs)
    return fail(YCNR_ERR_INVALID, "set_ratings_banded: nBands %d outside [1, %d] (a row's band slabs are added as one short float32 chain)", nBands, kFewSlabs);
  if (h->copt.factorsCount > kMaxFactors || h->kPad)
    return fail(YCNR_ERR_UNSUPPORTED, "set_ratings_banded: factorsCount %d (the banded half-step is built for the one-wave kernels: k <= %d, float32 k %% 4 == 0)",
                h->opt.factorsCount, kMaxFactors);
  const int world = h->comm.active() ? h->comm.world : 1, rank = h->comm.active() ? h->comm.rank : 0;
  if (world > kFewSlabs) return fail(YCNR_ERR_UNSUPPORTED, "set_ratings_banded: at most %d ranks", kFewSlabs);
  if (world > 1 && h->comm.transport == YCNR_COMM_SHM)
    return fail(YCNR_ERR_UNSUPPORTED, "set_ratings_banded: the host-staged shm stand-in does not carry band slabs (use ipc or rccl)");
  const int64_t rows = h->rows(side), cols = h->rows(1 - side);
  for (int b = 0; b <= nBands; ++b)
    if (bandBounds[b] < 0 || bandBounds[b] > cols || (b > 0 && bandBounds[b] < bandBounds[b - 1]))
      return fail(YCNR_ERR_INVALID, "set_ratings_banded: bandBounds must ascend within [0, %lld]", (long long)cols);
  if (bandBounds[0] != 0 || bandBounds[nBands] != cols) return fail(YCNR_ERR_INVALID, "set_ratings_banded: the bands must tile the columns [0, %lld)", (long long)cols);
  if (rankBands[0] != 0 || rankBands[world] != nBands || ownerBounds[0] != 0 || ownerBounds[world] != rows)
    return fail(YCNR_ERR_INVALID, "set_ratings_banded: rankBands must tile the %d bands and ownerBounds the %lld rows over the %d rank(s)", nBands, (long long)rows, world);
  for (int r = 0; r < world; ++r)
    if (rankBands[r + 1] < rankBands[r] || ownerBounds[r + 1] < ownerBounds[r]) return fail(YCNR_ERR_INVALID, "set_ratings_banded: rankBands / ownerBounds must ascend");
  HIP_TRY(hipSetDevice(h->opt.device));
  std::vector<Part> staged(1);  // staged in locals: a failure frees them and leaves the previous upload intact
  Part &part = staged[0];
  BandedSide B;
  int rc = YCNR_OK;
  const size_t ts = h->ts();
  const int bl = (int)rankBands[rank], bh = (int)rankBands[rank + 1], bpr = bh - bl;
  std::vector<int64_t> hp;
  std::vector<double> counts((size_t)rows * (size_t)nBands, 0.0);
  auto build = [&]() -> int {
    hipError_t e = part.create_events();
    if (e == hipSuccess) e = new_event(B.evRecv, false);
    for (int i = 0; i < kFewSlabs && e == hipSuccess; ++i) e = new_event(B.evStage[i], false);
    if (e != hipSuccess) return fail(YCNR_ERR_HIP, "set_ratings_banded: hipEventCreate: %s", hipGetErrorString(e));
    int r1 = upload_ratings(h, part.R, rows, cols, rowPtr, indx, vals, 0, rows, memKind, hp, "set_ratings_banded");
    if (r1) return r1;
    if (bpr <= 0 && part.R.nnz > 0) return fail(YCNR_ERR_INVALID, "set_ratings_banded: rank %d has no band but %lld ratings", rank, (long long)part.R.nnz);
    if (bpr > 0)
      if (int r2 = check_index_bounds(part.R.dIndx.get(), part.R.nnz, bandBounds[bl], bandBounds[bh], h->stream, "set_ratings_banded")) return r2;
    // where every row's ratings cross this rank's inner band boundaries (rows are sorted by column id)
    const int64_t base = hp[0];
    std::vector<int64_t> qRow, cuts;
    std::vector<int32_t> keys;
    for (int64_t r = 0; r < rows; ++r)
      if (hp[r + 1] != hp[r]) qRow.push_back(r);
    for (int b = bl + 1; b < bh; ++b) keys.push_back((int32_t)bandBounds[b]);
    const BoundQueries q = bound_queries(hp.data(), qRow, keys);
    if (int r3 = lower_bound_i32(part.R.dIndx.get(), q.beg, q.end, q.key, cuts, h->stream)) return r3;
    for (size_t i = 0; i < qRow.size(); ++i) {
      const int64_t r = qRow[i];
      int64_t p = hp[r] - base;
      for (int j = 0; j < bpr; ++j) {
        const int64_t q = j + 1 < bpr ? cuts[i * (size_t)(bpr - 1) + j] : hp[r + 1] - base;
        if (q < p) return fail(YCNR_ERR_INVALID, "set_ratings_banded: the column ids of row %lld are not ascending", (long long)r);
        counts[(size_t)r * nBands + (size_t)(bl + j)] = (double)(q - p);
        p = q;
      }
    }
    return YCNR_OK;
  };
  rc = build();
  // the ratings of every (row, band) on every rank: the owners skip empty bands, lambda n needs the row's total, and the chunk
  // length follows the ratings of the WHOLE side -- collective, a rank whose upload failed takes part with what it has
  if (world > 1) {
    const std::string why = g_last_error;
    const int rca = comm_allreduce_sum(h->comm, counts.data(), (int64_t)counts.size());
    if (rc) g_last_error = why;
    else rc = rca;
  }
  auto finish = [&]() -> int {
    // the side's row pointer, from the agreed counts.  One rank of an emulated world never sees the counts of the other
    // ranks' bands: it sizes the chunks for a side `world` times its own share, as the real run would
    std::vector<int64_t> sidePtr((size_t)rows + 1, 0);
    for (int64_t r = 0; r < rows; ++r) {
      int64_t t = 0;
      for (int b = 0; b < nBands; ++b) t += (int64_t)counts[(size_t)r * nBands + b];
      sidePtr[(size_t)r + 1] = sidePtr[(size_t)r] + t;
    }
    const SideNnz sn = side_nnz(sidePtr.data(), rows, h->comm.active() && h->comm.transport == YCNR_COMM_STUB ? world : 1);
    const int64_t chunk = h->autoChunk ? auto_chunk(sn.nnz, sn.splitNnz) : h->copt.chunkRatings;
    B.nBands = nBands;
    B.world = world;
    B.rank = rank;
    B.rankBands.assign(rankBands, rankBands + world + 1);
    B.ownerBounds.assign(ownerBounds, ownerBounds + world + 1);
    B.slabElems = slab_regs(h->shape(side)) * 64;
    BandedPlan plan = plan_banded(hp.data(), counts.data(), nBands, rankBands, ownerBounds, rank, world, chunk, B.slabElems);
    if (plan.error) return fail(YCNR_ERR_UNSUPPORTED, "set_ratings_banded: %s", plan.error);
    static_cast<BandedLayout &>(B) = plan;
    B.nSums = (int64_t)plan.sums.size();
    B.recvSlabs = B.recvSlab0[(size_t)world];
    Schedule &S = part.S;
    S.nUnits = (int64_t)plan.units.size();
    S.nSlabs = S.nUnits;
    S.nSplit = (int64_t)plan.owned.size();
    S.solvedRows = S.nSplit;
    S.maxRowSlabs = nBands;
    B.ownedSolved = S.nSplit;
    if (S.nUnits) {
      HIP_TRY(hipMalloc(S.dUnits.put(), sizeof(Unit) * plan.units.size()));
      HIP_TRY(hipMemcpy(S.dUnits.get(), plan.units.data(), sizeof(Unit) * plan.units.size(), hipMemcpyHostToDevice));
    }
    if (B.nSums) {
      HIP_TRY(hipMalloc(B.dSums.put(), sizeof(SlabSum) * plan.sums.size()));
      HIP_TRY(hipMemcpy(B.dSums.get(), plan.sums.data(), sizeof(SlabSum) * plan.sums.size(), hipMemcpyHostToDevice));
    }
    if (S.nSplit) {
      HIP_TRY(hipMalloc(S.dSplit.put(), sizeof(SplitRow) * plan.owned.size()));
      HIP_TRY(hipMemcpy(S.dSplit.get(), plan.owned.data(), sizeof(SplitRow) * plan.owned.size(), hipMemcpyHostToDevice));
    }
    const size_t slabBytes = (size_t)B.slabElems * ts;
    HIP_TRY(hipMalloc(S.dSlabs.put(), std::max<size_t>((size_t)(B.bandSlabs + B.tmpSlabs) * slabBytes, 64)));
    HIP_TRY(hipMalloc(B.dRecv.put(), std::max<size_t>((size_t)B.recvSlabs * slabBytes, 64)));
    HIP_TRY(hipMemset(B.dRecv.get(), 0, std::max<size_t>((size_t)B.recvSlabs * slabBytes, 64)));
    // the owners' table as pointers: a rank's own band slabs are in its arena, the other ranks' arrive in dRecv
    std::vector<const void *> table(plan.table.size(), nullptr);
    for (size_t i = 0; i < table.size(); ++i)
      if (plan.table[i].src >= 0)
        table[i] = (const char *)(plan.table[i].src == rank ? S.dSlabs.get() : B.dRecv.get()) + (size_t)plan.table[i].slab * slabBytes;
    HIP_TRY(hipMalloc(B.dTable.put(), std::max<size_t>(sizeof(void *) * table.size(), 64)));
    if (!table.empty()) HIP_TRY(hipMemcpy((void *)B.dTable.get(), table.data(), sizeof(void *) * table.size(), hipMemcpyHostToDevice));
    B.on = true;
    return YCNR_OK;
  };
  if (!rc) rc = finish();
  // IPC: the peers push their band slabs into dRecv -- published here, collectively (a rank that failed says so in its slot)
  if (h->comm.active() && h->comm.transport == YCNR_COMM_IPC) {
    const std::string why = g_last_error;
    const int rcp = ipc_publish_extra(h->comm, side, rc ? nullptr : B.dRecv.get(), rc != YCNR_OK);
    if (rc) g_last_error = why;
    else rc = rcp;
  }
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->drop_graphs();
  h->parts[side].swap(staged);  // the previous upload is freed as `staged` goes out of scope
  h->banded[side] = std::move(B);
  // the solved rows travel like a sharded side's: one piece per rank (ycnr_als_exchange, the exchange behind the half-step)
  h->bounds[side].clear();
  for (int r = 0; r < world; ++r) {
    h->bounds[side].push_back(ownerBounds[r]);
    h->bounds[side].push_back(ownerBounds[r + 1]);
  }
  return YCNR_OK;
}

int ycnr_als_set_rmse_ratings(ycnr_als *h, int which, const int64_t *rowPtr, const int32_t *indx,
                              const void *vals, int64_t rowBegin, int64_t rowEnd, int memKind) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (which != YCNR_RMSE_VALIDATE && which != YCNR_RMSE_TEST) return fail(YCNR_ERR_INVALID, "bad rmse set %d", which);
  std::vector<int64_t> hp;
  Ratings &R = h->rmse[which];
  int rc = upload_ratings(h, R, h->opt.totalUsersCount, h->opt.totalItemsCount, rowPtr, indx, vals, rowBegin,
                          rowEnd, memKind, hp, "set_rmse_ratings");
  if (rc) return rc;
  const int64_t base = hp[0];
  for (auto &v : hp) v -= base;
  hipError_t e = hipMalloc(R.dRowPtr.put(), sizeof(int64_t) * hp.size());
  if (e == hipSuccess) e = hipMemcpy(R.dRowPtr.get(), hp.data(), sizeof(int64_t) * hp.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    R = Ratings();  // never "loaded" without its row pointers
    return fail(e == hipErrorOutOfMemory ? YCNR_ERR_NOMEM : YCNR_ERR_HIP, "set_rmse_ratings: %s", hipGetErrorString(e));
  }
  return YCNR_OK;
}

int ycnr_als_set_factors(ycnr_als *h, int side, const void *src, int memKind) {
  if (!h || !src) return fail(YCNR_ERR_INVALID, "null argument");
  if (side != 0 && side != 1) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  HIP_TRY(hipSetDevice(h->opt.device));
  int rc = copy_in(h->factors[side], src, (size_t)h->rows(side) * h->opt.factorsCount * h->ts(), memKind, h->stream);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return YCNR_OK;
}

int ycnr_als_get_factors(ycnr_als *h, int side, void *dst, int64_t rowBegin, int64_t rowCount, int memKind) {
  if (!h || !dst) return fail(YCNR_ERR_INVALID, "null argument");
  if (side != 0 && side != 1) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  if (rowBegin < 0 || rowCount < 0 || rowBegin + rowCount > h->rows(side))
    return fail(YCNR_ERR_INVALID, "get_factors: rows [%lld, +%lld) outside the matrix", (long long)rowBegin,
                (long long)rowCount);
  HIP_TRY(hipSetDevice(h->opt.device));
  const size_t rowBytes = (size_t)h->opt.factorsCount * h->ts();
  HIP_TRY(hipMemcpyAsync(dst, (const char *)h->factors[side] + (size_t)rowBegin * rowBytes, (size_t)rowCount * rowBytes,
                         memKind == YCNR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return YCNR_OK;
}

int ycnr_als_factors_ptr(ycnr_als *h, int side, void **p) {
  if (!h || !p) return fail(YCNR_ERR_INVALID, "null argument");
  if (side != 0 && side != 1) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  *p = h->factors[side];
  return YCNR_OK;
}

int ycnr_als_bind_factors(ycnr_als *h, int side, void *p) {
  if (!h || !p) return fail(YCNR_ERR_INVALID, "null argument");
  if (side != 0 && side != 1) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  HIP_TRY(hipSetDevice(h->opt.device));
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess || attr.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return fail(YCNR_ERR_INVALID, "bind_factors: not a device pointer");
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->factorsMem[side].reset();
  h->drop_graphs();
  h->factors[side] = p;
  return YCNR_OK;
}

// kernels of one piece of the shard, on the handle's stream, timed by the piece's events
// branches: the small-upload form (chunks -> reduce, row kernel and dual classes as parallel branches, no per-kernel
// timing events) that ycnr_als_step_async captures into a hipGraph
// inOrder: every kernel of the piece on `stream`, one after the other (a piece of several: two pieces are in flight on the two
// piece streams and fill each other's tails; side streams per piece cost a fork and a join per side stream, and a wait on an
// event of ANOTHER hardware queue costs the step's stream tens of microseconds -- in the trace of one GPU's eighth of the
// MAL-scale user side, 4 pieces, the joins were 100 - 300 us of gaps in a 2.2 ms half-step)
static int launch_part(ycnr_als *h, int side, Part &part, hipStream_t stream, bool branches = false, bool inOrder = false) {
  const Ratings &R = part.R;
  const Schedule &S = part.S;
  hipEvent_t evs[5];  // the raw view of the piece's timing events that the launch_* functions record
  for (int i = 0; i < 5; ++i) evs[i] = part.ev[i].get();
  hipEvent_t *ev = branches ? nullptr : evs;
  const StepShape shape = h->shape(side);
  const PathKind path = step_path(shape.f64, shape.k);
  if (h->copt.dtype == YCNR_F32) {
    // (copt.factorsCount = kPad when the matrices are padded)
    StepArgs<float> a = h->kPad ? step_args<float>(h, side, part, h->padded[1 - side].get(), h->padded[side].get())
                                : step_args<float>(h, side, part, h->factors[1 - side], h->factors[side]);
    if (h->kPad) a.kReal = h->opt.factorsCount;
    if (h->planes[1 - side] && h->planesValid[1 - side] && use_planes(shape, env_flags())) {
      a.planes = h->planes[1 - side].get();
      a.planesBytes = (uint32_t)(h->rows(1 - side) * planes_row_bytes(slab_nb(h->copt.factorsCount), planes_pack(h->copt.factorsCount)));
    }
    DualPlan dp;
    dp.noX6 = (h->copt.flags & YCNR_FLAG_NO_BF16X6) != 0;
    dp.fewSlabs = S.maxRowSlabs <= kFewSlabs;
    if (S.dualMax > 0) {
      dp.nPrimal = S.nPrimal;
      dp.first = S.dualFirst;
      dp.count = S.dualCount;
      // (the fork and join cost nine more runtime calls per half-step: with a few hundred rows,
      // where the half-step is bound by the launches themselves, they made it slower)
      if (duals_on_side_streams(shape, env_flags(), S.dualRows, branches, inOrder)) {
        // (a captured small half-step keeps two branches for its dual classes: every branch is a join, 30 - 60 us each)
        dp.nSide = branches ? std::min(2, side_streams()) : side_streams();
        for (int i = 0; i < dp.nSide; ++i) {
          if (!h->sideStream[i]) HIP_TRY(hipStreamCreateWithFlags(h->sideStream[i].put(), hipStreamNonBlocking));
          dp.side[i] = h->sideStream[i].get();
          dp.join[i] = part.join[i].get();
        }
      }
    }
    dp.fork = part.fork.get();
    if (branches) {
      dp.slabStream = h->pieceStream[0].get();
      dp.slabJoin = part.slabJoin.get();
    }
    int rc;
    if (path == kAnyK)
      rc = launch_step_gen<float>(a, S.genBatches, stream, ev, dp);
    else if (path == kWorkgroup)
      rc = launch_step_big(a, S.nUnits, S.nSlabs, S.nSplit, stream, ev, dp, S.dRowSlabs.get(), S.rowSlabRows);
    else
      rc = launch_step<float>(a, S.nUnits, S.nSlabs, S.nSplit, stream, ev, (h->copt.flags & YCNR_FLAG_LDS_SOLVER) != 0, dp,
                              use_valu_edge(shape), use_slab_x6(shape));
    if (rc || !h->kPad) return rc;
    // the piece's solved rows back into the caller's matrix (before its exchange)
    const int64_t nr = R.rowEnd - R.rowBegin, n = nr * h->opt.factorsCount;
    if (n > 0) {
      hipLaunchKernelGGL(unpad_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const float *)h->padded[side].get(),
                         (float *)h->factors[side], R.rowBegin, nr, h->opt.factorsCount, h->kPad);
      HIP_TRY(hipGetLastError());
    }
    return YCNR_OK;
  }
  const StepArgs<double> a = step_args<double>(h, side, part, h->factors[1 - side], h->factors[side]);
  if (path == kAnyK) return launch_step_gen<double>(a, S.genBatches, stream, ev, DualPlan());
  DualPlan dpd;  // float64 has no dual classes; the chunk branch of the small-upload form applies
  dpd.fork = part.fork.get();
  if (branches) {
    dpd.slabStream = h->pieceStream[0].get();
    dpd.slabJoin = part.slabJoin.get();
  }
  return launch_step<double>(a, S.nUnits, S.nSlabs, S.nSplit, stream, ev, (h->copt.flags & YCNR_FLAG_LDS_SOLVER) != 0, dpd);
}

// row ranges of piece c of every rank (sharded upload)
static void part_ranges(const ycnr_als *h, int side, int c, std::vector<int64_t> &begin, std::vector<int64_t> &end) {
  const int world = h->comm.world, np = (int)h->parts[side].size();
  begin.resize((size_t)world);
  end.resize((size_t)world);
  for (int r = 0; r < world; ++r) {
    begin[(size_t)r] = h->bounds[side][(size_t)r * (np + 1) + c];
    end[(size_t)r] = h->bounds[side][(size_t)r * (np + 1) + c + 1];
  }
}

}  // extern "C"

// bookkeeping of a half-step that has just been enqueued: what the step info reports besides the times, and its place among
// the half-steps ycnr_als_sync will complete
static void note_enqueued(ycnr_als *h, int side, const std::vector<Part> &parts) {
  h->info.struct_size = (int32_t)sizeof(ycnr_als_step_info);
  h->info.side = side;
  h->info.parts = (int32_t)parts.size();
  for (const Part &p : parts) {
    const Schedule &S = p.S;
    h->info.rows += S.solvedRows;
    h->info.ratings += p.R.nnz;
    h->info.units += S.nUnits;
    h->info.splitRows += S.nSplit;
    h->info.fusedRows += S.solvedRows - S.nSplit;
    h->info.fusedRatings += S.fusedRatings;
    if (S.dualMax > 0) {
      h->info.dualRows += S.dualRows;
      h->info.dualRatings += S.dualRatings;
      h->info.dualFlops += S.dualFlops;
      // (not told whether the piece ran in order, as one of several in flight: DESIGN.md section 8)
      if (duals_on_side_streams(h->shape(side), env_flags(), S.dualRows, false, false)) h->info.dualOverlapped = 1;
    }
  }
  h->infoPending = true;
  h->infoSide = side;
  // (the same side twice without a sync: its events have been re-recorded, the earlier half-step's times are gone)
  int np = 0;
  for (int i = 0; i < h->nPend; ++i)
    if (h->pendOrder[i] != side) h->pendOrder[np++] = h->pendOrder[i];
  h->pendOrder[np++] = side;
  h->nPend = np;
  h->pend[side].info = h->info;
  h->pend[side].graphRun = h->graphRun;
  h->pend[side].exchanged = h->exchangedInStep;
}

// One half-step of a side sharded by bands of columns (ycnr_als_set_ratings_banded): owner group by owner group the chunk
// Gramians of this rank's ratings (+ the sums of the segments that were cut into several chunks), every group's band slabs
// sent to its owner while the next group is computed; then the owned rows' band slabs added in band order + solve, and the
// solved rows exchanged like a sharded side's.  RCCL: everything stream-ordered.  IPC (the functional path of the one-GPU
// tests): the pushes are completed with a host barrier before the owners reduce.
template <typename T>
static int step_banded_t(ycnr_als *h, int side) {
  BandedSide &B = h->banded[side];
  Part &part = h->parts[side][0];
  Schedule &S = part.S;
  Comm &c = h->comm;
  const bool comm = c.active() && B.world > 1;
  if (comm && (c.world != B.world || c.rank != B.rank)) return fail(YCNR_ERR_STATE, "step: the banded upload of this side was made for another communicator");
  hipStream_t stream = h->stream;
  const size_t ts = sizeof(T), slabBytes = (size_t)B.slabElems * ts;
  if (comm && c.transport == YCNR_COMM_IPC) {
    if (c.pendingFinish) {  // (as ycnr_als_step_async: a half-step the peers were still pushing must be complete first)
      HIP_TRY(hipStreamSynchronize(stream));
      if (int rcf = ipc_finish(c)) return rcf;
    }
    if (int rcb = ipc_enter(c)) return rcb;
  }
  const StepArgs<T> a = step_args<T>(h, side, part, h->factors[1 - side], h->factors[side]);
  // the chunk kernel and the band reduce of this k (no row kernel, no dual classes)
  RowKernels<T> rk;
  if (int rc = row_kernels<T>(a, (h->copt.flags & YCNR_FLAG_LDS_SOLVER) != 0, use_valu_edge(h->shape(side)), use_slab_x6(h->shape(side)), false, rk)) return rc;
  if (int rc = set_max_lds(reinterpret_cast<const void *>(rk.band), rk.ldsReduce)) return rc;
  HIP_TRY(hipEventRecord(part.ev[0].get(), stream));
  const int bpr = (int)(B.rankBands[(size_t)B.rank + 1] - B.rankBands[(size_t)B.rank]);
  // The groups are dealt over up to four streams (the handle's two piece streams and two of its side streams): a group is an
  // eighth of the rows -- about one round of waves -- and its longest chunk sets its kernel's length, so the kernels of several
  // groups have to be in flight for the chip to be full (eight launches in stream order: 2.8 ms per rank and item half-step at
  // MAL scale; over two streams 1.8; one launch over all groups, which could not signal a group's completion: 1.2).
  int nStreams = 1;
  hipStream_t gs[kFewSlabs] = {stream, stream, stream, stream, stream, stream, stream, stream};
  if (B.world > 1 && !(h->opt.flags & YCNR_FLAG_NO_OVERLAP) && !env_flags().noOverlap) {
    static const int want = getenv("YCNR_BAND_STREAMS") ? std::max(1, std::min(2 + kSideStreams, atoi(getenv("YCNR_BAND_STREAMS")))) : 4;
    nStreams = std::min(want, B.world);
    for (int i = 0; i < nStreams; ++i) {
      if (i < 2) {
        gs[i] = h->pieceStream[i].get();
      } else {
        if (!h->sideStream[i - 2]) HIP_TRY(hipStreamCreateWithFlags(h->sideStream[i - 2].put(), hipStreamNonBlocking));
        gs[i] = h->sideStream[i - 2].get();
      }
    }
    HIP_TRY(hipEventRecord(h->evStepStart.get(), stream));
    for (int i = 0; i < nStreams; ++i) HIP_TRY(hipStreamWaitEvent(gs[i], h->evStepStart.get(), 0));
  }
  const bool twoStreams = nStreams > 1;
  // stages per launch: consecutive stages' units (and sums) are contiguous, one launch covers `batch` of them -- enough units to
  // fill the chip -- and their band slabs leave together when it has finished
  static const int batchEnv = getenv("YCNR_BAND_BATCH") ? std::max(1, atoi(getenv("YCNR_BAND_BATCH"))) : 0;
  const int batch = batchEnv ? batchEnv : 1;
  for (int s = 1; s <= B.world; ++s) {
    const int g = (B.rank + s) % B.world;  // the own group last: its slabs do not travel
    const int b0 = ((s - 1) / batch) * batch + 1, b1 = std::min(B.world, b0 + batch - 1);  // the stages launched together with s
    hipStream_t ps = gs[((s - 1) / batch) % nStreams];
    if (s == b0) {
      int64_t nu = 0, ns = 0;
      const int g0 = (B.rank + b0) % B.world;
      for (int t = b0; t <= b1; ++t) {
        nu += B.groupUnits[(size_t)((B.rank + t) % B.world)];
        ns += B.groupSums[(size_t)((B.rank + t) % B.world)];
      }
      if (nu > 0x7fffffffLL) return fail(YCNR_ERR_UNSUPPORTED, "too many work units for one launch (%lld)", (long long)nu);
      if (nu > 0) {
        StepArgs<T> ag = a;
        ag.units = S.dUnits.get() + B.groupUnit0[(size_t)g0];
        hipLaunchKernelGGL(rk.chunk, dim3((unsigned)nu), dim3(64), 0, ps, ag);
        HIP_TRY(hipGetLastError());
      }
      if (ns > 0) {
        hipLaunchKernelGGL(als_slab_sum_kernel<T>, dim3((unsigned)ns), dim3(256), 0, ps, (T *)S.dSlabs.get(), (const SlabSum *)B.dSums.get() + B.groupSum0[(size_t)g0], B.slabElems);
        HIP_TRY(hipGetLastError());
      }
    }
    HIP_TRY(hipEventRecord(B.evStage[s - 1].get(), ps));
    if (!comm || g == B.rank) continue;
    const int from = (B.rank - s + B.world) % B.world;  // the rank whose stage-s group this rank is
    const int64_t sendSlabs = (B.ownerBounds[(size_t)g + 1] - B.ownerBounds[(size_t)g]) * bpr;
    const int64_t ownN = B.ownerBounds[(size_t)B.rank + 1] - B.ownerBounds[(size_t)B.rank];
    const int64_t recvSlabs = ownN * (B.rankBands[(size_t)from + 1] - B.rankBands[(size_t)from]);
    h->info.exchangeBytes += (sendSlabs + recvSlabs) * (int64_t)slabBytes;
    if (c.transport == YCNR_COMM_STUB) continue;  // (one rank of an emulated world: the bytes are counted, nothing travels)
    HIP_TRY(hipStreamWaitEvent(c.stream, B.evStage[s - 1].get(), 0));
    const char *src = (const char *)S.dSlabs.get() + (size_t)B.groupSlab0[(size_t)g] * slabBytes;
    if (c.transport == YCNR_COMM_RCCL) {
      const ncclDataType_t dt = ts == 8 ? ncclDouble : ncclFloat;
      NCCL_TRY(c.api, c.api->GroupStart());
      if (sendSlabs > 0) NCCL_TRY(c.api, c.api->Send(src, (size_t)sendSlabs * (size_t)B.slabElems, dt, g, c.nccl, c.stream));
      if (recvSlabs > 0)
        NCCL_TRY(c.api, c.api->Recv((char *)B.dRecv.get() + (size_t)B.recvSlab0[(size_t)from] * slabBytes, (size_t)recvSlabs * (size_t)B.slabElems, dt, from, c.nccl, c.stream));
      NCCL_TRY(c.api, c.api->GroupEnd());
    } else if (c.transport == YCNR_COMM_IPC) {
      if (c.extra[side].size() != (size_t)c.world || (sendSlabs > 0 && !c.extra[side][(size_t)g].ptr))
        return fail(YCNR_ERR_STATE, "ipc: the band-slab buffer of rank %d is not mapped", g);
      // where this rank's slabs start in g's receive buffer: behind those of the ranks before it (g itself sends nothing)
      int64_t off = 0;
      const int64_t gRows = B.ownerBounds[(size_t)g + 1] - B.ownerBounds[(size_t)g];
      for (int r = 0; r < B.rank; ++r)
        if (r != g) off += gRows * (B.rankBands[(size_t)r + 1] - B.rankBands[(size_t)r]);
      if (sendSlabs > 0)
        HIP_TRY(hipMemcpyAsync(c.extra[side][(size_t)g].ptr + (size_t)off * slabBytes, src, (size_t)sendSlabs * slabBytes, hipMemcpyDeviceToDevice, c.stream));
    } else {
      return fail(YCNR_ERR_UNSUPPORTED, "step: this transport does not carry band slabs");
    }
  }
  // the step's stream joins the piece streams: the last stage of each (enqueued behind every launch, as in ycnr_als_step_async)
  if (twoStreams) {
    const int nb = (B.world + batch - 1) / batch;  // the last launch of every stream in use
    for (int bi = std::max(0, nb - nStreams); bi < nb; ++bi) HIP_TRY(hipStreamWaitEvent(stream, B.evStage[std::min(B.world, (bi + 1) * batch) - 1].get(), 0));
  }
  for (int i = 1; i <= 3; ++i) HIP_TRY(hipEventRecord(part.ev[i].get(), stream));  // (no row kernel, no dual classes)
  if (comm && c.transport == YCNR_COMM_RCCL) {
    HIP_TRY(hipEventRecord(B.evRecv.get(), c.stream));
    HIP_TRY(hipStreamWaitEvent(stream, B.evRecv.get(), 0));
  } else if (comm && c.transport == YCNR_COMM_IPC) {
    HIP_TRY(hipStreamSynchronize(c.stream));  // this rank's pushes have landed ...
    if (int rcb = shm_barrier(c)) return rcb;  // ... and everybody's
  }
  if (S.nSplit > 0x7fffffffLL) return fail(YCNR_ERR_UNSUPPORTED, "too many split rows for one launch (%lld)", (long long)S.nSplit);
  if (S.nSplit > 0) {
    hipLaunchKernelGGL(rk.band, dim3((unsigned)S.nSplit), dim3(64), rk.ldsReduce, stream, a, reinterpret_cast<const T *const *>(B.dTable.get()), (int32_t)B.nBands);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(part.ev[4].get(), stream));
  h->exchangedInStep = comm;
  if (comm) {
    std::vector<int64_t> xb((size_t)B.world), xe((size_t)B.world);
    for (int r = 0; r < B.world; ++r) {
      xb[(size_t)r] = B.ownerBounds[(size_t)r];
      xe[(size_t)r] = B.ownerBounds[(size_t)r + 1];
    }
    int rc = comm_exchange(c, h->factors[side], side, h->opt.factorsCount, ts, xb.data(), xe.data(), stream, part.ready.get(), part.x0.get(), part.x1.get(), &h->info.exchangeBytes);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(h->evComputeEnd.get(), stream));
    if (c.transport != YCNR_COMM_SHM) HIP_TRY(hipStreamWaitEvent(stream, part.x1.get(), 0));
  }
  HIP_TRY(hipMemcpyAsync(h->hErr.get(), h->dErr.get(), sizeof(ErrInfo), hipMemcpyDeviceToHost, stream));
  return YCNR_OK;
}

extern "C" {

int ycnr_als_step_async(ycnr_als *h, int side) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (side != YCNR_BY_USER && side != YCNR_BY_ITEM) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  std::vector<Part> &parts = h->parts[side];
  if (parts.empty()) return fail(YCNR_ERR_STATE, "step: set_ratings was not called for this side");
  HIP_TRY(hipSetDevice(h->opt.device));
  if (h->banded[side].on) {
    memset(&h->info, 0, sizeof h->info);
    h->graphRun = false;
    h->planesValid[1 - side] = false;
    const int rcb = h->opt.dtype == YCNR_F64 ? step_banded_t<double>(h, side) : step_banded_t<float>(h, side);
    if (rcb) return rcb;
    note_enqueued(h, side, parts);
    return YCNR_OK;
  }
  // With a communicator and a sharded upload the half-step includes its exchange: the rows of piece
  // c travel (on the communicator's stream) while piece c + 1 is being solved, and the step's
  // stream waits for the last piece to land -- the next half-step reads the whole matrix.
  const bool exchange = h->comm.active() && !h->bounds[side].empty() && !h->deferExchange[side];
  if (exchange && h->bounds[side].size() != (size_t)h->comm.world * (parts.size() + 1))
    return fail(YCNR_ERR_STATE, "step: the sharded upload of this side was made for another communicator (bounds of %zu values, world %d x %zu pieces)",
                h->bounds[side].size(), h->comm.world, parts.size());
  h->exchangedInStep = exchange;
  if (exchange) {
    // IPC, a half-step enqueued behind one that has not been completed by ycnr_als_sync (back-to-back
    // ycnr_als_step_async calls): the peers' pushes of THAT half-step land in this rank's replica at the peers' pace, and
    // this half-step reads that matrix as its fixed side -- so the pending half-step is completed here first (this rank's
    // stream drained, then the end-of-step barrier: every rank's pushes have landed everywhere).  Receiver-posted
    // transports (RCCL, SHM) order this on the stream.  Collective like the call itself: every rank sees the same flag.
    if (h->comm.transport == YCNR_COMM_IPC && h->comm.pendingFinish) {
      HIP_TRY(hipStreamSynchronize(h->stream));
      if (int rcf = ipc_finish(h->comm)) return rcf;
    }
    if (int rcb = ipc_enter(h->comm)) return rcb;  // push transport: no peer is still preparing its replica
  }
  // (behind the completion of a pending IPC half-step, like the planes below: the pad reads the matrix the peers were pushing
  // into -- in front of that guard, back-to-back half-steps of a padded upload could pad rows that were still on their way)
  if (h->kPad) {
    // the FIXED side in full; of the solved side only this rank's rows (launch_part copies them back piece by
    // piece, the rows without ratings among them unchanged)
    const int s = 1 - side;
    const int64_t n = h->rows(s) * h->kPad;
    hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const float *)h->factors[s],
                       h->padded[s].get(), (int64_t)0, h->rows(s), h->opt.factorsCount, h->kPad);
    HIP_TRY(hipGetLastError());
    for (const Part &p : parts) {
      const int64_t nr = p.R.rowEnd - p.R.rowBegin, m = nr * h->kPad;
      if (m <= 0) continue;
      hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, (const float *)h->factors[side],
                         h->padded[side].get(), p.R.rowBegin, nr, h->opt.factorsCount, h->kPad);
      HIP_TRY(hipGetLastError());
    }
  }
  // (behind the completion of a pending IPC half-step above: the planes are read from the matrix the peers were pushing into)
  // the fixed matrix of this half-step as bf16 planes, once for all its waves (12.7 K x 100 floats at MAL scale: microseconds);
  // a replayed graph holds the launch itself (it was captured in front of the piece's kernels)
  // (not for uploads below kGraphMinRatings, whose half-step is a handful of launches: one more launch costs what the planes save)
  int64_t sideRatings = 0;
  for (const Part &p : parts) sideRatings += p.R.nnz;
  const bool planesNow = use_planes(h->shape(side), env_flags()) && sideRatings >= kGraphMinRatings;
  if (!planesNow) h->planesValid[1 - side] = false;
  auto split_planes = [&]() -> int {
    if (!planesNow) return YCNR_OK;
    h->planesValid[1 - side] = true;
    const int s = 1 - side, nb = slab_nb(h->copt.factorsCount);
    const bool pack = planes_pack(h->copt.factorsCount);
    const int64_t n = h->rows(s) * nb * 4;
    hipLaunchKernelGGL(als_split_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->kPad ? (const float *)h->padded[s].get() : (const float *)h->factors[s], h->planes[s].get(),
                       h->rows(s), h->copt.factorsCount, nb, pack ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return YCNR_OK;
  };
  if (planesNow && !h->planes[1 - side].get())
    HIP_TRY(hipMalloc(h->planes[1 - side].put(), (size_t)h->rows(1 - side) * (size_t)planes_row_bytes(slab_nb(h->copt.factorsCount), planes_pack(h->copt.factorsCount))));
  memset(&h->info, 0, sizeof h->info);
  // Small uploads (the ML-100k / ML-1M shapes): ~15 launches, forks and joins of a half-step whose kernels each fill a
  // fraction of the chip.  Captured once in the branch form (launch_part) and replayed: one launch per half-step.
  h->graphRun = false;
  {
    ycnr_als::GraphSlot &gs = h->graph[side];
    // (a padded upload -- kPad -- is captured too: the pads above are plain launches in front of the graph, the unpad of the piece's rows is part of it)
    const bool graphable = ycnr::graphable(h->shape(side), env_flags(), exchange, parts.size(), parts[0].R.nnz, h->stream == h->ownStream.get());
    if (graphable && gs.state == 1) {
      for (int i = 0; i < side_streams(); ++i)  // (not inside the capture)
        if (!h->sideStream[i]) HIP_TRY(hipStreamCreateWithFlags(h->sideStream[i].put(), hipStreamNonBlocking));
      gs.state = -1;
      hipGraph_t g = nullptr;
      if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed) == hipSuccess) {
        int rc = split_planes();
        if (rc == YCNR_OK) rc = launch_part(h, side, parts[0], h->stream, true);
        hipError_t ce = hipMemcpyAsync(h->hErr.get(), h->dErr.get(), sizeof(ErrInfo), hipMemcpyDeviceToHost, h->stream);
        hipError_t ee = hipStreamEndCapture(h->stream, &g);
        if (rc == YCNR_OK && ce == hipSuccess && ee == hipSuccess && g && hipGraphInstantiate(&gs.exec, g, nullptr, nullptr, 0) == hipSuccess)
          gs.state = 2;
        if (g) (void)hipGraphDestroy(g);
      }
      (void)hipGetLastError();
    } else if (graphable && gs.state == 0) {
      gs.state = 1;
    }
    if (graphable && gs.state == 2) {
      Part &p = parts[0];
      HIP_TRY(hipEventRecord(p.ev[0].get(), h->stream));
      HIP_TRY(hipGraphLaunch(gs.exec, h->stream));
      HIP_TRY(hipEventRecord(p.ev[4].get(), h->stream));
      h->graphRun = true;
    }
  }
  if (!h->graphRun)
    if (int rcs = split_planes()) return rcs;
  std::vector<int64_t> xb, xe;
  // several pieces: alternating over the two piece streams (unless YCNR_FLAG_NO_OVERLAP / the staged SHM stand-in,
  // whose exchange blocks the host); one piece: on the step's stream itself
  const bool twoStreams = parts.size() > 1 && !(h->opt.flags & YCNR_FLAG_NO_OVERLAP) && !env_flags().noOverlap &&
                          !(exchange && h->comm.transport == YCNR_COMM_SHM);
  if (twoStreams) {
    HIP_TRY(hipEventRecord(h->evStepStart.get(), h->stream));
    for (int i = 0; i < 2; ++i) HIP_TRY(hipStreamWaitEvent(h->pieceStream[i].get(), h->evStepStart.get(), 0));
  }
  for (size_t c = 0; c < parts.size() && !h->graphRun; ++c) {
    hipStream_t ps = twoStreams ? h->pieceStream[c & 1].get() : h->stream;
    static const bool pieceSides = getenv("YCNR_PIECE_SIDE_STREAMS") != nullptr;  // A/B: round 3's form (side streams inside every piece)
    int rc = launch_part(h, side, parts[c], ps, false, twoStreams && !pieceSides);
    if (rc) return rc;
    if (exchange) {
      part_ranges(h, side, (int)c, xb, xe);
      rc = comm_exchange(h->comm, h->factors[side], side, h->opt.factorsCount, h->ts(), xb.data(), xe.data(), ps, parts[c].ready.get(),
                         parts[c].x0.get(), parts[c].x1.get(), &h->info.exchangeBytes);
      if (rc) return rc;
    }
    if (twoStreams && c + 2 >= parts.size()) HIP_TRY(hipEventRecord(parts[c].done.get(), ps));  // the last piece of each stream
  }
  // ... joins the step's stream -- enqueued only now, behind every piece's launches: streams share hardware queues (the
  // runtime has 4 or 8 for all the streams of a process), a hardware queue is served in order, and a wait for piece c enqueued
  // on the step's stream BEFORE the launches of piece c + 1 held those launches back whenever the two streams shared a queue
  // (kernel trace of one GPU's eighth of the MAL-scale user side: the fourth piece started when the third had ended).
  if (twoStreams && !h->graphRun)
    for (size_t c = parts.size() >= 2 ? parts.size() - 2 : 0; c < parts.size(); ++c) HIP_TRY(hipStreamWaitEvent(h->stream, parts[c].done.get(), 0));
  if (exchange) {
    HIP_TRY(hipEventRecord(h->evComputeEnd.get(), h->stream));
    if (h->comm.transport != YCNR_COMM_SHM) HIP_TRY(hipStreamWaitEvent(h->stream, parts.back().x1.get(), 0));  // (SHM is synchronous)
  }
  if (!h->graphRun) HIP_TRY(hipMemcpyAsync(h->hErr.get(), h->dErr.get(), sizeof(ErrInfo), hipMemcpyDeviceToHost, h->stream));
  note_enqueued(h, side, parts);
  return YCNR_OK;
}

int ycnr_als_sync(ycnr_als *h) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->opt.device));
  HIP_TRY(hipStreamSynchronize(h->stream));  // (polling hipStreamQuery instead was measured: no difference, the runtime's wait spins)
  if (int rcf = ipc_finish(h->comm)) return rcf;  // IPC: every rank's pushes have landed everywhere
  const int nPend = h->infoPending ? h->nPend : 0;
  h->infoPending = false;
  h->nPend = 0;
  for (int pi = 0; pi < nPend; ++pi) {
    const int pside = h->pendOrder[pi];
    const bool last = pi + 1 == nPend;
    h->info = h->pend[pside].info;
    h->graphRun = h->pend[pside].graphRun;
    h->exchangedInStep = h->pend[pside].exchanged;
    const std::vector<Part> &parts = h->parts[pside];
    float ms = 0;
    if (h->graphRun && !parts.empty()) {
      // one interval for the whole half-step: chunks -> reduce, the row kernel and the dual classes ran as branches of one graph
      HIP_TRY(hipEventElapsedTime(&ms, parts[0].ev[0].get(), parts[0].ev[4].get()));
      h->info.gramSolveMs = ms;
      h->info.dualOverlapped = 1;
    }
    for (const Part &p : parts) {
      if (h->graphRun) break;
      HIP_TRY(hipEventElapsedTime(&ms, p.ev[0].get(), p.ev[1].get()));
      h->info.gramSlabMs += ms;
      HIP_TRY(hipEventElapsedTime(&ms, p.ev[1].get(), p.ev[2].get()));
      h->info.gramSolveMs += ms;
      HIP_TRY(hipEventElapsedTime(&ms, p.ev[2].get(), p.ev[3].get()));
      h->info.dualSolveMs += ms;
      HIP_TRY(hipEventElapsedTime(&ms, p.ev[3].get(), p.ev[4].get()));
      h->info.reduceSolveMs += ms;
      if (h->exchangedInStep) {
        HIP_TRY(hipEventElapsedTime(&ms, p.x0.get(), p.x1.get()));
        h->info.exchangeMs += ms;
      }
    }
    if (!parts.empty()) {
      h->info.totalMs = 0;
      for (const Part &p : parts) {  // (pieces run two at a time: the last one need not end last)
        HIP_TRY(hipEventElapsedTime(&ms, parts.front().ev[0].get(), p.ev[4].get()));
        h->info.totalMs = std::max(h->info.totalMs, ms);
      }
      if (h->exchangedInStep) {
        if (h->comm.transport != YCNR_COMM_SHM) {
          // what the step's stream still had to wait for after its own last kernel
          HIP_TRY(hipEventElapsedTime(&ms, h->evComputeEnd.get(), parts.back().x1.get()));
          h->info.exposedExchangeMs = ms > 0 ? ms : 0;
        } else {
          h->info.exposedExchangeMs = h->info.exchangeMs;  // the staged stand-in blocks the stream
          HIP_TRY(hipEventElapsedTime(&ms, parts.back().x0.get(), parts.back().x1.get()));
          h->info.totalMs -= h->info.exchangeMs - ms;  // kernels only (the last exchange lies behind the last kernel)
        }
      }
    }
    // (the error counter is cumulative and copied at the end of every half-step: with two half-steps in flight the rows
    // counted since the last sync are reported with the last one)
    ErrInfo ei = *h->hErr.get();  // copied by the step's stream, which has drained
    ei.count = last ? ei.count - h->errSeen : 0;
    h->errSeen += ei.count;
    h->info.numericErrors = ei.count;
    h->infoOf[pside] = h->info;
#ifdef YCNR_WG_STAMPS
    if (const char *path = getenv("YCNR_DUMP_STAMPS")) {
      std::vector<unsigned char> buf(kErrBytes);
      HIP_TRY(hipMemcpy(buf.data(), h->dErr.get(), kErrBytes, hipMemcpyDeviceToHost));
      if (FILE *f = fopen(path, "wb")) {
        fwrite(buf.data(), 1, buf.size(), f);
        fclose(f);
      }
    }
#endif
    if (ei.count > 0 && !env_flags().ignoreNumeric)  // the env var exists for timing experiments with ablated kernels
      return fail(YCNR_ERR_NUMERIC, "%d row(s) had a normal matrix that is not positive definite (e.g. row %d)",
                  ei.count, ei.firstRow);
  }
  return YCNR_OK;
}

int ycnr_als_step(ycnr_als *h, int side) {
  int rc = ycnr_als_step_async(h, side);
  if (rc) return rc;
  return ycnr_als_sync(h);
}

int ycnr_als_last_step_info(ycnr_als *h, ycnr_als_step_info *info) {
  if (!h || !info) return fail(YCNR_ERR_INVALID, "null argument");
  if (h->infoPending) return fail(YCNR_ERR_STATE, "last_step_info: call ycnr_als_sync first");
  *info = h->info;
  return YCNR_OK;
}

int ycnr_als_step_info_of(ycnr_als *h, int side, ycnr_als_step_info *info) {
  if (!h || !info) return fail(YCNR_ERR_INVALID, "null argument");
  if (side != YCNR_BY_USER && side != YCNR_BY_ITEM) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  if (h->infoPending) return fail(YCNR_ERR_STATE, "step_info_of: call ycnr_als_sync first");
  if (h->infoOf[side].struct_size == 0) return fail(YCNR_ERR_STATE, "step_info_of: no half-step of this side has been completed");
  *info = h->infoOf[side];
  return YCNR_OK;
}

int ycnr_als_rmse(ycnr_als *h, int which, double shift, int nPortions, const int64_t *portionRowEnd, double *out) {
  if (!h || !out) return fail(YCNR_ERR_INVALID, "null argument");
  if (which != YCNR_RMSE_VALIDATE && which != YCNR_RMSE_TEST) return fail(YCNR_ERR_INVALID, "bad rmse set %d", which);
  const Ratings &R = h->rmse[which];
  if (!R.loaded) return fail(YCNR_ERR_STATE, "rmse: set_rmse_ratings was not called for this set");
  if (nPortions < 0 || (nPortions > 0 && !portionRowEnd)) return fail(YCNR_ERR_INVALID, "bad portions");
  HIP_TRY(hipSetDevice(h->opt.device));
  const int64_t nRows = R.rowEnd - R.rowBegin;
  std::vector<int64_t> ends;
  if (nPortions == 0) {
    ends.push_back(nRows);
  } else {
    int64_t prev = 0;
    for (int p = 0; p < nPortions; ++p) {
      int64_t e = portionRowEnd[p] - R.rowBegin;  // global -> local, clipped to the shard
      e = std::max<int64_t>(0, std::min(nRows, e));
      if (e < prev) return fail(YCNR_ERR_INVALID, "rmse: portionRowEnd must be ascending");
      ends.push_back(e);
      prev = e;
    }
  }
  // One workgroup per piece of at most ceil(nRows / 4096) rows, so that a caller's portioning
  // (one portion = the whole set when nPortions == 0; the reference's default is 10 000 ratings)
  // does not decide how much of the GPU works; the pieces of a portion are added in row order.
  const int nPort = (int)ends.size();
  const int64_t pieceRows = std::max<int64_t>(1, (nRows + 4095) / 4096);
  std::vector<int64_t> pieceEnds;
  std::vector<int> pieceOf;
  {
    int64_t prev = 0;
    for (int p = 0; p < nPort; ++p) {
      if (ends[p] == prev) {
        pieceEnds.push_back(prev);
        pieceOf.push_back(p);
      }
      for (int64_t x = prev; x < ends[p]; x += pieceRows) {
        pieceEnds.push_back(std::min(ends[p], x + pieceRows));
        pieceOf.push_back(p);
      }
      prev = ends[p];
    }
  }
  const int np = (int)pieceEnds.size();
  std::vector<double> part((size_t)3 * np);
  DevPtr<int64_t> dEnds;
  DevPtr<double> dOut;
  Event ev0, ev1;  // the kernel alone (ycnr_als_last_rmse_ms)
  HIP_TRY(hipMalloc(dEnds.put(), sizeof(int64_t) * np));
  HIP_TRY(hipMalloc(dOut.put(), sizeof(double) * 3 * np));
  HIP_TRY(hipMemcpyAsync(dEnds.get(), pieceEnds.data(), sizeof(int64_t) * np, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipEventCreate(ev0.put()));
  HIP_TRY(hipEventCreate(ev1.put()));
  HIP_TRY(hipEventRecord(ev0.get(), h->stream));
  if (h->opt.dtype == YCNR_F32) {
    RmseArgs<float> a{R.dRowPtr.get(), R.dIndx.get(), (const float *)R.dVals.get(), (const float *)h->factors[0],
                      (const float *)h->factors[1], dEnds.get(), dOut.get(), shift, R.rowBegin, h->opt.factorsCount};
    launch_rmse(a, np, h->stream);
  } else {
    RmseArgs<double> a{R.dRowPtr.get(), R.dIndx.get(), (const double *)R.dVals.get(), (const double *)h->factors[0],
                       (const double *)h->factors[1], dEnds.get(), dOut.get(), shift, R.rowBegin, h->opt.factorsCount};
    launch_rmse(a, np, h->stream);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ev1.get(), h->stream));
  HIP_TRY(hipMemcpyAsync(part.data(), dOut.get(), sizeof(double) * 3 * np, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  float ms = 0;
  h->lastRmseMs = hipEventElapsedTime(&ms, ev0.get(), ev1.get()) == hipSuccess ? (double)ms : -1.0;
  for (int i = 0; i < 3 * nPort; ++i) out[i] = 0.0;
  for (int j = 0; j < np; ++j)
    for (int t = 0; t < 3; ++t) out[3 * pieceOf[j] + t] += part[(size_t)3 * j + t];
  return YCNR_OK;
}

int ycnr_als_last_rmse_ms(ycnr_als *h, double *ms) {
  if (!h || !ms) return fail(YCNR_ERR_INVALID, "null argument");
  if (h->lastRmseMs < 0) return fail(YCNR_ERR_STATE, "last_rmse_ms: no RMSE pass has run on this handle");
  *ms = h->lastRmseMs;
  return YCNR_OK;
}

// ---- top-N recommend from the handle's own matrices (recommend_kernels.hip.h) ----
extern "C++" {
namespace {
constexpr int64_t kRecFusedBatch = 65536;  // users per launch of the fused kernel (bounds the partial lists)

// one batch of the fused path: scores + per-workgroup lists, then the merge into the output layout
template <typename T>
void launch_topn(ycnr_als *h, const void *users, int64_t u0, int64_t nb, unsigned yblk, size_t lds, double shift, double thr, int take, int limit) {
  const unsigned ublk = (unsigned)((nb + 15) / 16);
  hipLaunchKernelGGL(recommend_topn_kernel<T>, dim3(ublk, yblk), dim3(256), lds, h->stream, (const T *)users,
                     (const int32_t *)h->rec[ycnr_als::REC_USER_IDS].get() + u0, nb, (const T *)h->factors[YCNR_BY_ITEM], h->opt.totalItemsCount,
                     (int)h->opt.factorsCount, shift, thr, (const int64_t *)h->rec[ycnr_als::REC_SKIP_PTR].get() + u0,
                     (const int32_t *)h->rec[ycnr_als::REC_SKIP].get(), take, (double *)h->rec[ycnr_als::REC_PART_V].get(),
                     (int32_t *)h->rec[ycnr_als::REC_PART_I].get());
  hipLaunchKernelGGL(recommend_topn_merge_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, h->stream, (const double *)h->rec[ycnr_als::REC_PART_V].get(),
                     (const int32_t *)h->rec[ycnr_als::REC_PART_I].get(), nb, (int)yblk, take, limit, (int32_t *)h->rec[ycnr_als::REC_IDS].get() + u0 * limit,
                     (double *)h->rec[ycnr_als::REC_PRED].get() + u0 * limit, (int32_t *)h->rec[ycnr_als::REC_CNT].get() + u0);
}

// one batch of the score-matrix path: the kernels of ycnr_recommend_items on the gathered user rows
template <typename T>
void launch_scores_select(ycnr_als *h, const void *users, int64_t u0, int64_t nb, bool valu, bool anySkip, double shift, double minRating, int take, int limit) {
  const int k = h->opt.factorsCount;
  const int64_t totalItems = h->opt.totalItemsCount;
  const size_t kp = (size_t)((k + 15) & ~15);
  T *rows = (T *)h->rec[ycnr_als::REC_ROWS].get();
  double *scores = (double *)h->rec[ycnr_als::REC_SCORES].get();
  const int64_t *skipPtr = (const int64_t *)h->rec[ycnr_als::REC_SKIP_PTR].get() + u0;
  hipLaunchKernelGGL(gather_rows_kernel<T>, dim3((unsigned)((nb * k + 255) / 256)), dim3(256), 0, h->stream, (const T *)users,
                     (const int32_t *)h->rec[ycnr_als::REC_USER_IDS].get() + u0, nb, k, rows);
  const unsigned ublk = (unsigned)((nb + 15) / 16);
  const unsigned yblk = (unsigned)std::max<int64_t>(1, std::min<int64_t>((totalItems + 63) / 64, (8 * device_cus() + ublk - 1) / ublk));
  if (valu)
    hipLaunchKernelGGL((recommend_scores_kernel<T, 1>), dim3((unsigned)nb), dim3(256), (size_t)k * sizeof(T), h->stream, (const T *)rows, nb,
                       (const T *)h->factors[YCNR_BY_ITEM], totalItems, k, shift, minRating, scores);
  else
    hipLaunchKernelGGL(recommend_scores_mfma_kernel<T>, dim3(ublk, yblk), dim3(256), 16 * kp * sizeof(T), h->stream, (const T *)rows, nb,
                       (const T *)h->factors[YCNR_BY_ITEM], totalItems, k, shift, minRating, scores);
  if (anySkip)
    hipLaunchKernelGGL(recommend_skip_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, skipPtr, (const int32_t *)h->rec[ycnr_als::REC_SKIP].get(), totalItems,
                       scores);
  hipLaunchKernelGGL(recommend_select_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, scores, totalItems, take, limit,
                     (int32_t *)h->rec[ycnr_als::REC_IDS].get() + u0 * limit, (double *)h->rec[ycnr_als::REC_PRED].get() + u0 * limit,
                     (int32_t *)h->rec[ycnr_als::REC_CNT].get() + u0);
}

// The validated request of ycnr_als_recommend / ycnr_als_recommend_for_ratings on the handle's stream: top-N of the rows
// userIds[.] of `users` (a device matrix [. x factorsCount]: the handle's user matrix, or the rows a fold-in has just solved
// with userIds == null = rows 0 .. nUsers - 1).  started: the caller has recorded recEv[0] (its own kernels count into deviceMs).
// dStatus (may be null): users with a non-zero status get an empty list.  beforeSync (may be empty): further copies to the host.
int recommend_run(ycnr_als *h, const void *users, int64_t nUsers, const int32_t *userIds, const int64_t *skipPtr, const int32_t *skipIds,
                  double globalAvgShift, double minRecommendRating, int32_t limit, int32_t *outIds, double *outPredict, int32_t *outCount,
                  double *deviceMs, bool started, const int32_t *dStatus, const std::function<int()> &beforeSync) {
  const int64_t nSkip = skipPtr[nUsers];
  const int k = h->opt.factorsCount;
  const int64_t totalItems = h->opt.totalItemsCount;
  const size_t ts = h->ts();
  const int take = limit - 1;  // lib/YcnrController.js:268-269
  HIP_TRY(hipSetDevice(h->opt.device));
  for (Event &ev : h->recEv)
    if (!ev) HIP_TRY(hipEventCreate(ev.put()));
  if (take == 0) {  // the reference returns nothing; still ordered behind the half-steps in flight
    if (started) HIP_TRY(hipEventRecord(h->recEv[1].get(), h->stream));
    if (beforeSync)
      if (int rc = beforeSync()) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int64_t u = 0; u < nUsers; ++u) {
      outIds[u] = -1;
      outPredict[u] = 0.0;
      outCount[u] = 0;
    }
    if (deviceMs) *deviceMs = 0.0;
    if (deviceMs && started) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, h->recEv[0].get(), h->recEv[1].get()));
      *deviceMs = ms;
    }
    return YCNR_OK;
  }
  // the same choice of score kernel as ycnr_recommend_items, so that the predicts are the same bits -- its A/B switch
  // YCNR_RECOMMEND_VALU included: with the variable set there is NO fused path here (include/ycnr_als.h says so; a timing taken
  // with it set is the score-matrix path's)
  const size_t kp = (size_t)((k + 15) & ~15);
  const bool valu = getenv("YCNR_RECOMMEND_VALU") != nullptr || 16 * kp * ts > 48 * 1024;
  const bool fused = !valu && take <= kTopMaxTake;
  typedef ycnr_als A;
  HIP_TRY(h->rec[A::REC_USER_IDS].reserve((size_t)nUsers * 4));
  HIP_TRY(h->rec[A::REC_SKIP_PTR].reserve((size_t)(nUsers + 1) * 8));
  HIP_TRY(h->rec[A::REC_SKIP].reserve(std::max<size_t>((size_t)nSkip * 4, 8)));
  HIP_TRY(h->rec[A::REC_IDS].reserve((size_t)nUsers * limit * 4));
  HIP_TRY(h->rec[A::REC_PRED].reserve((size_t)nUsers * limit * 8));
  HIP_TRY(h->rec[A::REC_CNT].reserve((size_t)nUsers * 4));
  // the item range of a user tile over enough workgroups to fill the chip four times, at least 16 tiles (4 per wave) each
  const int64_t ntiles = (totalItems + 15) / 16;
  auto parts_of = [&](int64_t nb) {
    const int64_t ublk = (nb + 15) / 16;
    return std::max<int64_t>(1, std::min<int64_t>((ntiles + 15) / 16, (4 * (int64_t)device_cus() + ublk - 1) / ublk));
  };
  const int64_t batch = fused ? std::min(nUsers, kRecFusedBatch)
                              : std::max<int64_t>(1, std::min<int64_t>(nUsers, ((int64_t)1 << 27) / std::max<int64_t>(1, totalItems)));  // scores <= 1 GB
  if (fused) {
    const int64_t last = nUsers % batch ? nUsers % batch : batch;
    const size_t lists = (size_t)std::max(batch * parts_of(batch), last * parts_of(last));
    HIP_TRY(h->rec[A::REC_PART_V].reserve(lists * take * 8));
    HIP_TRY(h->rec[A::REC_PART_I].reserve(lists * take * 4));
  } else {
    HIP_TRY(h->rec[A::REC_ROWS].reserve((size_t)batch * k * ts));
    HIP_TRY(h->rec[A::REC_SCORES].reserve((size_t)batch * totalItems * 8));
  }
  // everything below is enqueued on the handle's stream: behind the half-steps in flight, like ycnr_als_rmse
  if (userIds) {
    HIP_TRY(hipMemcpyAsync(h->rec[A::REC_USER_IDS].get(), userIds, (size_t)nUsers * 4, hipMemcpyHostToDevice, h->stream));
  } else {
    hipLaunchKernelGGL(foldin_iota_kernel, dim3((unsigned)((nUsers + 255) / 256)), dim3(256), 0, h->stream, (int32_t *)h->rec[A::REC_USER_IDS].get(), nUsers);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(h->rec[A::REC_SKIP_PTR].get(), skipPtr, (size_t)(nUsers + 1) * 8, hipMemcpyHostToDevice, h->stream));
  if (nSkip) HIP_TRY(hipMemcpyAsync(h->rec[A::REC_SKIP].get(), skipIds, (size_t)nSkip * 4, hipMemcpyHostToDevice, h->stream));
  if (!started) HIP_TRY(hipEventRecord(h->recEv[0].get(), h->stream));
  const double thr = minRecommendRating < -DBL_MAX ? -DBL_MAX : minRecommendRating;  // (-inf is "out" in the score matrix: it never competes)
  const size_t lds = std::max<size_t>(16 * kp * ts, (size_t)64 * take * 12);
  for (int64_t u0 = 0; u0 < nUsers; u0 += batch) {
    const int64_t nb = std::min(batch, nUsers - u0);
    if (fused) {
      if (h->opt.dtype == YCNR_F32) launch_topn<float>(h, users, u0, nb, (unsigned)parts_of(nb), lds, globalAvgShift, thr, take, limit);
      else launch_topn<double>(h, users, u0, nb, (unsigned)parts_of(nb), lds, globalAvgShift, thr, take, limit);
    } else {
      if (h->opt.dtype == YCNR_F32) launch_scores_select<float>(h, users, u0, nb, valu, nSkip > 0, globalAvgShift, minRecommendRating, take, limit);
      else launch_scores_select<double>(h, users, u0, nb, valu, nSkip > 0, globalAvgShift, minRecommendRating, take, limit);
    }
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(YCNR_ERR_HIP, "recommend launch: %s", hipGetErrorString(le));
  }
  if (dStatus) {
    hipLaunchKernelGGL(foldin_clear_lists_kernel, dim3((unsigned)((nUsers * limit + 255) / 256)), dim3(256), 0, h->stream, dStatus, nUsers, (int)limit,
                       (int32_t *)h->rec[A::REC_IDS].get(), (double *)h->rec[A::REC_PRED].get(), (int32_t *)h->rec[A::REC_CNT].get());
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(h->recEv[1].get(), h->stream));
  HIP_TRY(hipMemcpyAsync(outIds, h->rec[A::REC_IDS].get(), (size_t)nUsers * limit * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(outPredict, h->rec[A::REC_PRED].get(), (size_t)nUsers * limit * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(outCount, h->rec[A::REC_CNT].get(), (size_t)nUsers * 4, hipMemcpyDeviceToHost, h->stream));
  if (beforeSync)
    if (int rc = beforeSync()) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (deviceMs) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->recEv[0].get(), h->recEv[1].get()));
    *deviceMs = ms;
  }
  return YCNR_OK;
}

// skip lists of a request: offsets from 0, never decreasing, ids strictly ascending per user
int check_skip_lists(const char *what, int64_t nUsers, const int64_t *skipPtr, const int32_t *skipIds) {
  if (skipPtr[0] != 0) return fail(YCNR_ERR_INVALID, "%s: skipPtr[0] != 0", what);
  for (int64_t u = 0; u < nUsers; ++u) {
    if (skipPtr[u + 1] > skipPtr[u] && !skipIds) return fail(YCNR_ERR_INVALID, "%s: null skipIds", what);
    if (skipPtr[u + 1] < skipPtr[u]) return fail(YCNR_ERR_INVALID, "%s: skipPtr decreases at user %lld", what, (long long)u);
    for (int64_t q = skipPtr[u] + 1; q < skipPtr[u + 1]; ++q)
      if (skipIds[q] <= skipIds[q - 1]) return fail(YCNR_ERR_INVALID, "%s: skip ids of user %lld are not strictly ascending", what, (long long)u);
  }
  return YCNR_OK;
}

// ---- fold-in (foldin_kernels.hip.h): rows solved from ratings that arrive in the call ----

// the request of ycnr_als_fold_in / ycnr_als_recommend_for_ratings; YCNR_ERR_INVALID before anything is touched
int fold_check(const char *what, const ycnr_als *h, int side, int64_t nRows, const int64_t *rowPtr, const int32_t *indx, const void *vals,
               const int32_t *storeIds) {
  if (!rowPtr) return fail(YCNR_ERR_INVALID, "%s: null rowPtr", what);
  if (rowPtr[0] != 0) return fail(YCNR_ERR_INVALID, "%s: rowPtr[0] != 0", what);
  for (int64_t r = 0; r < nRows; ++r)
    if (rowPtr[r + 1] < rowPtr[r]) return fail(YCNR_ERR_INVALID, "%s: rowPtr decreases at row %lld", what, (long long)r);
  const int64_t total = rowPtr[nRows], fixedRows = h->rows(1 - side);
  if (total > 0 && (!indx || !vals)) return fail(YCNR_ERR_INVALID, "%s: null indx / vals", what);
  for (int64_t q = 0; q < total; ++q)
    if (indx[q] < 0 || indx[q] >= fixedRows)
      return fail(YCNR_ERR_INVALID, "%s: column id %d at position %lld is outside [0, %lld)", what, indx[q], (long long)q, (long long)fixedRows);
  if (storeIds) {
    std::vector<int32_t> ids(storeIds, storeIds + nRows);
    std::sort(ids.begin(), ids.end());
    if (nRows > 0 && (ids.front() < 0 || ids.back() >= h->rows(side)))
      return fail(YCNR_ERR_INVALID, "%s: a store id is outside [0, %lld)", what, (long long)h->rows(side));
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return fail(YCNR_ERR_INVALID, "%s: a store id is repeated", what);
  }
  return YCNR_OK;
}

// factorsCount > 128: the step kernels out of place, as the level-1 portion op drives them (als_calc_portion): the plan of a
// piece with every row in primal form, the solved rows into FOLD_ROWS, the fixed side = the handle's own device matrix
template <typename T>
int fold_launch_steps(ycnr_als *h, int side, int64_t nRows, const int64_t *rowPtr, double lambda) {
  typedef ycnr_als A;
  const int k = h->opt.factorsCount;
  const PlanParams P = out_of_place_plan_params(std::is_same<T, double>::value, k, gen_arena_bytes());
  const size_t slabElems = (size_t)step_slab_elems(P.kind, k);
  h->foldPlan = plan_piece(rowPtr, 0, nRows, P);  // (kept on the handle: its lists are the source of the copies below)
  const PiecePlan &plan = h->foldPlan;
  HIP_TRY(h->rec[A::FOLD_UNITS].reserve(sizeof(Unit) * std::max<size_t>(1, plan.units.size())));
  HIP_TRY(h->rec[A::FOLD_SPLIT].reserve(sizeof(SplitRow) * std::max<size_t>(1, plan.split.size())));
  HIP_TRY(h->rec[A::FOLD_SLABS].reserve(sizeof(T) * std::max<size_t>(1, (size_t)plan.arenaSlabs * slabElems)));
  HIP_TRY(h->rec[A::FOLD_ERR].reserve(sizeof(ErrInfo)));
  if (!plan.units.empty())
    HIP_TRY(hipMemcpyAsync(h->rec[A::FOLD_UNITS].get(), plan.units.data(), sizeof(Unit) * plan.units.size(), hipMemcpyHostToDevice, h->stream));
  if (!plan.split.empty())
    HIP_TRY(hipMemcpyAsync(h->rec[A::FOLD_SPLIT].get(), plan.split.data(), sizeof(SplitRow) * plan.split.size(), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemsetAsync(h->rec[A::FOLD_ERR].get(), 0, sizeof(ErrInfo), h->stream));
  StepArgs<T> a{(const Unit *)h->rec[A::FOLD_UNITS].get(), (const SplitRow *)h->rec[A::FOLD_SPLIT].get(), (const int32_t *)h->rec[A::FOLD_INDX].get(),
                (const T *)h->rec[A::FOLD_VALS].get(), (const T *)h->factors[1 - side], (const T *)h->dZeros.get(), (T *)h->rec[A::FOLD_ROWS].get(),
                (T *)h->rec[A::FOLD_SLABS].get(), (ErrInfo *)h->rec[A::FOLD_ERR].get(), lambda, k, 0, 0, 0u};
  return launch_out_of_place<T>(a, plan, h->stream);
}

// Uploads the (validated) request and enqueues its solve on the handle's stream; records recEv[0] in front of the kernels.
// Afterwards FOLD_ROWS holds nRows x factorsCount solved rows and FOLD_STATUS their status, both on the device.
template <typename T>
int fold_enqueue(ycnr_als *h, int side, int64_t nRows, const int64_t *rowPtr, const int32_t *indx, const void *vals, const int32_t *storeIds) {
  typedef ycnr_als A;
  const int k = h->opt.factorsCount;
  const int64_t total = rowPtr[nRows];
  const double lambda = side == YCNR_BY_USER ? h->opt.userFactReg : h->opt.itemFactReg;
  HIP_TRY(h->rec[A::FOLD_PTR].reserve((size_t)(nRows + 1) * 8));
  HIP_TRY(h->rec[A::FOLD_INDX].reserve(std::max<size_t>((size_t)total * 4 + 64, 8)));
  HIP_TRY(h->rec[A::FOLD_VALS].reserve(std::max<size_t>((size_t)total * sizeof(T) + 64, 8)));
  HIP_TRY(h->rec[A::FOLD_ROWS].reserve((size_t)nRows * k * sizeof(T)));
  HIP_TRY(h->rec[A::FOLD_STATUS].reserve((size_t)nRows * 4));
  if (storeIds)
    HIP_TRY(h->rec[A::FOLD_STORE].reserve((size_t)nRows * 4));
  for (Event &ev : h->recEv)
    if (!ev) HIP_TRY(hipEventCreate(ev.put()));
  // everything below is enqueued on the handle's stream: behind the half-steps in flight, like ycnr_als_rmse
  HIP_TRY(hipMemcpyAsync(h->rec[A::FOLD_PTR].get(), rowPtr, (size_t)(nRows + 1) * 8, hipMemcpyHostToDevice, h->stream));
  if (total) {
    HIP_TRY(hipMemcpyAsync(h->rec[A::FOLD_INDX].get(), indx, (size_t)total * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->rec[A::FOLD_VALS].get(), vals, (size_t)total * sizeof(T), hipMemcpyHostToDevice, h->stream));
  }
  if (storeIds) HIP_TRY(hipMemcpyAsync(h->rec[A::FOLD_STORE].get(), storeIds, (size_t)nRows * 4, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipEventRecord(h->recEv[0].get(), h->stream));
  T *store = storeIds ? (T *)h->factors[side] : nullptr;
  if (k <= kFoldMaxK) {
    FoldArgs<T> fa{(const int64_t *)h->rec[A::FOLD_PTR].get(), (const int32_t *)h->rec[A::FOLD_INDX].get(), (const T *)h->rec[A::FOLD_VALS].get(),
                   (const T *)h->factors[1 - side], (T *)h->rec[A::FOLD_ROWS].get(), (int32_t *)h->rec[A::FOLD_STATUS].get(), store,
                   (const int32_t *)h->rec[A::FOLD_STORE].get(), lambda, k};
    const size_t lds = foldin_lds_bytes(k);
    if (int rc = set_max_lds(reinterpret_cast<const void *>(als_foldin_kernel<T>), lds)) return rc;
    hipLaunchKernelGGL(als_foldin_kernel<T>, dim3((unsigned)nRows), dim3(256), lds, h->stream, fa);
    HIP_TRY(hipGetLastError());
    return YCNR_OK;
  }
  if (total > 0)
    if (int rc = fold_launch_steps<T>(h, side, nRows, rowPtr, lambda)) return rc;
  if (total == 0) {
    HIP_TRY(h->rec[A::FOLD_ERR].reserve(sizeof(ErrInfo)));
    HIP_TRY(hipMemsetAsync(h->rec[A::FOLD_ERR].get(), 0, sizeof(ErrInfo), h->stream));
  }
  hipLaunchKernelGGL(foldin_finish_kernel<T>, dim3((unsigned)nRows), dim3(256), 0, h->stream, (const int64_t *)h->rec[A::FOLD_PTR].get(),
                     (const ErrInfo *)h->rec[A::FOLD_ERR].get(), nRows, k, (T *)h->rec[A::FOLD_ROWS].get(), (int32_t *)h->rec[A::FOLD_STATUS].get(), store,
                     (const int32_t *)h->rec[A::FOLD_STORE].get());
  HIP_TRY(hipGetLastError());
  return YCNR_OK;
}
int fold_enqueue_any(ycnr_als *h, int side, int64_t nRows, const int64_t *rowPtr, const int32_t *indx, const void *vals, const int32_t *storeIds) {
  return h->opt.dtype == YCNR_F64 ? fold_enqueue<double>(h, side, nRows, rowPtr, indx, vals, storeIds)
                                  : fold_enqueue<float>(h, side, nRows, rowPtr, indx, vals, storeIds);
}
}  // namespace
}  // extern "C++"

int ycnr_als_recommend(ycnr_als *h, int64_t nUsers, const int32_t *userIds, const int64_t *skipPtr, const int32_t *skipIds,
                       double globalAvgShift, double minRecommendRating, int32_t limit, int32_t *outIds, double *outPredict,
                       int32_t *outCount, double *deviceMs) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (nUsers < 0 || limit < 1 || limit > 4096) return fail(YCNR_ERR_INVALID, "ycnr_als_recommend: bad nUsers / limit");
  if (nUsers == 0) {
    if (deviceMs) *deviceMs = 0.0;
    return YCNR_OK;
  }
  if (!userIds || !skipPtr || !outIds || !outPredict || !outCount) return fail(YCNR_ERR_INVALID, "ycnr_als_recommend: null argument");
  for (int64_t u = 0; u < nUsers; ++u)
    if (userIds[u] < 0 || userIds[u] >= h->opt.totalUsersCount)
      return fail(YCNR_ERR_INVALID, "ycnr_als_recommend: user id %d at position %lld is outside [0, %lld)", userIds[u], (long long)u,
                  (long long)h->opt.totalUsersCount);
  if (int rc = check_skip_lists("ycnr_als_recommend", nUsers, skipPtr, skipIds)) return rc;
  return recommend_run(h, h->factors[YCNR_BY_USER], nUsers, userIds, skipPtr, skipIds, globalAvgShift, minRecommendRating, limit, outIds, outPredict,
                       outCount, deviceMs, false, nullptr, std::function<int()>());
}

int ycnr_als_fold_in(ycnr_als *h, int side, int64_t nRows, const int64_t *rowPtr, const int32_t *indx, const void *vals,
                     const int32_t *storeIds, void *outRows, int32_t *outStatus, double *deviceMs) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (side != YCNR_BY_USER && side != YCNR_BY_ITEM) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  if (nRows < 0 || nRows > 0x7fffffffLL) return fail(YCNR_ERR_INVALID, "ycnr_als_fold_in: bad nRows");
  if (nRows == 0) {
    if (deviceMs) *deviceMs = 0.0;
    return YCNR_OK;
  }
  if (!outRows || !outStatus) return fail(YCNR_ERR_INVALID, "ycnr_als_fold_in: null argument");
  if (int rc = fold_check("ycnr_als_fold_in", h, side, nRows, rowPtr, indx, vals, storeIds)) return rc;
  HIP_TRY(hipSetDevice(h->opt.device));
  if (int rc = fold_enqueue_any(h, side, nRows, rowPtr, indx, vals, storeIds)) return rc;
  typedef ycnr_als A;
  HIP_TRY(hipEventRecord(h->recEv[1].get(), h->stream));
  HIP_TRY(hipMemcpyAsync(outRows, h->rec[A::FOLD_ROWS].get(), (size_t)nRows * h->opt.factorsCount * h->ts(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(outStatus, h->rec[A::FOLD_STATUS].get(), (size_t)nRows * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (deviceMs) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->recEv[0].get(), h->recEv[1].get()));
    *deviceMs = ms;
  }
  return YCNR_OK;
}

int ycnr_als_recommend_for_ratings(ycnr_als *h, int64_t nUsers, const int64_t *ratPtr, const int32_t *ratIds, const void *ratVals,
                                   const int64_t *skipPtr, const int32_t *skipIds, double globalAvgShift, double minRecommendRating,
                                   int32_t limit, int32_t *outIds, double *outPredict, int32_t *outCount, void *outRows, int32_t *outStatus,
                                   double *deviceMs) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (nUsers < 0 || nUsers > 0x7fffffffLL || limit < 1 || limit > 4096) return fail(YCNR_ERR_INVALID, "ycnr_als_recommend_for_ratings: bad nUsers / limit");
  if (nUsers == 0) {
    if (deviceMs) *deviceMs = 0.0;
    return YCNR_OK;
  }
  if (!skipPtr || !outIds || !outPredict || !outCount || !outStatus) return fail(YCNR_ERR_INVALID, "ycnr_als_recommend_for_ratings: null argument");
  if (int rc = fold_check("ycnr_als_recommend_for_ratings", h, YCNR_BY_USER, nUsers, ratPtr, ratIds, ratVals, nullptr)) return rc;
  if (int rc = check_skip_lists("ycnr_als_recommend_for_ratings", nUsers, skipPtr, skipIds)) return rc;
  HIP_TRY(hipSetDevice(h->opt.device));
  if (int rc = fold_enqueue_any(h, YCNR_BY_USER, nUsers, ratPtr, ratIds, ratVals, nullptr)) return rc;
  typedef ycnr_als A;
  const size_t rowBytes = (size_t)nUsers * h->opt.factorsCount * h->ts();
  // the solved rows never leave the device between the two halves; their copy to the host rides behind the top-N
  auto copies = [&]() -> int {
    if (outRows) HIP_TRY(hipMemcpyAsync(outRows, h->rec[A::FOLD_ROWS].get(), rowBytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(outStatus, h->rec[A::FOLD_STATUS].get(), (size_t)nUsers * 4, hipMemcpyDeviceToHost, h->stream));
    return YCNR_OK;
  };
  return recommend_run(h, h->rec[A::FOLD_ROWS].get(), nUsers, nullptr, skipPtr, skipIds, globalAvgShift, minRecommendRating, limit, outIds, outPredict,
                       outCount, deviceMs, true, (const int32_t *)h->rec[A::FOLD_STATUS].get(), copies);
}

// ---- multi-GPU exchange (comm_impl.hip.h) ----

int ycnr_comm_unique_id(int transport, void *id) {
  if (!id) return fail(YCNR_ERR_INVALID, "ycnr_comm_unique_id: null id");
  memset(id, 0, YCNR_COMM_ID_BYTES);
  if (transport == YCNR_COMM_RCCL) {
    const RcclApi *api = nullptr;
    int rc = rccl_api(&api);
    if (rc) return rc;
    ncclUniqueId uid;
    NCCL_TRY(api, api->GetUniqueId(&uid));
    memcpy(id, &uid, sizeof uid);
    return YCNR_OK;
  }
  if (transport == YCNR_COMM_STUB) return YCNR_OK;
  if (transport == YCNR_COMM_SHM || transport == YCNR_COMM_IPC) {
    FILE *f = fopen("/dev/urandom", "rb");
    if (!f || fread(id, 1, 16, f) != 16) {
      if (f) fclose(f);
      return fail(YCNR_ERR_HIP, "ycnr_comm_unique_id: cannot read /dev/urandom");
    }
    fclose(f);
    return YCNR_OK;
  }
  return fail(YCNR_ERR_INVALID, "ycnr_comm_unique_id: unknown transport %d", transport);
}

int ycnr_als_comm_init(ycnr_als *h, int transport, const void *id, int rank, int world) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (h->comm.transport != YCNR_COMM_NONE) return fail(YCNR_ERR_STATE, "comm_init: the handle already has a communicator");
  HIP_TRY(hipSetDevice(h->opt.device));
  // the staged stand-in needs room for the larger matrix (an exchange never stages more than one side)
  const size_t big = (size_t)std::max(h->opt.totalUsersCount, h->opt.totalItemsCount) * h->opt.factorsCount * h->ts();
  int rc = comm_setup(h->comm, id, transport, rank, world, std::max<size_t>(big, (size_t)1 << 20));
  if (!rc && transport == YCNR_COMM_IPC) rc = ipc_publish(h->comm, h->factors);
  if (rc) comm_release(h->comm);
  return rc;
}

int ycnr_als_comm_info(ycnr_als *h, int32_t out[4]) {
  if (!h || !out) return fail(YCNR_ERR_INVALID, "null argument");
  out[0] = h->comm.transport;
  out[1] = h->comm.rank;
  out[2] = h->comm.world;
  out[3] = -1;
  if (h->comm.transport == YCNR_COMM_RCCL && h->comm.nccl && h->comm.api && h->comm.api->CommCount) {
    int n = -1;
    NCCL_TRY(h->comm.api, h->comm.api->CommCount(h->comm.nccl, &n));
    out[3] = n;
  }
  return YCNR_OK;
}

int ycnr_als_comm_destroy(ycnr_als *h) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  (void)hipSetDevice(h->opt.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  comm_release(h->comm);
  // exchange ranges belong to the communicator they were made for: a later ycnr_als_set_ratings[_sharded] renews them
  h->bounds[0].clear();
  h->bounds[1].clear();
  return YCNR_OK;
}

int ycnr_als_defer_exchange(ycnr_als *h, int side, int deferred) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (side != 0 && side != 1) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  h->deferExchange[side] = deferred != 0;
  return YCNR_OK;
}

int ycnr_als_exchange(ycnr_als *h, int side) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (side != 0 && side != 1) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  if (!h->comm.active()) return YCNR_OK;
  if (h->bounds[side].empty() || h->parts[side].empty()) return fail(YCNR_ERR_STATE, "exchange: no sharded upload for this side");
  HIP_TRY(hipSetDevice(h->opt.device));
  const int world = h->comm.world, np = (int)h->parts[side].size();
  if (h->bounds[side].size() != (size_t)world * (size_t)(np + 1)) return fail(YCNR_ERR_STATE, "exchange: the sharded upload was made for another communicator");
  std::vector<int64_t> b((size_t)world), e((size_t)world);
  for (int r = 0; r < world; ++r) {
    b[(size_t)r] = h->bounds[side][(size_t)r * (np + 1)];
    e[(size_t)r] = h->bounds[side][(size_t)r * (np + 1) + np];
  }
  Part &p0 = h->parts[side][0];
  if (int rcb = ipc_enter(h->comm)) return rcb;
  int rc = comm_exchange(h->comm, h->factors[side], side, h->opt.factorsCount, h->ts(), b.data(), e.data(), h->stream, p0.ready.get(), p0.x0.get(), p0.x1.get(), nullptr);
  if (rc) return rc;
  if (h->comm.transport != YCNR_COMM_SHM) HIP_TRY(hipStreamSynchronize(h->comm.stream));
  return ipc_finish(h->comm);
}

int ycnr_als_allreduce_sum(ycnr_als *h, double *vals, int64_t n) {
  if (!h || (n > 0 && !vals)) return fail(YCNR_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(h->opt.device));
  return comm_allreduce_sum(h->comm, vals, n);
}

int ycnr_als_broadcast_factors(ycnr_als *h, int side, int root) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (side != 0 && side != 1) return fail(YCNR_ERR_INVALID, "bad side %d", side);
  HIP_TRY(hipSetDevice(h->opt.device));
  return comm_broadcast(h->comm, h->factors[side], side, (size_t)h->rows(side) * h->opt.factorsCount * h->ts(), root, h->stream);
}

// One self-addressed send / receive pair and one all-reduce through the handle's communicator:
// lets a single-GPU box prove that the RCCL calls of the exchange run (tests/test_gpu_comm.py).
int ycnr_als_comm_selftest(ycnr_als *h, int64_t nFloats) {
  if (!h) return fail(YCNR_ERR_INVALID, "null handle");
  if (h->comm.transport == YCNR_COMM_NONE) return fail(YCNR_ERR_STATE, "comm_selftest: no communicator");
  if (nFloats < 1) return fail(YCNR_ERR_INVALID, "comm_selftest: nFloats < 1");
  HIP_TRY(hipSetDevice(h->opt.device));
  Comm &c = h->comm;
  std::vector<float> src((size_t)nFloats), got((size_t)nFloats);
  for (int64_t i = 0; i < nFloats; ++i) src[(size_t)i] = (float)((i * 2654435761u) % 65521) + 0.25f * (float)c.rank;
  double sum[3] = {1.0 + c.rank, 2.0, -0.5 * c.rank};
  if (c.transport == YCNR_COMM_RCCL) {
    DevPtr<void> a, b;
    HIP_TRY(hipMalloc(a.put(), sizeof(float) * (size_t)nFloats));
    HIP_TRY(hipMalloc(b.put(), sizeof(float) * (size_t)nFloats));
    HIP_TRY(hipMemcpy(a.get(), src.data(), sizeof(float) * (size_t)nFloats, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b.get(), 0, sizeof(float) * (size_t)nFloats));
    NCCL_TRY(c.api, c.api->GroupStart());
    NCCL_TRY(c.api, c.api->Send(a.get(), (size_t)nFloats, ncclFloat, c.rank, c.nccl, c.stream));
    NCCL_TRY(c.api, c.api->Recv(b.get(), (size_t)nFloats, ncclFloat, c.rank, c.nccl, c.stream));
    NCCL_TRY(c.api, c.api->GroupEnd());
    HIP_TRY(hipStreamSynchronize(c.stream));
    HIP_TRY(hipMemcpy(got.data(), b.get(), sizeof(float) * (size_t)nFloats, hipMemcpyDeviceToHost));
    if (memcmp(got.data(), src.data(), sizeof(float) * (size_t)nFloats) != 0)
      return fail(YCNR_ERR_STATE, "comm_selftest: the self-addressed ncclSend / ncclRecv pair did not return the bytes sent");
  }
  int rc = comm_allreduce_sum(c, sum, 3);
  if (rc) return rc;
  const double w = c.world;
  const double want[3] = {w + w * (w - 1) / 2, 2.0 * w, -0.5 * w * (w - 1) / 2};
  for (int i = 0; i < 3; ++i)
    if (!(fabs(sum[i] - want[i]) <= 1e-12 * (1 + fabs(want[i])))) return fail(YCNR_ERR_STATE, "comm_selftest: all-reduce gave %g, expected %g", sum[i], want[i]);
  return YCNR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------ level 1

namespace {

// Per-thread state of the level-1 portion ops: the reference calls mw_calcTrainAlsPortion ~11 500
// times per MAL half-step (EmfBase.js:99-103: 10 000 ratings per portion), so stream, device
// buffers and -- when the host pins it -- the fixed factor matrix stay alive between calls.
struct L1State {
  int device = -1;
  Stream stream;
  GrowBuf<ArenaAlloc> io, slabs, misc;  // io: [solved | ErrInfo | units | split | indx | vals | compacted fixed rows]; misc: zero row
  // page-locked host image of io: ONE copy in (everything behind the solved rows) and ONE copy out (solved rows +
  // ErrInfo) per portion instead of five pageable copies, two memsets and two copies back
  GrowBuf<PinnedAlloc> hostIo;
  // fixed matrix pinned by ycnr_{s,d}AlsPinFixedFactors
  const void *pinnedHost = nullptr;
  int64_t pinnedRows = 0;
  int pinnedK = 0, pinnedDtype = -1;
  GrowBuf<ArenaAlloc> pinned;
};
struct L1Ctx : L1State {
  void release() {  // on the state's device, with its stream drained, before the members go
    if (device >= 0) (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream.get());
    static_cast<L1State &>(*this) = L1State();
  }
  ~L1Ctx() { release(); }
};

L1Ctx &l1ctx() {
  static thread_local L1Ctx c;
  return c;
}

// stream + the small fixed buffers, on the calling thread's current device
int l1_prepare(L1Ctx &C) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (C.device != dev) {
    C.release();
    C.device = dev;
  }
  if (!C.stream) HIP_TRY(hipStreamCreateWithFlags(C.stream.put(), hipStreamNonBlocking));
  if (!C.misc.get()) {
    HIP_TRY(C.misc.reserve(kZeroRowBytes));
    HIP_TRY(hipMemsetAsync(C.misc.get(), 0, kZeroRowBytes, C.stream.get()));
  }
  return YCNR_OK;
}

template <typename T>
int pin_fixed(const T *fixed, int64_t rows, int k, int dtype) {
  if (!fixed || rows < 1 || k < 1) return fail(YCNR_ERR_INVALID, "AlsPinFixedFactors: bad argument");
  L1Ctx &C = l1ctx();
  int rc = l1_prepare(C);
  if (rc) return rc;
  const size_t bytes = (size_t)rows * k * sizeof(T);
  HIP_TRY(C.pinned.reserve(bytes));
  HIP_TRY(hipMemcpyAsync(C.pinned.get(), fixed, bytes, hipMemcpyHostToDevice, C.stream.get()));
  HIP_TRY(hipStreamSynchronize(C.stream.get()));
  C.pinnedHost = fixed;
  C.pinnedRows = rows;
  C.pinnedK = k;
  C.pinnedDtype = dtype;
  return YCNR_OK;
}

// Shared body of ycnr_{s,d}AlsCalcPortion.  Unless the caller has pinned this fixed matrix, the portion's
// column ids are compacted on the host (a 10 000-rating portion never needs more than 10 000 fixed
// rows) and only those rows are uploaded; the solved rows are scattered back into the caller's matrix.
template <typename T>
int64_t als_calc_portion(double lambda, int k, const int32_t *alsRows, const int32_t *alsIndx, const T *alsVals,
                         const T *fixedFactors, int64_t fixedRows, T *solvedFactors, int64_t solvedRows, int dtype) {
  if (!alsRows || !alsIndx || !alsVals || !fixedFactors || !solvedFactors)
    return fail(YCNR_ERR_INVALID, "AlsCalcPortion: null argument");
  if (k < 1) return fail(YCNR_ERR_INVALID, "AlsCalcPortion: k < 1");
  if (k > kMaxFactorsAny) return fail(YCNR_ERR_UNSUPPORTED, "factorsCount %d > %d is not supported by this build", k, kMaxFactorsAny);
  if (!(lambda >= 0)) return fail(YCNR_ERR_INVALID, "AlsCalcPortion: negative lambda");
  const int nRows = alsRows[0];
  if (nRows < 0) return fail(YCNR_ERR_INVALID, "AlsCalcPortion: alsRows[0] < 0");
  if (nRows == 0) return 0;
  std::vector<int64_t> rowPtr((size_t)nRows + 1, 0);
  for (int r = 0; r < nRows; ++r) {
    const int rowId = alsRows[1 + 2 * r], cols = alsRows[2 + 2 * r];
    if (rowId < 0 || rowId >= solvedRows) return fail(YCNR_ERR_INVALID, "AlsCalcPortion: rowId %d outside [0, %lld)", rowId, (long long)solvedRows);
    if (cols < 0) return fail(YCNR_ERR_INVALID, "AlsCalcPortion: negative cols");
    rowPtr[r + 1] = rowPtr[r] + cols;
  }
  const int64_t total = rowPtr[nRows];
  if (total == 0) return 0;
  int32_t lo = alsIndx[0], hi = alsIndx[0];
  for (int64_t i = 1; i < total; ++i) {
    lo = std::min(lo, alsIndx[i]);
    hi = std::max(hi, alsIndx[i]);
  }
  if (lo < 0 || hi >= fixedRows)
    return fail(YCNR_ERR_INVALID, "AlsCalcPortion: column id out of range (min %d, max %d, fixedRows %lld)", lo, hi, (long long)fixedRows);
  L1Ctx &C = l1ctx();
  int rc = l1_prepare(C);
  if (rc) return rc;
  // The reference's host updates its matrices in place: the matrix pinned for 'byUser' is the one 'byItem' writes.
  // A portion that SOLVES into the pinned host range makes the device copy stale: drop the pin (the host pins
  // again at its next 'startTrainStep'; until then portions upload the rows they need).
  if (C.pinnedHost) {
    const char *pb = (const char *)C.pinnedHost, *pe = pb + (size_t)C.pinnedRows * C.pinnedK * tsize(C.pinnedDtype);
    const char *sb = (const char *)solvedFactors, *se = sb + (size_t)solvedRows * k * sizeof(T);
    if (sb < pe && pb < se) C.pinnedHost = nullptr;
  }
  const bool pinned = C.pinnedHost == fixedFactors && C.pinnedRows == fixedRows && C.pinnedK == k && C.pinnedDtype == dtype;
  // compact the referenced fixed rows unless the whole matrix is resident
  std::vector<int32_t> uniq, remap;  // remap: fixed row -> compacted row when the fixed side is small enough to mark
  if (!pinned) {
    if (fixedRows <= 16 * total) {
      remap.assign((size_t)fixedRows, -1);
      for (int64_t i = 0; i < total; ++i) remap[alsIndx[i]] = 0;
      for (int64_t r = 0; r < fixedRows; ++r)
        if (remap[r] == 0) {
          remap[r] = (int32_t)uniq.size();
          uniq.push_back((int32_t)r);
        }
    } else {
      uniq.assign(alsIndx, alsIndx + total);
      std::sort(uniq.begin(), uniq.end());
      uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    }
  }
  // the plan of a piece of the resident trainer (build_part) with every row in primal form and the split rows in row order;
  // any-k path: solved in batches whose images fit the arena
  const PlanParams P = out_of_place_plan_params(std::is_same<T, double>::value, k, gen_arena_bytes());
  const size_t slabElems = (size_t)step_slab_elems(P.kind, k);
  const PiecePlan plan = plan_piece(rowPtr.data(), 0, nRows, P);
  const std::vector<Unit> &units = plan.units;
  const std::vector<SplitRow> &split = plan.split;
#define L1_TRY(expr)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess)                                                                             \
      return fail(e_ == hipErrorOutOfMemory ? YCNR_ERR_NOMEM : YCNR_ERR_HIP, "%s failed: %s", #expr,  \
                  hipGetErrorString(e_));                                                             \
  } while (0)
  // layout of the io arena (device) and of its page-locked host image, 256-byte aligned parts
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t oSolved = 0, bSolved = sizeof(T) * (size_t)nRows * k;
  const size_t oErr = al(oSolved + bSolved);
  const size_t oUnits = al(oErr + sizeof(ErrInfo)), oSplit = al(oUnits + sizeof(Unit) * std::max<size_t>(1, units.size()));
  const size_t oIndx = al(oSplit + sizeof(SplitRow) * std::max<size_t>(1, split.size()));
  const size_t oVals = al(oIndx + sizeof(int32_t) * (size_t)total + 64);
  const size_t oFixed = al(oVals + sizeof(T) * (size_t)total + 64);
  const size_t ioBytes = al(oFixed + (pinned ? 0 : sizeof(T) * uniq.size() * (size_t)k));
  L1_TRY(C.io.reserve(ioBytes));
  L1_TRY(C.hostIo.reserve(ioBytes));
  L1_TRY(C.slabs.reserve(sizeof(T) * std::max<size_t>(1, (size_t)plan.arenaSlabs * slabElems)));
  char *hb = (char *)C.hostIo.get(), *db = (char *)C.io.get();
  memset(hb + oErr, 0, sizeof(ErrInfo));
  if (!units.empty()) memcpy(hb + oUnits, units.data(), sizeof(Unit) * units.size());
  if (!split.empty()) memcpy(hb + oSplit, split.data(), sizeof(SplitRow) * split.size());
  if (pinned) {
    memcpy(hb + oIndx, alsIndx, sizeof(int32_t) * (size_t)total);
  } else {
    int32_t *cidx = (int32_t *)(hb + oIndx);
    if (!remap.empty()) {
      for (int64_t i = 0; i < total; ++i) cidx[i] = remap[alsIndx[i]];
    } else {
      for (int64_t i = 0; i < total; ++i) cidx[i] = (int32_t)(std::lower_bound(uniq.begin(), uniq.end(), alsIndx[i]) - uniq.begin());
    }
    T *cfix = (T *)(hb + oFixed);
    for (size_t u = 0; u < uniq.size(); ++u) memcpy(cfix + u * k, fixedFactors + (size_t)uniq[u] * k, sizeof(T) * k);
  }
  memcpy(hb + oVals, alsVals, sizeof(T) * (size_t)total);
  hipStream_t stream = C.stream.get();
  ErrInfo *dErr = (ErrInfo *)(db + oErr);
  T *dZeros = (T *)C.misc.get();
  L1_TRY(hipMemcpyAsync(db + oErr, hb + oErr, ioBytes - oErr, hipMemcpyHostToDevice, stream));
  {
    // rows are numbered 0..nRows-1 on the device and scattered to rowId on the host
    const T *dFixed = pinned ? (const T *)C.pinned.get() : (const T *)(db + oFixed);
    StepArgs<T> a{(const Unit *)(db + oUnits), (const SplitRow *)(db + oSplit), (const int32_t *)(db + oIndx), (const T *)(db + oVals), dFixed, dZeros,
                  (T *)(db + oSolved), (T *)C.slabs.get(), dErr, lambda, k, 0, 0, 0u};
    if ((rc = launch_out_of_place<T>(a, plan, stream))) return rc;
  }
  // rows without ratings are never written by the kernels and never copied back below
  L1_TRY(hipMemcpyAsync(hb + oSolved, db + oSolved, oErr + sizeof(ErrInfo), hipMemcpyDeviceToHost, stream));
  L1_TRY(hipStreamSynchronize(stream));
#undef L1_TRY
  const ErrInfo ei = *(const ErrInfo *)(hb + oErr);
  const T *hostSolved = (const T *)(hb + oSolved);
  if (ei.count > 0)
    return fail(YCNR_ERR_NUMERIC, "%d row(s) of the portion had a normal matrix that is not positive definite", ei.count);
  for (int r = 0; r < nRows; ++r) {
    if (rowPtr[r + 1] == rowPtr[r]) continue;  // cols == 0: left untouched
    memcpy(solvedFactors + (size_t)alsRows[1 + 2 * r] * k, hostSolved + (size_t)r * k, sizeof(T) * k);
  }
  return total;
}

template <typename T>
int rmse_portion(int k, const int32_t *rows, const int32_t *indx, const T *vals, const T *uF, int64_t usersRows,
                 const T *iF, int64_t itemsRows, double shift, double *out3, int dtype) {
  if (!rows || !indx || !vals || !uF || !iF || !out3) return fail(YCNR_ERR_INVALID, "RmsePortion: null argument");
  if (k < 1) return fail(YCNR_ERR_INVALID, "RmsePortion: k < 1");
  const int nRows = rows[0];
  out3[0] = out3[1] = out3[2] = 0;
  if (nRows < 0) return fail(YCNR_ERR_INVALID, "RmsePortion: rmseRows[0] < 0");
  if (nRows == 0) return YCNR_OK;
  // compact users and items, then run the resident kernel on the compacted problem
  std::vector<int64_t> rowPtr((size_t)nRows + 1, 0);
  for (int r = 0; r < nRows; ++r) {
    const int u = rows[1 + 2 * r], cols = rows[2 + 2 * r];
    if (u < 0 || u >= usersRows || cols < 0) return fail(YCNR_ERR_INVALID, "RmsePortion: bad row entry %d", r);
    rowPtr[r + 1] = rowPtr[r] + cols;
  }
  const int64_t total = rowPtr[nRows];
  if (total == 0) return YCNR_OK;
  std::vector<int32_t> uniq(indx, indx + total);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  if (uniq.front() < 0 || uniq.back() >= itemsRows) return fail(YCNR_ERR_INVALID, "RmsePortion: item id out of range");
  std::vector<int32_t> cidx((size_t)total);
  for (int64_t i = 0; i < total; ++i)
    cidx[i] = (int32_t)(std::lower_bound(uniq.begin(), uniq.end(), indx[i]) - uniq.begin());
  std::vector<T> cI(uniq.size() * (size_t)k), cU((size_t)nRows * k);
  for (size_t j = 0; j < uniq.size(); ++j) memcpy(&cI[j * k], iF + (size_t)uniq[j] * k, sizeof(T) * k);
  for (int r = 0; r < nRows; ++r) memcpy(&cU[(size_t)r * k], uF + (size_t)rows[1 + 2 * r] * k, sizeof(T) * k);

  ycnr_als_options o{};
  o.struct_size = (int32_t)sizeof o;
  o.device = 0;
  o.dtype = dtype;
  o.factorsCount = k;
  o.totalUsersCount = nRows;
  o.totalItemsCount = (int64_t)uniq.size();
  ycnr_als *h = nullptr;
  int rc = ycnr_als_create(&o, &h);
  if (rc) return rc;
  rc = ycnr_als_set_factors(h, YCNR_BY_USER, cU.data(), YCNR_MEM_HOST);
  if (!rc) rc = ycnr_als_set_factors(h, YCNR_BY_ITEM, cI.data(), YCNR_MEM_HOST);
  if (!rc) rc = ycnr_als_set_rmse_ratings(h, YCNR_RMSE_VALIDATE, rowPtr.data(), cidx.data(), vals, 0, nRows, YCNR_MEM_HOST);
  if (!rc) rc = ycnr_als_rmse(h, YCNR_RMSE_VALIDATE, shift, 0, nullptr, out3);
  ycnr_als_destroy(h);
  return rc;
}

}  // namespace

extern "C" {

int64_t ycnr_sAlsCalcPortion(double lambda, int k, const int32_t *alsRows, const int32_t *alsIndx, const float *alsVals,
                             const float *fixedFactors, int64_t fixedRows, float *solvedFactors, int64_t solvedRows) {
  return als_calc_portion<float>(lambda, k, alsRows, alsIndx, alsVals, fixedFactors, fixedRows, solvedFactors,
                                 solvedRows, YCNR_F32);
}

int64_t ycnr_dAlsCalcPortion(double lambda, int k, const int32_t *alsRows, const int32_t *alsIndx, const double *alsVals,
                             const double *fixedFactors, int64_t fixedRows, double *solvedFactors, int64_t solvedRows) {
  return als_calc_portion<double>(lambda, k, alsRows, alsIndx, alsVals, fixedFactors, fixedRows, solvedFactors,
                                  solvedRows, YCNR_F64);
}

int ycnr_sAlsPinFixedFactors(const float *fixedFactors, int64_t fixedRows, int k) {
  return pin_fixed<float>(fixedFactors, fixedRows, k, YCNR_F32);
}
int ycnr_dAlsPinFixedFactors(const double *fixedFactors, int64_t fixedRows, int k) {
  return pin_fixed<double>(fixedFactors, fixedRows, k, YCNR_F64);
}
int ycnr_AlsUnpinFixedFactors(void) {
  l1ctx().pinnedHost = nullptr;
  return YCNR_OK;
}
int ycnr_AlsReleasePortionState(void) {
  l1ctx().release();
  return YCNR_OK;
}

int ycnr_sRmsePortion(int k, const int32_t *rmseRows, const int32_t *rmseIndx, const float *rmseVals,
                      const float *userFactors, int64_t usersRows, const float *itemFactors, int64_t itemsRows,
                      double globalAvgShift, double *out3) {
  return rmse_portion<float>(k, rmseRows, rmseIndx, rmseVals, userFactors, usersRows, itemFactors, itemsRows,
                             globalAvgShift, out3, YCNR_F32);
}

int ycnr_dRmsePortion(int k, const int32_t *rmseRows, const int32_t *rmseIndx, const double *rmseVals,
                      const double *userFactors, int64_t usersRows, const double *itemFactors, int64_t itemsRows,
                      double globalAvgShift, double *out3) {
  return rmse_portion<double>(k, rmseRows, rmseIndx, rmseVals, userFactors, usersRows, itemFactors, itemsRows,
                              globalAvgShift, out3, YCNR_F64);
}

}  // extern "C"
