// What the host translation units of libgpso_hip.so share (api.hip, engine_points.hip, engine_variational.hip): the context
// behind the C-ABI's handle, the current-device guard, the pool of host-side resources, the two status macros and the
// file-level constants.  note_launch_error and ensure_dyn_lds are declared in kernels.hpp; api.hip defines them.
#pragma once
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gpso_hip.h"
#include "best_call.hpp"
#include "common.hpp"
#include "fit_call.hpp"
#include "kernels.hpp"
#include "rccl_api.hpp"
#include "theta.hpp"

namespace gpso::host {

constexpr int kMaxD = 48;                      // padded input dimension limit (LDS budgets)
constexpr int64_t kLeafChunk = (int64_t)1 << 20;  // leaves processed per pass of the tile kernel
// GPSO_OPT_PARK_BYTES as a context is created: 256 MB, the best median of the sweeps 0 | 64 | 128 | 256 MB at C3
// (profiles/park_reload_ab_sweep_c3.txt, park_reload_ab_pairs.txt; -DGPSO_PARK_BYTES_DEFAULT=... builds the other arms)
// GPSO_OPT_SCREEN as a context is created (-DGPSO_SCREEN_DEFAULT=0 builds the unscreened arm of an A/B through bench.py)
#ifndef GPSO_SCREEN_DEFAULT
#define GPSO_SCREEN_DEFAULT 1
#endif
// GPSO_OPT_SURVIVOR_TILE as a context is created (-DGPSO_SURVIVOR_TILE_DEFAULT=1 builds the wide arm of an A/B through bench.py)
#ifndef GPSO_SURVIVOR_TILE_DEFAULT
#define GPSO_SURVIVOR_TILE_DEFAULT 0
#endif
#ifndef GPSO_PARK_BYTES_DEFAULT
#define GPSO_PARK_BYTES_DEFAULT (256 << 20)
#endif
constexpr int64_t kParkBytesDefault = GPSO_PARK_BYTES_DEFAULT;
constexpr int kHyperHeader = 8;                // doubles in front of the lengthscales
static_assert(kThetaMaxLs == kGradMaxLs, "a Theta holds as many lengthscales as the gradient kernels take");
using FitScratch = gpso::FitScratch<kGradMaxLs, kHyperHeader, kMaxD>;  // (fit_call.hpp: the pinned scratch of a fit call)
using FitCall = gpso::FitCall<FitScratch>;

struct EngineCore;  // (engine_core.hpp)

}  // namespace gpso::host

// current-device guard: HIP calls act on the calling thread's current device
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = (prev == dev) || hipSetDevice(dev) == hipSuccess;
    if (prev == dev) prev = -1;  // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

struct gpso_ctx {
  int device = 0;
  int dtype = GPSO_F64;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev[8] = {};  // [0..1] spare, [2..3] a point call (points_begin / points_end) or a best-UCB call (finish_best), [4..5] fit, [6..7] the collective of a sharded call
  std::vector<hipEvent_t> tile_ev;  // start/stop pairs around the leaf-tile kernel, one per chunk (how many were recorded: TileSpan)
  double last_ms[4] = {0, 0, 0, 0};
  bool timing = true;  // GPSO_OPT_TIMING: does the call in flight record the event pairs gpso_last_ms reads (two to four HIP calls)?
  int timing_every = 1;  // ... 0: never, 1: every fit / predict-type call, k: every k-th one (the others leave gpso_last_ms alone)
  long timed_calls = 0;
  void tick_timing() { timing = timing_every > 0 && (timed_calls++ % timing_every) == 0; }
  // multi-GPU group (gpso_comm_init): one RCCL communicator per context, collectives on ctx->stream
  ncclComm_t comm = nullptr;
  // gpso_comm_abort (callable from another thread): the communicator is gone -- not to be destroyed again, and not to be
  // handed to a collective again either (need_comm refuses until gpso_comm_destroy + gpso_comm_init)
  std::atomic<bool> comm_aborted{false};
  int rank = 0, world = 1;
  // leaves scored / leaves asked for by the last predict-type call; [2] GPSO_FITMATH_* of the last fit; [3] workgroups per
  // leaf tile of this context's last split-kernel launch
  int64_t last_count[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // ([4] is not stored: gpso_last_count)
  int cu_count = 256;  // compute units of `device` (gpso_create): sizes the split predict kernels' and the bf16 GEMMs' grids
  std::string err;
  gpso::host::EngineCore* eng = nullptr;
  hipEvent_t ev_wait = nullptr;  // completion marker of the call in flight
  hipStream_t side_stream = nullptr;  // look-ahead of the two-level fits (kernels.hpp: FitPlanes)
  hipEvent_t ev_col = nullptr, ev_chain = nullptr;
  hipStream_t inv_stream = nullptr;   // the overlapped inverse of the two-level double fit
  hipEvent_t ev_panel = nullptr, ev_inv = nullptr;
  double* pinned = nullptr;      // pinned host scratch for the small result read-backs
  size_t pinned_doubles = 0;
  double* stage = nullptr;       // pinned staging of small host inputs (training data, bounds)
  size_t stage_doubles = 0;
  // gpso_best_ucb_begin / _end: two calls may be in flight; each has a pinned result slot of its own and a completion event
  static constexpr int kSlots = 2;
  static constexpr size_t kSlotDoubles = 4 * 1024 + 4;  // nseg <= 1024 per asynchronous call (+ the completion token)
  gpso::BestTicket<hipEvent_t> tickets[kSlots];  // (best_call.hpp: the enqueue's record, the completion event, in use)
  double* slot_host = nullptr;   // [kSlots][kSlotDoubles], pinned
  int next_ticket = 0;           // tickets are handed out in turn (the other one where that one is still open)
  int slots_busy() const { return (int)tickets[0].in_use + (int)tickets[1].in_use; }

  // A blocking wait parks the thread on an interrupt and costs tens of microseconds to wake up -- the device work of a small fit.
  // The calling thread is blocked in this library anyway: poll done() (hipErrorNotReady: go on) for up to kSpinMs, then block().
  template <int kPollMask, typename Done, typename Block>
  static hipError_t spin_then_block(Done&& done, Block&& block) {
    constexpr double kSpinMs = 20.0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0;; ++it) {
      const hipError_t e = done();
      if (e != hipErrorNotReady) return e;
      if ((it & kPollMask) == kPollMask &&
          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > kSpinMs)
        return block();
    }
  }
  // wait for everything queued on s
  hipError_t wait(hipStream_t s) {
    const hipError_t e = hipEventRecord(ev_wait, s);
    if (e != hipSuccess) return e;
    return spin_then_block<63>([&] { return hipEventQuery(ev_wait); }, [&] { return hipStreamSynchronize(s); });
  }
  hipError_t wait_event(hipEvent_t ev) { return spin_then_block<63>([&] { return hipEventQuery(ev); }, [&] { return hipEventSynchronize(ev); }); }
  double* pinned_scratch(size_t doubles) {
    if (doubles > pinned_doubles) {
      if (pinned) (void)hipHostFree(pinned);
      pinned = nullptr;
      pinned_doubles = 0;
      const size_t want = std::max<size_t>(doubles, 256);
      // (fine-grained -- hipHostMallocCoherent --: kernels write their records and the completion token here WHILE they run,
      // and the host reads them behind a system-scope release; coarse-grained host memory is only coherent at kernel boundaries)
      if (hipHostMalloc(reinterpret_cast<void**>(&pinned), want * 8, hipHostMallocCoherent) != hipSuccess) return nullptr;
      std::memset(pinned, 0, want * 8);  // (no stale completion token)
      pinned_doubles = want;
    }
    return pinned;
  }
  // Completion tokens (round 5): where the last kernel of a call is a single workgroup it writes a sequence number behind
  // its records in pinned host memory and the host spins on THAT word -- no event to record, no driver call per poll.  A
  // token that does not arrive within kSpinMs falls back to a blocking wait (where a failed launch surfaces as before).
  // (process-wide: a pinned buffer handed on by a destroyed context -- ContextPool -- never holds a number a later call waits for)
  static std::atomic<uint64_t>& seq_counter() {
    static std::atomic<uint64_t> c{0};
    return c;
  }
  double next_token() { return (double)(seq_counter().fetch_add(1) + 1); }  // (exact in a double for 2^53 calls)
  hipError_t wait_token(const double* word, double token, hipStream_t s) {
    const volatile double* w = word;
    auto arrived = [&] { return *w == token ? (std::atomic_thread_fence(std::memory_order_acquire), hipSuccess) : hipErrorNotReady; };
    return spin_then_block<1023>(arrived, [&] { return hipStreamSynchronize(s); });
  }

  // staging buffer for host -> device copies that must not force a stream synchronisation.  It is
  // reused by the next call, so wait for the copies of the previous one first (they are long done in
  // practice: every entry point ends with a wait on the stream).
  double* pinned_stage(size_t doubles) {
    if (stream) (void)hipStreamSynchronize(stream);
    if (doubles > stage_doubles) {
      if (stage) (void)hipHostFree(stage);
      stage = nullptr;
      stage_doubles = 0;
      const size_t want = std::max<size_t>(doubles, 4096);
      if (hipHostMalloc(reinterpret_cast<void**>(&stage), want * 8, hipHostMallocDefault) != hipSuccess) return nullptr;
      stage_doubles = want;
    }
    return stage;
  }

  int fail(int code, const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
};

// Host-side resources of a context -- its stream, its events, its pinned buffers -- cost ~2 ms to create and ~1 ms to
// destroy (tools/context_cost.py), a sixth of a whole 50-evaluation GPSO run whose surrogate lives for 32 ms.  gpso_destroy
// hands them to a small per-device pool and gpso_create takes them from there (at most kKeep sets per device are kept; they
// are released at process exit by the runtime).  Device memory is not pooled.
struct ContextPool {
  struct Set {
    hipStream_t stream = nullptr;
    hipEvent_t ev_wait = nullptr, ev[8] = {};
    double *pinned = nullptr, *stage = nullptr;
    size_t pinned_doubles = 0, stage_doubles = 0;
  };
  static constexpr int kKeep = 4, kDevices = 64;
  std::mutex mu;
  std::vector<Set> free_sets[kDevices];
  static ContextPool& get() {
    static ContextPool* p = new ContextPool();  // (never destroyed: no HIP calls from a static destructor)
    return *p;
  }
  bool take(int device, Set& out) {
    if (device < 0 || device >= kDevices) return false;
    std::lock_guard<std::mutex> lock(mu);
    if (free_sets[device].empty()) return false;
    out = free_sets[device].back();
    free_sets[device].pop_back();
    return true;
  }
  bool give(int device, const Set& s) {
    if (device < 0 || device >= kDevices) return false;
    std::lock_guard<std::mutex> lock(mu);
    if ((int)free_sets[device].size() >= kKeep) return false;
    free_sets[device].push_back(s);
    return true;
  }
};

#define HIPCHECK(call)                                                                     \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return ctx->fail(e_ == hipErrorOutOfMemory ? GPSO_E_OOM : GPSO_E_HIP, "%s failed: %s", \
                       #call, hipGetErrorString(e_));                                      \
  } while (0)

#define RCCLCHECK(call)                                                                              \
  do {                                                                                               \
    ncclResult_t r_ = (call);                                                                        \
    if (r_ != ncclSuccess)                                                                           \
      return ctx->fail(GPSO_E_RCCL, "%s failed: %s", #call, RcclApi::get().GetErrorString(r_));      \
  } while (0)
