// C-ABI of libgpso_hip.so (see include/gpso_hip.h): context, device memory, call sequencing.
// No torch, no BLAS/solver libraries: every kernel launched here is hand-written (predict.hip,
// fit.hip, grow.hip).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <utility>
#include <limits>
#include <vector>

#include "../../include/gpso_hip.h"
#include "batch.hpp"
#include "best_call.hpp"
#include "common.hpp"
#include "devbuf.hpp"
#include "fit_call.hpp"
#include "kernels.hpp"
#include "screen.hpp"
#include "rccl_api.hpp"
#include "resident.hpp"
#include "theta.hpp"

using namespace gpso;

namespace gpso {

namespace {
thread_local std::string g_launch_error;
std::mutex g_lds_mutex;
std::set<std::pair<const void*, int>> g_lds_done;  // (kernel, device) pairs already opted in
}  // namespace

void note_launch_error(const char* msg) {
  if (g_launch_error.empty()) g_launch_error = msg;
}

int ensure_dyn_lds(const void* fn, int bytes) {
  if (bytes <= 64 * 1024) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    note_launch_error("hipGetDevice failed");
    return GPSO_E_HIP;
  }
  std::lock_guard<std::mutex> lock(g_lds_mutex);
  if (g_lds_done.count({fn, dev})) return 0;
  // the attribute belongs to the DEVICE's function object: every device a context lives on opts in
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) {
    note_launch_error((std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e)).c_str());
    return GPSO_E_HIP;
  }
  g_lds_done.insert({fn, dev});
  return 0;
}

}  // namespace gpso

namespace {

thread_local std::string g_create_error;

constexpr int kMaxD = 48;                      // padded input dimension limit (LDS budgets)
constexpr int64_t kLeafChunk = (int64_t)1 << 20;  // leaves processed per pass of the tile kernel
// GPSO_OPT_PARK_BYTES as a context is created: 256 MB, the best median of the sweeps 0 | 64 | 128 | 256 MB at C3
// (profiles/park_reload_ab_sweep_c3.txt, park_reload_ab_pairs.txt; -DGPSO_PARK_BYTES_DEFAULT=... builds the other arms)
// GPSO_OPT_SCREEN as a context is created (-DGPSO_SCREEN_DEFAULT=0 builds the unscreened arm of an A/B through bench.py)
#ifndef GPSO_SCREEN_DEFAULT
#define GPSO_SCREEN_DEFAULT 1
#endif
#ifndef GPSO_PARK_BYTES_DEFAULT
#define GPSO_PARK_BYTES_DEFAULT (256 << 20)
#endif
constexpr int64_t kParkBytesDefault = GPSO_PARK_BYTES_DEFAULT;
constexpr int kHyperHeader = 8;                // doubles in front of the lengthscales
static_assert(kThetaMaxLs == kGradMaxLs, "a Theta holds as many lengthscales as the gradient kernels take");
using FitScratch = gpso::FitScratch<kGradMaxLs, kHyperHeader, kMaxD>;  // (fit_call.hpp: the pinned scratch of a fit call)
using FitCall = gpso::FitCall<FitScratch>;

struct Engine {
  virtual ~Engine() {}
  virtual int set_data(const double* X, const double* y, int64_t n, int d) = 0;
  // theta crosses this interface as one Theta (theta.hpp): lik is the noise variance, the likelihood's variance or its scale.
  // (gpso_fit_eval / gpso_fit_eval_loo: th is NULL when the caller passed no lengthscales -- refused where it always was)
  virtual int fit_eval(const Theta* th, double* nlml, double* grad) = 0;
  virtual int set_posterior(const double* X, const double* L, const double* alpha, int64_t n, int d, const Theta& th) = 0;
  // leave-one-out predictive of the resident fitted posterior / one evaluation of the LOO-CV objective (loo.hip)
  virtual int loo(double* mean, double* var, double* lpd, double* loss) = 0;
  virtual int fit_eval_loo(const Theta* th, double* loss, double* grad, double* nlml) = 0;
  virtual int fit_batch_max() = 0;
  virtual int fit_eval_batch(int kernel, const double* th, int nv, int n_ls, double* loss, double* grad, int* info) = 0;
  virtual int fit_eval_batch_check(int kernel, int b, int n_ls) = 0;
  virtual int set_noise_diag(const double* s, int64_t n) = 0;
  virtual bool has_noise_diag() const = 0;
  virtual int append(const double* Xnew, const double* ynew, const double* snew, int64_t k, double* nlml) = 0;
  virtual int predict(const void* xs, int xs_dtype, int xs_mem, int64_t m, double* mean,
                      double* var, int out_mem) = 0;
  // mean, var and their gradients in the test points, from the dense factor (predict_grad.hip)
  virtual int predict_grad(const void* xs, int xs_dtype, int xs_mem, int64_t m, double* mean, double* var, double* dmean,
                           double* dvar, int out_mem) = 0;
  // the joint predictive at m test points: mean and full covariance, or draws and their arg-max (joint.hip)
  virtual int predict_joint(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, double* mean, double* cov,
                            int out_mem) = 0;
  virtual int sample_joint(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, const double* z, int64_t s,
                           double* samples, int64_t* best_idx, double* best_val) = 0;
  // pathwise posterior draws: functions kept on the context, evaluated at any number of points (paths.hip)
  virtual int paths_draw(const double* omega, const double* phase, int64_t f, const double* w, const double* eps, int64_t s) = 0;
  virtual int paths_draw_q(const double* omega, const double* phase, int64_t f, const double* w, const double* eps, int64_t s) = 0;
  virtual int paths_eval(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, double* values,
                         int out_mem, int64_t* best_idx, double* best_val) = 0;
  virtual void paths_info(int64_t* s, int64_t* f) const = 0;
  // the latent cross-covariance of two point sets, and q leaves of one set picked greedily under hallucinated updates (batch.hip)
  virtual int cross_cov(const void* xa, int xs_dtype, int xs_mem, int64_t m, const double* xb, int b, double* cov, int out_mem) = 0;
  virtual int best_batch(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, double obs_noise, int q, int64_t* idx,
                         double* mean, double* var, double* value, int* n_picked, double* var_after, int out_mem) = 0;
  // mean, var and the acquisition column of every leaf (each output nullable)
  virtual int acq_values(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, double* mean, double* var,
                         double* value, int out_mem) = 0;
  // GPSO_ACQ_MES: the sampled maxima a context keeps for the epilogues (the caller's numbers: nothing here drops them)
  virtual int set_maxima(const double* ystar, int k) = 0;
  double maxima_host[GPSO_ACQ_MAX_MAXIMA] = {};
  int maxima_k = 0;
  const double* maxima_dev = nullptr;
  // sum_j log Phi((y_i - mean_j) / s_j) at g thresholds (maxcdf.hip)
  virtual int max_logcdf(const double* mean, const double* var, int mem, int64_t m, double var_sub, const double* y, int g,
                         double* logcdf, int64_t* n_used) = 0;
  virtual int best_ucb(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off,
                       int nseg, const AcqSpec& acq, int64_t* idx, double* mean, double* var,
                       double* ucb) = 0;
  virtual int best_ucb_begin(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
                             const AcqSpec& acq, const double* bounds, int depth) = 0;
  virtual int best_ucb_end(int ticket, int64_t* idx, double* mean, double* var, double* ucb) = 0;
  virtual int screen_probe(const void* xs, int xs_dtype, int xs_mem, int64_t m, double varsigma, double* my, double* ub,
                           double* flag, double* info) = 0;
  virtual int screen_list(int64_t max_rows, int64_t* key, float* rows, int64_t* live) = 0;
  virtual int grow(const double* bounds, int nseg, int d, int depth, double* out) = 0;
  virtual int best_ucb_grow(const double* bounds, int nseg, int depth, const AcqSpec& acq,
                            int64_t* idx, double* mean, double* var, double* ucb) = 0;
  virtual int get_matrix(int which, double* out) = 0;
  virtual int get_vector(int which, double* out) = 0;
  virtual int posterior_buffers(void** ptrs, int64_t* nbytes, int cap) = 0;
  virtual int posterior_span(void** ptr, int64_t* offset, int64_t* nbytes) = 0;
  virtual int posterior_span_at(int64_t offset, int64_t nbytes, void** ptr) = 0;
  virtual int posterior_hash(uint64_t* out) = 0;
  virtual int alloc_posterior(int64_t n, int d) = 0;
  virtual int adopt_posterior() = 0;
  virtual int64_t padded_n() const = 0;
  virtual void problem_shape(int64_t* n_out, int* d_out) const = 0;
  virtual int set_option(int option, int value) = 0;
  virtual int set_option_f64(int option, double value) = 0;
  virtual int precision_info(double* out) = 0;
  virtual int broadcast_posterior(int root) = 0;
  virtual int broadcast_posterior_rows(int root) = 0;
  virtual int posterior_dirty_ranges(int64_t* offsets, int64_t* nbytes, int cap) = 0;
  virtual int posterior_mark_synced() = 0;
  virtual int best_ucb_sharded(const void* xs, int xs_dtype, int xs_mem, int64_t m_local, int64_t m_global,
                               const int64_t* seg_off, int nseg, double varsigma, int64_t* idx, double* mean,
                               double* var, double* ucb) = 0;
  virtual int best_ucb_grow_sharded(const double* bounds, int nseg, int depth, double varsigma, int64_t* idx,
                                    double* mean, double* var, double* ucb) = 0;
  // the two halves of the sharded calls for an arbitrary (rank, world), without a communicator
  virtual int shard_winners(int rank, int world, const void* xs, int xs_dtype, int xs_mem, int64_t m_local,
                            int64_t m_global, const int64_t* seg_off, int nseg, double varsigma, double* payload) = 0;
  virtual int shard_winners_grow(int rank, int world, const double* bounds, int nseg, int depth, double varsigma,
                                 double* payload) = 0;
  virtual int fold_winners(const double* gathered, int world, int64_t m_global, const int64_t* seg_off, int nseg,
                           int64_t* idx, double* mean, double* var, double* ucb) = 0;
  // variational GP (vgp.hip)
  virtual int vgp_set_q(const double* mu, const double* S, int64_t n) = 0;
  virtual int vgp_get_q(double* mu, double* S) = 0;
  virtual int vgp_extend_q() = 0;
  virtual int vgp_natgrad(const Theta& th, double gamma) = 0;
  virtual int vgp_elbo(const Theta& th, double* loss, double* grad) = 0;
  virtual int vgp_posterior(const Theta& th) = 0;
  virtual int vgp_set_likelihood(int kind, double df, int n_gh, const double* gh_x, const double* gh_w) = 0;
  // sparse GP regression on inducing points (sgpr.hip)
  virtual int sgpr_set_inducing(const double* Z, int64_t m) = 0;
  virtual int sgpr_select_inducing(const Theta& th, int64_t m, int64_t* idx_out) = 0;
  virtual int sgpr_get_inducing(double* Z, int64_t* m_out, int64_t* n_data_out) = 0;
  virtual int sgpr_get_factor(int which, double* out) = 0;
  virtual int sgpr_bound(const Theta& th, double* loss, double* grad) = 0;
  virtual int sgpr_posterior(const Theta& th, double* delta_out) = 0;
  // ... and at a moving Z (inducing.hip): Z (nullable) replaces the resident inducing rows in place
  virtual int sgpr_move_inducing(const double* Z) = 0;
  virtual int sgpr_bound_z(const Theta& th, const double* Z, double* loss, double* grad, double* grad_z) = 0;
  virtual int svgp_elbo_z(const Theta& th, const double* Z, double* loss, double* grad, double* grad_z) = 0;
  // sparse variational GP on inducing points (svgp.hip)
  // s2 > 0: the conjugate start at that noise variance (th.lik is not read); else the prior (th is not read)
  virtual int svgp_init_q(const Theta& th, double s2) = 0;
  virtual int svgp_set_q(const double* mu, const double* S, int64_t m) = 0;
  virtual int svgp_get_q(double* mu, double* S) = 0;
  virtual int svgp_natgrad(const Theta& th, double gamma) = 0;
  virtual int svgp_elbo(const Theta& th, double* loss, double* grad) = 0;
  virtual int svgp_posterior(const Theta& th, double* delta_out) = 0;
  int vlik_kind = GPSO_LIK_GAUSSIAN;  // the VGP's likelihood (GPSO_LIK_*): what slot n_ls + 1 of u means
};

// contiguous share [lo, hi) of m items for `rank` of `world`: global order is preserved across ranks
inline void shard_range(int64_t m, int rank, int world, int64_t* lo, int64_t* hi) {
  const int64_t base = m / world, extra = m % world;
  *lo = rank * base + std::min<int64_t>(rank, extra);
  *hi = *lo + base + (rank < extra ? 1 : 0);
}

}  // namespace

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
  int64_t last_count[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // ([4] is not stored: gpso_last_count)
  int cu_count = 256;  // compute units of `device` (gpso_create): sizes the split predict kernels' and the bf16 GEMMs' grids
  std::string err;
  Engine* eng = nullptr;
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

namespace {

// TF: fit type (Gram, Cholesky, L^-1, alpha);  TP: predict / apply type.
//   GPSO_F64   -> EngineT<double, double>
//   GPSO_F32   -> EngineT<float, float>
//   GPSO_MIXED -> EngineT<double, float>
template <typename TF, typename TP>
struct EngineT : Engine {
  gpso_ctx* ctx;
  explicit EngineT(gpso_ctx* c) : ctx(c) {
    check = sizeof(TP) == 4;  // float predict arithmetic: self-test on by default
    // default tolerances: a double factor with a float apply measures 1e-6 .. 3e-5 (bf16x3) -> 1e-4; an
    // all-float engine is a 1e-4-class instrument already at noise 1e-3 -> 1e-3
    tol_var = tol_mean = (sizeof(TF) == 4) ? 1.0e-3 : 1.0e-4;
  }
  static constexpr bool kFloatPredict = sizeof(TP) == 4;

  // problem
  int64_t n = 0, npad = 0;
  int d = 0, dp = 0;
  // which of the buffers below mean something (resident.hpp: the record and its transitions, its only writers)
  gpso::Resident res{kFloatPredict ? GPSO_MATH_F16X3 : GPSO_MATH_NATIVE};
  using Post = gpso::Post;
  using Copy = gpso::Copy;
  KernParams kp{0, 1.0, 1e-3, 0.0};
  int n_ls = 1;
  std::vector<double> ls_host;

  // device buffers.  Fit side: xs64 / xnorm64 (scaled inputs, always double), K, Lf, linv, work, kinvb,
  // white, alpha_f in TF.  Predict side: linv_p, alpha in TP; xs_p64 (+ xnorm64) or xs_p32 / xnorm32
  // in the generation type.
  DevBuf xs_h16, c16_scal;  // fp16 piece pairs of xs32 in the fp16 contraction's fragment order, and their scale (4 floats)
  DevBuf x64, y64, hyper, xs64, xnorm64, xs_p64, xs32, xnorm32, xs_p32, K, Lf, linv, work, kinvb, linv_p,
      white, alpha_f, alpha, logdet, scal, gpart, apart, kinv_diag, getter_tmp;
  // split-bf16 copy of L^-1 (float predict with GPSO_OPT_PREDICT_MATH != native)
  DevBuf linv_b;
  DevBuf pl_L, pl_X, pl_XT, pl_WT;  // bf16 plane sets of the two-level float fit (kernels.hpp: FitPlanes)
  DevBuf app;                       // scratch of gpso_append (kernels.hpp: append_scratch_doubles)
  std::vector<double> x_host, y_host;  // host mirror of the training data (gpso_append's refit path needs all of it)
  // per-point observation noise (gpso_set_noise_diag): K_y = k(X, X) + diag(noise + s_i), s fixed.  sdiag [npad] on the
  // device (zero padding), read wherever a fit adds `noise` to a diagonal; s_dev() is NULL while none is set, and every
  // such site then runs what it ran before the vector existed
  DevBuf sdiag;
  std::vector<double> s_host;  // [n] host mirror (the refit paths of gpso_append, GPSO_VEC_NOISE_DIAG)
  double s_max = 0.0;          // max s_i: fit_plane_scales' bounds
  const double* s_dev() const { return res.have_s ? static_cast<const double*>(sdiag.p) : nullptr; }
  bool has_noise_diag() const override { return res.have_s; }
  int fit_overlap = 2;              // GPSO_OPT_FIT_OVERLAP (bit 0 look-ahead, bit 1 overlapped inverse: the default): two-level double fits overlap chains, updates and the inverse (0: sequential, round 5)
  int fit_planes_mode = 2;          // GPSO_OPT_FIT_BF16_SYRK: 0 f32 MFMA | 1 bf16 pieces (6 MFMAs per product) | 2 fp16 pieces (3) where representable
  // predict math, the OPTION (what the posterior uses: res.math).  GPSO_MATH_AUTO walks the ladder fp16 split (3 MFMAs per
  // product) -> bf16x6 -> f32 MFMA kernel, one rung down each time the posterior's self-test fails on it (selftest_with_fallback)
  static constexpr int kAutoFirst = kFloatPredict ? GPSO_MATH_F16X3 : GPSO_MATH_NATIVE;
  bool math_auto = kFloatPredict;
  // generation of the cross-Gram tile in float-predict contexts, the OPTION (what the posterior uses: res.gen_eff32).  AUTO:
  // a posterior whose float form misses the tolerances moves to double generation and is tested again (decide_generation)
  int gen_mode = GPSO_GEN_AUTO;
  int split_variant = GPSO_SPLIT_KERNEL_AUTO;  // GPSO_OPT_SPLIT_KERNEL
  int row_loop = 1;  // GPSO_OPT_ROW_LOOP (leaf_split.hpp: leaf_row_splits)
  // GPSO_OPT_PARK_BYTES (leaf_split.hpp, PARK): the budget of the parked cross-Gram pieces of the default split predict kernel,
  // and the buffer that holds them -- allocated by the first launch that parks, reused by every later call and chunk
  int64_t park_bytes = kParkBytesDefault;
  DevBuf park_buf;
  size_t park_refused = 0;  // the smallest size an allocation of park_buf failed at: not asked for again (a new budget clears it)
  static void* park_cb(void* owner, size_t bytes) {
    auto* self = static_cast<EngineT*>(owner);
    if (self->park_buf.bytes >= bytes) return self->park_buf.p;
    if (self->park_refused != 0 && bytes >= self->park_refused) return nullptr;
    if (self->park_buf.ensure(bytes, self->st(), false)) {  // (no room: this launch and the later ones of its size park nothing)
      (void)hipGetLastError();
      self->park_refused = bytes;
      return nullptr;
    }
    return self->park_buf.p;
  }
  int contraction = GPSO_CONTRACTION_AUTO;     // GPSO_OPT_CONTRACTION
  // the x.x* contraction of the fp16-split kernel runs on the fp16 pipe under float generation (D_pad + 1 slots in at most
  // two chunks of 32: every D this library accepts).  Measured in one process on one posterior (tools/c16_check.py,
  // profiles/r04_c16_check.jsonl), fp16 pipe against the f32 instruction: D = 6 +4 %, 12 +8 %, 20 +17 %, 33 +28 %, 40 +30 %
  bool c16_in_use(bool gen64) const {
    if (!kFloatPredict || gen64 || res.c16_fallback || !f16_split() || contraction == GPSO_CONTRACTION_F32 || leaf_c16_chunks(dp / 4) > 2) return false;
    return leaf_bf16_lds_bytes(2, dp / 4, 4, true) <= 160 * 1024;
  }
  bool small_calls = true, one_launch = true, one_launch_everywhere = false;  // GPSO_OPT_SMALL_CALLS
  bool fuse_prep = true;  // GPSO_OPT_FUSED_PREP: float leaves are scaled in the fp16-contraction kernel's prologue (same bits)
  int64_t single_level_max = -1;  // < 0: library default
  bool fused_small = true;        // GPSO_OPT_FIT_FUSED_SMALL
  std::vector<int64_t> segoff_cache;  // what the device copy of seg_off currently holds
  // A best-UCB call in flight (best_call.hpp): the entry point's plan goes down, the enqueue's record comes back.
  using BestPlan = gpso::BestPlan; using BestCall = gpso::BestCall; using BestKind = gpso::BestKind;
  // the pinned memory the call's last kernel -- about to be launched -- writes nseg records to, and the token behind them
  double* result_host(const BestPlan& plan, BestCall& call, int nseg) { return call.writes_host(plan.slot ? plan.slot : ctx->pinned_scratch((size_t)nseg * 4 + 3)); }
  double arm_token(BestCall& call, bool single_workgroup, int nseg) { return call.arm_token(single_workgroup, nseg, ctx->next_token()); }
  DevBuf extra_cnt;                  // small growth calls: rows appended behind the analytic slots (zero between calls)
  // predict workspace
  DevBuf leaves_raw, leaves_s, lnorm, pvar, pmean, omean, ovar, oucb, segoff, best, oidx, ovals, grow_key,
      live_cnt, best_pos, gath, wbase, ovals2, bhdr;
  DevBuf acq_maxima, mcdf_work, mcdf_in;  // GPSO_ACQ_MES's maxima; gpso_max_logcdf's partials and staged columns
  // screened best-UCB calls (screen.hip): every leaf's mean, the blocks' maxima, the compaction's counts per part, the
  // survivors' raw rows, the control words (live rows, count, T'), the probe's columns.  The survivors' indices travel in grow_key.
  DevBuf screen_my, screen_bmax, screen_cnt, screen_rows, screen_ctl, screen_cols;
  // the compact list the last gpso_screen_probe left, copied out behind it (gpso_screen_list): indices, raw rows [live][d]
  std::vector<int64_t> probe_key;
  std::vector<float> probe_rows;
  bool probe_listed = false;
  int screen_mode = GPSO_SCREEN_DEFAULT;  // GPSO_OPT_SCREEN
  DevBuf batch_theta;  // theta records of a batched evaluation (fit_eval_batch)
  DevBuf loov, loo_scal;  // leave-one-out: the per-point vectors (kernels.hpp: kLoo*) and [0] loss, [8 ..] gradient
  DevBuf pg_ts, pg_norm, pg_work, pg_out;  // gpso_predict_grad: scaled test points of a chunk, the workspace, host-bound results
  // gpso_predict_joint / gpso_sample_joint: scaled test points, V (+ partial |v|^2), partial tiles, mean, Sigma; then the
  // Cholesky's buffers (factor, inverse, scratch, diagonal, info), the normals, the draws and their winners
  DevBuf pj_ts, pj_norm, pj_v, pj_part, pj_mu, pj_sigma, pj_l, pj_linv, pj_cwork, pj_diag, pj_info, pj_z, pj_f, pj_best;
  // gpso_paths_draw / gpso_paths_eval (paths.hip): the resident path set -- frequencies, phases, weights and v^T, padded as
  // the kernels read them; res.paths_valid says whether it means something -- and the set a draw in progress builds, swapped
  // in when it succeeds (a failed draw leaves the resident one as it was).  Then the draw's scratch (eps, Phi(X) w^T, R, U)
  // and the evaluation's: scaled points and values of one chunk, segment offsets, running winners
  struct PathSet {
    DevBuf omega, phase, w, vt;
    int64_t s = 0, f = 0, ldw = 0;
  };
  PathSet pth, pth_next;
  DevBuf pth_eps, pth_p, pth_r, pth_u, pth_x /* gpso_paths_draw_q: Lu^-1 Phi(Zr) w^T */, pe_ts, pe_norm, pe_vals, pe_seg, pe_best;
  // gpso_cross_cov / gpso_best_batch (batch.hip): scaled points of a chunk and their norms, the points b (raw, scaled, norms),
  // K_b | U | W and the latent variances, host-bound results; then the batch call's own: every scaled leaf and its norm, mean,
  // s2, the value column, G, the live flags, the blocks' maxima, the state words and the pick's scaled row
  DevBuf cc_ts, cc_norm, cc_braw, cc_tb, cc_bnorm, cc_vec, cc_lv, cc_out;
  DevBuf bb_ts, bb_norm, bb_mean, bb_s2, bb_val, bb_g, bb_live, bb_bmax, bb_state, bb_tp;
  // precision self-test
  bool check = false;
  bool can_selftest() const { return check && res.st_have && res.have_data; }  // (posteriors from outside carry no targets)
  double tol_var = 1.0e-4, tol_mean = 1.0e-4;
  double st_vals[6] = {0, 0, 0, 0, 0, 0};
  DevBuf st_mean, st_var, st_out;

  int64_t padded_n() const override { return npad; }
  void problem_shape(int64_t* n_out, int* d_out) const override {
    *n_out = n;
    *d_out = d;
  }

  // generation type actually used by the resident posterior
  bool gen_double() const { return !kFloatPredict || !res.gen_eff32; }
  // the split-bf16 kernel keeps its leaf fragments in LDS: with double generation they do not fit the
  // 160 KB for D > 24 (bf16x6) / D > 36 (bf16x3) -- those calls run the native f32 kernel instead (accuracy
  // decides the generation type, the kernel follows)
  bool bf16_fits(bool gen64) const {
    return c16_in_use(gen64) || leaf_bf16_lds_bytes(nsplit(), dp / 4, gen64 ? 8 : 4) <= 160 * 1024;
  }
  int nsplit() const { return res.math == GPSO_MATH_BF16X6 ? 3 : 2; }
  bool f16_split() const { return res.math == GPSO_MATH_F16X3; }
  // bytes of the split copy of L^-1: the planes and, behind them, one 256-byte slot for the power-of-two scale of the
  // fp16 split (2 floats, written on the device at packing time) -- it travels with the planes in a hand-off.  Under
  // GPSO_MATH_AUTO room for three planes whatever the stage, so that both sides of a hand-off list the same sizes.
  // Round 4: the 256-byte scale slot sits IN FRONT of the planes, so that the part of the buffer a posterior uses
  // (slot + nsplit planes) is a prefix of it -- the posterior arena sends exactly that (posterior_span).
  size_t split_planes_alloc() const { return (size_t)(math_auto ? 3 : nsplit()) * npad * npad * 2; }
  size_t split_bytes() const { return split_planes_alloc() + 256; }
  size_t split_bytes_in_use() const { return (size_t)nsplit() * npad * npad * 2 + 256; }
  float* f16_scale() const { return reinterpret_cast<float*>(linv_b.p); }
  void* split_planes() const { return static_cast<char*>(linv_b.p) + 256; }
  // max |L^-1| of the fp16 split comes out of the fit's own pass over L^-1 (white_kernel leaves row maxima,
  // alpha_sum_kernel folds them into the scale slot): no extra pass, no memset.  f16_handed_at: where this fit's solve
  // was told to leave it (cleared by every packing and at the start of every fit).
  DevBuf amax_rows;
  const void* f16_handed_at = nullptr;
  // -> where the fit's pass leaves the maximum, nullptr when the fp16 split does not apply to this posterior
  float* f16_max_for_fit() {
    f16_handed_at = nullptr;
    if constexpr (!kFloatPredict) return nullptr;
    if (!f16_split() || !bf16_usable()) return nullptr;
    if (ensure(linv_b, split_bytes()) != GPSO_OK || ensure(amax_rows, (size_t)npad * 4) != GPSO_OK) return nullptr;
    f16_handed_at = f16_scale();
    return f16_scale();
  }
  bool bf16_usable() const { return res.split_usable(kFloatPredict, npad); }

  // An evaluation WITH gradient is a step of the hyper-parameter search: the next call is another evaluation, not a
  // prediction, and its 16-bit pieces of L^-1 (10 us at C3, 0.5 ms at C5) would be packed for nothing.  They are packed
  // when something first asks for them: every predict-type call, the self-test and the hand-off paths come through
  // decide_generation(), which calls this.
  int ensure_split_pieces() {
    if (res.linv_b != Copy::Deferred) return GPSO_OK;
    if (res.chol_valid) return pack_bf16();
    res.split_packed(false);
    return GPSO_OK;
  }
  // (re)build the bf16 pieces of L^-1 from the fit-type L^-1 resident in `linv`
  int pack_bf16() {
    res.split_packed(false);
    if (!bf16_usable()) return GPSO_OK;
    int rc = ensure(linv_b, split_bytes());
    if (rc) return rc;
    if (f16_split()) {
      const bool have_max = f16_handed_at != nullptr && f16_handed_at == f16_scale();
      launch_pack_linv_f16<TF>(st(), as<TF>(linv), n, npad, f16_scale(), split_planes(), have_max);
      f16_handed_at = nullptr;
    } else {
      launch_pack_linv_bf16<TF>(st(), nsplit(), as<TF>(linv), n, npad, split_planes());
    }
    HIPCHECK(hipGetLastError());
    res.split_packed(true);
    return GPSO_OK;
  }

  int set_option(int option, int value) override {
    switch (option) {
      case GPSO_OPT_FIT_SINGLE_LEVEL_MAX:
        if (value < 0) return ctx->fail(GPSO_E_ARG, "single-level limit %d must be >= 0", value);
        single_level_max = value;
        return GPSO_OK;
      case GPSO_OPT_FIT_BF16_SYRK:
        if (value < 0 || value > 2) return ctx->fail(GPSO_E_ARG, "fit plane mode must be 0 (f32 MFMA), 1 (bf16 pieces) or 2 (fp16 pieces)");
        fit_planes_mode = value;
        return GPSO_OK;
      case GPSO_OPT_ROW_LOOP:
        if (value < -1) return ctx->fail(GPSO_E_ARG, "row loop: 0, 1, a split count >= 2 or -1 (one workgroup per leaf tile)");
        row_loop = value;
        return GPSO_OK;
      case GPSO_OPT_PARK_BYTES:
        if (value < 0) return ctx->fail(GPSO_E_ARG, "park bytes: 0 (off) or a budget in bytes");
        park_bytes = value;
        park_refused = 0;
        return GPSO_OK;
      case GPSO_OPT_SCREEN:
        if (value < 0 || value > 2) return ctx->fail(GPSO_E_ARG, "screen: 0 (off), 1 (large calls) or 2 (every call it applies to)");
        screen_mode = value;
        return GPSO_OK;
      case GPSO_OPT_FIT_OVERLAP:
        if (value < 0) return ctx->fail(GPSO_E_ARG, "fit overlap must be >= 0");
        fit_overlap = value;
        return GPSO_OK;
      case GPSO_OPT_TIMING:
        if (value < 0 || value > 1000000) return ctx->fail(GPSO_E_ARG, "timing must be 0 (off), 1 (every call) or k (every k-th call)");
        ctx->timing_every = value;
        ctx->timed_calls = 0;  // (the next fit / predict-type call is a sampled one)
        ctx->timing = value != 0;
        if (!ctx->timing) ctx->last_ms[0] = ctx->last_ms[1] = ctx->last_ms[2] = ctx->last_ms[3] = 0.0;
        return GPSO_OK;
      case GPSO_OPT_FIT_FUSED_SMALL:
        if (value != 0 && value != 1) return ctx->fail(GPSO_E_ARG, "fused small fit must be 0 or 1");
        fused_small = value != 0;
        return GPSO_OK;
      case GPSO_OPT_SMALL_CALLS:
        if (value < 0 || value > 3) return ctx->fail(GPSO_E_ARG, "small calls must be 0 .. 3");
        small_calls = value != 0;
        one_launch = value == 1 || value == 3;
        one_launch_everywhere = value == 3;
        return GPSO_OK;
      case GPSO_OPT_FUSED_PREP:
        if (value != 0 && value != 1) return ctx->fail(GPSO_E_ARG, "fused prep must be 0 or 1");
        fuse_prep = value != 0;
        return GPSO_OK;
      case GPSO_OPT_CONTRACTION:
        if (value != GPSO_CONTRACTION_AUTO && value != GPSO_CONTRACTION_F32 && value != GPSO_CONTRACTION_F16) return ctx->fail(GPSO_E_ARG, "unknown contraction %d", value);
        if (value != contraction) {
          contraction = value;
          res.contraction_changed();
        }
        return GPSO_OK;
      case GPSO_OPT_SPLIT_KERNEL:
        if (value < GPSO_SPLIT_KERNEL_AUTO || value > GPSO_SPLIT_KERNEL_FUSED32) return ctx->fail(GPSO_E_ARG, "unknown split kernel %d", value);
        if (value == GPSO_SPLIT_KERNEL_FUSED32 && !gpso::leaf_step32_built())
          return ctx->fail(GPSO_E_ARG, "the 32x32x16 step is not in this build (measured slower: leaf_split.hpp, GPSO_STEP32)");
        split_variant = value;
        return GPSO_OK;
      case GPSO_OPT_PRECISION_CHECK:
        if (value != 0 && value != 1) return ctx->fail(GPSO_E_ARG, "precision check must be 0 or 1");
        check = value != 0;
        return GPSO_OK;
      case GPSO_OPT_GENERATION:
        if (value != GPSO_GEN_F64 && value != GPSO_GEN_F32 && value != GPSO_GEN_AUTO)
          return ctx->fail(GPSO_E_ARG, "unknown generation mode %d", value);
        if (!kFloatPredict) {
          if (value == GPSO_GEN_F32) return ctx->fail(GPSO_E_ARG, "GPSO_GEN_F32 needs a float-predict context");
          return GPSO_OK;
        }
        if (value != gen_mode) {
          if (res.has_post() && !res.have_data && value != GPSO_GEN_F64)
            return ctx->fail(GPSO_E_STATE, "set GPSO_OPT_GENERATION before installing a posterior");
          gen_mode = value;
          reset_generation();
        }
        return GPSO_OK;
      case GPSO_OPT_PREDICT_MATH:
        break;
      default:
        return ctx->fail(GPSO_E_ARG, "unknown option %d", option);
    }
    if (value != GPSO_MATH_NATIVE && value != GPSO_MATH_BF16X3 && value != GPSO_MATH_BF16X6 && value != GPSO_MATH_F16X3 &&
        value != GPSO_MATH_AUTO)
      return ctx->fail(GPSO_E_ARG, "unknown predict math %d", value);
    if (value != GPSO_MATH_NATIVE && value != GPSO_MATH_AUTO && !kFloatPredict)
      return ctx->fail(GPSO_E_ARG, "split (bf16 / fp16) predict math needs a GPSO_F32 or GPSO_MIXED context");
    const bool want_auto = value == GPSO_MATH_AUTO;
    if (want_auto) value = kAutoFirst;
    if (value == res.math && want_auto == math_auto && !res.math_native_fallback) return GPSO_OK;
    math_auto = want_auto;
    res.math_chosen(value);
    reset_generation();
    if (res.chol_valid) {  // L^-1 is resident: make the new mode usable right away
      int rc = pack_bf16();
      if (rc) return rc;
    }
    return GPSO_OK;
  }

  int set_option_f64(int option, double value) override {
    if (!(value > 0.0)) return ctx->fail(GPSO_E_ARG, "tolerance %g must be positive", value);
    if (option == GPSO_OPTF_TOL_VAR) tol_var = value;
    else if (option == GPSO_OPTF_TOL_MEAN) tol_mean = value;
    else return ctx->fail(GPSO_E_ARG, "unknown floating-point option %d", option);
    return GPSO_OK;
  }

  hipStream_t st() const { return ctx->stream; }
  // calls that replace or change the posterior are refused while an asynchronous best-UCB call is open: its kernels
  // may still be reading what the call would overwrite
  int refuse_if_async(const char* what) {
    if (ctx->slots_busy() == 0) return GPSO_OK;
    return ctx->fail(GPSO_E_STATE, "%s while %d asynchronous best-UCB call(s) are open: gpso_best_ucb_end them first", what, ctx->slots_busy());
  }
  double* ls_dev() const { return static_cast<double*>(hyper.p) + kHyperHeader; }
  template <typename U>
  U* as(const DevBuf& b) const { return static_cast<U*>(b.p); }

  // room for at least `bytes` in b (devbuf.hpp: grow-only; the stream is synchronised before an old block is freed)
  int ensure(DevBuf& b, size_t bytes, bool keep = false) {
    const size_t had = b.bytes;
    const BufStatus r = b.ensure(bytes, st(), keep);
    if (!r) return GPSO_OK;
    if (r.step == BufStep::View)
      return ctx->fail(GPSO_E_STATE, "internal: a slice of the posterior arena (%zu bytes) was asked to hold %zu", had, bytes);
    // (indexed by BufStep, in the words these steps have always failed with)
    static const char* const call[] = {"", "", "hipMalloc(&b.p, bytes)", "hipMemcpyAsync(np_, b.p, b.bytes, hipMemcpyDeviceToDevice, st())",
                                       "hipStreamSynchronize(st())", "hipFree(b.p)"};
    const hipError_t e = (hipError_t)r.err;
    return ctx->fail(e == hipErrorOutOfMemory ? GPSO_E_OOM : GPSO_E_HIP, "%s failed: %s", call[(int)r.step], hipGetErrorString(e));
  }
  // like ensure(), but the old contents survive a re-allocation
  int ensure_keep(DevBuf& b, size_t bytes) { return ensure(b, bytes, true); }

  // launcher-side errors (hipFuncSetAttribute, unsupported GEMM shapes) + the HIP launch status
  int launch_status() {
    HIPCHECK(hipGetLastError());
    if (!gpso::g_launch_error.empty()) {
      const std::string msg = gpso::g_launch_error;
      gpso::g_launch_error.clear();
      return ctx->fail(GPSO_E_HIP, "%s", msg.c_str());
    }
    return GPSO_OK;
  }

  int shape(int64_t n_, int d_) {
    if (n_ < 1) return ctx->fail(GPSO_E_ARG, "need at least one training point (n=%lld)", (long long)n_);
    if (d_ < 1 || d_ > kMaxD) return ctx->fail(GPSO_E_ARG, "input dimension %d outside [1, %d]", d_, kMaxD);
    if (n_ > 65536) return ctx->fail(GPSO_E_ARG, "n=%lld above the supported 65536", (long long)n_);
    n = n_;
    d = d_;
    // Float-predict contexts pad N > 128 to a multiple of 256, the row block of the split predict kernels: with a pad of
    // 128 every N in (256 k + 128, 256 k + 256] ran them and every N in (256 k, 256 k + 128] fell to the f32 MFMA kernel
    // (3.2x the time per flop) -- half of all N.  The padding rows are identity rows of the factor: the blocked
    // factorisation does the same operations on the real rows, up to two 64-column steps more on the padding.
    const int64_t pad = (kFloatPredict && n > kPadN) ? 2 * kPadN : kPadN;
    npad = (n + pad - 1) / pad * pad;
    dp = (d + 3) / 4 * 4;
    int rc;
    // (room for the padded size: gpso_append adds rows in place)
    if ((rc = ensure(x64, (size_t)npad * d * 8))) return rc;
    if ((rc = ensure(y64, (size_t)npad * 8))) return rc;
    if ((rc = carve_posterior())) return rc;
    if (kFloatPredict) {
      if ((rc = ensure(xs32, (size_t)npad * dp * 4))) return rc;
      if ((rc = ensure(xnorm32, (size_t)npad * 4))) return rc;
      if ((rc = ensure(xs_p32, (size_t)npad * dp * 4))) return rc;
      if ((rc = ensure(xs_h16, (size_t)(npad / 16) * leaf_c16_chunks(dp / 4) * 2048))) return rc;
      if ((rc = ensure(c16_scal, 16))) return rc;
    }
    return GPSO_OK;
  }

  // ---- the posterior arena (round 4) ----------------------------------------------------------------------------
  // Everything a peer needs to predict lives in ONE allocation, laid out as
  //     [ packed L^-1 | hyper block | X / l | its MFMA fragments | norms | alpha | split pieces of L^-1 (scale slot, planes) ]
  // (each slice 256-byte aligned), so that what a posterior actually uses is one contiguous range whichever predict
  // math it runs -- native: [packed L^-1 .. alpha], split: [hyper .. the planes in use] -- and gpso_broadcast_posterior
  // moves it with ONE ncclBroadcast.  The layout is a function of (N_pad, D_pad, predict type) only: every rank of a
  // group carves the same offsets.  The slices are DevBuf views of the arena.
  DevBuf arena;
  int64_t arena_npad = -1;
  int arena_dp = -1;
  static size_t up256(size_t b) { return (b + 255) / 256 * 256; }
  bool split_slot_exists() const { return kFloatPredict && npad % 256 == 0; }
  int carve_posterior() {
    if (arena.p != nullptr && arena_npad == npad && arena_dp == dp) return GPSO_OK;
    const size_t b_linv = up256(packed_linv_elems(npad) * sizeof(TP));
    const size_t b_hyper = up256((size_t)(kHyperHeader + kMaxD) * 8);
    const size_t b_xs = up256((size_t)npad * dp * 8);
    const size_t b_norm = up256((size_t)npad * 8);
    const size_t b_alpha = up256((size_t)npad * sizeof(TP));
    // room for three planes whatever the option: GPSO_OPT_PREDICT_MATH may change after the shape is known
    const size_t b_split = split_slot_exists() ? up256((size_t)3 * npad * npad * 2 + 256) : 0;
    const size_t total = b_linv + b_hyper + 2 * b_xs + b_norm + b_alpha + b_split;
    if (arena.bytes < total) {  // (the old slices go first: whatever becomes of the arena, none of them points into a freed block)
      arena_npad = -1;
      for (DevBuf* b : {&linv_p, &hyper, &xs64, &xs_p64, &xnorm64, &alpha, &linv_b}) b->drop();
      int rc = ensure(arena, total);
      if (rc) return rc;
    }
    size_t off = 0;
    auto slice = [&](DevBuf& b, size_t bytes) {
      b.slice(arena, off, bytes);
      off += bytes;
    };
    slice(linv_p, b_linv);
    slice(hyper, b_hyper);
    slice(xs64, b_xs);
    slice(xs_p64, b_xs);
    slice(xnorm64, b_norm);
    slice(alpha, b_alpha);
    slice(linv_b, b_split);
    arena_npad = npad;
    arena_dp = dp;
    res.recarved();
    return GPSO_OK;
  }
  // the contiguous range of the arena the resident posterior uses: offset into the arena and length
  void posterior_range(size_t* off, size_t* bytes) const {
    const char* base = static_cast<const char*>(arena.p);
    if (math_in_use() != GPSO_MATH_NATIVE) {
      *off = (size_t)(static_cast<const char*>(hyper.p) - base);
      *bytes = (size_t)(static_cast<const char*>(linv_b.p) - static_cast<const char*>(hyper.p)) + split_bytes_in_use();
    } else {
      *off = 0;
      *bytes = (size_t)(static_cast<const char*>(alpha.p) - base) + alpha.bytes;
    }
  }

  // ---- what the peers of a group hold of THIS posterior (round 6: gpso_broadcast_posterior_rows) --------------------------------
  // A hand-off (gpso_broadcast_posterior, or a span copy followed by gpso_posterior_mark_synced / gpso_adopt_posterior)
  // records the rows the other side then holds; gpso_append extends the posterior in place and leaves the record alone, so
  // the NEXT hand-off may move only what the appends wrote -- the new rows of the scaled inputs and of each predict-ready
  // copy of L^-1, alpha, the hyper block -- instead of the whole range (C5: ~1.1 MB instead of 1.07 GB for 7 points).
  // Anything that makes another posterior clears it (res.sync_n: posterior_dropped), an append that crosses a power of two of the
  // fp16 scale repacks all rows (res.sync_scale).
  // the scale slot's [1] (2^-sa) of the fp16 split as the device holds it now; 0 where it does not apply
  int current_split_scale(float* out) {
    *out = 0.0f;
    if (!(kFloatPredict && f16_split() && bf16_usable() && res.linv_b == Copy::Valid)) return GPSO_OK;
    float* h = reinterpret_cast<float*>(ctx->pinned_scratch(256) + 124);  // (a slot of the scratch nothing else reads)
    HIPCHECK(hipMemcpyAsync(h, f16_scale() + 1, 4, hipMemcpyDeviceToHost, st()));
    HIPCHECK(hipStreamSynchronize(st()));
    *out = *h;
    return GPSO_OK;
  }
  // ranges of the arena (offset, bytes) that differ between the posterior of the first n0 rows and this one of n rows at the
  // same hyper-parameters, predict math and fp16 scale -- the same list on every rank (a function of n0, n, the layout)
  void rows_ranges(int64_t n0, std::vector<std::pair<int64_t, int64_t>>& out) const {
    out.clear();
    const char* base = static_cast<const char*>(arena.p);
    auto rel = [&](const DevBuf& b, size_t off, size_t bytes) {
      if (bytes) out.push_back({(int64_t)(static_cast<const char*>(b.p) - base + off), (int64_t)bytes});
    };
    const int64_t rt0 = n0 / 16, rt1 = (n - 1) / 16, npad16 = npad / 16;
    rel(hyper, 0, (size_t)(kHyperHeader + kMaxD) * 8);
    rel(xs64, (size_t)n0 * dp * 8, (size_t)(n - n0) * dp * 8);
    rel(xs_p64, (size_t)rt0 * dp * 16 * 8, (size_t)(rt1 + 1 - rt0) * dp * 16 * 8);  // MFMA fragments: 16-row groups
    rel(xnorm64, (size_t)n0 * 8, (size_t)(n - n0) * 8);
    rel(alpha, 0, (size_t)npad * sizeof(TP));  // alpha_1 += R^T a_2: every entry moved
    if (math_in_use() != GPSO_MATH_NATIVE) {
      rel(linv_b, 0, 256);  // the scale slot
      for (int s_ = 0; s_ < nsplit(); ++s_)  // plane s: tile row rt at ((s npad16 + rt) npad 32) bytes behind the slot
        rel(linv_b, 256 + ((size_t)s_ * npad16 + rt0) * npad * 32, (size_t)(rt1 + 1 - rt0) * npad * 32);
    } else {
      const size_t t0 = (size_t)rt0 * (rt0 + 1) / 2, t1 = (size_t)(rt1 + 1) * (rt1 + 2) / 2;  // tiles row-major over the triangle
      rel(linv_p, t0 * 256 * sizeof(TP), (t1 - t0) * 256 * sizeof(TP));
    }
  }
  // can the peers be brought up to date by rows?  (root side; scale = current_split_scale)
  bool rows_apply(float scale) const {
    return res.has_post() && res.sync_n >= 0 && res.sync_n <= n && res.sync_math == math_in_use() && scale == res.sync_scale &&
           (res.sync_n == n || res.sync_n / 16 <= (n - 1) / 16);
  }

  int ensure_fit_buffers() {
    int rc;
    const size_t s = sizeof(TF);
    if ((rc = ensure(K, (size_t)npad * npad * s))) return rc;
    if ((rc = ensure(Lf, (size_t)npad * npad * s))) return rc;
    if ((rc = ensure(linv, (size_t)npad * npad * s))) return rc;
    if ((rc = ensure(work, (size_t)npad * npad * s))) return rc;
    if ((rc = ensure(white, (size_t)npad * s))) return rc;
    if ((rc = ensure(alpha_f, (size_t)npad * s))) return rc;
    if ((rc = ensure(logdet, (size_t)npad * 8))) return rc;
    if ((rc = ensure(kinv_diag, (size_t)npad * 8))) return rc;
    if ((rc = ensure(apart, alpha_part_doubles(npad) * 8))) return rc;
    if ((rc = ensure(scal, (size_t)(8 + kGradMaxLs + 3) * 8))) return rc;
    const size_t nt = (size_t)(npad / 64);
    if ((rc = ensure(gpart, nt * nt * (size_t)(kGradMaxLs + 2) * 8))) return rc;
    return GPSO_OK;
  }

  // GPSO_OK, or the message of what theta_refusal / theta_shape_refusal (theta.hpp) found.  what_lik: the likelihood
  // parameter's name at this entry point
  int theta_status(const ThetaRefusal& r, const char* what_lik = "noise variance") {
    switch (r.rule) {
      case ThetaRule::None: return GPSO_OK;
      case ThetaRule::Lik: return ctx->fail(GPSO_E_ARG, "%s %g must be positive", what_lik, r.value);
      case ThetaRule::Kernel: return ctx->fail(GPSO_E_ARG, "unknown kernel id %d", r.index);
      case ThetaRule::Nls: return ctx->fail(GPSO_E_ARG, "n_ls=%d must be 1 or D=%d", r.index, d);
      case ThetaRule::Lengthscale: return ctx->fail(GPSO_E_ARG, "lengthscale[%d]=%g must be positive", r.index, r.value);
      case ThetaRule::Variance: return ctx->fail(GPSO_E_ARG, "kernel variance %g must be positive", r.value);
    }
    return GPSO_OK;
  }
  // the resident theta, as a fit at the same hyper-parameters takes it (gpso_append's refit)
  Theta resident_theta() const {
    Theta th;
    theta_from_parts(kp.kernel, ls_host.data(), n_ls, kp.variance, kp.noise, kp.mean_c, &th);
    return th;
  }

  // the lengthscale of every padded input dimension, as the hyper block and the one-launch kernels take them: an isotropic
  // one repeated, the last of n_ls behind them
  static void expand_ls(const double* ls, int n_ls, double* row) {
    for (int k = 0; k < kMaxD; ++k) row[k] = ls[n_ls == 1 ? 0 : std::min(k, n_ls - 1)];
  }
  // th.lik: the noise variance of the hyper block.  upload = false: the caller's kernel writes the device copy of the block
  // itself (fused small fit).  stage: a fit call's FitCall::theta_stage(); NULL: the scratch is asked for here
  int set_theta(const Theta& th, bool upload = true, double* stage = nullptr) {
    if (int rc = theta_status(theta_refusal(th, d, false))) return rc;
    kp.kernel = th.kernel;
    kp.variance = th.variance;
    kp.noise = th.lik;
    kp.mean_c = th.mean_c;
    n_ls = th.n_ls;
    ls_host.assign(th.ls, th.ls + n_ls);
    if (!upload) return GPSO_OK;
    // staged in pinned memory (FitScratch::kThetaAt; the read-backs lie below it): the copy is then a plain stream
    // operation and needs no host synchronisation here
    double* scratch = stage ? nullptr : ctx->pinned_scratch(FitScratch::doubles(false));
    if (!stage && !scratch) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    double* h = stage ? stage : scratch + FitScratch::kThetaAt;
    std::memset(h, 0, FitScratch::kThetaDoubles * 8);
    h[0] = (double)n; h[1] = (double)d; h[2] = (double)th.kernel; h[3] = (double)n_ls;
    h[4] = th.variance; h[5] = th.lik; h[6] = th.mean_c;
    expand_ls(th.ls, n_ls, h + kHyperHeader);
    HIPCHECK(hipMemcpyAsync(hyper.p, h, FitScratch::kThetaDoubles * 8, hipMemcpyHostToDevice, st()));
    return GPSO_OK;
  }

  // X / lengthscale for the fit (double) and, packed as MFMA fragments, for the predict generation
  int scale_inputs() {
    launch_scale_x<double>(st(), as<double>(x64), n, npad, d, dp, ls_dev(), as<double>(xs64), as<double>(xnorm64),
                           as<double>(xs_p64));
    return GPSO_OK;
  }
  void reset_generation() {
    f16_handed_at = nullptr;  // (a fit that failed between its solve and its packing leaves nothing behind)
    res.reset_generation(kFloatPredict, math_auto, gen_mode);
  }
  // float copies of the scaled inputs, made when a float-generation predict first needs them, from the
  // double ones (resident after a fit AND after a hand-off): two short launches, not two per loss evaluation
  int ensure_generation_inputs() {
    if (gen_double() || res.gen32_inputs_ok) return GPSO_OK;
    launch_gen_inputs_f32(st(), as<double>(xs64), npad, dp, as<float>(xs32), as<float>(xnorm32), as<float>(xs_p32));
    launch_gen_inputs_f16(st(), as<float>(xs32), as<float>(xnorm32), npad, dp, as<float>(c16_scal), xs_h16.p);
    res.gen_inputs_made();
    return GPSO_OK;
  }

  // ------------------------------------------------------------------------------------------
  int set_data(const double* X, const double* y, int64_t n_, int d_) override { return put_rows(X, y, n_, d_, false); }
  // keep_stash: the rows are the inducing points of the stashed training set (gpso_sgpr_set_inducing), not new data
  int put_rows(const double* X, const double* y, int64_t n_, int d_, bool keep_stash) {
    if (!X || !y) return ctx->fail(GPSO_E_ARG, "X / y must not be NULL");
    int rc = refuse_if_async("gpso_set_data");
    if (rc) return rc;
    rc = shape(n_, d_);
    if (rc) return rc;
    // small problems (the optimiser loop: N <= a few hundred) are staged through pinned memory so that
    // the call needs no stream synchronisation; large ones copy straight from the caller's pages
    const size_t doubles = (size_t)n * d + (size_t)n;
    double* stage = doubles <= (1u << 17) ? ctx->pinned_stage(doubles) : nullptr;
    if (stage) {
      std::memcpy(stage, X, (size_t)n * d * 8);
      std::memcpy(stage + (size_t)n * d, y, (size_t)n * 8);
      HIPCHECK(hipMemcpyAsync(x64.p, stage, (size_t)n * d * 8, hipMemcpyHostToDevice, st()));
      HIPCHECK(hipMemcpyAsync(y64.p, stage + (size_t)n * d, (size_t)n * 8, hipMemcpyHostToDevice, st()));
    } else {
      HIPCHECK(hipMemcpyAsync(x64.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, st()));
      HIPCHECK(hipMemcpyAsync(y64.p, y, (size_t)n * 8, hipMemcpyHostToDevice, st()));
      HIPCHECK(hipStreamSynchronize(st()));
    }
    if (X != x_host.data()) x_host.assign(X, X + (size_t)n * d);
    if (y != y_host.data()) y_host.assign(y, y + (size_t)n);
    s_host.clear();  // (every gpso_set_data clears the per-point noise: it belonged to the rows just replaced)
    s_max = 0.0;
    res.new_data(keep_stash);
    return GPSO_OK;
  }

  // s[n_] >= 0 beside the resident data (NULL: none); the posterior is invalidated as by new data
  int set_noise_diag(const double* sv, int64_t n_) override {
    if (!res.have_data) return ctx->fail(GPSO_E_STATE, "gpso_set_noise_diag before gpso_set_data");
    int rc = refuse_if_async("gpso_set_noise_diag");
    if (rc) return rc;
    if (n_ != n) return ctx->fail(GPSO_E_ARG, "gpso_set_noise_diag: n=%lld does not match the resident data (N=%lld)", (long long)n_, (long long)n);
    double top = 0.0;
    if (sv != nullptr) {
      for (int64_t i = 0; i < n; ++i) {
        if (!(sv[i] >= 0.0) || !std::isfinite(sv[i]))
          return ctx->fail(GPSO_E_ARG, "gpso_set_noise_diag: s[%lld]=%g must be finite and >= 0", (long long)i, sv[i]);
        top = std::max(top, sv[i]);
      }
      if ((rc = ensure(sdiag, (size_t)npad * 8))) return rc;
      double* stage = ctx->pinned_stage((size_t)npad);  // (waits for the stream)
      if (!stage) return ctx->fail(GPSO_E_OOM, "pinned host staging");
      std::memcpy(stage, sv, (size_t)n * 8);
      std::memset(stage + n, 0, (size_t)(npad - n) * 8);
      HIPCHECK(hipMemcpyAsync(sdiag.p, stage, (size_t)npad * 8, hipMemcpyHostToDevice, st()));
      if (sv != s_host.data()) s_host.assign(sv, sv + (size_t)n);
    } else {
      s_host.clear();
    }
    s_max = top;
    res.noise_changed(sv != nullptr);
    return GPSO_OK;
  }

  int fit_eval(const Theta* th, double* nlml, double* grad) override { return fit_eval_impl(th, nlml, grad, nullptr, nullptr); }
  // One evaluation of the LOO-CV objective: the fit with a gradient as gpso_fit_eval runs it -- so L, L^-1, alpha, the
  // packed copies and the hyper block come out the same bits -- and behind it, on the same stream, the LOO launches (loo.hip)
  int fit_eval_loo(const Theta* th, double* loss, double* grad, double* nlml) override {
    if (sizeof(TF) == 4)
      return ctx->fail(GPSO_E_ARG, "gpso_fit_eval_loo needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context (the LOO objective "
                                   "of a float factor is not supported)");
    double g_nlml[kGradMaxLs + 3], f_loo = 0.0;  // (the NLML gradient is computed whether or not the caller wants it)
    return fit_eval_impl(th, nlml, g_nlml, loss ? loss : &f_loo, grad);
  }

  // ---- one fit call (fit_call.hpp): the plan is decided here and goes down, the stages fill the record ----
  int fit_eval_impl(const Theta* thp, double* nlml, double* grad, double* loo_loss, double* loo_grad) {
    ctx->tick_timing();
    const FitPlan plan = FitPlan::make(grad != nullptr, loo_loss != nullptr, fused_small && small_fit_eligible(n, dp), ctx->timing, n);
    if (!res.have_data) return ctx->fail(GPSO_E_STATE, "%s before gpso_set_data", plan.who);
    if (!thp) return ctx->fail(GPSO_E_ARG, "lengthscales must not be NULL");
    const Theta& th = *thp;
    int rc = refuse_if_async(plan.who);
    if (rc) return rc;
    if (plan.loo && n < 2) return ctx->fail(GPSO_E_ARG, "gpso_fit_eval_loo needs at least two training points (N=%lld)", (long long)n);
    FitCall call = FitCall::begun(ctx->pinned_scratch(FitScratch::doubles(plan.loo)));
    if (!call.scratch) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    if (plan.loo && (rc = ensure_loo_buffers())) return rc;
    if ((rc = ensure_fit_buffers())) return rc;
    if ((rc = set_theta(th, plan.theta_from_host(), call.theta_stage()))) return rc;
    // (tile rows of linv_p beyond a one-launch fit's that may hold old data; every other fit writes, or will write, all 8)
    const int zero_tile_rows = res.fit_begun(plan.tile_rows());
    reset_generation();
    hipStream_t s = st();
    if ((rc = fit_span_begin(s))) return rc;
    if (grad && (rc = ensure(kinvb, (size_t)npad * npad * sizeof(TF)))) return rc;
    ctx->last_count[2] = plan.small ? GPSO_FITMATH_SMALL : (sizeof(TF) == 8 ? GPSO_FITMATH_F64 : GPSO_FITMATH_F32);  // (fit_planes_for: the plane paths' own)
    if ((rc = plan.small ? enqueue_small_fit(plan, call, th, zero_tile_rows, s) : enqueue_dense_fit(plan, call, th, s))) return rc;
    if (!plan.split_deferred() && (rc = pack_bf16())) return rc;
    if ((rc = enqueue_loo_tail(plan, call, th, s))) return rc;
    return finish_fit(plan, call, s, nlml, grad, loo_loss, loo_grad);
  }

  // The timed span of a fit-side call (gpso_fit_eval*, gpso_fit_eval_u_batch, gpso_append): last_ms[2] is the stream time
  // between the two.  The close comes behind the call's last launch: it asks whether every launch went out, records its
  // event BEFORE `wait` ends the call and reads the time behind it
  int fit_span_begin(hipStream_t s) {
    if (ctx->timing) HIPCHECK(hipEventRecord(ctx->ev[4], s));
    return GPSO_OK;
  }
  template <typename Wait>
  int fit_span_end(hipStream_t s, Wait&& wait /* -> hipError_t */) {
    if (int rc = launch_status()) return rc;
    if (ctx->timing) HIPCHECK(hipEventRecord(ctx->ev[5], s));
    HIPCHECK(wait());
    float ms = 0;
    if (ctx->timing && hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]) == hipSuccess) ctx->last_ms[2] = ms;
    return GPSO_OK;
  }

  // N <= 128: the whole evaluation in ONE launch (fit.hip: small_fit_kernel)
  int enqueue_small_fit(const FitPlan& plan, FitCall& call, const Theta& th, int zero_tile_rows, hipStream_t s) {
    SmallFitArgs a{};
    a.x64 = as<double>(x64); a.y64 = as<double>(y64); a.hyper = as<double>(hyper);
    expand_ls(th.ls, n_ls, a.ls);
    a.n = (int)n; a.d = d; a.dp = dp; a.kernel = th.kernel; a.n_ls = n_ls; a.want_grad = plan.grad ? 1 : 0;
    a.zero_tile_rows = zero_tile_rows;
    a.variance = th.variance; a.noise = th.lik; a.mean_c = th.mean_c;
    a.sdiag = s_dev();
    a.xs64 = as<double>(xs64); a.xnorm64 = as<double>(xnorm64); a.xs_p64 = as<double>(xs_p64);
    a.Lf = Lf.p; a.linv = linv.p; a.kinv = plan.grad ? kinvb.p : nullptr;
    a.white = white.p; a.alpha_f = alpha_f.p; a.alpha_p = alpha.p; a.linv_p = linv_p.p;
    a.diag64 = as<double>(logdet); a.kinv_diag = as<double>(kinv_diag); a.scal = as<double>(scal);
    // the loss, the factorisation's verdict and the gradient land in pinned host memory straight from the kernel
    a.scal_host = call.readback();
    a.done_token = call.arm_fit_token(plan.timed ? 0.0 : ctx->next_token());
    return launch_small_fit<TF, TP>(s, a) ? launch_status() : GPSO_OK;
  }

  // Side streams and events of the two-level fits (FitPlanes), made when the first such fit needs them.  Every object under
  // its own check: what a failed call left half done the next one completes.  The look-ahead stream of a double fit gets
  // the highest priority, a float fit's is plain non-blocking
  int ensure_fit_streams(bool with_inverse) {
    int lo_p = 0, hi_p = 0;
    if (ctx->side_stream == nullptr && sizeof(TF) == 8) {
      (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);  // (hi_p = the numerically smallest = highest priority)
      HIPCHECK(hipStreamCreateWithPriority(&ctx->side_stream, hipStreamNonBlocking, hi_p));
    }
    if (ctx->side_stream == nullptr) HIPCHECK(hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
    if (with_inverse && ctx->inv_stream == nullptr) HIPCHECK(hipStreamCreateWithFlags(&ctx->inv_stream, hipStreamNonBlocking));
    hipEvent_t* const evs[4] = {&ctx->ev_col, &ctx->ev_chain, &ctx->ev_panel, &ctx->ev_inv};  // (the last two: the inverse's)
    for (int i = 0; i < (with_inverse ? 4 : 2); ++i)
      if (*evs[i] == nullptr) HIPCHECK(hipEventCreateWithFlags(evs[i], hipEventDisableTiming));
    return GPSO_OK;
  }
  // What launch_potrf gets beside the matrices at these hyper-parameters: *use stays NULL for a single-level fit (and a
  // two-level one that runs as round 5's did), else it is `planes`, filled
  int fit_planes_for(const Theta& th, FitPlanes& planes, const FitPlanes** use) {
    if constexpr (sizeof(TF) == 4) {
      if (fit_planes_mode == 0 || npad <= (single_level_max >= 0 ? single_level_max : 3584)) return GPSO_OK;
      for (DevBuf* b : {&pl_L, &pl_X, &pl_XT, &pl_WT})
        if (int rc = ensure(*b, fit_plane_set_bytes(npad))) return rc;
      planes = FitPlanes{static_cast<unsigned short*>(pl_L.p), static_cast<unsigned short*>(pl_X.p),
                         static_cast<unsigned short*>(pl_XT.p), static_cast<unsigned short*>(pl_WT.p),
                         (int64_t)npad * npad, (int)(npad / 32)};
      if (int rc = ensure_fit_streams(false)) return rc;
      planes.cu_count = ctx->cu_count;
      // fp16 pieces (three MFMAs per product) when the hyper-parameters leave every plane set inside fp16's range
      // after its power-of-two scaling; bf16 pieces (six) otherwise -- the fallback rung
      if (fit_planes_mode == 2) (void)fit_plane_scales(th.variance, th.lik, planes, res.have_s ? s_max : 0.0);
      ctx->last_count[2] = planes.np == 2 ? GPSO_FITMATH_F16X3 : GPSO_FITMATH_BF16X6;
    } else {
      // double fits above the single-level limit (round 6): the diagonal blocks' chains are looked ahead on a side stream
      // and the level-doubling inverse runs on a third one, pair by pair, as soon as the panels it reads are final
      // (fit.hip: launch_potrf) -- GPSO_OPT_FIT_OVERLAP = 0 keeps round 5's sequential schedule (same bits either way)
      if (!fit_overlap || potrf_is_single_level<TF>(npad, single_level_max)) return GPSO_OK;
      if (int rc = ensure_fit_streams(true)) return rc;
      planes.inv = ctx->inv_stream;
      planes.ev_panel = ctx->ev_panel;
      planes.ev_inv = ctx->ev_inv;
      planes.overlap = fit_overlap;
    }
    planes.side = ctx->side_stream;
    planes.ev_col = ctx->ev_col;
    planes.ev_chain = ctx->ev_chain;
    *use = &planes;
    return GPSO_OK;
  }

  // any N: Gram, factorisation, inverse, alpha and the NLML, the gradient where wanted, the native-type packing
  int enqueue_dense_fit(const FitPlan& plan, FitCall& call, const Theta& th, hipStream_t s) {
    if (int rc = scale_inputs()) return rc;
    int* info_dev = reinterpret_cast<int*>(as<double>(scal) + 1);
    launch_gram<TF>(s, as<double>(xs64), as<double>(xnorm64), n, npad, dp, kp, as<TF>(K), info_dev, s_dev());
    // (the single-level factorisation writes all of L^-1 that is ever read: no 4 N_pad^2-byte zero fill -- 10 us at C3)
    const bool single_level = potrf_is_single_level<TF>(npad, single_level_max);
    if (!single_level) HIPCHECK(hipMemsetAsync(linv.p, 0, (size_t)npad * npad * sizeof(TF), s));
    FitPlanes planes{};
    const FitPlanes* pl = nullptr;
    if (int rc = fit_planes_for(th, planes, &pl)) return rc;
    const int done = launch_potrf<TF>(s, as<TF>(K), as<TF>(Lf), as<TF>(linv), as<TF>(work),
                                      plan.grad ? as<TF>(kinvb) : nullptr, n, npad, as<double>(logdet), info_dev,
                                      single_level_max, pl);
    bool inv_done = (done & 1) != 0, xt_ready = false;
    // (the single-level path leaves the padding blocks of L^-1 unwritten; the K^-1 = L^-T L^-1 GEMM of launch_gradient
    // would read them -- that path always builds K^-1 beside the factorisation: hold it to that)
    if (plan.grad && single_level && (done & 2) == 0)
      return ctx->fail(GPSO_E_STATE, "internal: the single-level factorisation did not leave K^-1 for the gradient");
    if constexpr (sizeof(TF) == 4) {
      if (!inv_done && pl != nullptr && trtri_bf16_applies(npad, fit_outer_panel(npad))) {
        launch_trtri_bf16(s, as<float>(linv), planes, npad, fit_outer_panel(npad), plan.grad);
        inv_done = true;
        xt_ready = true;
      }
    }
    if (!inv_done) launch_trtri<TF>(s, as<TF>(Lf), as<TF>(linv), as<TF>(work), npad, fit_outer_panel(npad));
    float* linv_max_out = f16_max_for_fit();  // (may allocate amax_rows: before the argument list below)
    launch_solve_alpha<TF>(s, as<TF>(linv), as<double>(y64), n, npad, th.mean_c, as<double>(logdet),
                           as<TF>(white), as<TF>(alpha_f), as<double>(apart), as<double>(kinv_diag),
                           as<double>(scal), alpha.p, sizeof(TP) == 8, as<float>(amax_rows), linv_max_out);
    if (plan.grad)
      launch_gradient<TF>(s, as<TF>(linv), as<TF>(alpha_f), as<double>(xs64), as<double>(xnorm64), n, npad, d, dp,
                          n_ls, ls_dev(), kp, as<TF>(kinvb), (done & 2) != 0, as<double>(gpart),
                          as<double>(scal) + 8, xt_ready ? &planes : nullptr);
    // the packed f32 / f64 copy of L^-1 feeds the NATIVE tile kernel only: a posterior that is going to predict with
    // split math (the default of float-predict contexts) packs it when -- if ever -- something asks for it
    // (ensure_linv_p: the self-test walking down GPSO_MATH_AUTO's ladder, a hand-off of all buffers)
    call.linv_p_left(bf16_usable());
    if (!call.linv_p_deferred) launch_pack_linv<TF, TP>(s, as<TF>(linv), n, npad, as<TP>(linv_p));  // (alpha's predict-type copy: alpha_sum_kernel)
    return GPSO_OK;
  }

  // the LOO launches behind the fit, on the same stream (loo.hip); a plan without LOO enqueues nothing
  int enqueue_loo_tail(const FitPlan& plan, FitCall& call, const Theta& th, hipStream_t s) {
    if constexpr (sizeof(TF) == 8) {
      if (plan.loo && plan.small) {
        // N <= 128: ONE workgroup behind the one-launch fit, its scalars straight into pinned host memory
        LooSmallArgs a{};
        a.kinv = as<double>(kinvb); a.alpha = as<double>(alpha_f); a.kinv_diag = as<double>(kinv_diag);
        a.y64 = as<double>(y64); a.xs = as<double>(xs64); a.ls = ls_dev();
        a.n = (int)n; a.npad = (int)npad; a.dp = dp; a.kernel = th.kernel; a.n_ls = n_ls; a.variance = th.variance;
        a.vec = nullptr; a.scal = as<double>(loo_scal); a.scal_host = call.loo_readback();
        a.done_token = call.arm_loo_token(plan.timed ? 0.0 : ctx->next_token());
        if (launch_loo_small(s, a)) return launch_status();
      } else if (plan.loo) {
        // any N: S = diag(sqrt c) K^-1 in the Gram buffer, M = S^T S in the factorisation's scratch (both free behind the
        // fit), 2 W over S, then the NLML gradient's own contraction with (kinv := 2 W, alpha := 0); kinvb stays K_y^-1
        double* vec = as<double>(loov);
        launch_loo_points<double>(s, as<double>(alpha_f), as<double>(kinv_diag), as<double>(y64), n, npad, vec, as<double>(loo_scal));
        launch_loo_weights(s, as<double>(kinvb), as<double>(alpha_f), vec, as<double>(K), as<double>(work), n, npad);
        launch_gradient<double>(s, as<double>(linv), vec + (size_t)kLooZero * npad, as<double>(xs64), as<double>(xnorm64), n, npad,
                                d, dp, n_ls, ls_dev(), kp, as<double>(K), true, as<double>(gpart), as<double>(loo_scal) + 8);
        launch_loo_mean_grad(s, vec, n, npad, as<double>(loo_scal) + 8 + n_ls + 2);
        HIPCHECK(hipMemcpyAsync(call.loo_readback(), loo_scal.p, FitScratch::kLooDoubles * 8, hipMemcpyDeviceToHost, s));
      }
    }
    return GPSO_OK;
  }

  // closes the span, brings the dense fit's scalars over, waits as the record says, and hands out what the call computed
  int finish_fit(const FitPlan& plan, const FitCall& call, hipStream_t s, double* nlml, double* grad, double* loo_loss, double* loo_grad) {
    const double *host = call.readback(), *loo_host = call.loo_readback();
    const int rc = fit_span_end(s, [&]() -> hipError_t {
      const hipError_t e = plan.small ? hipSuccess : hipMemcpyAsync(call.readback(), scal.p, FitScratch::kReadbackDoubles * 8, hipMemcpyDeviceToHost, s);
      if (e != hipSuccess) return e;
      const FitWait how = call.wait_on(plan);
      return how == FitWait::Stream ? ctx->wait(s) : ctx->wait_token(call.token_word(how), call.token(how), s);
    });
    if (rc) return rc;
    int info;
    std::memcpy(&info, &host[1], sizeof(int));
    if (info != INT_MAX)
      return ctx->fail(GPSO_E_NOTPD, "K + noise*I is not positive definite: Cholesky failed at pivot %d", info);
    if (nlml) *nlml = host[0];
    if (grad)  // device order: ls..., variance, noise, then -sum(alpha)
      for (int h = 0; h < n_ls + 3; ++h) grad[h] = host[8 + h];
    if (plan.loo) {
      *loo_loss = loo_host[0];
      if (loo_grad)
        for (int h = 0; h < n_ls + 3; ++h) loo_grad[h] = loo_host[8 + h];
    }
    res.fit_done(plan.grad, call.linv_p_deferred, plan.split_deferred(), bf16_usable());
    return GPSO_OK;
  }
  // the LOO vectors and scalars on the device (gpso_loo, gpso_fit_eval_loo)
  int ensure_loo_buffers() {
    if (int rc = ensure(loov, (size_t)kLooVecs * npad * 8)) return rc;
    return ensure(loo_scal, FitScratch::kLooDoubles * 8);
  }
  // ---- leave-one-out predictive of the resident fitted posterior (loo.hip): reads alpha and kinv_diag, changes nothing a
  // predict or a later call reads
  int loo(double* mean, double* var, double* lpd, double* loss) override {
    if (!(res.post == Post::Fitted && res.st_have && res.have_data && res.chol_valid))
      return ctx->fail(GPSO_E_STATE, "gpso_loo needs a posterior fitted with targets on this context (gpso_set_data + gpso_fit_eval)");
    int rc = refuse_if_async("gpso_loo");
    if (rc) return rc;
    if (n < 2) return ctx->fail(GPSO_E_ARG, "gpso_loo needs at least two training points (N=%lld)", (long long)n);
    if ((rc = ensure_loo_buffers())) return rc;
    hipStream_t s = st();
    double* vec = as<double>(loov);
    launch_loo_points<TF>(s, as<TF>(alpha_f), as<double>(kinv_diag), as<double>(y64), n, npad, vec, as<double>(loo_scal));
    if ((rc = launch_status())) return rc;
    if (mean) HIPCHECK(hipMemcpyAsync(mean, vec + (size_t)kLooMean * npad, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (var) HIPCHECK(hipMemcpyAsync(var, vec + (size_t)kLooVar * npad, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (lpd) HIPCHECK(hipMemcpyAsync(lpd, vec + (size_t)kLooLpd * npad, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (loss) HIPCHECK(hipMemcpyAsync(loss, loo_scal.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return GPSO_OK;
  }

  // ---- batched evaluation (multi-start hyper-parameter search): fit.hip small_fit_batch_kernel -------------------------
  // entries one launch may hold for the resident data: one workgroup per CU where the one-launch fit applies, else none
  int fit_batch_max() override { return (res.have_data && fused_small && small_fit_eligible(n, dp)) ? kSmallBatchMax : 0; }

  // everything a batched call is refused for, before anything is touched
  int fit_eval_batch_check(int kernel, int b, int n_ls_) override {
    if (!res.have_data) return ctx->fail(GPSO_E_STATE, "gpso_fit_eval_u_batch before gpso_set_data");
    int rc = refuse_if_async("gpso_fit_eval_u_batch");
    if (rc) return rc;
    if ((rc = theta_status(theta_shape_refusal(kernel, n_ls_, d)))) return rc;
    if (b < 1) return ctx->fail(GPSO_E_ARG, "a batch needs at least one entry (b=%d)", b);
    const int cap = fit_batch_max();
    if (cap == 0) {
      if (!fused_small) return ctx->fail(GPSO_E_ARG, "no batched evaluation: GPSO_OPT_FIT_FUSED_SMALL is off (gpso_fit_batch_max = 0)");
      if (n > 128) return ctx->fail(GPSO_E_ARG, "no batched evaluation for N > 128 (N=%lld; gpso_fit_batch_max = 0)", (long long)n);
      return ctx->fail(GPSO_E_ARG, "no batched evaluation for N > 64 with a padded D > 32 (N=%lld, D=%d; gpso_fit_batch_max = 0)",
                       (long long)n, d);
    }
    if (b > cap) return ctx->fail(GPSO_E_ARG, "b=%d entries exceed the limit of %d per call (gpso_fit_batch_max)", b, cap);
    return GPSO_OK;
  }

  // nv <= fit_batch_max() constrained hyper-parameter vectors th[nv][n_ls + 3] = (ls..., variance, noise, c), every one
  // acceptable to set_theta; loss[nv], grad[nv][n_ls + 3] (nullable), info[nv] (failing pivot or INT_MAX).  One launch;
  // no member that describes the resident posterior is touched.
  int fit_eval_batch(int kernel, const double* th, int nv, int n_ls_, double* loss, double* grad, int* info) override {
    ctx->tick_timing();
    const int H = n_ls_ + 3;
    int rc = ensure(batch_theta, (size_t)nv * kSmallBatchTheta * 8);
    if (rc) return rc;
    double* stage = ctx->pinned_stage((size_t)nv * kSmallBatchTheta);  // (waits for the stream)
    if (!stage) return ctx->fail(GPSO_E_OOM, "pinned host staging");
    for (int e = 0; e < nv; ++e) {
      double* r = stage + (size_t)e * kSmallBatchTheta;
      const double* t = th + (size_t)e * H;
      std::memset(r, 0, kSmallBatchTheta * 8);
      r[0] = t[n_ls_]; r[1] = t[n_ls_ + 1]; r[2] = t[n_ls_ + 2];
      expand_ls(t, n_ls_, r + kHyperHeader);
    }
    // results: straight into pinned host memory from the kernel (as the single fit's scalars), read behind the wait
    const size_t out_doubles = (size_t)nv * (1 + H) + ((size_t)nv + 1) / 2;
    double* host = ctx->pinned_scratch(out_doubles);
    if (!host) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    hipStream_t s = st();
    HIPCHECK(hipMemcpyAsync(batch_theta.p, stage, (size_t)nv * kSmallBatchTheta * 8, hipMemcpyHostToDevice, s));
    if ((rc = fit_span_begin(s))) return rc;
    SmallBatchArgs a{};
    a.x64 = as<double>(x64); a.y64 = as<double>(y64); a.theta = as<double>(batch_theta);
    a.loss = host; a.grad = host + nv; a.info = reinterpret_cast<int*>(host + (size_t)nv * (1 + H));
    a.n = (int)n; a.d = d; a.dp = dp; a.kernel = kernel; a.n_ls = n_ls_; a.want_grad = grad ? 1 : 0;
    a.sdiag = s_dev();
    if (launch_small_fit_batch<TF, TP>(s, a, nv)) {
      rc = launch_status();
      return rc ? rc : ctx->fail(GPSO_E_HIP, "internal: the batched fit refused %d entries", nv);
    }
    if ((rc = fit_span_end(s, [&] { return ctx->wait(s); }))) return rc;
    std::memcpy(loss, a.loss, (size_t)nv * 8);
    if (grad) std::memcpy(grad, a.grad, (size_t)nv * H * 8);
    std::memcpy(info, a.info, (size_t)nv * sizeof(int));
    return GPSO_OK;
  }

  // the packed native-type L^-1, made on demand from the resident factor's inverse
  int ensure_linv_p() {
    if (res.linv_p != Copy::Deferred || !res.chol_valid) return GPSO_OK;
    launch_pack_linv<TF, TP>(st(), as<TF>(linv), n, npad, as<TP>(linv_p));
    res.linv_p_packed();
    return launch_status();
  }

  // gpso_append where extending in place does not pay (`refit` says why): the posterior of the n + k points from scratch at
  // the resident hyper-parameters.  Returns 1, or the refit's negative status with the first n points' posterior put back
  int append_by_refit(const double* Xn, const double* yn, const double* sn, int64_t k, bool sn_nonzero, const char* refit, double* nlml) {
    const int64_t n_new = n + k;
    std::vector<double> X(x_host), y(y_host);
    X.insert(X.end(), Xn, Xn + (size_t)k * d);
    y.insert(y.end(), yn, yn + (size_t)k);
    // (set_data clears the per-point noise: the refit carries it along, the new points' values behind the resident ones)
    const bool with_s = res.have_s || sn_nonzero, had_s = res.have_s;
    std::vector<double> sv;
    if (with_s) {
      sv = res.have_s ? s_host : std::vector<double>((size_t)n, 0.0);
      if (sn != nullptr) sv.insert(sv.end(), sn, sn + (size_t)k);
      else sv.resize((size_t)n_new, 0.0);
    }
    const Theta th = resident_theta();
    const int d_ = d;
    const int64_t n_old = n;
    int rc = set_data(X.data(), y.data(), n_new, d_);
    if (rc == GPSO_OK && with_s) rc = set_noise_diag(sv.data(), n_new);
    if (rc == GPSO_OK) rc = fit_eval(&th, nlml, nullptr);
    if (rc < 0) {
      // the header's promise holds on this path too: a failed append leaves the posterior of the first n points resident
      // (set_data dropped it: put the old points back and refit at the resident hyper-parameters -- the fit that
      // succeeded before the call)
      const std::string why = ctx->err;
      X.resize((size_t)n_old * d_);
      y.resize((size_t)n_old);
      int rc2 = set_data(X.data(), y.data(), n_old, d_);
      if (rc2 == GPSO_OK && had_s) {
        sv.resize((size_t)n_old);
        rc2 = set_noise_diag(sv.data(), n_old);
      }
      if (rc2 == GPSO_OK) rc2 = fit_eval(&th, nullptr, nullptr);
      if (rc2 < 0) return ctx->fail(rc, "%s (and the posterior of the first %lld points could not be restored: status %d -- "
                                        "gpso_set_data + gpso_fit_eval start over)", why.c_str(), (long long)n_old, rc2);
      return ctx->fail(rc, "%s (the posterior of the first %lld points is resident again)", why.c_str(), (long long)n_old);
    }
    ctx->fail(1, "gpso_append: posterior of the %lld points refitted from scratch at the resident hyper-parameters (%s)",
              (long long)n_new, refit);
    return 1;
  }

  // ---- rank-k append at the resident hyper-parameters (append.hip) ------------------------------------------------------
  // Returns GPSO_OK when the resident factor was extended in place, 1 when the posterior of the n + k points was refitted
  // from scratch at the same hyper-parameters instead (gpso_last_error says why), or a negative status.
  // sn (nullable = zeros): the per-point noise of the new points; a context without a vector gets one (zeros for the
  // resident rows) when some sn[j] is not zero
  int append(const double* Xn, const double* yn, const double* sn, int64_t k, double* nlml) override {
    ctx->tick_timing();
    if (!Xn || !yn) return ctx->fail(GPSO_E_ARG, "Xnew / ynew must not be NULL");
    if (k < 1) return ctx->fail(GPSO_E_ARG, "need at least one new point (k=%lld)", (long long)k);
    bool sn_nonzero = false;
    if (sn != nullptr)
      for (int64_t j = 0; j < k; ++j) {
        if (!(sn[j] >= 0.0) || !std::isfinite(sn[j]))
          return ctx->fail(GPSO_E_ARG, "gpso_append_noise: snew[%lld]=%g must be finite and >= 0", (long long)j, sn[j]);
        sn_nonzero = sn_nonzero || sn[j] > 0.0;
      }
    switch (res.post) {
      case Post::Svgp: return ctx->fail(GPSO_E_STATE, "gpso_append on an SVGP predictive: its rows are the inducing points; set the grown data and train again");
      case Post::Sgpr: return ctx->fail(GPSO_E_STATE, "gpso_append on an SGPR predictive: its rows are the inducing points; set the grown data and train again");
      case Post::Vgp: return ctx->fail(GPSO_E_STATE, "gpso_append on a VGP predictive: append the data and train q again");
      default: break;
    }
    if (int rca = refuse_if_async("gpso_append")) return rca;
    if (!res.have_data || !res.has_post() || !res.chol_valid || (int64_t)y_host.size() != n)
      return ctx->fail(GPSO_E_STATE, "gpso_append needs a posterior fitted on this context (gpso_set_data + gpso_fit_eval)");
    const int64_t n_new = n + k;
    if (n_new > 65536) return ctx->fail(GPSO_E_ARG, "n=%lld above the supported 65536", (long long)n_new);
    const char* refit = nullptr;
    if (k > kAppendMax) refit = "more than 64 new points in one call";
    else if (n_new > npad) refit = "the padded size grows: every buffer changes its layout";
    else if (fused_small && small_fit_eligible(n_new, dp)) refit = "N <= 128: the one-launch fit is the shorter exact update";
    // (measured, float, N = 2048: append of 64 points 0.55 ms, of 7 points 0.06 ms, posterior fit 0.52 ms -- the k x k corner
    // is factorised by one workgroup; at N = 8192 the same 64 points take 1.1 ms against 4.2: profiles/r05_append_bench.jsonl)
    else if (k > 32 && npad < 4096) refit = "more than 32 new points beside fewer than 4096: the refit is as fast";
    if (refit != nullptr) return append_by_refit(Xn, yn, sn, k, sn_nonzero, refit, nlml);
    hipStream_t s = st();
    int rc;
    const int kpad = append_kp((int)k);
    if ((rc = ensure(app, append_scratch_doubles(npad, kpad) * 8))) return rc;
    // the first per-point noise of this context: the resident rows carry zeros.  The context only COUNTS as carrying a
    // vector (res.have_s) once the append has succeeded: a failed one leaves it as it found it
    const bool new_s = !res.have_s && sn_nonzero, use_s = res.have_s || new_s;
    if (new_s) {
      if ((rc = ensure(sdiag, (size_t)npad * 8))) return rc;
      HIPCHECK(hipMemsetAsync(sdiag.p, 0, (size_t)npad * 8, s));
    }
    double* stage = ctx->pinned_stage((size_t)k * d + 2 * (size_t)k);  // (waits for the stream)
    double* host = ctx->pinned_scratch(8);
    if (!stage || !host) return ctx->fail(GPSO_E_OOM, "pinned host staging");
    if ((rc = fit_span_begin(s))) return rc;
    // (no copies: append_cross_kernel reads the new points from this pinned buffer and files them in x64 / y64 itself)
    std::memcpy(stage, Xn, (size_t)k * d * 8);
    std::memcpy(stage + (size_t)k * d, yn, (size_t)k * 8);
    const bool pass_s = use_s && sn != nullptr;
    if (pass_s) std::memcpy(stage + (size_t)k * d + (size_t)k, sn, (size_t)k * 8);
    AppendArgs a{};
    a.x64 = as<double>(x64); a.y64 = as<double>(y64); a.ls = ls_dev();
    a.xnew = stage; a.ynew = stage + (size_t)k * d;
    a.snew = pass_s ? stage + (size_t)k * d + (size_t)k : nullptr;
    a.sdiag = use_s ? as<double>(sdiag) : nullptr;
    a.n = n; a.npad = npad; a.k = (int)k; a.d = d; a.dp = dp; a.kernel = kp.kernel;
    a.variance = kp.variance; a.noise = kp.noise; a.mean_c = kp.mean_c;
    a.xs64 = as<double>(xs64); a.xnorm64 = as<double>(xnorm64); a.xs_p64 = as<double>(xs_p64);
    a.diag64 = as<double>(logdet); a.nlml = as<double>(scal); a.kinv_diag = as<double>(kinv_diag);
    a.alpha_p = alpha.p; a.hyper = as<double>(hyper); a.host_out = host;
    // the fp16 split's scale follows max |L^-1|: the slot holds it when the pieces are built, or when the fit's solve
    // handed it over for a packing still to come
    const bool f16_max_live = kFloatPredict && f16_split() && bf16_usable() &&
                              (res.linv_b == Copy::Valid || (res.linv_b == Copy::Deferred && f16_handed_at != nullptr && f16_handed_at == f16_scale()));
    a.f16_scal = f16_max_live ? f16_scale() : nullptr;
    host[0] = host[1] = 0.0;
    launch_append<TF, TP>(s, a, app.p, as<TF>(linv), as<TF>(Lf), as<TF>(white), as<TF>(alpha_f));
    // the 16-row tiles that hold new rows, in whichever predict-ready copies of L^-1 are built (the others are made on
    // demand from the extended matrix)
    const int64_t rt0 = n / 16;
    auto repack = [&](int64_t rows) {
      if (res.linv_b == Copy::Valid) {
        if (f16_split()) launch_pack_linv_f16<TF>(s, as<TF>(linv), rows, npad, f16_scale(), split_planes(), true, rt0);
        else launch_pack_linv_bf16<TF>(s, nsplit(), as<TF>(linv), rows, npad, split_planes(), rt0);
      }
      if (res.linv_p == Copy::Valid) launch_pack_linv<TF, TP>(s, as<TF>(linv), rows, npad, as<TP>(linv_p), rt0);
    };
    repack(n_new);
    if ((rc = fit_span_end(s, [&] { return ctx->wait(s); }))) return rc;
    if (host[1] != 1.0) {
      // K22 + noise I - L21 L21^T is not positive definite: the posterior of the n points is still what the device holds
      // (append_cols_kernel did not run); the tiles just repacked and the scaled-input rows go back to their padding state
      const int pivot = (int)host[2];
      repack(n);
      if (res.have_s) HIPCHECK(hipMemsetAsync(as<double>(sdiag) + n, 0, (size_t)k * 8, s));  // (back to padding; a vector this call made is simply not adopted)
      (void)scale_inputs();
      res.append_refused();
      HIPCHECK(hipStreamSynchronize(s));
      return ctx->fail(GPSO_E_NOTPD, "K + noise*I is not positive definite: the appended block's Cholesky failed at pivot %d "
                       "(the posterior of the first %lld points is unchanged)", pivot, (long long)n);
    }
    x_host.insert(x_host.end(), Xn, Xn + (size_t)k * d);
    y_host.insert(y_host.end(), yn, yn + (size_t)k);
    if (new_s) {
      s_host.assign((size_t)n, 0.0);
      s_max = 0.0;
    }
    if (use_s) {
      if (pass_s) s_host.insert(s_host.end(), sn, sn + (size_t)k);
      else s_host.resize((size_t)n_new, 0.0);
      if (pass_s) s_max = std::max(s_max, *std::max_element(sn, sn + (size_t)k));
    }
    n = n_new;
    if (nlml) *nlml = host[0];
    res.appended(new_s);
    return GPSO_OK;
  }


  int set_posterior(const double* X, const double* L, const double* alpha64, int64_t n_, int d_, const Theta& th) override {
    if (!X || !L || !alpha64) return ctx->fail(GPSO_E_ARG, "NULL argument");
    int rc = refuse_if_async("gpso_set_posterior");
    if (rc) return rc;
    rc = shape(n_, d_);
    if (rc) return rc;
    if ((rc = ensure_fit_buffers())) return rc;
    if ((rc = set_theta(th))) return rc;
    if ((rc = ensure(getter_tmp, (size_t)n * n * 8 + (size_t)n * 8))) return rc;
    hipStream_t s = st();
    double* tmp = as<double>(getter_tmp);
    HIPCHECK(hipMemcpyAsync(x64.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(tmp, L, (size_t)n * n * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(tmp + (size_t)n * n, alpha64, (size_t)n * 8, hipMemcpyHostToDevice, s));
    s_host.clear();
    s_max = 0.0;
    res.install_begun();
    reset_generation();
    if ((rc = scale_inputs())) return rc;
    HIPCHECK(hipMemsetAsync(linv.p, 0, (size_t)npad * npad * sizeof(TF), s));
    launch_install_chol<TF>(s, tmp, n, npad, as<TF>(Lf), as<TF>(linv));
    launch_trtri<TF>(s, as<TF>(Lf), as<TF>(linv), as<TF>(work), npad, kFitBlock);
    HIPCHECK(hipMemsetAsync(alpha_f.p, 0, (size_t)npad * sizeof(TF), s));
    launch_convert_in<TF>(s, tmp + (size_t)n * n, as<TF>(alpha_f), 1, n, npad);
    launch_pack_linv<TF, TP>(s, as<TF>(linv), n, npad, as<TP>(linv_p));
    launch_convert_vec<TF, TP>(s, as<TF>(alpha_f), as<TP>(alpha), npad);
    if ((rc = pack_bf16())) return rc;
    HIPCHECK(hipStreamSynchronize(s));  // the caller's host buffers are free again on return
    if ((rc = launch_status())) return rc;
    res.installed();
    return GPSO_OK;
  }

  // ---- variational GP (GPflow 2 VGP, whitened, Gaussian likelihood) ----------------------------
  // q(v) = N(mu, S S^T) lives here beside the training data: vq_mu [N_pad], vq_S [N_pad^2] (lower; identity on the padding).
  // Every product is a whole-matrix float64 GEMM (launch_dgemm), every factorisation the fit's launch_potrf; the calls leave
  // the fit's buffers (K, Lf, linv, work) holding VGP intermediates, so they invalidate any GPR posterior first.
  DevBuf vq_mu, vq_S, vA, vB, vC, vvec, vsmall;
  int64_t vq_n = -1, vq_npad = -1;  // shape q was made for (another shape: q restarts at the prior)
  static constexpr double kVgpJitter = 1.0e-6;  // GPflow's default_jitter, in the K of the ELBO and of the predictive
  enum { kVgpR = 0, kVgpFvar = 1, kVgpSrow = 2, kVgpH = 3, kVgpH2 = 4, kVgpZero = 5, kVgpVecs = 6 };
  double* vvec_at(int k) const { return as<double>(vvec) + (size_t)k * npad; }
  // vsmall: [0, 6) the -ELBO sums, [8, 8 + kGradMaxLs + 3) the gradient (launch_gradient: n_ls + 3 doubles), then the four
  // int verdicts of the factorisations (Gram, Lambda, Sigma, I - Sigma) in two doubles of their own
  static constexpr int kVgpGradAt = 8, kVgpInfoAt = kVgpGradAt + kGradMaxLs + 3, kVgpSmall = kVgpInfoAt + 2;
  static_assert(kVgpGradAt >= 6 && kVgpInfoAt >= kVgpGradAt + kGradMaxLs + 3, "vsmall layout: sums, gradient and verdicts overlap");
  int* vinfo() const { return reinterpret_cast<int*>(as<double>(vsmall) + kVgpInfoAt); }
  // a general scalar likelihood (vlik_kind != GPSO_LIK_GAUSSIAN): df, the Gauss-Hermite rule on the device (vgh: [0, 64)
  // nodes x sqrt(2), [64, 128) weights / sqrt(pi)) and the per-point vectors of the quadrature (vlvec)
  DevBuf vgh, vlvec;
  double vlik_df = 0.0;
  int vlik_n_gh = 0;
  enum { kLikM = 0, kLikV = 1, kLikGm = 2, kLikA = 3, kLikT = 4, kLikVe = 5, kLikDve = 6, kLikMu = 7, kLikVecs = 8 };
  double* lvec_at(int k) const { return as<double>(vlvec) + (size_t)k * npad; }
  // the f-free part of log p(y | f) at the likelihood parameter p (Student-t: the scale; Gaussian: the variance)
  double vlik_const(double p) const {
    if (vlik_kind == GPSO_LIK_STUDENT_T)
      return std::lgamma(0.5 * (vlik_df + 1.0)) - std::lgamma(0.5 * vlik_df) -
             0.5 * (std::log(p * p) + std::log(vlik_df) + std::log(M_PI));
    return -0.5 * (std::log(2.0 * M_PI) + std::log(p));
  }
  // m = L mu + c, v = rownorm(L S) (A := L S), then the quadrature at q: gm, a, t, VE, dVE/dp
  void vgp_quadrature(const double* L, double* A, double p, double mean_c) {
    hipStream_t s = st();
    launch_vgp_gemv(s, L, false, as<double>(vq_mu), 0.0, 1.0, mean_c, nullptr, lvec_at(kLikM), n, npad);
    launch_dgemm(s, L, false, as<double>(vq_S), false, A, npad, 1.0, 0.0);
    launch_vgp_rownorm(s, A, lvec_at(kLikV), n, npad);
    launch_vgp_quad(s, as<double>(y64), lvec_at(kLikM), lvec_at(kLikV), as<double>(vgh), vlik_n_gh, vlik_kind, p, vlik_df,
                    vlik_const(p), mean_c, lvec_at(kLikGm), lvec_at(kLikA), lvec_at(kLikT), lvec_at(kLikVe),
                    lvec_at(kLikDve), n, npad);
  }

  int vgp_set_likelihood(int kind, double df, int n_gh, const double* gh_x, const double* gh_w) override {
    if (sizeof(TF) != 8) return ctx->fail(GPSO_E_ARG, "the variational GP needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context");
    if (kind != GPSO_LIK_GAUSSIAN && kind != GPSO_LIK_STUDENT_T && kind != GPSO_LIK_GAUSSIAN_GH)
      return ctx->fail(GPSO_E_ARG, "unknown likelihood kind %d", kind);
    if (kind != GPSO_LIK_GAUSSIAN) {
      if (n_gh < 1 || n_gh > 64) return ctx->fail(GPSO_E_ARG, "n_gh=%d outside [1, 64]", n_gh);
      if (!gh_x || !gh_w) return ctx->fail(GPSO_E_ARG, "gh_x / gh_w must not be NULL");
      if (kind == GPSO_LIK_STUDENT_T && !(df > 2.0))
        return ctx->fail(GPSO_E_ARG, "Student-t df=%g: need df > 2 (a finite predictive variance)", df);
    }
    int rc = refuse_if_async("gpso_vgp_set_likelihood");
    if (rc) return rc;
    if (kind != GPSO_LIK_GAUSSIAN) {
      if ((rc = ensure(vgh, 128 * 8))) return rc;
      double host[128] = {};
      for (int k = 0; k < n_gh; ++k) {  // (GPflow's ndiagquad: x sqrt(2), w / sqrt(pi))
        host[k] = gh_x[k] * std::sqrt(2.0);
        host[64 + k] = gh_w[k] / std::sqrt(M_PI);
      }
      HIPCHECK(hipMemcpyAsync(vgh.p, host, sizeof(host), hipMemcpyHostToDevice, st()));
      HIPCHECK(hipStreamSynchronize(st()));
    }
    vlik_kind = kind;
    vlik_df = kind == GPSO_LIK_STUDENT_T ? df : 0.0;
    vlik_n_gh = kind == GPSO_LIK_GAUSSIAN ? 0 : n_gh;
    return launch_status();
  }

  int vgp_begin(bool sparse = false /* the rows are inducing points: the SGPR's factors go too */) {
    if (sizeof(TF) != 8) return ctx->fail(GPSO_E_ARG, "the variational GP needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context");
    if (!res.have_data) return ctx->fail(GPSO_E_STATE, "VGP call before gpso_set_data");
    int rc = refuse_if_async("a VGP call");
    if (rc) return rc;
    if ((rc = ensure_fit_buffers())) return rc;
    const size_t mat = (size_t)npad * npad * 8;
    for (DevBuf* b : {&vA, &vB, &vC, &vq_S})
      if ((rc = ensure(*b, mat))) return rc;
    if ((rc = ensure(vq_mu, (size_t)npad * 8))) return rc;
    if ((rc = ensure(vvec, (size_t)kVgpVecs * npad * 8))) return rc;
    if ((rc = ensure(vsmall, kVgpSmall * 8))) return rc;
    if (vlik_kind != GPSO_LIK_GAUSSIAN && (rc = ensure(vlvec, (size_t)kLikVecs * npad * 8))) return rc;
    if (vq_n != n || vq_npad != npad) vgp_prior();
    res.variational_begun(sparse);
    reset_generation();
    return GPSO_OK;
  }
  void vgp_prior() {
    (void)hipMemsetAsync(vq_mu.p, 0, (size_t)npad * 8, st());
    launch_vgp_pad_identity(st(), as<double>(vq_S), 0, npad, nullptr);
    vq_n = n;
    vq_npad = npad;
  }
  // A (destroyed: lower triangle read, identity padding) = Lout Lout^T; Linv = Lout^-1.  Both leave as clean lower triangles:
  // zero above the diagonal, pad_diag on the diagonal of the padding, zero elsewhere on it
  int vgp_chol(double* A, double* Lout, double* Linv, int* info, double pad_diag) {
    hipStream_t s = st();
    HIPCHECK(hipMemsetAsync(Linv, 0, (size_t)npad * npad * 8, s));
    const int done = launch_potrf<double>(s, A, Lout, Linv, as<double>(work), nullptr, n, npad, as<double>(logdet), info,
                                          single_level_max, nullptr);
    if (!(done & 1)) launch_trtri<double>(s, Lout, Linv, as<double>(work), npad, fit_outer_panel(npad));
    launch_vgp_clean_lower(s, Lout, Lout, n, npad, pad_diag);
    launch_vgp_clean_lower(s, Linv, Linv, n, npad, pad_diag);
    return GPSO_OK;
  }
  // L = chol(k(X, X) + 1e-6 I) into Lf, L^-1 into linv (clean lower, zero padding)
  int vgp_factor(const Theta& th) {
    int rc = set_theta(th.with_lik(kVgpJitter));
    if (rc) return rc;
    if ((rc = scale_inputs())) return rc;
    launch_gram<double>(st(), as<double>(xs64), as<double>(xnorm64), n, npad, dp, kp, as<double>(K), vinfo() + 0);
    return vgp_chol(as<double>(K), as<double>(Lf), as<double>(linv), vinfo() + 0, 0.0);
  }
  // wait for the stream, then the verdicts of the factorisations (out: host copy of vsmall)
  // (kind: whose factorisations these are -- the names in a failure's message)
  int vgp_finish(double** out, Post kind = Post::Vgp) {
    double* host = ctx->pinned_scratch(kVgpSmall);
    if (!host) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    HIPCHECK(hipMemcpyAsync(host, vsmall.p, kVgpSmall * 8, hipMemcpyDeviceToHost, st()));
    HIPCHECK(ctx->wait(st()));
    int rc = launch_status();
    if (rc) return rc;
    int info[4];
    std::memcpy(info, host + kVgpInfoAt, sizeof(info));
    static const char* what[4] = {"k(X, X) + 1e-6 I", "the natural parameter Lambda", "the covariance S S^T of q",
                                  "I - S S^T (reversed order)"};
    static const char* what_sgpr[4] = {"Kuu = k(Z, Z) + 1e-6 I", "B = I + A A^T", "(unused)", "I - B^-1 (reversed order)"};
    static const char* what_svgp[4] = {"Kuu = k(Z, Z) + 1e-6 I", "the natural parameter Lambda", "the covariance S S^T of q",
                                       "I - S S^T (reversed order)"};
    for (int q = 0; q < 4; ++q)
      if (info[q] != INT_MAX)
        return ctx->fail(GPSO_E_NOTPD, "%s is not positive definite: Cholesky failed at pivot %d",
                         (kind == Post::Svgp ? what_svgp : kind == Post::Sgpr ? what_sgpr : what)[q], info[q]);
    *out = host;
    return GPSO_OK;
  }
  void vgp_reset_info() {
    for (int q = 0; q < 4; ++q) launch_vgp_pad_identity(st(), nullptr, 0, 0, vinfo() + q);  // (INT_MAX; no matrix)
  }

  int vgp_set_q(const double* mu, const double* S, int64_t n_) override {
    if (sizeof(TF) != 8) return ctx->fail(GPSO_E_ARG, "the variational GP needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context");
    if (!res.have_data) return ctx->fail(GPSO_E_STATE, "gpso_vgp_set_q before gpso_set_data");
    if (n_ != n) return ctx->fail(GPSO_E_ARG, "q of %lld points for training data of %lld", (long long)n_, (long long)n);
    int rc = vgp_begin();
    if (rc) return rc;
    if (mu == nullptr || S == nullptr) {  // NULL: the prior
      vgp_prior();
      HIPCHECK(ctx->wait(st()));
      return launch_status();
    }
    if ((rc = ensure(getter_tmp, (size_t)n * n * 8 + (size_t)n * 8))) return rc;
    double* tmp = as<double>(getter_tmp);
    hipStream_t s = st();
    HIPCHECK(hipMemcpyAsync(tmp, S, (size_t)n * n * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(vq_mu.p, 0, (size_t)npad * 8, s));
    HIPCHECK(hipMemcpyAsync(vq_mu.p, mu, (size_t)n * 8, hipMemcpyHostToDevice, s));
    launch_vgp_pad_identity(s, as<double>(vq_S), 0, npad, nullptr);
    launch_convert_in<double>(s, tmp, as<double>(vq_S), n, n, npad);
    launch_vgp_clean_lower(s, as<double>(vq_S), as<double>(vq_S), n, npad, 1.0);
    HIPCHECK(hipStreamSynchronize(s));  // (the caller's host buffers are free again on return)
    vq_n = n;
    vq_npad = npad;
    return launch_status();
  }
  // data that grew behind the rows q was made for (the caller keeps those rows first, in the same order): q keeps its
  // leading block and takes the prior (mu = 0, an identity block of S) for the new rows -- on the device, no host copy.
  // Inside one padded size the padding of q already IS that prior; a new padded size re-lays the leading block out.
  int vgp_extend_q() override {
    if (sizeof(TF) != 8) return ctx->fail(GPSO_E_ARG, "the variational GP needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context");
    if (!res.have_data) return ctx->fail(GPSO_E_STATE, "gpso_vgp_extend_q before gpso_set_data");
    if (vq_n < 1 || vq_n > n) return ctx->fail(GPSO_E_STATE, "no variational state of at most %lld rows to extend", (long long)n);
    int rc = refuse_if_async("gpso_vgp_extend_q");
    if (rc) return rc;
    hipStream_t s = st();
    if (vq_npad != npad) {
      DevBuf nS, nmu;  // (an early return frees them: q stays as it was)
      if ((rc = ensure(nS, (size_t)npad * npad * 8))) return rc;
      if ((rc = ensure(nmu, (size_t)npad * 8))) return rc;
      launch_vgp_pad_identity(s, as<double>(nS), 0, npad, nullptr);
      HIPCHECK(hipMemsetAsync(nmu.p, 0, (size_t)npad * 8, s));
      HIPCHECK(hipMemcpy2DAsync(nS.p, (size_t)npad * 8, vq_S.p, (size_t)vq_npad * 8, (size_t)vq_n * 8, (size_t)vq_n,
                                hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipMemcpyAsync(nmu.p, vq_mu.p, (size_t)vq_n * 8, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipStreamSynchronize(s));
      vq_S = std::move(nS);
      vq_mu = std::move(nmu);
    }
    vq_n = n;
    vq_npad = npad;
    HIPCHECK(ctx->wait(s));
    return launch_status();
  }
  int vgp_get_q(double* mu, double* S) override {
    if (vq_n != n || vq_npad != npad || vq_n < 1) return ctx->fail(GPSO_E_STATE, "no variational state for the resident data");
    int rc;
    if ((rc = ensure(getter_tmp, (size_t)n * n * 8 + (size_t)n * 8))) return rc;
    double* tmp = as<double>(getter_tmp);
    hipStream_t s = st();
    if (S) {
      launch_convert_out<double>(s, as<double>(vq_S), npad, tmp, n, n, 0);
      HIPCHECK(hipMemcpyAsync(S, tmp, (size_t)n * n * 8, hipMemcpyDeviceToHost, s));
    }
    if (mu) HIPCHECK(hipMemcpyAsync(mu, vq_mu.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return launch_status();
  }

  // the update of q = N(qmu, qS qS^T) from the step's natural parameters Lambda* (vA, destroyed; identity padding) and h*
  // (vvec kVgpH), at the context's size n: gamma-mixing with q's current natural parameters (Lambda = S^-T S^-1, h =
  // Lambda mu), then GPflow's natural_to_meanvarsqrt into (mu_out, S_out); the verdicts in vinfo() 1 and 2
  int vgp_natural_update(const double* qmu, const double* qS, double gamma, double* mu_out, double* S_out) {
    hipStream_t s = st();
    double *A = as<double>(vA), *B = as<double>(vB), *Cm = as<double>(vC);
    double *h = vvec_at(kVgpH), *h2 = vvec_at(kVgpH2);
    int rc;
    if (gamma != 1.0) {
      // the current natural parameters: Lambda = S^-T S^-1, h = Lambda mu
      HIPCHECK(hipMemsetAsync(Cm, 0, (size_t)npad * npad * 8, s));
      launch_install_chol<double>(s, qS, npad, npad, B, Cm);
      launch_trtri<double>(s, B, Cm, as<double>(work), npad, kFitBlock);
      launch_vgp_clean_lower(s, Cm, Cm, n, npad, 0.0);
      launch_dgemm(s, Cm, true, Cm, false, B, npad, 1.0, 0.0);
      launch_vgp_gemv(s, B, false, qmu, 0.0, 1.0, 0.0, nullptr, h2, n, npad);
      launch_vgp_axpby(s, B, A, npad * npad, 1.0 - gamma, gamma);
      launch_vgp_axpby(s, h2, h, npad, 1.0 - gamma, gamma);
    }
    launch_vgp_pad_identity(s, A, n, npad, vinfo() + 1);
    // V = chol(Lambda)^-1, Sigma = V^T V, mu = Sigma h, S = chol(Sigma)
    if ((rc = vgp_chol(A, B, Cm, vinfo() + 1, 0.0))) return rc;
    launch_dgemm(s, Cm, true, Cm, false, A, npad, 1.0, 0.0);
    launch_vgp_gemv(s, A, false, h, 0.0, 1.0, 0.0, nullptr, mu_out, n, npad);
    launch_vgp_pad_identity(s, A, n, npad, vinfo() + 2);
    return vgp_chol(A, S_out, Cm, vinfo() + 2, 1.0);
  }

  // one natural-gradient step on q at theta (GPflow's NaturalGradient with a conjugate likelihood, gamma in (0, 1])
  int vgp_natgrad(const Theta& th, double gamma) override {
    const double s2 = th.lik, mean_c = th.mean_c;
    if (!(gamma > 0.0 && gamma <= 1.0)) return ctx->fail(GPSO_E_ARG, "natural-gradient step %g outside (0, 1]", gamma);
    int rc = vgp_begin();
    if (rc) return rc;
    hipStream_t s = st();
    vgp_reset_info();
    if ((rc = vgp_factor(th))) return rc;
    double *L = as<double>(Lf), *A = as<double>(vA), *B = as<double>(vB), *h = vvec_at(kVgpH);
    const bool general = vlik_kind != GPSO_LIK_GAUSSIAN;
    if (!general) {
      launch_vgp_pad_identity(s, A, 0, npad, nullptr);          // A := I
      launch_dgemm(s, L, true, L, false, A, npad, 1.0 / s2, 1.0);  // Lambda* = I + L^T L / s2
      launch_vgp_gemv(s, L, true, as<double>(y64), mean_c, 1.0 / s2, 0.0, nullptr, h, n, npad);  // h* = L^T (y - c) / s2
    } else {
      // the per-point derivatives at the current q (s2: the likelihood's parameter), then
      // Lambda* = I + L^T diag(a) L and h* = L^T (gm + a (m - c))
      vgp_quadrature(L, A, s2, mean_c);
      launch_vgp_rowscale(s, L, lvec_at(kLikA), B, n, npad);
      launch_vgp_pad_identity(s, A, 0, npad, nullptr);
      launch_dgemm(s, L, true, B, false, A, npad, 1.0, 1.0);
      launch_vgp_gemv(s, L, true, lvec_at(kLikT), 0.0, 1.0, 0.0, nullptr, h, n, npad);
    }
    // GPflow's natural_to_meanvarsqrt: V = chol(Lambda)^-1, Sigma = V^T V, mu = Sigma h, S = chol(Sigma)
    // (a general likelihood builds the new q in scratch -- mu in its vector, S in the Gram's buffer, free by now -- and
    // commits it only when every factorisation held: GPflow's natgrad assigns nothing when natural_to_meanvarsqrt fails)
    double* mu_out = general ? lvec_at(kLikMu) : as<double>(vq_mu);
    double* S_out = general ? as<double>(K) : as<double>(vq_S);
    if ((rc = vgp_natural_update(as<double>(vq_mu), as<double>(vq_S), gamma, mu_out, S_out))) return rc;
    double* host;
    if ((rc = vgp_finish(&host))) {
      if (!general) vgp_prior();  // (a failed Gaussian step leaves q at the prior, not half written; a general one: q as it was)
      return rc;
    }
    if (general) {
      HIPCHECK(hipMemcpyAsync(vq_mu.p, mu_out, (size_t)npad * 8, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipMemcpyAsync(vq_S.p, S_out, (size_t)npad * npad * 8, hipMemcpyDeviceToDevice, s));
      HIPCHECK(ctx->wait(s));
      return launch_status();
    }
    return GPSO_OK;
  }

  // -ELBO at fixed q and its gradient in the constrained theta: grad[n_ls + 3] = (ls..., variance, s2, c)
  int vgp_elbo(const Theta& th, double* loss, double* grad) override {
    const double s2 = th.lik, mean_c = th.mean_c;
    int rc = vgp_begin();
    if (rc) return rc;
    hipStream_t s = st();
    vgp_reset_info();
    if ((rc = vgp_factor(th))) return rc;
    double *L = as<double>(Lf), *Li = as<double>(linv), *A = as<double>(vA), *B = as<double>(vB), *Cm = as<double>(vC);
    double *Sq = as<double>(vq_S), *mu = as<double>(vq_mu), *r = vvec_at(kVgpR);
    const bool general = vlik_kind != GPSO_LIK_GAUSSIAN;
    if (!general) {
      launch_vgp_gemv(s, L, false, mu, 0.0, 1.0, mean_c, as<double>(y64), r, n, npad);  // r = y - (L mu + c)
      launch_dgemm(s, L, false, Sq, false, A, npad, 1.0, 0.0);                           // L S
      launch_vgp_rownorm(s, A, vvec_at(kVgpFvar), n, npad);                              // fvar
      launch_vgp_rownorm(s, Sq, vvec_at(kVgpSrow), n, npad);
      launch_dgemm(s, A, false, Sq, true, B, npad, 1.0, 0.0);                            // L Sigma = (L S) S^T
      launch_vgp_elbo_sums(s, r, vvec_at(kVgpFvar), mu, vvec_at(kVgpSrow), Sq, n, npad, as<double>(vsmall));
    } else {
      vgp_quadrature(L, A, s2, mean_c);                                                  // A = L S; gm, a, VE, dVE/dp
      launch_vgp_rownorm(s, Sq, vvec_at(kVgpSrow), n, npad);
      launch_dgemm(s, A, false, Sq, true, B, npad, 1.0, 0.0);                            // L Sigma
      launch_vgp_lik_sums(s, lvec_at(kLikVe), lvec_at(kLikDve), lvec_at(kLikGm), mu, vvec_at(kVgpSrow), Sq, n, npad,
                          as<double>(vsmall));
    }
    if (grad) {
      if (!general) launch_vgp_lbar(s, B, r, mu, n, npad, 1.0 / s2);   // Lbar
      else launch_vgp_lbar_w(s, B, lvec_at(kLikA), lvec_at(kLikGm), mu, n, npad);  // Lbar = tril(diag(a) L Sigma - gm mu^T)
      launch_dgemm(s, L, true, B, false, Cm, npad, 1.0, 0.0);          // P = L^T Lbar
      launch_vgp_phi_sym(s, Cm, A, n, npad);                           // M = Phi(P) + Phi(P)^T
      launch_dgemm(s, A, false, Li, false, B, npad, 1.0, 0.0);         // M L^-1
      launch_dgemm(s, Li, true, B, false, Cm, npad, 1.0, 0.0);         // 2 Kbar = L^-T M L^-1
      HIPCHECK(hipMemsetAsync(vvec_at(kVgpZero), 0, (size_t)npad * 8, s));
      // the NLML gradient's contraction with K^-1 := 2 Kbar and alpha := 0: W = Kbar, sum_ij Kbar_ij dK_ij / dtheta
      launch_gradient<double>(s, Li, vvec_at(kVgpZero), as<double>(xs64), as<double>(xnorm64), n, npad, d, dp, n_ls, ls_dev(),
                              kp, Cm, true, as<double>(gpart), as<double>(vsmall) + kVgpGradAt, nullptr);
    }
    double* host;
    if ((rc = vgp_finish(&host))) return rc;
    const double N = (double)n;
    if (general) {  // -sum VE + KL; d/dp = -sum dVE/dp, d/dc = -sum gm
      *loss = -host[0] + 0.5 * (host[4] + host[3] - N - host[5]);
      if (grad) {
        for (int k = 0; k <= n_ls; ++k) grad[k] = host[kVgpGradAt + k];
        grad[n_ls + 1] = -host[1];
        grad[n_ls + 2] = -host[2];
      }
      return GPSO_OK;
    }
    const double data = 0.5 * N * std::log(2.0 * M_PI * s2) + (host[1] + host[2]) / (2.0 * s2);
    const double kl = 0.5 * (host[4] + host[3] - N - host[5]);
    *loss = data + kl;
    if (grad) {
      for (int k = 0; k <= n_ls; ++k) grad[k] = host[kVgpGradAt + k];  // lengthscales..., kernel variance
      grad[n_ls + 1] = N / (2.0 * s2) - (host[1] + host[2]) / (2.0 * s2 * s2);
      grad[n_ls + 2] = -host[0] / s2;
    }
    return GPSO_OK;
  }

  // install under a quadrature likelihood: G = chol J (I - Sigma / (1 + delta)) J into vC (G^-1 in vA), with the
  // smallest delta of 0, 1e-8, 2e-8, 4e-8, ... <= 1 that makes it positive definite.  A non-log-concave likelihood (the
  // Student-t: a < 0 in its tails) can leave Sigma above I in a direction, where the predict kernels' one-term form
  // k** - |C k*|^2 cannot hold var_f exactly; the install then serves k** - k*^T L^-T ((1 + delta) I - Sigma) L^-1 k*
  // + delta k**, i.e. var_f + delta (k** - |L^-1 k*|^2), in [var_f, var_f + delta k**].
  int vgp_shifted_root(double* delta_out, bool sigma_ready = false /* K already holds Sigma (the SGPR install: B^-1) */,
                       const double* qS = nullptr /* the root of Sigma when it is not the VGP's (the SVGP's q) */) {
    hipStream_t s = st();
    double *A = as<double>(vA), *B = as<double>(vB), *Cm = as<double>(vC), *Sig = as<double>(K);
    if (!qS) qS = as<double>(vq_S);
    if (!sigma_ready) launch_dgemm(s, qS, false, qS, true, Sig, npad, 1.0, 0.0);  // Sigma (K is free here)
    int* host = reinterpret_cast<int*>(ctx->pinned_scratch(kVgpSmall));
    if (!host) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    for (double delta = 0.0; delta <= 1.0; delta = (delta == 0.0 ? 1.0e-8 : 2.0 * delta)) {
      HIPCHECK(hipMemsetAsync(A, 0, (size_t)npad * npad * 8, s));
      launch_vgp_axpby(s, Sig, A, npad * npad, 1.0 / (1.0 + delta), 0.0);
      launch_vgp_reverse(s, A, B, n, npad, 0, vinfo() + 3);
      int rc = vgp_chol(B, Cm, A, vinfo() + 3, 0.0);
      if (rc) return rc;
      HIPCHECK(hipMemcpyAsync(host, vinfo(), 4 * sizeof(int), hipMemcpyDeviceToHost, s));
      HIPCHECK(ctx->wait(s));
      if ((rc = launch_status())) return rc;
      if (host[0] != INT_MAX || (sigma_ready && host[1] != INT_MAX) || host[3] == INT_MAX) {  // (a Gram -- or the SGPR's B -- that failed is vgp_finish's to report)
        *delta_out = delta;
        return GPSO_OK;
      }
    }
    return ctx->fail(GPSO_E_NOTPD, sigma_ready ? "I - B^-1: no shift delta <= 1 makes it positive definite"
                                               : "I - S S^T: no shift delta <= 1 makes it positive definite (q far above the prior)");
  }

  // install the predictive at theta: L^-1 := C = R L^-1 (I - S S^T = R^T R), alpha := L^-T mu, noise := s2, mean := c --
  // every predict path then serves the VGP unchanged
  int vgp_posterior(const Theta& th) override {
    const double s2 = th.lik;
    int rc = vgp_begin();
    if (rc) return rc;
    hipStream_t s = st();
    vgp_reset_info();
    if ((rc = vgp_factor(th))) return rc;
    double *Li = as<double>(linv), *A = as<double>(vA), *B = as<double>(vB), *Cm = as<double>(vC), *Sq = as<double>(vq_S);
    launch_vgp_gemv(s, Li, true, as<double>(vq_mu), 0.0, 1.0, 0.0, nullptr, as<double>(alpha_f), n, npad);  // beta
    if (vlik_kind == GPSO_LIK_GAUSSIAN) {
      launch_dgemm(s, Sq, false, Sq, true, A, npad, 1.0, 0.0);        // Sigma
      launch_vgp_reverse(s, A, B, n, npad, 0, vinfo() + 3);           // J (I - Sigma) J
      if ((rc = vgp_chol(B, Cm, A, vinfo() + 3, 0.0))) return rc;     // G
      launch_vgp_reverse(s, Cm, B, n, npad, 1, nullptr);              // R = J G^T J
      launch_dgemm(s, B, false, Li, false, A, npad, 1.0, 0.0);        // C = R L^-1
      HIPCHECK(hipMemcpyAsync(Li, A, (size_t)npad * npad * 8, hipMemcpyDeviceToDevice, s));
      if ((rc = set_theta(th))) return rc;
    } else {
      double shift = 0.0;
      if ((rc = vgp_shifted_root(&shift))) return rc;                 // G of J (I - Sigma / (1 + delta)) J
      launch_vgp_reverse(s, Cm, B, n, npad, 1, nullptr);              // R
      launch_dgemm(s, B, false, Li, false, A, npad, std::sqrt(1.0 + shift), 0.0);  // C = sqrt(1 + delta) R L^-1
      HIPCHECK(hipMemcpyAsync(Li, A, (size_t)npad * npad * 8, hipMemcpyDeviceToDevice, s));
      // the likelihood's variance in the predictive: scale^2 df / (df - 2) (Student-t, closed form) or s2; + delta k**
      const double noise = vlik_kind == GPSO_LIK_STUDENT_T ? s2 * s2 * vlik_df / (vlik_df - 2.0) : s2;
      if ((rc = set_theta(th.with_lik(noise + shift * th.variance)))) return rc;
    }
    return install_predictive(Post::Vgp);
  }
  // what the three variational installs share once linv holds C and alpha_f holds beta: the predict-ready copies, the
  // factorisations' verdicts, and the posterior's kind
  int install_predictive(Post kind) {
    hipStream_t s = st();
    int rc;
    double* host;
    launch_pack_linv<TF, TP>(s, as<TF>(linv), n, npad, as<TP>(linv_p));
    launch_convert_vec<TF, TP>(s, as<TF>(alpha_f), as<TP>(alpha), npad);
    if (!(rc = pack_bf16())) rc = vgp_finish(&host, kind);
    res.variational_ready(kind, rc == GPSO_OK);
    return rc;
  }


  // ---- sparse GP regression on inducing points (GPflow 2 SGPR, Gaussian likelihood, Z fixed) --------
  // gpso_sgpr_set_inducing / gpso_sgpr_select_inducing move the training data (N rows) into buffers of their own (sgX raw,
  // sgY) and make Z the context's resident rows (n = M): Kuu, its factor and everything M x M then run through the fit's
  // buffers and kernels at size M_pad exactly as the VGP's do at N_pad, the installed predictive is a posterior over the M
  // rows Z that every predict path serves, and the rectangular [M_pad x N_pad] work lives in sgKuf / sgA / sgW.
  DevBuf sgX, sgY, sgXs, sgXn, sgKuf, sgA, sgW, sgPart, sgM1, sgM2, sgM3, sgvecN, sgvecM, sgsmall, sggpart, sgidx;
  DevBuf sgZpart, sgZg;  // the moving-Z evaluations' slice partials and dF/dZ [M x D] (inducing.hip)
  std::vector<double> sg_xh;  // host mirror of the training inputs (the rows greedy selection gathers Z from)
  int64_t sg_n = 0, sg_npad = 0;
  enum { kSgE = 0, kSgW = 1, kSgT = 2, kSgVecsN = 3 };
  enum { kSgAe = 0, kSgCv = 1, kSgMu = 2, kSgAvec = 3, kSgRows = 4, kSgZero = 5, kSgVecsM = 6 };
  static constexpr int kSgGradAt = 16, kSgSmall = kSgGradAt + kGradMaxLs + 1;
  double* sgn_at(int k) const { return as<double>(sgvecN) + (size_t)k * sg_npad; }
  double* sgm_at(int k) const { return as<double>(sgvecM) + (size_t)k * npad; }

  int sgpr_need_f64() {
    if (sizeof(TF) != 8) return ctx->fail(GPSO_E_ARG, "SGPR needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context");
    return GPSO_OK;
  }
  // the resident rows are the caller's data: keep them as the SGPR's training set
  int sgpr_stash() {
    if (res.sg_have) return GPSO_OK;
    if (!res.have_data) return ctx->fail(GPSO_E_STATE, "SGPR call before gpso_set_data");
    int rc;
    sg_n = n;
    sg_npad = npad;  // (a multiple of 128: the tile GEMM's k and n extents)
    if ((rc = ensure(sgX, (size_t)sg_npad * d * 8))) return rc;
    if ((rc = ensure(sgY, (size_t)sg_npad * 8))) return rc;
    HIPCHECK(hipMemcpyAsync(sgX.p, x64.p, (size_t)sg_n * d * 8, hipMemcpyDeviceToDevice, st()));
    HIPCHECK(hipMemcpyAsync(sgY.p, y64.p, (size_t)sg_n * 8, hipMemcpyDeviceToDevice, st()));
    HIPCHECK(hipStreamSynchronize(st()));
    sg_xh = x_host;
    res.stashed();
    return GPSO_OK;
  }

  int sgpr_set_inducing(const double* Z, int64_t m) override {
    int rc = sgpr_need_f64();
    if (rc) return rc;
    if (!Z) return ctx->fail(GPSO_E_ARG, "Z must not be NULL");
    if (m < 1 || m > 65536) return ctx->fail(GPSO_E_ARG, "m=%lld outside [1, 65536]", (long long)m);
    if (!res.sg_have && !res.have_data) return ctx->fail(GPSO_E_STATE, "gpso_sgpr_set_inducing before gpso_set_data");
    if ((rc = refuse_if_async("gpso_sgpr_set_inducing"))) return rc;
    for (int64_t e = 0; e < m * (int64_t)d; ++e)
      if (!std::isfinite(Z[e])) return ctx->fail(GPSO_E_ARG, "Z holds a non-finite value at element %lld", (long long)e);
    if ((rc = sgpr_stash())) return rc;
    std::vector<double> zeros((size_t)m, 0.0), zc(Z, Z + (size_t)m * d);  // (Z may alias the mirror set_data overwrites)
    rc = put_rows(zc.data(), zeros.data(), m, d, true);
    if (rc) {  // (a HIP / allocation failure: the arguments were checked above.  The resident rows are unknown now)
      res.rows_unknown();
      return rc;
    }
    svq_m = -1;  // (the SVGP's q restarts at the prior on the new Z)
    return GPSO_OK;
  }

  int sgpr_select_inducing(const Theta& th, int64_t m, int64_t* idx_out) override {
    int rc = sgpr_need_f64();
    if (rc) return rc;
    if (!res.sg_have && !res.have_data) return ctx->fail(GPSO_E_STATE, "gpso_sgpr_select_inducing before gpso_set_data");
    if ((rc = refuse_if_async("gpso_sgpr_select_inducing"))) return rc;
    const int64_t N = res.sg_have ? sg_n : n;
    if (m < 1 || m > N) return ctx->fail(GPSO_E_ARG, "m=%lld outside [1, N=%lld]", (long long)m, (long long)N);
    if ((rc = theta_status(theta_refusal(th, d, false)))) return rc;
    // (from here on the call replaces whatever posterior was resident: the hyper block is the selection's)
    res.selection_begun();
    if ((rc = set_theta(th.with_lik(kVgpJitter)))) return rc;
    if ((rc = sgpr_stash())) return rc;
    if ((rc = ensure(sgXs, (size_t)sg_npad * dp * 8))) return rc;
    if ((rc = ensure(sgXn, (size_t)sg_npad * 8))) return rc;
    if ((rc = ensure(sgW, (size_t)m * sg_npad * 8))) return rc;
    if ((rc = ensure(sgvecN, (size_t)kSgVecsN * sg_npad * 8))) return rc;
    if ((rc = ensure(sgsmall, kSgSmall * 8))) return rc;
    if ((rc = ensure(sgidx, (size_t)m * 8))) return rc;
    hipStream_t s = st();
    launch_scale_x<double>(s, as<double>(sgX), sg_n, sg_npad, d, dp, ls_dev(), as<double>(sgXs), as<double>(sgXn), nullptr);
    launch_sgpr_greedy(s, as<double>(sgXs), sg_n, sg_npad, dp, kp, (int)m, as<double>(sgW), sgn_at(0), as<double>(sgsmall),
                       as<int64_t>(sgidx));
    std::vector<int64_t> idx((size_t)m);
    HIPCHECK(hipMemcpyAsync(idx.data(), sgidx.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if ((rc = launch_status())) return rc;
    std::vector<double> Z((size_t)m * d);
    for (int64_t j = 0; j < m; ++j) {
      if (idx[j] == -1)
        return ctx->fail(GPSO_E_NOTPD, "greedy selection: k(X, X) is numerically of rank %lld < m=%lld at these hyper-parameters "
                         "(the largest remaining conditional variance is below 1e-12 of the kernel variance): ask for fewer inducing points",
                         (long long)j, (long long)m);
      if (idx[j] < 0 || idx[j] >= sg_n) return ctx->fail(GPSO_E_HIP, "greedy selection returned row %lld of %lld", (long long)idx[j], (long long)sg_n);
      std::memcpy(&Z[(size_t)j * d], &sg_xh[(size_t)idx[j] * d], (size_t)d * 8);
    }
    if (idx_out) std::memcpy(idx_out, idx.data(), (size_t)m * 8);
    return sgpr_set_inducing(Z.data(), m);
  }

  int sgpr_get_inducing(double* Z, int64_t* m_out, int64_t* n_data_out) override {
    if (!res.sg_have || !res.sg_have_z) return ctx->fail(GPSO_E_STATE, "no inducing points set (gpso_sgpr_set_inducing / gpso_sgpr_select_inducing)");
    if (m_out) *m_out = n;
    if (n_data_out) *n_data_out = sg_n;
    if (Z) std::memcpy(Z, x_host.data(), (size_t)n * d * 8);
    return GPSO_OK;
  }

  // the intermediates of the last successful gpso_sgpr_bound_u, for checks against a reference
  int sgpr_get_factor(int which, double* out) override {
    if (!out) return ctx->fail(GPSO_E_ARG, "out must not be NULL");
    if (which < GPSO_SGPR_KUF || which > GPSO_SGPR_CV) return ctx->fail(GPSO_E_ARG, "unknown SGPR factor id %d", which);
    if (!res.sg_have || !res.sg_have_z || !res.sg_factors)
      return ctx->fail(GPSO_E_STATE, "gpso_sgpr_get_factor: no gpso_sgpr_bound_u result resident (any later call but a getter drops it)");
    int rc = refuse_if_async("gpso_sgpr_get_factor");
    if (rc) return rc;
    const double* src = which == GPSO_SGPR_KUF ? as<double>(sgKuf) : which == GPSO_SGPR_LU ? as<double>(Lf)
                        : which == GPSO_SGPR_LB ? as<double>(vC) : sgm_at(kSgCv);
    const int64_t rows = n, cols = which == GPSO_SGPR_KUF ? sg_n : which == GPSO_SGPR_CV ? 1 : n;
    const int64_t ld = which == GPSO_SGPR_KUF ? sg_npad : which == GPSO_SGPR_CV ? 1 : npad;
    HIPCHECK(hipMemcpy2DAsync(out, (size_t)cols * 8, src, (size_t)ld * 8, (size_t)cols * 8, (size_t)rows, hipMemcpyDeviceToHost, st()));
    HIPCHECK(hipStreamSynchronize(st()));
    return GPSO_OK;
  }

  // Lu (Lf), Lu^-1 (linv), Kuf, A, A A^T (vA), LB (vC), LB^-1 (sgM2), e, A e, cv at theta; the verdicts in vinfo() 0 and 1
  int sgpr_factor(const Theta& th, const char* who) {
    const double s2 = th.lik, mean_c = th.mean_c;
    int rc = sgpr_need_f64();
    if (rc) return rc;
    if (!res.sg_have || !res.sg_have_z)
      return ctx->fail(GPSO_E_STATE, "%s needs the data and the inducing points: gpso_set_data, then gpso_sgpr_set_inducing or gpso_sgpr_select_inducing", who);
    // (what set_theta would refuse, refused here: a rejected call leaves the resident posterior as it was)
    if ((rc = theta_status(theta_refusal(th, d, true), "noise variance"))) return rc;
    if ((rc = vgp_begin(true))) return rc;
    if ((rc = sparse_workspace(false))) return rc;
    const int nsplit = sparse_nsplit();
    hipStream_t s = st();
    vgp_reset_info();
    if ((rc = vgp_factor(th))) return rc;  // Kuu = k(Z, Z) + 1e-6 I, Lu, Lu^-1
    const double sig = std::sqrt(s2);
    double *Li = as<double>(linv), *Kuf = as<double>(sgKuf), *A = as<double>(sgA);
    launch_scale_x<double>(s, as<double>(sgX), sg_n, sg_npad, d, dp, ls_dev(), as<double>(sgXs), as<double>(sgXn), nullptr);
    launch_sgpr_cross_gram(s, as<double>(xs64), as<double>(sgXs), n, npad, sg_n, sg_npad, dp, kp, Kuf);
    launch_dgemm_rect(s, Li, npad, 1, Kuf, sg_npad, 1, A, sg_npad, npad, sg_npad, npad, 1.0 / sig, 0.0);  // A = Lu^-1 Kuf / sigma
    // A A^T: the long-K product, split along N into nsplit partial products summed in a fixed order
    launch_dgemm_rect(s, A, sg_npad, 1, A, 1, sg_npad, as<double>(sgPart), npad, npad, npad, sg_npad, 1.0, 0.0, nsplit);
    launch_sgpr_splitk_sum(s, as<double>(sgPart), nsplit, n, npad, as<double>(vA), as<double>(vB), vinfo() + 1);
    if ((rc = vgp_chol(as<double>(vB), as<double>(vC), as<double>(sgM2), vinfo() + 1, 0.0))) return rc;  // LB, LB^-1
    launch_sgpr_resid(s, as<double>(sgY), mean_c, sgn_at(kSgE), sg_n, sg_npad);
    launch_sgpr_gemv(s, A, false, sgn_at(kSgE), 1.0, sgm_at(kSgAe), n, npad, sg_n, sg_npad);
    launch_vgp_gemv(s, as<double>(sgM2), false, sgm_at(kSgAe), 0.0, 1.0 / sig, 0.0, nullptr, sgm_at(kSgCv), n, npad);
    return GPSO_OK;
  }

  int sgpr_bound(const Theta& th, double* loss, double* grad) override {
    return sgpr_bound_impl(th, loss, grad, nullptr, "gpso_sgpr_bound_u");
  }

  // grad_z (nullable, with grad): also d(-F)/dZ [M * D], from the weights the theta gradient has just formed
  int sgpr_bound_impl(const Theta& th, double* loss, double* grad, double* grad_z, const char* who) {
    const double variance = th.variance, s2 = th.lik;
    int rc = sgpr_factor(th, who);
    if (rc) return rc;
    if (grad_z && (rc = inducing_buffers())) return rc;
    hipStream_t s = st();
    const double b = 1.0 / s2;
    double *Li = as<double>(linv), *Kuf = as<double>(sgKuf), *AAT = as<double>(vA), *T1 = as<double>(vB), *LB = as<double>(vC);
    double *LBi = as<double>(sgM2), *G1 = as<double>(K), *M1 = as<double>(sgM1), *M3 = as<double>(sgM3);
    if (grad) {
      launch_dgemm(s, LBi, false, Li, false, T1, npad, 1.0, 0.0);   // T1 = LB^-1 Lu^-1
      launch_vgp_gemv(s, T1, true, sgm_at(kSgCv), 0.0, s2, 0.0, nullptr, sgm_at(kSgAvec), n, npad);  // a = Q^-1 Kuf e
      launch_sgpr_gemv(s, Kuf, true, sgm_at(kSgAvec), 1.0, sgn_at(kSgW), n, npad, sg_n, sg_npad);    // w = Kfu a
      launch_dgemm(s, T1, true, T1, false, G1, npad, 1.0, 0.0);     // Q^-1
      launch_dgemm(s, Li, true, Li, false, M1, npad, 1.0, 0.0);     // Kuu^-1
      launch_vgp_axpby(s, M1, G1, npad * npad, b, -b);              // G1 = b (Kuu^-1 - Q^-1)
      launch_dgemm_rect(s, G1, npad, 1, Kuf, sg_npad, 1, as<double>(sgW), sg_npad, npad, sg_npad, npad, 1.0, 0.0);  // G1 Kuf
      launch_sgpr_tvec(s, sgn_at(kSgE), sgn_at(kSgW), b * b, -b * b * b, sgn_at(kSgT), sg_n, sg_npad);
      // dF/dKuf = G1 Kuf + a t^T, contracted with dKuf/dtheta tile by tile
      launch_sgpr_cross_grad(s, as<double>(sgW), sgm_at(kSgAvec), sgn_at(kSgT), as<double>(xs64), as<double>(sgXs), n, npad,
                             sg_n, sg_npad, dp, n_ls, ls_dev(), kp, as<double>(sggpart), as<double>(sgsmall) + kSgGradAt);
      launch_dgemm(s, AAT, false, Li, false, M1, npad, 1.0, 0.0);   // A A^T Lu^-1
      launch_dgemm(s, Li, true, M1, false, M3, npad, 1.0, 0.0);     // P = Lu^-T A A^T Lu^-1
      launch_sgpr_wuu(s, G1, M3, sgm_at(kSgAvec), b, M1, n, npad);  // -2 dF/dKuu (M1 is free again)
      HIPCHECK(hipMemsetAsync(sgm_at(kSgZero), 0, (size_t)npad * 8, s));
      // the Kuu part: the NLML gradient's contraction with K^-1 := -2 dF/dKuu and alpha := 0
      launch_gradient<double>(s, Li, sgm_at(kSgZero), as<double>(xs64), as<double>(xnorm64), n, npad, d, dp, n_ls, ls_dev(), kp,
                              M1, true, as<double>(gpart), as<double>(vsmall) + kVgpGradAt, nullptr);
      launch_vgp_rownorm(s, LBi, sgm_at(kSgRows), n, npad);
      // dF/dKuf = G1 Kuf + a t^T is of F, dF/dKuu = -M1 / 2 of F: the loss takes the cross part with -1, the Kuu part with +1
      if (grad_z && (rc = launch_inducing_grad(s, as<double>(sgW), sgm_at(kSgAvec), sgn_at(kSgT), M1, as<double>(xs64),
                                               as<double>(sgXs), n, npad, sg_n, sg_npad, d, dp, ls_dev(), kp, -1.0, 1.0,
                                               as<double>(sgZpart), as<double>(sgZg))))
        return rc;
    }
    launch_sgpr_sums(s, LB, AAT, sgm_at(kSgCv), sgn_at(kSgE), grad ? sgn_at(kSgW) : nullptr, grad ? sgm_at(kSgRows) : nullptr, n,
                     npad, sg_n, as<double>(sgsmall));
    double* host;
    if ((rc = vgp_finish(&host, Post::Sgpr))) return rc;
    double guu[kGradMaxLs + 1];
    for (int k = 0; k <= n_ls; ++k) guu[k] = grad ? host[kVgpGradAt + k] : 0.0;
    double* h = ctx->pinned_scratch(kSgSmall);
    if (!h) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    HIPCHECK(hipMemcpyAsync(h, sgsmall.p, kSgSmall * 8, hipMemcpyDeviceToHost, s));
    if (grad && grad_z) HIPCHECK(hipMemcpyAsync(grad_z, sgZg.p, (size_t)n * d * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx->wait(s));
    const double N = (double)sg_n, M = (double)n;
    const double F = -0.5 * N * std::log(2.0 * M_PI) - h[0] - 0.5 * N * std::log(s2) - 0.5 * b * h[1] + 0.5 * h[2] -
                     0.5 * N * variance * b + 0.5 * h[3];
    *loss = -F;
    res.bound_ready();
    if (grad) {
      // d(-F)/dtheta: the Kuu contraction already is of -F; the cross one is of F; Kdiag: dF/dvariance = -N b / 2
      for (int k = 0; k <= n_ls; ++k) grad[k] = guu[k] - h[kSgGradAt + k];
      grad[n_ls] += 0.5 * N * b;
      const double dF_db = 0.5 * N * s2 - 0.5 * s2 * (M - h[8]) - 0.5 * h[1] + b * h[4] - 0.5 * b * b * h[5] -
                           0.5 * N * variance + 0.5 * s2 * h[3];
      grad[n_ls + 1] = b * b * dF_db;
      grad[n_ls + 2] = -(b * h[6] - b * b * h[7]);
    }
    return GPSO_OK;
  }

  // install the predictive over the rows Z: L^-1 := C = sqrt(1 + delta) R Lu^-1 (I - B^-1 / (1 + delta) = R^T R, delta the
  // smallest of 0, 1e-8, 2e-8, ... that factors), alpha := Lu^-T LB^-T cv, noise := s2 + delta variance, mean := c
  int sgpr_posterior(const Theta& th, double* delta_out) override {
    int rc = sgpr_factor(th, "gpso_sgpr_posterior");
    if (rc) return rc;
    hipStream_t s = st();
    double *Li = as<double>(linv), *LBi = as<double>(sgM2);
    launch_vgp_gemv(s, LBi, true, sgm_at(kSgCv), 0.0, 1.0, 0.0, nullptr, sgm_at(kSgMu), n, npad);        // mu = LB^-T cv
    launch_vgp_gemv(s, Li, true, sgm_at(kSgMu), 0.0, 1.0, 0.0, nullptr, as<double>(alpha_f), n, npad);   // beta = Lu^-T mu
    launch_dgemm(s, LBi, true, LBi, false, as<double>(K), npad, 1.0, 0.0);                               // B^-1
    double shift = 0.0;
    if ((rc = vgp_shifted_root(&shift, true))) return rc;                                                // G in vC
    launch_vgp_reverse(s, as<double>(vC), as<double>(vB), n, npad, 1, nullptr);                          // R
    launch_dgemm(s, as<double>(vB), false, Li, false, as<double>(vA), npad, std::sqrt(1.0 + shift), 0.0);
    HIPCHECK(hipMemcpyAsync(Li, vA.p, (size_t)npad * npad * 8, hipMemcpyDeviceToDevice, s));
    if ((rc = set_theta(th.with_lik(th.lik + shift * th.variance)))) return rc;
    if ((rc = install_predictive(Post::Sgpr))) return rc;
    if (delta_out) *delta_out = shift;
    return GPSO_OK;
  }

  // ---- sparse variational GP on inducing points (GPflow 2 SVGP, whitened, full q_sqrt, full batch) --------
  // Z and the training data are the SGPR's (gpso_sgpr_set_inducing / gpso_sgpr_select_inducing: Z the resident rows, n = M),
  // the likelihood the VGP's (gpso_vgp_set_likelihood).  q(v) = N(mu, S S^T) over the M inducing values lives in svq_mu
  // [M_pad] and svq_S [M_pad^2] (lower; identity on the padding), made for the resident Z: a new Z restarts it at the
  // prior.  A = Lu^-1 Kuf sits in the SGPR's sgA (without its 1 / sigma); svB holds S^T A, later the cross weight g;
  // svD the column-scaled A diag(a).  The M x M work runs through the fit's and the VGP's buffers at M_pad.
  DevBuf svq_mu, svq_S, svB, svD, svvecN;
  int64_t svq_m = -1, svq_mpad = -1;  // the rows q was made for (-1: none; the next call starts q at the prior)
  enum { kSvM = 0, kSvV = 1, kSvGm = 2, kSvA = 3, kSvT = 4, kSvVe = 5, kSvDve = 6, kSvVecsN = 7 };
  double* svn_at(int k) const { return as<double>(svvecN) + (size_t)k * sg_npad; }
  // the long-K products A A^T (SGPR) and A diag(a) A^T (SVGP) are split along N into this many fixed-order partial products
  int sparse_nsplit() const {
    int ns = 1;
    while (ns < 16 && sg_npad % (256 * ns) == 0 && sg_npad / (2 * ns) >= 512) ns *= 2;
    return ns;
  }
  // the rectangular [M_pad x N_pad] and square [M_pad^2] work of an evaluation at the resident M and N.  Each family asks
  // for its own third rectangle(s) and N-vectors only: sgW / sgvecN the SGPR, svB / svD / svvecN the SVGP
  int sparse_workspace(bool svgp) {
    const size_t rect = (size_t)npad * sg_npad * 8, sq = (size_t)npad * npad * 8;
    int rc;
    if ((rc = ensure(sgKuf, rect)) || (rc = ensure(sgA, rect))) return rc;
    if (svgp) {
      if ((rc = ensure(svB, rect)) || (rc = ensure(svD, rect))) return rc;
    } else if ((rc = ensure(sgW, rect))) {
      return rc;
    }
    for (DevBuf* b : {&sgM1, &sgM2, &sgM3})
      if ((rc = ensure(*b, sq))) return rc;
    if ((rc = ensure(sgPart, sq * sparse_nsplit()))) return rc;
    if ((rc = ensure(sgXs, (size_t)sg_npad * dp * 8))) return rc;
    if ((rc = ensure(sgXn, (size_t)sg_npad * 8))) return rc;
    if ((rc = svgp ? ensure(svvecN, (size_t)kSvVecsN * sg_npad * 8) : ensure(sgvecN, (size_t)kSgVecsN * sg_npad * 8))) return rc;
    if ((rc = ensure(sgvecM, (size_t)kSgVecsM * npad * 8))) return rc;
    if ((rc = ensure(sgsmall, kSgSmall * 8))) return rc;
    return ensure(sggpart, (size_t)(npad / 64) * (sg_npad / 64) * (kGradMaxLs + 1) * 8);
  }

  int svgp_need_z(const char* who) {
    int rc = sgpr_need_f64();
    if (rc) return rc;
    if (!res.sg_have || !res.sg_have_z)
      return ctx->fail(GPSO_E_STATE, "%s needs the data and the inducing points: gpso_set_data, then gpso_sgpr_set_inducing or gpso_sgpr_select_inducing", who);
    return GPSO_OK;
  }
  void svgp_prior() {
    (void)hipMemsetAsync(svq_mu.p, 0, (size_t)npad * 8, st());
    launch_vgp_pad_identity(st(), as<double>(svq_S), 0, npad, nullptr);
    svq_m = n;
    svq_mpad = npad;
  }
  // q's buffers at the resident M; the prior when q was made for other rows
  int svgp_q() {
    int rc;
    if (svq_m == n && svq_mpad == npad) return GPSO_OK;
    if ((rc = ensure(svq_mu, (size_t)npad * 8))) return rc;
    if ((rc = ensure(svq_S, (size_t)npad * npad * 8))) return rc;
    svgp_prior();
    return GPSO_OK;
  }

  // Lu (Lf), Lu^-1 (linv) at theta; rect: also Kuf (sgKuf) and A = Lu^-1 Kuf (sgA).  The verdict of Kuu in vinfo() 0
  int svgp_begin(const Theta& th, const char* who, bool rect) {
    int rc = svgp_need_z(who);
    if (rc) return rc;
    if ((rc = theta_status(theta_refusal(th, d, true), "likelihood parameter"))) return rc;
    if ((rc = vgp_begin(true))) return rc;
    if ((rc = svgp_q())) return rc;
    if (rect && (rc = sparse_workspace(true))) return rc;
    hipStream_t s = st();
    vgp_reset_info();
    if ((rc = vgp_factor(th))) return rc;  // Kuu = k(Z, Z) + 1e-6 I, Lu, Lu^-1
    if (!rect) return GPSO_OK;
    launch_scale_x<double>(s, as<double>(sgX), sg_n, sg_npad, d, dp, ls_dev(), as<double>(sgXs), as<double>(sgXn), nullptr);
    launch_sgpr_cross_gram(s, as<double>(xs64), as<double>(sgXs), n, npad, sg_n, sg_npad, dp, kp, as<double>(sgKuf));
    launch_dgemm_rect(s, as<double>(linv), npad, 1, as<double>(sgKuf), sg_npad, 1, as<double>(sgA), sg_npad, npad, sg_npad,
                      npad, 1.0, 0.0);  // A = Lu^-1 Kuf
    return GPSO_OK;
  }

  // the moments of q(f) at the training points (fm = A^T mu + c; fv = variance - |A_j|^2 + |S^T A_j|^2 when want_v) and
  // the per-point terms of the likelihood there: gm, a = -2 dVE/dv, t = gm + a (fm - c), VE, dVE/dp (closed form for the
  // Gaussian -- gauss -- else the VGP's Gauss-Hermite kernel)
  void svgp_pointwise(double variance, double p, double mean_c, bool want_v, bool gauss) {
    hipStream_t s = st();
    double *A = as<double>(sgA), *B = want_v ? as<double>(svB) : nullptr;
    if (want_v)
      launch_dgemm_rect(s, as<double>(svq_S), 1, npad, A, sg_npad, 1, B, sg_npad, npad, sg_npad, npad, 1.0, 0.0);  // S^T A
    launch_svgp_moments(s, A, B, as<double>(svq_mu), variance, mean_c, svn_at(kSvM), svn_at(kSvV), n, sg_n, sg_npad);
    if (gauss)
      launch_svgp_gauss(s, as<double>(sgY), svn_at(kSvM), svn_at(kSvV), p, mean_c, svn_at(kSvGm), svn_at(kSvA), svn_at(kSvT),
                        svn_at(kSvVe), svn_at(kSvDve), sg_n, sg_npad);
    else
      launch_vgp_quad(s, as<double>(sgY), svn_at(kSvM), svn_at(kSvV), as<double>(vgh), vlik_n_gh, vlik_kind, p, vlik_df,
                      vlik_const(p), mean_c, svn_at(kSvGm), svn_at(kSvA), svn_at(kSvT), svn_at(kSvVe), svn_at(kSvDve), sg_n,
                      sg_npad);
  }

  // P = A diag(a) A^T (into aat) and I + P (into lam, identity padding): the long-K product in its fixed split-K order
  void svgp_adat(double* aat, double* lam) {
    hipStream_t s = st();
    const int ns = sparse_nsplit();
    launch_svgp_colscale(s, as<double>(sgA), svn_at(kSvA), as<double>(svD), n, npad, sg_n, sg_npad);  // D = A diag(a)
    launch_dgemm_rect(s, as<double>(sgA), sg_npad, 1, as<double>(svD), 1, sg_npad, as<double>(sgPart), npad, npad, npad,
                      sg_npad, 1.0, 0.0, ns);
    launch_sgpr_splitk_sum(s, as<double>(sgPart), ns, n, npad, aat, lam, nullptr);
  }

  // one natural-gradient step on q (gamma in (0, 1]): Lambda* = I + A diag(a) A^T, h* = A t at the current q, then the
  // VGP's mixing and natural_to_meanvarsqrt at size M.  conj: the Gaussian step at noise variance p whatever the likelihood
  // (the conjugate start).  The new q is built in scratch and committed only when every factorisation held: a failed
  // step returns GPSO_E_NOTPD with q exactly as it was, for every likelihood.
  int svgp_step(const Theta& th, double gamma, bool conj, const char* who) {
    const double variance = th.variance, p = th.lik, mean_c = th.mean_c;
    if (!(gamma > 0.0 && gamma <= 1.0)) return ctx->fail(GPSO_E_ARG, "natural-gradient step %g outside (0, 1]", gamma);
    int rc = svgp_begin(th, who, true);
    if (rc) return rc;
    hipStream_t s = st();
    const bool gauss = conj || vlik_kind == GPSO_LIK_GAUSSIAN;
    svgp_pointwise(variance, p, mean_c, !gauss, gauss);  // (the Gaussian's a and t do not depend on fv)
    svgp_adat(as<double>(sgM1), as<double>(vA));          // Lambda* in vA
    launch_sgpr_gemv(s, as<double>(sgA), false, svn_at(kSvT), 1.0, vvec_at(kVgpH), n, npad, sg_n, sg_npad);  // h* = A t
    double *mu_out = sgm_at(kSgMu), *S_out = as<double>(K);
    if ((rc = vgp_natural_update(as<double>(svq_mu), as<double>(svq_S), gamma, mu_out, S_out))) return rc;
    double* host;
    if ((rc = vgp_finish(&host, Post::Svgp))) return rc;
    HIPCHECK(hipMemcpyAsync(svq_mu.p, mu_out, (size_t)npad * 8, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipMemcpyAsync(svq_S.p, S_out, (size_t)npad * npad * 8, hipMemcpyDeviceToDevice, s));
    HIPCHECK(ctx->wait(s));
    return launch_status();
  }

  int svgp_natgrad(const Theta& th, double gamma) override { return svgp_step(th, gamma, false, "gpso_svgp_natgrad"); }

  int svgp_init_q(const Theta& th, double s2) override {
    if (s2 > 0.0) return svgp_step(th.with_lik(s2), 1.0, true, "gpso_svgp_init_q");
    int rc = svgp_need_z("gpso_svgp_init_q");
    if (rc || (rc = vgp_begin()) || (rc = svgp_q())) return rc;
    svgp_prior();
    HIPCHECK(ctx->wait(st()));
    return launch_status();
  }

  int svgp_set_q(const double* mu, const double* S, int64_t m) override {
    int rc = svgp_need_z("gpso_svgp_set_q");
    if (rc) return rc;
    if (m != n) return ctx->fail(GPSO_E_ARG, "q of %lld inducing values for %lld inducing points", (long long)m, (long long)n);
    if ((rc = vgp_begin()) || (rc = svgp_q())) return rc;
    hipStream_t s = st();
    if (mu == nullptr || S == nullptr) {
      svgp_prior();
      HIPCHECK(ctx->wait(s));
      return launch_status();
    }
    if ((rc = ensure(getter_tmp, (size_t)n * n * 8 + (size_t)n * 8))) return rc;
    double* tmp = as<double>(getter_tmp);
    HIPCHECK(hipMemcpyAsync(tmp, S, (size_t)n * n * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(svq_mu.p, 0, (size_t)npad * 8, s));
    HIPCHECK(hipMemcpyAsync(svq_mu.p, mu, (size_t)n * 8, hipMemcpyHostToDevice, s));
    launch_vgp_pad_identity(s, as<double>(svq_S), 0, npad, nullptr);
    launch_convert_in<double>(s, tmp, as<double>(svq_S), n, n, npad);
    launch_vgp_clean_lower(s, as<double>(svq_S), as<double>(svq_S), n, npad, 1.0);
    HIPCHECK(hipStreamSynchronize(s));  // (the caller's host buffers are free again on return)
    return launch_status();
  }

  int svgp_get_q(double* mu, double* S) override {
    int rc = svgp_need_z("gpso_svgp_get_q");
    if (rc || (rc = refuse_if_async("gpso_svgp_get_q")) || (rc = svgp_q())) return rc;
    if ((rc = ensure(getter_tmp, (size_t)n * n * 8 + (size_t)n * 8))) return rc;
    double* tmp = as<double>(getter_tmp);
    hipStream_t s = st();
    if (S) {
      launch_convert_out<double>(s, as<double>(svq_S), npad, tmp, n, n, 0);
      HIPCHECK(hipMemcpyAsync(S, tmp, (size_t)n * n * 8, hipMemcpyDeviceToHost, s));
    }
    if (mu) HIPCHECK(hipMemcpyAsync(mu, svq_mu.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return launch_status();
  }

  // -ELBO = -sum VE + KL(q || N(0, I)) at fixed q and its gradient in the constrained theta: grad[n_ls + 3] = (ls...,
  // variance, p, c).  With Abar = dELBO/dA = mu gm^T - (Sigma - I) A diag(a):  dELBO/dKuf = Lu^-T Abar = g + a' gm^T
  // (g = Lu^-T (I - Sigma) A diag(a), a' = Lu^-T mu), contracted tile by tile; d(-ELBO)/dLu = tril(Lu^-T Abar A^T) =
  // tril(T P + a' (A gm)^T) (T = Lu^-T (I - Sigma), P = A diag(a) A^T), taken to Kuu through the VGP's Cholesky backward
  // pass and the fit's contraction; the k_diag term sum dVE/dv = -sum a / 2 joins the variance.
  int svgp_elbo(const Theta& th, double* loss, double* grad) override {
    return svgp_elbo_impl(th, loss, grad, nullptr, "gpso_svgp_elbo_u");
  }

  // grad_z (nullable, with grad): also d(-ELBO)/dZ [M * D] at fixed q (whitened: q stays valid while Z moves; the k_diag
  // term does not depend on Z)
  int svgp_elbo_impl(const Theta& th, double* loss, double* grad, double* grad_z, const char* who) {
    const double variance = th.variance, p = th.lik, mean_c = th.mean_c;
    int rc = svgp_begin(th, who, true);
    if (rc) return rc;
    if (grad_z && (rc = inducing_buffers())) return rc;
    hipStream_t s = st();
    double *Sq = as<double>(svq_S), *mu = as<double>(svq_mu), *A = as<double>(sgA), *Li = as<double>(linv);
    svgp_pointwise(variance, p, mean_c, true, vlik_kind == GPSO_LIK_GAUSSIAN);
    launch_vgp_rownorm(s, Sq, sgm_at(kSgRows), n, npad);
    launch_svgp_sums(s, svn_at(kSvVe), svn_at(kSvDve), svn_at(kSvGm), svn_at(kSvA), sg_n, mu, sgm_at(kSgRows), Sq, n, npad,
                     as<double>(sgsmall));
    if (grad) {
      double *P = as<double>(sgM1), *Sig = as<double>(sgM2), *T = as<double>(vC), *X1 = as<double>(vA), *X2 = as<double>(vB);
      svgp_adat(P, as<double>(sgM3));                                   // P = A diag(a) A^T; D = A diag(a) in svD
      launch_dgemm(s, Sq, false, Sq, true, Sig, npad, 1.0, 0.0);        // Sigma
      launch_vgp_pad_identity(s, X2, 0, npad, nullptr);
      launch_vgp_axpby(s, Sig, X2, npad * npad, -1.0, 1.0);             // I - Sigma
      launch_dgemm(s, Li, true, X2, false, T, npad, 1.0, 0.0);          // T = Lu^-T (I - Sigma)
      launch_dgemm_rect(s, T, npad, 1, as<double>(svD), sg_npad, 1, as<double>(svB), sg_npad, npad, sg_npad, npad, 1.0,
                        0.0);                                           // g = T A diag(a)
      launch_vgp_gemv(s, Li, true, mu, 0.0, 1.0, 0.0, nullptr, sgm_at(kSgAvec), n, npad);  // a' = Lu^-T mu
      launch_sgpr_cross_grad(s, as<double>(svB), sgm_at(kSgAvec), svn_at(kSvGm), as<double>(xs64), as<double>(sgXs), n, npad,
                             sg_n, sg_npad, dp, n_ls, ls_dev(), kp, as<double>(sggpart), as<double>(sgsmall) + kSgGradAt);
      launch_sgpr_gemv(s, A, false, svn_at(kSvGm), -1.0, sgm_at(kSgAe), n, npad, sg_n, sg_npad);  // -A gm
      launch_dgemm(s, T, false, P, false, X1, npad, 1.0, 0.0);          // T P
      launch_vgp_lbar(s, X1, sgm_at(kSgAvec), sgm_at(kSgAe), n, npad, 1.0);  // Lbar = tril(T P + a' (A gm)^T)
      launch_dgemm(s, as<double>(Lf), true, X1, false, T, npad, 1.0, 0.0);  // Lu^T Lbar
      launch_vgp_phi_sym(s, T, X2, n, npad);                            // M = Phi + Phi^T
      launch_dgemm(s, X2, false, Li, false, X1, npad, 1.0, 0.0);        // M Lu^-1
      launch_dgemm(s, Li, true, X1, false, T, npad, 1.0, 0.0);          // 2 Kbar = Lu^-T M Lu^-1
      HIPCHECK(hipMemsetAsync(sgm_at(kSgZero), 0, (size_t)npad * 8, s));
      launch_gradient<double>(s, Li, sgm_at(kSgZero), as<double>(xs64), as<double>(xnorm64), n, npad, d, dp, n_ls, ls_dev(), kp,
                              T, true, as<double>(gpart), as<double>(vsmall) + kVgpGradAt, nullptr);
      // dELBO/dKuf = g + a' gm^T is of the ELBO, T = 2 d(-ELBO)/dKuu of the loss: -1 and +1 as in the SGPR
      if (grad_z && (rc = launch_inducing_grad(s, as<double>(svB), sgm_at(kSgAvec), svn_at(kSvGm), T, as<double>(xs64),
                                               as<double>(sgXs), n, npad, sg_n, sg_npad, d, dp, ls_dev(), kp, -1.0, 1.0,
                                               as<double>(sgZpart), as<double>(sgZg))))
        return rc;
    }
    double* host;
    if ((rc = vgp_finish(&host, Post::Svgp))) return rc;
    double guu[kGradMaxLs + 1];
    for (int k = 0; k <= n_ls; ++k) guu[k] = grad ? host[kVgpGradAt + k] : 0.0;
    double* h = ctx->pinned_scratch(kSgSmall);
    if (!h) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    HIPCHECK(hipMemcpyAsync(h, sgsmall.p, kSgSmall * 8, hipMemcpyDeviceToHost, s));
    if (grad && grad_z) HIPCHECK(hipMemcpyAsync(grad_z, sgZg.p, (size_t)n * d * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx->wait(s));
    *loss = -h[0] + 0.5 * (h[5] + h[4] - (double)n - h[6]);
    if (grad) {
      // the Kuu contraction is of -ELBO, the cross one of the ELBO; k_diag: d(-ELBO)/dvariance = -sum dVE/dv = sum a / 2
      for (int k = 0; k <= n_ls; ++k) grad[k] = guu[k] - h[kSgGradAt + k];
      grad[n_ls] += 0.5 * h[3];
      grad[n_ls + 1] = -h[1];
      grad[n_ls + 2] = -h[2];
    }
    return GPSO_OK;
  }

  // install the predictive over the rows Z: the VGP's install with L := Lu and q := the SVGP's q (C = sqrt(1 + delta) R
  // Lu^-1 with I - S S^T / (1 + delta) = R^T R, beta = Lu^-T mu, noise := the likelihood's variance + delta variance)
  int svgp_posterior(const Theta& th, double* delta_out) override {
    const double p = th.lik;
    int rc = svgp_begin(th, "gpso_svgp_posterior", false);
    if (rc) return rc;
    hipStream_t s = st();
    double *Li = as<double>(linv), *A = as<double>(vA), *B = as<double>(vB), *Cm = as<double>(vC);
    launch_vgp_gemv(s, Li, true, as<double>(svq_mu), 0.0, 1.0, 0.0, nullptr, as<double>(alpha_f), n, npad);  // beta
    double shift = 0.0;
    if ((rc = vgp_shifted_root(&shift, false, as<double>(svq_S)))) return rc;  // G of J (I - Sigma / (1 + delta)) J
    launch_vgp_reverse(s, Cm, B, n, npad, 1, nullptr);                         // R
    launch_dgemm(s, B, false, Li, false, A, npad, std::sqrt(1.0 + shift), 0.0);  // C = sqrt(1 + delta) R Lu^-1
    HIPCHECK(hipMemcpyAsync(Li, A, (size_t)npad * npad * 8, hipMemcpyDeviceToDevice, s));
    const double noise = vlik_kind == GPSO_LIK_STUDENT_T ? p * p * vlik_df / (vlik_df - 2.0) : p;
    if ((rc = set_theta(th.with_lik(noise + shift * th.variance)))) return rc;
    if ((rc = install_predictive(Post::Svgp))) return rc;
    if (delta_out) *delta_out = shift;
    return GPSO_OK;
  }

  // ---- the sparse models at a moving Z (inducing.hip) ---------------------------------------------
  // Z replaces the resident inducing rows IN PLACE: same M, the training data buffers untouched, no allocation, no upload
  // of X or y, the SVGP's q kept (it is whitened: valid at any Z).  Everything that could refuse the call is checked
  // before the rows are touched, so a rejected call leaves the context as it was.
  int inducing_buffers() {
    int rc = ensure(sgZpart, (size_t)(inducing_slices(npad, sg_npad) + 1) * npad * (dp + 1) * 8);
    if (rc) return rc;
    return ensure(sgZg, (size_t)n * d * 8);
  }
  int inducing_args(const char* who, const double* Z) {
    int rc = sgpr_need_f64();
    if (rc) return rc;
    if (!res.sg_have || !res.sg_have_z)
      return ctx->fail(GPSO_E_STATE, "%s needs the data and the inducing points: gpso_set_data, then gpso_sgpr_set_inducing or gpso_sgpr_select_inducing", who);
    if ((rc = refuse_if_async(who))) return rc;
    if (Z)
      for (int64_t e = 0; e < n * (int64_t)d; ++e)
        if (!std::isfinite(Z[e])) return ctx->fail(GPSO_E_ARG, "Z holds a non-finite value at element %lld", (long long)e);
    return GPSO_OK;
  }
  int inducing_put(const double* Z) {
    const size_t doubles = (size_t)n * d;
    double* stage = doubles <= (1u << 17) ? ctx->pinned_stage(doubles) : nullptr;
    if (stage) {
      std::memcpy(stage, Z, doubles * 8);
      HIPCHECK(hipMemcpyAsync(x64.p, stage, doubles * 8, hipMemcpyHostToDevice, st()));
    } else {
      HIPCHECK(hipMemcpyAsync(x64.p, Z, doubles * 8, hipMemcpyHostToDevice, st()));
      HIPCHECK(hipStreamSynchronize(st()));
    }
    if (Z != x_host.data()) std::memcpy(x_host.data(), Z, doubles * 8);
    // (whatever was built on the old rows is gone; the data, q and the likelihood stay)
    res.inducing_moved();
    return GPSO_OK;
  }

  int sgpr_move_inducing(const double* Z) override {
    if (!Z) return ctx->fail(GPSO_E_ARG, "Z must not be NULL");
    int rc = inducing_args("gpso_sgpr_move_inducing", Z);
    if (rc) return rc;
    return inducing_put(Z);
  }

  int sgpr_bound_z(const Theta& th, const double* Z, double* loss, double* grad, double* grad_z) override {
    int rc = inducing_args("gpso_sgpr_bound_uz", Z);
    if (rc || (rc = theta_status(theta_refusal(th, d, true), "noise variance"))) return rc;
    if (Z && (rc = inducing_put(Z))) return rc;
    return sgpr_bound_impl(th, loss, grad, grad_z, "gpso_sgpr_bound_uz");
  }

  int svgp_elbo_z(const Theta& th, const double* Z, double* loss, double* grad, double* grad_z) override {
    int rc = inducing_args("gpso_svgp_elbo_uz", Z);
    if (rc || (rc = theta_status(theta_refusal(th, d, true), "likelihood parameter"))) return rc;
    if (Z && (rc = inducing_put(Z))) return rc;
    return svgp_elbo_impl(th, loss, grad, grad_z, "gpso_svgp_elbo_uz");
  }

  // ------------------------------------------------------------------------------------------
  // leaves already on the device as raw coordinates (dtype xs_dtype) -> mean/var(/ucb) device arrays.
  // TG = generation type (double unless the context is float-predict with GPSO_GEN_F32).
  // defer (nullable): the caller's arg-max can finalise the leaves itself (launch_seg_argmax / launch_keyed_argmax with
  // a LeafFinalize) -- when the batch is ONE chunk the finalize launch is skipped and *defer says what to finalise;
  // otherwise defer->part_var stays NULL and the leaves are finalised here as before
  // are the tile kernel's event pairs recorded, and how many were (collect_tile_ms).  open: the survivors of a screened call -- the
  // pair's first event stands in front of the mean pass already, and the split launch's counters keep describing that pass
  struct TileSpan { bool timed; bool open = false; int pairs = 0; };
  int ensure_tile_events(int pairs) {
    while ((int)ctx->tile_ev.size() < 2 * pairs) {
      hipEvent_t e;
      HIPCHECK(hipEventCreate(&e));
      ctx->tile_ev.push_back(e);
    }
    return GPSO_OK;
  }
  template <typename TG>
  int score_leaves_t(const void* xs_dev, int xs_dtype, int64_t m, const AcqSpec& acq, bool want_ucb,
                     double* mean_dev, double* var_dev, double* ucb_dev, TileSpan& span, const int64_t* m_live, LeafFinalize* defer,
                     bool prepared = false /* leaves_s / lnorm already hold the scaled rows (one chunk): no prep launch */) {
    // row blocks of L^-1 = partial sums per leaf: the split-bf16 kernel always works on 256-row blocks,
    // the native kernels on the shape leaf_tiles_bm picks
    const bool use_bf16 = bf16_usable() && res.linv_b == Copy::Valid && bf16_fits(sizeof(TG) == 8);
    if (!use_bf16) {
      int rcp = ensure_linv_p();
      if (rcp) return rcp;
    }
    if (!use_bf16 && res.linv_p != Copy::Valid)
      return ctx->fail(GPSO_E_STATE, "this posterior was received with the split pieces of L^-1 only (the sender predicts with "
                                     "split math): the f32 MFMA kernel has nothing to read -- keep the sender's predict math, or "
                                     "hand the posterior over with gpso_posterior_buffers (all buffers)");
    const int nbi = use_bf16 ? (int)(npad / 256) : leaf_tiles_nbi<TP>(npad, dp / 4);
    const int64_t chunk = std::min<int64_t>(m, kLeafChunk);
    const int64_t cpad = (chunk + kLeafPad - 1) / kLeafPad * kLeafPad;
    int rc;
    if ((rc = ensure(leaves_s, (size_t)cpad * dp * sizeof(TG)))) return rc;
    if ((rc = ensure(lnorm, (size_t)cpad * sizeof(TG)))) return rc;
    if ((rc = ensure(pvar, (size_t)nbi * cpad * 8))) return rc;
    if ((rc = ensure(pmean, (size_t)nbi * cpad * 8))) return rc;
    hipStream_t s = st();
    span.pairs = 0;
    const int64_t keep_counts[3] = {ctx->last_count[3], ctx->last_count[5], ctx->last_count[6]};
    const TG* xsp = nullptr;
    const TG* xnr = nullptr;
    if constexpr (sizeof(TG) == 8) {
      xsp = as<double>(xs_p64);
      xnr = as<double>(xnorm64);
    } else {
      xsp = as<float>(xs_p32);
      xnr = as<float>(xnorm32);
    }
    // m_live counts live rows of the WHOLE batch; a batch processed in several chunks needs the count
    // per chunk (slots 1.. of live_cnt, filled on the device)
    const int nchunk = (int)((m + chunk - 1) / chunk);
    if (m_live != nullptr && nchunk > 1) {
      if ((rc = ensure_keep(live_cnt, (size_t)(1 + nchunk) * 8))) return rc;
      m_live = as<int64_t>(live_cnt);
      launch_chunk_live(s, m_live, chunk, nchunk, as<int64_t>(live_cnt) + 1);
    }
    for (int64_t off = 0; off < m; off += chunk) {
      const int64_t mc = std::min<int64_t>(chunk, m - off);
      const int64_t mp = (mc + kLeafPad - 1) / kLeafPad * kLeafPad;
      const int64_t* m_live_c = (m_live != nullptr && nchunk > 1) ? as<int64_t>(live_cnt) + 1 + off / chunk : m_live;
      // Round 5: the fp16-contraction kernels scale float leaves in their own prologue (one launch and one dependency gap
      // less per call: 12 us of a 740 us step at C3).  Only where nothing else reads the scaled copies: one chunk, all rows
      // live, the caller's leaves in float.  A NaN coordinate reaches the partial sums by itself on this path (no clamp in
      // float generation), so the finalize stage needs no norms.
      // The survivors of a screened call (span.open) are such a batch although only the device knows how many rows live: the
      // compaction leaves zero rows up to the edge of the last live leaf tile (screen.hip), the tiles behind it leave at once.
      RawLeaves rawl{};
      if constexpr (kFloatPredict && sizeof(TG) == 4) {
        if (fuse_prep && use_bf16 && !prepared && xs_dtype == GPSO_F32 && nchunk == 1 && (m_live_c == nullptr || span.open) &&
            c16_in_use(false)) {
          rawl.x = static_cast<const float*>(xs_dev) + off * d;
          rawl.ls = ls_dev();
          rawl.m = mc;
          rawl.d = d;
        }
      }
      const bool fused_prep = rawl.x != nullptr;
      if (fused_prep) {
        // (nothing to launch)
      } else if (prepared) {
        if (nchunk != 1) return ctx->fail(GPSO_E_STATE, "internal: prepared leaves in more than one chunk");
      } else {
        prep_points<TG>(s, xs_dev, xs_dtype, off, mc, mp, m_live_c, as<TG>(leaves_s), as<TG>(lnorm));
      }
      if ((rc = ensure_tile_events(span.pairs + 1))) return rc;
      if (span.timed && !span.open) HIPCHECK(hipEventRecord(ctx->tile_ev[2 * span.pairs], s));
      if (use_bf16) {
        if constexpr (kFloatPredict) {
          SplitLeafLaunch<TG> a;
          a.nsplit = nsplit(); a.linv_b = split_planes(); a.f16_inv_scale_a = f16_split() ? f16_scale() : nullptr;
          a.xs_p = xsp; a.xnorm = xnr; a.alpha = as<float>(alpha);
          a.xs_h16 = c16_in_use(sizeof(TG) == 8) ? xs_h16.p : nullptr; a.c16_scale = as<float>(c16_scal);
          a.leaves_s = as<TG>(leaves_s); a.lnorm = as<TG>(lnorm); a.raw = rawl; a.m_live = m_live_c;
          a.part_var = as<double>(pvar); a.part_mean = as<double>(pmean);
          a.npad = npad; a.dp4 = dp / 4; a.mpad = mp; a.n_rows = n;
          a.step32 = split_variant == GPSO_SPLIT_KERNEL_FUSED32; a.row_loop = row_loop; a.cu_count = ctx->cu_count;
          a.splits_out = &ctx->last_count[3];
          a.park_bytes = park_bytes; a.park_scratch = &EngineT::park_cb; a.park_owner = this; a.park_out = &ctx->last_count[5];
          rc = launch_leaf_tiles_bf16<TG>(s, kp, a, split_variant);
          if (span.open) ctx->last_count[3] = keep_counts[0], ctx->last_count[5] = keep_counts[1], ctx->last_count[6] = keep_counts[2];
        }
      } else {
        rc = launch_leaf_tiles<TP, TG>(s, as<TP>(linv_p), xsp, xnr, as<TP>(alpha), as<TG>(leaves_s),
                                       as<TG>(lnorm), as<double>(pvar), as<double>(pmean), npad, dp / 4, mp, kp,
                                       m_live_c);
      }
      if (rc) return launch_status();
      if (span.timed) HIPCHECK(hipEventRecord(ctx->tile_ev[2 * span.pairs + 1], s));
      ++span.pairs;
      if (defer != nullptr && nchunk == 1 && want_ucb) {
        *defer = LeafFinalize{as<double>(pvar), as<double>(pmean), nbi, mp, kp.variance, kp.noise, kp.mean_c, acq.varsigma,
                              mean_dev, var_dev, ucb_dev, fused_prep ? nullptr : lnorm.p, sizeof(TG) == 8}.with(acq);
        continue;
      }
      launch_leaf_finalize(s, as<double>(pvar), as<double>(pmean), nbi, mp, mc, kp, acq, mean_dev + off,
                           var_dev + off, want_ucb ? ucb_dev + off : nullptr, fused_prep ? nullptr : lnorm.p, sizeof(TG) == 8);
    }
    return launch_status();  // (no host wait here: the kernel time is read after the call's final sync)
  }

  int score_device_leaves(const void* xs_dev, int xs_dtype, int64_t m, const AcqSpec& acq, bool want_ucb,
                          double* mean_dev, double* var_dev, double* ucb_dev, TileSpan& span, const int64_t* m_live = nullptr,
                          LeafFinalize* defer = nullptr, bool prepared = false) {
    if (defer != nullptr) *defer = LeafFinalize{};
    if constexpr (kFloatPredict) {
      if (!gen_double()) {
        int rc = ensure_generation_inputs();
        if (rc) return rc;
        return score_leaves_t<float>(xs_dev, xs_dtype, m, acq, want_ucb, mean_dev, var_dev, ucb_dev, span, m_live, defer, prepared);
      }
    }
    return score_leaves_t<double>(xs_dev, xs_dtype, m, acq, want_ucb, mean_dev, var_dev, ucb_dev, span, m_live, defer, prepared);
  }

  // after the stream has been synchronised: total leaf-tile kernel time of the call
  void collect_tile_ms(bool timed, int pairs) {
    if (!timed) return;
    float total = 0;
    for (int i = 0; i < pairs; ++i) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ctx->tile_ev[2 * i], ctx->tile_ev[2 * i + 1]) == hipSuccess) total += ms;
    }
    ctx->last_ms[0] = total;
  }

  // ---- precision self-test (see fit.hip: selftest_kernel) ---------------------------------------
  double tol_var_abs() const { return tol_var * kp.variance; }
  double tol_mean_abs() const { return tol_mean * std::max(st_vals[2], 1.0e-300); }
  // A float FACTOR (GPSO_F32) carries a backward error E that the training inputs see unamplified (there
  // the solve weights w = K_y^-1 k_i are ~ a unit vector) but a general leaf sees as w^T E w, i.e. times
  // |w|_1^2 <= sigma^2 |K_y^-1| =: kappa.  The bound itself is far too pessimistic (measured |w|^2 at the
  // leaves: 440 where kappa ~ 2.6e4); sqrt(kappa), with kappa estimated from max_i (K_y^-1)_ii, is a
  // CALIBRATED HEURISTIC: it covers every float32 case of tools/fuzz_gpu.py and tools/precision_probe.py
  // (profiles/r02*_precision*.jsonl).  GPSO_MIXED (double factor) needs no such factor and is exact.
  double amplification() const {
    return sizeof(TF) == 4 ? std::max(1.0, std::sqrt(kp.variance * st_vals[5])) : 1.0;
  }
  // margin > 1: the readings must sit that far INSIDE the tolerances
  bool st_pass(double margin = 1.0) const {
    const bool finite = std::isfinite(st_vals[0]) && std::isfinite(st_vals[1]) && std::isfinite(st_vals[3]);
    const double amp = amplification();  // var: w^T E w ~ |w|^2; mean: w^T E alpha ~ |w|
    return finite && margin * st_vals[0] * std::sqrt(amp) <= tol_mean_abs() && margin * st_vals[1] * amp <= tol_var_abs();
  }
  // GPSO_GEN_AUTO keeps float generation only when it is comfortably inside the tolerances: double
  // generation is typically 1e-6-class, and a posterior that float generation brings within a factor of
  // a few of the gate is better served by it
  static constexpr double kAutoMargin = 8.0;
  int run_selftest() {
    if (res.st_done) return GPSO_OK;
    if (!res.st_have || !res.have_data) return ctx->fail(GPSO_E_STATE, "self-test needs a posterior fitted on this context (gpso_fit_eval)");
    int rc;
    if ((rc = ensure(st_mean, (size_t)n * 8))) return rc;
    if ((rc = ensure(st_var, (size_t)n * 8))) return rc;
    if ((rc = ensure(st_out, 8 * 8))) return rc;  // 6 used
    TileSpan span{ctx->timing};
    if ((rc = score_device_leaves(x64.p, GPSO_F64, n, 0.0, false, as<double>(st_mean), as<double>(st_var), nullptr, span))) return rc;
    launch_selftest<TF>(st(), as<double>(st_mean), as<double>(st_var), as<double>(y64), as<TF>(alpha_f),
                        as<double>(kinv_diag), n, kp.noise, kp.mean_c, as<double>(st_out), s_dev());
    double* host = ctx->pinned_scratch(8);
    if (!host) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    HIPCHECK(hipMemcpyAsync(host, st_out.p, 6 * 8, hipMemcpyDeviceToHost, st()));
    HIPCHECK(ctx->wait(st()));
    if ((rc = launch_status())) return rc;
    for (int i = 0; i < 6; ++i) st_vals[i] = host[i];
    res.selftest_ran();
    return GPSO_OK;
  }
  // GPSO_GEN_AUTO: let the self-test choose the generation arithmetic of this posterior.  Without a
  // self-test (switched off, or a posterior installed from outside: no targets) the choice is double.
  int decide_generation() {
    if (int rcp = ensure_split_pieces()) return rcp;
    if (!kFloatPredict || res.gen_decided) return GPSO_OK;
    if (gen_mode != GPSO_GEN_AUTO) {
      res.generation_ruled();
      return GPSO_OK;
    }
    // Matern-1/2 is exp(-sqrt(r^2)): near r = 0 the square root turns the 1e-6-class error of a float r^2
    // into 1e-3 of k -- for leaves CLOSE to a training input, while AT the training inputs (where the
    // self-test looks) the float form cancels exactly.  The test cannot see it, so this kernel generates
    // in double.
    if (!can_selftest() || kp.kernel == GPSO_MATERN12) {
      res.generation_trial(false, res.c16_fallback);
      res.generation_ruled();
      return GPSO_OK;
    }
    int rc = run_selftest();
    if (rc) return rc;
    if (!st_pass(kAutoMargin) && res.gen_eff32) {
      // not comfortably inside with float generation: measure double generation as well
      double r32[6];
      std::copy(st_vals, st_vals + 6, r32);
      const bool pass32 = st_pass();
      const bool was_c16 = c16_in_use(false);
      if (pass32 && bf16_usable() && res.linv_b == Copy::Valid && !bf16_fits(true)) {
        // the split-bf16 kernel the caller opted into cannot hold double fragments at this D: double
        // generation would also mean the (slower) native kernel.  Inside the tolerances: stay.
        res.generation_ruled();
        return GPSO_OK;
      }
      res.generation_trial(false, res.c16_fallback);
      if ((rc = run_selftest())) return rc;
      // the float form of r^2 is what fails at small lengthscales / noise -- then double is clearly
      // better and stays.  Where the readings are the same within 1.5x the error is not the generation's
      // (a float factor's, the apply's): float generation is as good and is kept.
      const bool finite64 = std::isfinite(st_vals[0]) && std::isfinite(st_vals[1]);
      bool f32 = false, c32 = res.c16_fallback;  // (the ruling; st_vals end as the readings of what it keeps)
      if (pass32 && finite64 && r32[0] <= 1.5 * st_vals[0] && r32[1] <= 1.5 * st_vals[1]) {
        f32 = true;
        std::copy(r32, r32 + 6, st_vals);
      } else if (was_c16 && finite64) {
        // float generation with the contraction on the fp16 pipe is not as good as double here: before paying for double
        // generation (the f64 matrix instruction: 1.3x the kernel time at C3's shape), a look at float generation with
        // the f32 contraction of rounds 1-3 -- its r^2 AT a training input is closer to zero (same floats in the norms
        // and the products), which is where this test looks
        double r64[6];
        std::copy(st_vals, st_vals + 6, r64);
        res.generation_trial(true, true);
        if ((rc = run_selftest())) return rc;
        // (kept on the terms it is kept on when it runs first: comfortably inside the tolerances, or as good as double)
        f32 = c32 = st_pass(kAutoMargin) || (st_pass() && st_vals[0] <= 1.5 * r64[0] && st_vals[1] <= 1.5 * r64[1]);
        if (!f32) std::copy(r64, r64 + 6, st_vals);
      }
      res.generation_ruled(f32, c32);
      return GPSO_OK;
    }
    res.generation_ruled();
    return GPSO_OK;
  }
  // the self-test, and under GPSO_MATH_AUTO a second look with the f32 MFMA kernel where the split-bf16 apply
  // misses the tolerances on this posterior
  int selftest_with_fallback() {
    int rc = run_selftest();
    if (rc) return rc;
    if (!st_pass() && math_auto && bf16_usable() && res.linv_b == Copy::Valid) {
      if (res.math == GPSO_MATH_F16X3 && res.chol_valid) {  // next rung: six bf16 products (L^-1 is resident: repack)
        res.ladder_down(GPSO_MATH_BF16X6);
        if ((rc = pack_bf16())) return rc;
        if ((rc = run_selftest()) || st_pass()) return rc;
      }
      res.ladder_down(GPSO_MATH_NATIVE);
      rc = run_selftest();
    }
    return rc;
  }
  int math_in_use() const {
    return (bf16_usable() && res.linv_b == Copy::Valid && bf16_fits(gen_double())) ? res.math : GPSO_MATH_NATIVE;
  }
  // called at the top of every predict-type entry point
  int precision_gate() {
    int rc = decide_generation();
    if (rc) return rc;
    if (!can_selftest()) return GPSO_OK;
    if ((rc = selftest_with_fallback())) return rc;
    if (!st_pass())
      return ctx->fail(GPSO_E_PRECISION,
                       "float predict arithmetic fails the self-test on this posterior: at the training inputs "
                       "max |d mean| = %.3g (tolerance %.3g), max |d var| = %.3g (tolerance %.3g = %.1e sigma^2), "
                       "amplification applied %.3g (float factor: sigma^2 max (K_y^-1)_ii), min predicted var %.3g "
                       "at noise %.3g, max |alpha| %.3g; use a GPSO_MIXED or GPSO_F64 context",
                       st_vals[0], tol_mean_abs(), st_vals[1], tol_var_abs(), tol_var, amplification(), st_vals[3],
                       kp.noise, st_vals[4]);
    return GPSO_OK;
  }
  int precision_info(double* out) override {
    if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "no posterior resident");
    int rc = decide_generation();
    if (rc) return rc;
    if ((rc = selftest_with_fallback())) return rc;
    for (int i = 0; i < 5; ++i) out[i] = st_vals[i];
    out[5] = kp.variance;
    out[6] = tol_mean_abs();
    out[7] = tol_var_abs();
    out[8] = amplification();
    out[9] = st_vals[5];
    out[10] = gen_double() ? 0.0 : 1.0;
    out[11] = (double)math_in_use();
    if (!st_pass()) return ctx->fail(GPSO_E_PRECISION, "self-test: max |d mean| %.3g (tol %.3g), max |d var| %.3g (tol %.3g), amplification %.3g",
                                     st_vals[0], out[6], st_vals[1], out[7], out[8]);
    return GPSO_OK;
  }

  int stage_leaves(const void* xs, int xs_dtype, int xs_mem, int64_t m, const void** dev_ptr) {
    if (xs_mem == GPSO_MEM_DEVICE) {
      *dev_ptr = xs;
      return GPSO_OK;
    }
    const size_t bytes = (size_t)m * d * ((xs_dtype == GPSO_F64) ? 8 : 4);
    int rc = ensure(leaves_raw, bytes);
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(leaves_raw.p, xs, bytes, hipMemcpyHostToDevice, st()));
    *dev_ptr = leaves_raw.p;
    return GPSO_OK;
  }

  // ---- the frame of a call that evaluates the resident posterior at points the caller gives: what
  // such a call refuses about its points, who may read the dense double factor, what the call records, and the way from the
  // caller's coordinates to scaled rows.  A new point call starts from these
  static constexpr bool kDenseDouble = sizeof(TF) == 8;  // (GPSO_F64 and GPSO_MIXED contexts: predict_grad, joint, paths)
  int check_points(const void* xs, int xs_dtype, int xs_mem, int64_t m) {
    if (m > 0 && !xs) return ctx->fail(GPSO_E_ARG, "xs must not be NULL");
    if (xs_dtype != GPSO_F64 && xs_dtype != GPSO_F32) return ctx->fail(GPSO_E_ARG, "bad xs_dtype %d", xs_dtype);
    if (xs_mem != GPSO_MEM_HOST && xs_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "bad xs_mem %d", xs_mem);
    return GPSO_OK;
  }
  int need_dense_factor(const char* who) {
    if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "no posterior resident: call gpso_fit_eval / gpso_set_posterior first");
    if (res.post == Post::Adopted || !res.chol_valid)
      return ctx->fail(GPSO_E_STATE, "%s needs the dense factor of the posterior: an adopted posterior may have travelled without it", who);
    return refuse_if_async(who);
  }
  // open and close: last_ms[1] is the stream time between the two, and the counts and the time describe the same call.  The
  // open comes after the call's last refusal (a refused call leaves nothing in flight); the close records before it waits
  int points_begin(hipStream_t* stream) {
    hipStream_t s = *stream = st();
    if (ctx->timing) HIPCHECK(hipEventRecord(ctx->ev[2], s));
    return GPSO_OK;
  }
  static constexpr int64_t kNoCounts = -1;  // (gpso_paths_draw: no points, the counts stay the last point call's)
  int points_end(hipStream_t s, int64_t m) {
    if (ctx->timing) HIPCHECK(hipEventRecord(ctx->ev[3], s));
    HIPCHECK(ctx->wait(s));
    if (m != kNoCounts) ctx->last_count[0] = ctx->last_count[1] = m;
    float ms = 0;
    if (ctx->timing && hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->last_ms[1] = ms;
    return GPSO_OK;
  }
  // rows off .. off + mc of the staged points (dtype xs_dtype) -> mpad scaled rows and their norms
  template <typename TG>
  void prep_points(hipStream_t s, const void* dev, int xs_dtype, int64_t off, int64_t mc, int64_t mpad, const int64_t* m_live, TG* ts,
                   TG* norm) {
    if (xs_dtype == GPSO_F64)
      launch_prep_leaves<TG, double>(s, static_cast<const double*>(dev) + off * d, mc, mpad, d, dp, ls_dev(), m_live, ts, norm);
    else
      launch_prep_leaves<TG, float>(s, static_cast<const float*>(dev) + off * d, mc, mpad, d, dp, ls_dev(), m_live, ts, norm);
  }

  int check_predict_args(const void* xs, int xs_dtype, int xs_mem, int64_t m) {
    if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "no posterior resident: call gpso_fit_eval / gpso_set_posterior first");
    if (m < 0) return ctx->fail(GPSO_E_ARG, "negative leaf count");
    int rc = check_points(xs, xs_dtype, xs_mem, m);
    return rc ? rc : precision_gate();
  }

  int predict(const void* xs, int xs_dtype, int xs_mem, int64_t m, double* mean, double* var,
              int out_mem) override {
    return point_values(xs, xs_dtype, xs_mem, m, 0.0, false, mean, var, nullptr, out_mem);
  }
  // gpso_predict with the acquisition column (acq.hpp) beside mean and var: the same tiles, the same finalize kernel --
  // mean / var are gpso_predict's bits, the column is what gpso_best_acq ranks by.  Outputs the caller does not want
  // stay in the context's own buffers
  int acq_values(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, double* mean, double* var,
                 double* value, int out_mem) override {
    return point_values(xs, xs_dtype, xs_mem, m, acq, true, mean, var, value, out_mem);
  }
  // GPSO_ACQ_MES reads its maxima from this buffer (acq.hpp); no call of this context but the next set_maxima touches it
  int set_maxima(const double* ystar, int k) override {
    int rc = refuse_if_async("gpso_acq_set_maxima");
    if (rc) return rc;
    if (k < 0 || k > GPSO_ACQ_MAX_MAXIMA) return ctx->fail(GPSO_E_ARG, "k=%d maxima: 0..%d are kept", k, GPSO_ACQ_MAX_MAXIMA);
    if (k > 0 && !ystar) return ctx->fail(GPSO_E_ARG, "ystar must not be NULL");
    for (int i = 0; i < k; ++i)
      if (!std::isfinite(ystar[i])) return ctx->fail(GPSO_E_ARG, "ystar[%d] is not finite", i);
    if (k > 0) {
      if ((rc = ensure(acq_maxima, GPSO_ACQ_MAX_MAXIMA * 8))) return rc;
      HIPCHECK(hipStreamSynchronize(st()));  // (a blocking call's kernels are done; nothing reads the old set)
      HIPCHECK(hipMemcpy(acq_maxima.p, ystar, (size_t)k * 8, hipMemcpyHostToDevice));
      std::memcpy(maxima_host, ystar, (size_t)k * 8);
    }
    maxima_k = k;
    maxima_dev = k > 0 ? as<double>(acq_maxima) : nullptr;
    return GPSO_OK;
  }
  int max_logcdf(const double* mean, const double* var, int mem, int64_t m, double var_sub, const double* y, int g, double* logcdf,
                 int64_t* n_used) override {
    int rc = refuse_if_async("gpso_max_logcdf");
    if (rc) return rc;
    if (!mean || !var || !y || !logcdf) return ctx->fail(GPSO_E_ARG, "mean, var, y and logcdf must not be NULL");
    if (mem != GPSO_MEM_HOST && mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "bad mem %d", mem);
    if (m < 1 || g < 1 || g > kMaxCdfThresholds) return ctx->fail(GPSO_E_ARG, "m=%lld, g=%d: m >= 1 and g in 1..%d", (long long)m, g, kMaxCdfThresholds);
    if (var_sub != var_sub) return ctx->fail(GPSO_E_ARG, "var_sub is NaN");
    for (int i = 0; i < g; ++i)
      if (y[i] != y[i]) return ctx->fail(GPSO_E_ARG, "y[%d] is NaN", i);
    const int64_t nblk = max_logcdf_blocks(m);
    if ((rc = ensure(mcdf_work, (size_t)(nblk * kMaxCdfSlots + 2 * kMaxCdfSlots) * 8))) return rc;
    double* partial = as<double>(mcdf_work);
    double* y_dev = partial + nblk * kMaxCdfSlots;
    double* out_dev = y_dev + kMaxCdfSlots;
    const double *md = mean, *vd = var;
    if (mem == GPSO_MEM_HOST) {
      if ((rc = ensure(mcdf_in, (size_t)m * 16))) return rc;
      HIPCHECK(hipMemcpyAsync(mcdf_in.p, mean, (size_t)m * 8, hipMemcpyHostToDevice, st()));
      HIPCHECK(hipMemcpyAsync(as<double>(mcdf_in) + m, var, (size_t)m * 8, hipMemcpyHostToDevice, st()));
      md = as<double>(mcdf_in);
      vd = md + m;
    }
    HIPCHECK(hipMemcpyAsync(y_dev, y, (size_t)g * 8, hipMemcpyHostToDevice, st()));
    launch_max_logcdf(st(), md, vd, m, var_sub, y_dev, g, partial, out_dev);
    if ((rc = launch_status())) return rc;
    double out[kMaxCdfSlots];
    HIPCHECK(hipMemcpyAsync(out, out_dev, (size_t)(g + 1) * 8, hipMemcpyDeviceToHost, st()));
    HIPCHECK(hipStreamSynchronize(st()));
    std::memcpy(logcdf, out, (size_t)g * 8);
    if (n_used) *n_used = (int64_t)out[g];
    return GPSO_OK;
  }
  // the body of both: gpso_predict is gpso_predict_acq without the column (want_ucb false: nothing of it is allocated,
  // computed or copied) and with both of its outputs required
  int point_values(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, bool want_ucb, double* mean, double* var,
                   double* value, int out_mem) {
    ctx->tick_timing();
    int rc = check_predict_args(xs, xs_dtype, xs_mem, m);
    if (rc) return rc;
    if (m == 0) return GPSO_OK;
    if (!want_ucb && (!mean || !var)) return ctx->fail(GPSO_E_ARG, "mean / var must not be NULL");
    if (want_ucb && !mean && !var && !value) return ctx->fail(GPSO_E_ARG, "mean, var and value are all NULL");
    hipStream_t s;
    if ((rc = points_begin(&s))) return rc;
    const void* dev = nullptr;
    if ((rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
    const bool host = out_mem == GPSO_MEM_HOST;
    double *md = mean, *vd = var, *ud = value;
    if (host || !mean) {
      if ((rc = ensure(omean, (size_t)m * 8))) return rc;
      md = as<double>(omean);
    }
    if (host || !var) {
      if ((rc = ensure(ovar, (size_t)m * 8))) return rc;
      vd = as<double>(ovar);
    }
    if (want_ucb && (host || !value)) {
      if ((rc = ensure(oucb, (size_t)m * 8))) return rc;
      ud = as<double>(oucb);
    }
    TileSpan span{ctx->timing};
    if ((rc = score_device_leaves(dev, xs_dtype, m, acq, want_ucb, md, vd, ud, span))) return rc;
    if (host) {
      if (mean) HIPCHECK(hipMemcpyAsync(mean, md, (size_t)m * 8, hipMemcpyDeviceToHost, s));
      if (var) HIPCHECK(hipMemcpyAsync(var, vd, (size_t)m * 8, hipMemcpyDeviceToHost, s));
      if (value) HIPCHECK(hipMemcpyAsync(value, ud, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    }
    if ((rc = points_end(s, m))) return rc;
    collect_tile_ms(span.timed, span.pairs);
    return GPSO_OK;
  }

  // ---- mean, var and their gradients in the test points (predict_grad.hip).  Reads the dense fit-type
  // factor, alpha_f, xs64 and the hyper block and writes buffers of its own only: the posterior, its packed copies and the
  // self-test's verdicts stay as they are.  M is worked off in chunks of kPredictGradChunk, so the workspace is a few
  // N_pad x chunk doubles whatever M is
  int predict_grad(const void* xs, int xs_dtype, int xs_mem, int64_t m, double* mean, double* var, double* dmean, double* dvar,
                   int out_mem) override {
    if constexpr (!kDenseDouble) return ctx->fail(GPSO_E_ARG, "gpso_predict_grad needs a GPSO_F64 or GPSO_MIXED context (the dense factor in double)");
    ctx->tick_timing();
    if (m < 1) return ctx->fail(GPSO_E_ARG, "gpso_predict_grad needs at least one test point (m=%lld)", (long long)m);
    int rc = check_points(xs, xs_dtype, xs_mem, m);
    if (rc) return rc;
    if (!mean && !var && !dmean && !dvar) return ctx->fail(GPSO_E_ARG, "mean, var, dmean and dvar are all NULL");
    if ((rc = need_dense_factor("gpso_predict_grad"))) return rc;
    const int64_t chunk = std::min<int64_t>(kPredictGradChunk, (m + 63) / 64 * 64);
    if ((rc = ensure(pg_ts, (size_t)chunk * dp * 8))) return rc;
    if ((rc = ensure(pg_norm, (size_t)chunk * 8))) return rc;
    if ((rc = ensure(pg_work, predict_grad_workspace_doubles(npad, dp, chunk) * 8))) return rc;
    const bool to_host = out_mem == GPSO_MEM_HOST;
    double *md = mean, *vd = var, *dmd = dmean, *dvd = dvar;
    if (to_host) {
      if ((rc = ensure(pg_out, (size_t)m * (2 + 2 * (size_t)d) * 8))) return rc;
      double* o = as<double>(pg_out);
      md = mean ? o : nullptr;
      vd = var ? o + m : nullptr;
      dmd = dmean ? o + 2 * m : nullptr;
      dvd = dvar ? o + 2 * m + m * d : nullptr;
    }
    hipStream_t s;
    if ((rc = points_begin(&s))) return rc;
    const void* dev = nullptr;
    if ((rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
    PredictGradLaunch g;
    g.C = as<double>(linv); g.alpha = as<double>(alpha_f); g.xs = as<double>(xs64); g.ls = ls_dev();
    g.ts = as<double>(pg_ts); g.n = n; g.npad = npad; g.d = d; g.dp = dp; g.kp = kp; g.work = as<double>(pg_work);
    for (int64_t off = 0; off < m; off += chunk) {
      const int64_t mc = std::min(chunk, m - off), mpad = (mc + 63) / 64 * 64;
      prep_points<double>(s, dev, xs_dtype, off, mc, mpad, nullptr, as<double>(pg_ts), as<double>(pg_norm));
      g.m = mc;
      g.mean = md ? md + off : nullptr;
      g.var = vd ? vd + off : nullptr;
      g.dmean = dmd ? dmd + off * d : nullptr;
      g.dvar = dvd ? dvd + off * d : nullptr;
      if (launch_predict_grad(s, g) != 0) return launch_status();
      if ((rc = launch_status())) return rc;
    }
    if (to_host) {
      if (mean) HIPCHECK(hipMemcpyAsync(mean, md, (size_t)m * 8, hipMemcpyDeviceToHost, s));
      if (var) HIPCHECK(hipMemcpyAsync(var, vd, (size_t)m * 8, hipMemcpyDeviceToHost, s));
      if (dmean) HIPCHECK(hipMemcpyAsync(dmean, dmd, (size_t)m * d * 8, hipMemcpyDeviceToHost, s));
      if (dvar) HIPCHECK(hipMemcpyAsync(dvar, dvd, (size_t)m * d * 8, hipMemcpyDeviceToHost, s));
    }
    return points_end(s, m);
  }

  // ---- the joint predictive (joint.hip).  Like gpso_predict_grad it reads the dense fit-type factor,
  // alpha_f, xs64 and the hyper block and writes buffers of its own only.  joint_enqueue scales the test
  // points, forms V with predict_grad.hip's apply stage and launches mean and Sigma (into `cov`, leading dimension ldc)
  int joint_enqueue(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, double* mean_dev,
                    double* cov_dev, int64_t ldc, bool pad_identity) {
    const int64_t mc = (m + 63) / 64 * 64;
    int rc;
    if ((rc = ensure(pj_ts, (size_t)mc * dp * 8))) return rc;
    if ((rc = ensure(pj_norm, (size_t)mc * 8))) return rc;
    if ((rc = ensure(pj_v, predict_grad_apply_workspace_doubles(npad, mc) * 8))) return rc;
    if ((rc = ensure(pj_part, std::max<size_t>(joint_partial_doubles(n, m), 1) * 8))) return rc;
    hipStream_t s = st();
    const void* dev = nullptr;
    if ((rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
    prep_points<double>(s, dev, xs_dtype, 0, m, mc, nullptr, as<double>(pj_ts), as<double>(pj_norm));
    PredictGradLaunch g;
    g.C = as<double>(linv); g.xs = as<double>(xs64); g.ts = as<double>(pj_ts); g.n = n; g.npad = npad; g.m = m; g.d = d; g.dp = dp;
    g.kp = kp; g.work = as<double>(pj_v);
    if (launch_predict_grad_apply(s, g) != 0) return launch_status();
    JointLaunch j;
    j.V = as<double>(pj_v); j.ts = as<double>(pj_ts); j.alpha = as<double>(alpha_f); j.xs = as<double>(xs64);
    j.n = n; j.npad = npad; j.m = m; j.dp = dp; j.kp = kp; j.diag_add = diag_add; j.part = as<double>(pj_part);
    j.mean = mean_dev; j.cov = cov_dev; j.ldc = ldc; j.pad_identity = pad_identity;
    (void)launch_joint(s, j);  // (a refused shape is on record: launch_status reports it)
    return launch_status();
  }
  // the conditions gpso_predict_joint and gpso_sample_joint share with gpso_predict_grad
  int joint_check(const char* what, const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add) {
    if (m < 1 || m > kPredictGradChunk)
      return ctx->fail(GPSO_E_ARG, "%s takes 1 to %lld test points (m=%lld): the joint covariance of more is out of scope", what,
                       (long long)kPredictGradChunk, (long long)m);
    int rc = check_points(xs, xs_dtype, xs_mem, m);
    if (rc) return rc;
    if (!(diag_add == diag_add) || diag_add - diag_add != 0.0) return ctx->fail(GPSO_E_ARG, "diag_add must be finite");
    return need_dense_factor(what);
  }

  int predict_joint(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, double* mean, double* cov,
                    int out_mem) override {
    if constexpr (!kDenseDouble) return ctx->fail(GPSO_E_ARG, "gpso_predict_joint needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)");
    ctx->tick_timing();
    if (!cov) return ctx->fail(GPSO_E_ARG, "cov must not be NULL");
    int rc = joint_check("gpso_predict_joint", xs, xs_dtype, xs_mem, m, diag_add);
    if (rc) return rc;
    const bool to_host = out_mem == GPSO_MEM_HOST;
    double *md = mean, *cd = cov;
    if (to_host) {
      if ((rc = ensure(pj_mu, (size_t)m * 8))) return rc;
      if ((rc = ensure(pj_sigma, (size_t)m * m * 8))) return rc;
      md = mean ? as<double>(pj_mu) : nullptr;
      cd = as<double>(pj_sigma);
    }
    hipStream_t s;
    if ((rc = points_begin(&s))) return rc;
    if ((rc = joint_enqueue(xs, xs_dtype, xs_mem, m, diag_add, md, cd, m, false))) return rc;
    if (to_host) {
      if (mean) HIPCHECK(hipMemcpyAsync(mean, md, (size_t)m * 8, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipMemcpyAsync(cov, cd, (size_t)m * m * 8, hipMemcpyDeviceToHost, s));
    }
    return points_end(s, m);
  }

  // Sigma (identity on the padding up to a multiple of 128) -> launch_potrf as vgp_chol uses it -> F = mu 1^T + Z L^T ->
  // the arg-max per draw.  One wait at the end; a failing pivot is reported then and the outputs hold nothing of use
  int sample_joint(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, const double* z, int64_t ns,
                   double* samples, int64_t* best_idx, double* best_val) override {
    if constexpr (!kDenseDouble) return ctx->fail(GPSO_E_ARG, "gpso_sample_joint needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)");
    ctx->tick_timing();
    if (ns < 1 || ns > kJointMaxDraws)
      return ctx->fail(GPSO_E_ARG, "gpso_sample_joint takes 1 to %lld draws a call (s=%lld)", (long long)kJointMaxDraws, (long long)ns);
    if (!z) return ctx->fail(GPSO_E_ARG, "z must not be NULL");
    if (!samples && !best_idx && !best_val) return ctx->fail(GPSO_E_ARG, "samples, best_idx and best_val are all NULL");
    int rc = joint_check("gpso_sample_joint", xs, xs_dtype, xs_mem, m, diag_add);
    if (rc) return rc;
    if (ns > ((int64_t)1 << 31) / m) return ctx->fail(GPSO_E_ARG, "gpso_sample_joint: s * m above 2^31 (s=%lld, m=%lld)", (long long)ns, (long long)m);
    const int64_t mpad = (m + kPadN - 1) / kPadN * kPadN;
    const size_t mat = (size_t)mpad * mpad * 8;
    for (DevBuf* b : {&pj_sigma, &pj_l, &pj_linv, &pj_cwork})
      if ((rc = ensure(*b, mat))) return rc;
    if ((rc = ensure(pj_mu, (size_t)m * 8))) return rc;
    if ((rc = ensure(pj_diag, (size_t)mpad * 8))) return rc;
    if ((rc = ensure(pj_info, 256))) return rc;
    if ((rc = ensure(pj_z, (size_t)ns * m * 8))) return rc;
    if ((rc = ensure(pj_f, (size_t)ns * m * 8))) return rc;
    if ((rc = ensure(pj_best, (size_t)ns * 16))) return rc;
    int* info_host = reinterpret_cast<int*>(ctx->pinned_scratch(8));
    if (!info_host) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    hipStream_t s;
    if ((rc = points_begin(&s))) return rc;
    HIPCHECK(hipMemcpyAsync(pj_z.p, z, (size_t)ns * m * 8, hipMemcpyHostToDevice, s));
    int* info = static_cast<int*>(pj_info.p);
    launch_vgp_pad_identity(s, as<double>(pj_sigma), 0, mpad, info);  // (Sigma := I, info := INT_MAX; the tiles overwrite their part)
    if ((rc = joint_enqueue(xs, xs_dtype, xs_mem, m, diag_add, as<double>(pj_mu), as<double>(pj_sigma), mpad, true)))
      return rc;
    HIPCHECK(hipMemsetAsync(pj_linv.p, 0, mat, s));
    (void)launch_potrf<double>(s, as<double>(pj_sigma), as<double>(pj_l), as<double>(pj_linv), as<double>(pj_cwork), nullptr, m, mpad,
                               as<double>(pj_diag), info, -1, nullptr);
    HIPCHECK(hipMemcpyAsync(info_host, info, sizeof(int), hipMemcpyDeviceToHost, s));
    launch_joint_draw(s, as<double>(pj_l), mpad, as<double>(pj_z), as<double>(pj_mu), m, ns, as<double>(pj_f));
    int64_t* bi = as<int64_t>(pj_best);
    double* bv = reinterpret_cast<double*>(bi + ns);
    if (best_idx || best_val) launch_joint_argmax(s, as<double>(pj_f), m, ns, bi, bv);
    if ((rc = launch_status())) return rc;
    if (samples) HIPCHECK(hipMemcpyAsync(samples, pj_f.p, (size_t)ns * m * 8, hipMemcpyDeviceToHost, s));
    if (best_idx) HIPCHECK(hipMemcpyAsync(best_idx, bi, (size_t)ns * 8, hipMemcpyDeviceToHost, s));
    if (best_val) HIPCHECK(hipMemcpyAsync(best_val, bv, (size_t)ns * 8, hipMemcpyDeviceToHost, s));
    if ((rc = points_end(s, m))) return rc;
    if (*info_host != INT_MAX)
      return ctx->fail(GPSO_E_NOTPD, "gpso_sample_joint: Sigma + diag_add*I is not positive definite: Cholesky failed at pivot %d "
                                     "(a larger diag_add -- jitter -- is the remedy)", *info_host);
    return GPSO_OK;
  }

  // ---- pathwise posterior draws (paths.hip).  Both calls read the dense fit-type factor, the scaled
  // rows, y, the per-point noise and the hyper block and write buffers of their own only: the posterior, its packed copies and
  // the self-test's verdicts stay as they are.  gpso_paths_draw builds the set beside the resident one and swaps it in at the end
  static bool all_finite(const double* v, size_t len) {
    for (size_t i = 0; i < len; ++i)
      if (!std::isfinite(v[i])) return false;
    return true;
  }
  int paths_draw(const double* omega, const double* phase, int64_t f, const double* w, const double* eps, int64_t ns) override {
    return paths_draw_impl(false, "gpso_paths_draw", omega, phase, f, w, eps, ns);
  }
  // the draw of a variational posterior: v = beta + Lu^-T (Q eps - Lu^-1 Phi(Zr) w^T) from what the
  // install left in Lf (Lu), alpha_f (beta) and vq_S / svq_S / sgM2 (Q); Lu^-1 is rebuilt from Lf into vA (vB: the copy of
  // Lu with a unit diagonal on the padding, work: scratch) -- three buffers the install has finished with
  int paths_draw_q(const double* omega, const double* phase, int64_t f, const double* w, const double* eps, int64_t ns) override {
    return paths_draw_impl(true, "gpso_paths_draw_q", omega, phase, f, w, eps, ns);
  }
  int paths_draw_impl(bool variational, const char* who, const double* omega, const double* phase, int64_t f, const double* w,
                      const double* eps, int64_t ns) {
    if constexpr (!kDenseDouble) return ctx->fail(GPSO_E_ARG, "%s needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)", who);
    ctx->tick_timing();
    if (ns < 1 || ns > kPathsMaxDraws)
      return ctx->fail(GPSO_E_ARG, "%s takes 1 to %lld draws (s=%lld)", who, (long long)kPathsMaxDraws, (long long)ns);
    if (f < 1 || f > kPathsMaxFeatures)
      return ctx->fail(GPSO_E_ARG, "%s takes 1 to %lld features (f=%lld)", who, (long long)kPathsMaxFeatures, (long long)f);
    if (!omega || !phase || !w) return ctx->fail(GPSO_E_ARG, "omega, phase and w must not be NULL");
    if (!variational) {
      if (!(res.post == Post::Fitted && res.st_have && res.have_data && res.chol_valid))
        return ctx->fail(GPSO_E_STATE, "gpso_paths_draw needs a posterior fitted with targets on this context (gpso_set_data + gpso_fit_eval)");
    } else {
      if (res.post == Post::Fitted) return ctx->fail(GPSO_E_STATE, "gpso_paths_draw_q draws from a variational posterior: a fitted exact GP takes gpso_paths_draw");
      if (!(res.variational() && res.chol_valid))
        return ctx->fail(GPSO_E_STATE, "gpso_paths_draw_q needs a posterior installed by gpso_vgp_posterior, gpso_sgpr_posterior or gpso_svgp_posterior on this context");
      // (at present implied by the line above: q_factors is set with the kind and cleared only where the kind is -- no call
      // overwrites Lf, beta or the root of q and keeps the posterior.  The flag is for the first call that does)
      if (!res.q_factors)
        return ctx->fail(GPSO_E_STATE, "gpso_paths_draw_q: the install's factors (Lu, beta, the root of q) are not resident any more: install again");
    }
    int rc = refuse_if_async(who);
    if (rc) return rc;
    if (!all_finite(omega, (size_t)f * d) || !all_finite(phase, (size_t)f) || !all_finite(w, (size_t)ns * f) ||
        (eps && !all_finite(eps, (size_t)ns * n)))
      return ctx->fail(GPSO_E_ARG, "%s: omega, phase, w and eps must be finite", who);
    const int64_t f16 = (f + 15) / 16 * 16, spad = (ns + 63) / 64 * 64, n64 = (n + 63) / 64 * 64;
    PathSet& nx = pth_next;
    if ((rc = ensure(nx.omega, (size_t)f16 * dp * 8))) return rc;
    if ((rc = ensure(nx.phase, (size_t)f16 * 8))) return rc;
    if ((rc = ensure(nx.w, (size_t)ns * f16 * 8))) return rc;
    if ((rc = ensure(nx.vt, (size_t)spad * npad * 8))) return rc;
    if (eps && (rc = ensure(pth_eps, (size_t)ns * n * 8))) return rc;
    if ((rc = ensure(pth_p, (size_t)ns * n64 * 8))) return rc;
    if ((rc = ensure(pth_r, (size_t)n64 * spad * 8))) return rc;
    if ((rc = ensure(pth_u, (size_t)n64 * spad * 8))) return rc;
    if (variational && (rc = ensure(pth_x, (size_t)n64 * spad * 8))) return rc;
    // the layouts the kernels read: D_pad columns, rows up to a multiple of 16, zeros on the padding
    std::vector<double> ho((size_t)f16 * dp, 0.0), hp((size_t)f16, 0.0), hw((size_t)ns * f16, 0.0);
    for (int64_t j = 0; j < f; ++j) {
      std::memcpy(&ho[(size_t)j * dp], omega + (size_t)j * d, (size_t)d * 8);
      hp[(size_t)j] = phase[j];
    }
    for (int64_t r = 0; r < ns; ++r) std::memcpy(&hw[(size_t)r * f16], w + (size_t)r * f, (size_t)f * 8);
    hipStream_t s;
    if ((rc = points_begin(&s))) return rc;
    HIPCHECK(hipMemcpyAsync(nx.omega.p, ho.data(), ho.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(nx.phase.p, hp.data(), hp.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(nx.w.p, hw.data(), hw.size() * 8, hipMemcpyHostToDevice, s));
    if (eps) HIPCHECK(hipMemcpyAsync(pth_eps.p, eps, (size_t)ns * n * 8, hipMemcpyHostToDevice, s));
    PathsEvalLaunch g;  // Phi(X) w^T: the evaluation over the training rows, kernel part off
    g.ts = g.xs = as<double>(xs64); g.omega = as<double>(nx.omega); g.phase = as<double>(nx.phase); g.W = as<double>(nx.w);
    g.n = n; g.npad = npad; g.m = n; g.s = ns; g.f = f; g.ldw = f16; g.dp = dp; g.kp = kp; g.out = as<double>(pth_p); g.ldo = n64;
    if (launch_paths_eval(s, g) != 0) return launch_status();
    if (!variational) {
      launch_paths_solve(s, as<double>(linv), as<double>(y64), as<double>(pth_p), n64, eps ? as<double>(pth_eps) : nullptr, s_dev(), kp,
                         n, npad, ns, as<double>(pth_r), as<double>(pth_u), as<double>(nx.vt));
    } else {
      launch_vgp_clean_lower(s, as<double>(Lf), as<double>(vB), n, npad, 1.0);
      launch_trinv<double>(s, as<double>(vB), as<double>(vA), as<double>(work), npad);
      const bool sgpr = res.post == Post::Sgpr;
      const double* Q = sgpr ? as<double>(sgM2) : res.post == Post::Svgp ? as<double>(svq_S) : as<double>(vq_S);
      launch_paths_solve_q(s, as<double>(vA), Q, sgpr, as<double>(alpha_f), as<double>(pth_p), n64, eps ? as<double>(pth_eps) : nullptr, n,
                           npad, ns, as<double>(pth_r), as<double>(pth_u), as<double>(pth_x), as<double>(nx.vt));
    }
    if ((rc = launch_status())) return rc;
    if ((rc = points_end(s, kNoCounts))) return rc;
    nx.s = ns; nx.f = f; nx.ldw = f16;
    std::swap(pth, pth_next);
    res.paths_drawn();
    return GPSO_OK;
  }

  // M is worked off in chunks of kPathsChunk: values of one chunk [S][chunk], copied out and / or reduced into the running
  // winners per (draw, segment) before the next chunk overwrites them
  int paths_eval(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, double* values, int out_mem,
                 int64_t* best_idx, double* best_val) override {
    if constexpr (!kDenseDouble) return ctx->fail(GPSO_E_ARG, "gpso_paths_eval needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)");
    ctx->tick_timing();
    if (m < 1) return ctx->fail(GPSO_E_ARG, "gpso_paths_eval needs at least one point (m=%lld)", (long long)m);
    int rc = check_points(xs, xs_dtype, xs_mem, m);
    if (rc) return rc;
    if (!values && !best_idx && !best_val) return ctx->fail(GPSO_E_ARG, "values, best_idx and best_val are all NULL");
    if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "bad out_mem %d", out_mem);
    if (nseg < 1 || nseg > 1024) return ctx->fail(GPSO_E_ARG, "nseg=%d outside [1, 1024]", nseg);
    if (!res.paths_valid)
      return ctx->fail(GPSO_E_STATE, "no path set resident for this posterior: call gpso_paths_draw (every fit, append, new data, noise vector, install and hand-off ends the set)");
    if ((rc = refuse_if_async("gpso_paths_eval"))) return rc;
    std::vector<int64_t> so(nseg + 1);
    if (seg_off) {
      for (int i = 0; i <= nseg; ++i) so[i] = seg_off[i];
      if (so[0] != 0 || so[nseg] != m) return ctx->fail(GPSO_E_ARG, "seg_off must start at 0 and end at M");
      for (int i = 0; i < nseg; ++i)
        if (so[i + 1] < so[i]) return ctx->fail(GPSO_E_ARG, "seg_off must be non-decreasing");
    } else {
      if (nseg != 1) return ctx->fail(GPSO_E_ARG, "seg_off == NULL requires nseg == 1");
      so[0] = 0;
      so[1] = m;
    }
    const bool want_best = best_idx || best_val;
    const int64_t ns = pth.s, chunk = std::min<int64_t>(kPathsChunk, (m + 63) / 64 * 64);
    if ((rc = ensure(pe_ts, (size_t)chunk * dp * 8))) return rc;
    if ((rc = ensure(pe_norm, (size_t)chunk * 8))) return rc;
    if ((rc = ensure(pe_vals, (size_t)ns * chunk * 8))) return rc;
    if ((rc = ensure(pe_seg, (size_t)(nseg + 1) * 8))) return rc;
    if ((rc = ensure(pe_best, (size_t)ns * nseg * 16))) return rc;
    int64_t* bi = as<int64_t>(pe_best);
    double* bv = reinterpret_cast<double*>(bi + ns * nseg);
    std::vector<int64_t> hi_(want_best ? (size_t)ns * nseg : 0);
    std::vector<double> hv_(want_best ? (size_t)ns * nseg : 0);
    hipStream_t s;
    if ((rc = points_begin(&s))) return rc;
    const void* dev = nullptr;
    if ((rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
    if (want_best) {
      HIPCHECK(hipMemcpyAsync(pe_seg.p, so.data(), (size_t)(nseg + 1) * 8, hipMemcpyHostToDevice, s));
      HIPCHECK(hipMemsetAsync(pe_best.p, 0xFF, (size_t)ns * nseg * 16, s));  // (index -1: no winner yet; the value a NaN)
    }
    PathsEvalLaunch g;
    g.ts = as<double>(pe_ts); g.xs = as<double>(xs64); g.omega = as<double>(pth.omega); g.phase = as<double>(pth.phase);
    g.W = as<double>(pth.w); g.VT = as<double>(pth.vt);
    g.n = n; g.npad = npad; g.s = ns; g.f = pth.f; g.ldw = pth.ldw; g.dp = dp; g.kp = kp; g.out = as<double>(pe_vals); g.ldo = chunk;
    for (int64_t off = 0; off < m; off += chunk) {
      const int64_t mc = std::min(chunk, m - off), mpad = (mc + 63) / 64 * 64;
      prep_points<double>(s, dev, xs_dtype, off, mc, mpad, nullptr, as<double>(pe_ts), as<double>(pe_norm));
      g.m = mc;
      if (launch_paths_eval(s, g) != 0) return launch_status();
      if ((rc = launch_status())) return rc;
      if (values)
        HIPCHECK(hipMemcpy2DAsync(values + off, (size_t)m * 8, pe_vals.p, (size_t)chunk * 8, (size_t)mc * 8, (size_t)ns,
                                  out_mem == GPSO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
      if (want_best) launch_paths_argmax(s, as<double>(pe_vals), chunk, off, mc, as<int64_t>(pe_seg), nseg, ns, bi, bv);
    }
    if (want_best) {
      if ((rc = launch_status())) return rc;
      HIPCHECK(hipMemcpyAsync(hi_.data(), bi, hi_.size() * 8, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipMemcpyAsync(hv_.data(), bv, hv_.size() * 8, hipMemcpyDeviceToHost, s));
    }
    if ((rc = points_end(s, m))) return rc;
    for (size_t e = 0; e < hi_.size(); ++e) {  // indices relative to the segment start; an empty segment: -1 and a NaN
      if (best_idx) best_idx[e] = hi_[e] < 0 ? -1 : hi_[e] - so[e % nseg];
      if (best_val) best_val[e] = hv_[e];
    }
    return GPSO_OK;
  }
  void paths_info(int64_t* s_out, int64_t* f_out) const override {
    *s_out = res.paths_valid ? pth.s : 0;
    *f_out = res.paths_valid ? pth.f : 0;
  }

  // ---- latent cross-covariance and greedy batch selection (batch.hip).  Both calls read the dense
  // fit-type factor, the scaled rows and the hyper block -- gpso_best_batch also whatever gpso_acq_values reads -- and write
  // buffers of their own only: the posterior, its packed copies, the self-test's verdicts and a resident path set stay as they are
  int cross_cov(const void* xa, int xs_dtype, int xs_mem, int64_t m, const double* xb, int b, double* cov, int out_mem) override {
    if constexpr (!kDenseDouble) return ctx->fail(GPSO_E_ARG, "gpso_cross_cov needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)");
    ctx->tick_timing();
    if (m < 1) return ctx->fail(GPSO_E_ARG, "gpso_cross_cov needs at least one point (m=%lld)", (long long)m);
    if (b < 1 || b > kBatchMaxPicks) return ctx->fail(GPSO_E_ARG, "gpso_cross_cov takes 1 to %d points b (b=%d)", kBatchMaxPicks, b);
    int rc = check_points(xa, xs_dtype, xs_mem, m);
    if (rc) return rc;
    if (!xb || !cov) return ctx->fail(GPSO_E_ARG, "xb and cov must not be NULL");
    if ((rc = need_dense_factor("gpso_cross_cov"))) return rc;
    const int64_t chunk = std::min<int64_t>(kBatchChunk, (m + 63) / 64 * 64);
    if ((rc = ensure(cc_ts, (size_t)chunk * dp * 8))) return rc;
    if ((rc = ensure(cc_norm, (size_t)chunk * 8))) return rc;
    if ((rc = ensure(cc_braw, (size_t)kBatchMaxPicks * d * 8))) return rc;
    if ((rc = ensure(cc_tb, (size_t)kBatchMaxPicks * dp * 8))) return rc;
    if ((rc = ensure(cc_bnorm, (size_t)kBatchMaxPicks * 8))) return rc;
    if ((rc = ensure(cc_vec, batch_pick_workspace_doubles(n, npad, b) * 8))) return rc;
    if ((rc = ensure(cc_lv, (size_t)kBatchMaxPicks * 8))) return rc;
    const bool to_host = out_mem == GPSO_MEM_HOST;
    double* cd = cov;
    if (to_host) {
      if ((rc = ensure(cc_out, (size_t)b * m * 8))) return rc;
      cd = as<double>(cc_out);
    }
    hipStream_t s;
    if ((rc = points_begin(&s))) return rc;
    const void* dev = nullptr;
    if ((rc = stage_leaves(xa, xs_dtype, xs_mem, m, &dev))) return rc;
    HIPCHECK(hipMemcpyAsync(cc_braw.p, xb, (size_t)b * d * 8, hipMemcpyHostToDevice, s));
    prep_points<double>(s, cc_braw.p, GPSO_F64, 0, b, kBatchMaxPicks, nullptr, as<double>(cc_tb), as<double>(cc_bnorm));
    BatchPickLaunch pk;
    pk.C = as<double>(linv); pk.xs = as<double>(xs64); pk.tb = as<double>(cc_tb); pk.n = n; pk.npad = npad; pk.b = b; pk.dp = dp; pk.kp = kp;
    pk.Kb = as<double>(cc_vec); pk.U = pk.Kb + (size_t)b * npad; pk.W = pk.U + (size_t)b * npad; pk.lv = as<double>(cc_lv);
    if (launch_batch_pick_vectors(s, pk) != 0) return launch_status();
    BatchColLaunch g;
    g.ts = as<double>(cc_ts); g.tnorm = as<double>(cc_norm); g.xs = pk.xs; g.W = pk.W; g.tb = pk.tb; g.bnorm = as<double>(cc_bnorm);
    g.n = n; g.npad = npad; g.b = b; g.dp = dp; g.kp = kp; g.ldc = m;
    for (int64_t off = 0; off < m; off += chunk) {
      const int64_t mc = std::min(chunk, m - off), mpad = (mc + 63) / 64 * 64;
      prep_points<double>(s, dev, xs_dtype, off, mc, mpad, nullptr, as<double>(cc_ts), as<double>(cc_norm));
      g.m = mc;
      g.cov = cd + off;
      if (launch_batch_cross(s, g) != 0) return launch_status();
      if ((rc = launch_status())) return rc;
    }
    if (to_host) HIPCHECK(hipMemcpyAsync(cov, cd, (size_t)b * m * 8, hipMemcpyDeviceToHost, s));
    return points_end(s, m);
  }

  // Round 0 is gpso_acq_values on the batch (the context's predict path: its bits); every later round is double arithmetic
  // on top: pick vectors, one column launch, one finish launch.  All rounds are enqueued back to back, the picks stay on
  // the device, one wait at the end
  int best_batch(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, double obs_noise, int q, int64_t* idx,
                 double* mean, double* var, double* value, int* n_picked, double* var_after, int out_mem) override {
    if constexpr (!kDenseDouble) return ctx->fail(GPSO_E_ARG, "gpso_best_batch needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)");
    ctx->tick_timing();
    if (m < 1) return ctx->fail(GPSO_E_ARG, "gpso_best_batch needs at least one leaf (m=%lld)", (long long)m);
    if (q < 1 || q > kBatchMaxPicks) return ctx->fail(GPSO_E_ARG, "gpso_best_batch picks 1 to %d leaves (q=%d)", kBatchMaxPicks, q);
    if (m > kBatchMaxCells / q) return ctx->fail(GPSO_E_ARG, "gpso_best_batch: q * m above 2^27 (q=%d, m=%lld)", q, (long long)m);
    if (!xs) return ctx->fail(GPSO_E_ARG, "xs must not be NULL");
    if (!idx || !n_picked) return ctx->fail(GPSO_E_ARG, "idx and n_picked must not be NULL");
    if (!(obs_noise >= 0.0) || obs_noise - obs_noise != 0.0) return ctx->fail(GPSO_E_ARG, "obs_noise must be finite and not negative");
    int rc = check_predict_args(xs, xs_dtype, xs_mem, m);
    if (rc) return rc;
    if ((rc = need_dense_factor("gpso_best_batch"))) return rc;
    const int64_t mall = (m + 63) / 64 * 64, nblk = batch_round_blocks(m);
    if ((rc = ensure(bb_ts, (size_t)mall * dp * 8))) return rc;
    if ((rc = ensure(bb_norm, (size_t)mall * 8))) return rc;
    if ((rc = ensure(bb_mean, (size_t)m * 8))) return rc;
    if ((rc = ensure(bb_s2, (size_t)m * 8))) return rc;
    if ((rc = ensure(bb_val, (size_t)m * 8))) return rc;
    if ((rc = ensure(bb_g, (size_t)q * m * 8))) return rc;
    if ((rc = ensure(bb_live, (size_t)m))) return rc;
    if ((rc = ensure(bb_bmax, (size_t)nblk * 16))) return rc;
    if ((rc = ensure(bb_state, sizeof(BatchState)))) return rc;
    if ((rc = ensure(bb_tp, (size_t)kMaxD * 8))) return rc;
    if ((rc = ensure(cc_vec, batch_pick_workspace_doubles(n, npad, 1) * 8))) return rc;
    if ((rc = ensure(cc_lv, (size_t)kBatchMaxPicks * 8))) return rc;
    BatchState* host = reinterpret_cast<BatchState*>(ctx->pinned_scratch(sizeof(BatchState) / 8 + 1));
    if (!host) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    hipStream_t s;
    if ((rc = points_begin(&s))) return rc;
    const void* dev = nullptr;
    if ((rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
    BatchState* state = static_cast<BatchState*>(bb_state.p);
    HIPCHECK(hipMemsetAsync(state, 0, sizeof(BatchState), s));
    double *md = as<double>(bb_mean), *s2d = as<double>(bb_s2), *vald = as<double>(bb_val), *G = as<double>(bb_g);
    double* bmax_v = as<double>(bb_bmax);
    int64_t* bmax_i = reinterpret_cast<int64_t*>(bmax_v + nblk);
    unsigned char* live = static_cast<unsigned char*>(bb_live.p);
    TileSpan span{ctx->timing};
    if ((rc = score_device_leaves(dev, xs_dtype, m, acq, true, md, s2d, vald, span))) return rc;
    for (int64_t off = 0; off < m; off += kBatchChunk) {
      const int64_t mc = std::min(kBatchChunk, m - off), mpad = (mc + 63) / 64 * 64;
      prep_points<double>(s, dev, xs_dtype, off, mc, mpad, nullptr, as<double>(bb_ts) + off * dp, as<double>(bb_norm) + off);
    }
    launch_batch_init(s, vald, m, live, bmax_v, bmax_i);
    BatchPickLaunch pk;
    pk.C = as<double>(linv); pk.xs = as<double>(xs64); pk.tb = as<double>(bb_tp); pk.n = n; pk.npad = npad; pk.b = 1; pk.dp = dp; pk.kp = kp;
    pk.Kb = as<double>(cc_vec); pk.U = pk.Kb + npad; pk.W = pk.U + npad; pk.lv = as<double>(cc_lv); pk.st = state; pk.obs_noise = obs_noise;
    BatchColLaunch g;
    g.ts = as<double>(bb_ts); g.tnorm = as<double>(bb_norm); g.xs = pk.xs; g.W = pk.W; g.tb = pk.tb; g.n = n; g.npad = npad; g.m = m;
    g.dp = dp; g.kp = kp; g.st = state; g.G = G; g.s2 = s2d; g.mean = md; g.live = live; g.acq = acq; g.bmax_v = bmax_v; g.bmax_i = bmax_i;
    for (int t = 0; t < q; ++t) {
      launch_batch_finish(s, state, t, bmax_v, bmax_i, t == 0 ? batch_init_blocks(m) : nblk, g.ts, dp, md, s2d, G, m, live, as<double>(bb_tp));
      const bool last = t == q - 1;
      if (last && !var_after) break;
      pk.t = g.t = t;
      g.rank = !last;
      if (launch_batch_pick_vectors(s, pk) != 0) return launch_status();
      if (launch_batch_round(s, g) != 0) return launch_status();
    }
    if ((rc = launch_status())) return rc;
    HIPCHECK(hipMemcpyAsync(host, state, sizeof(BatchState), hipMemcpyDeviceToHost, s));
    if (var_after)
      HIPCHECK(hipMemcpyAsync(var_after, s2d, (size_t)m * 8, out_mem == GPSO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    if ((rc = points_end(s, m))) return rc;
    collect_tile_ms(span.timed, span.pairs);
    *n_picked = host->n_picked;
    for (int t = 0; t < host->n_picked; ++t) {
      idx[t] = host->idx[t];
      if (mean) mean[t] = host->mean[t];
      if (var) var[t] = host->var[t];
      if (value) value[t] = host->value[t];
    }
    return GPSO_OK;
  }

  // ---- best-UCB sequencing: enqueue the local work (winners stay on the device, no host wait) ->
  //      [multi-GPU: all-gather + fold] -> one read-back ------------------------------------------------
  // ---- one-launch small calls (predict.hip: leaf_tiles_v2_one_kernel) -------------------------------------------------
  // Applies when the native tile kernel runs this posterior with ONE row block (N_pad = 128 or 256) and the batch is
  // small.  Returns 0 when the call was enqueued (records on their way to ovals and pinned host memory), 2 when it does
  // not apply -- the caller goes on with the next-best sequence --, or a negative status.  mode: finish_best's read-back
  DevBuf one_ctl, one_partial, one_ppos;
  template <typename TG>
  int try_one_launch_t(const BestPlan& plan, BestCall& call, OneLaunch& one, int64_t total, int nseg, const AcqSpec& acq, int mode) {
    if (acq.kind == GPSO_ACQ_MES) return 2;  // (the tile kernel's epilogue keeps the maps it had: MES takes the next-best sequence)
    const int64_t cpad = (total + kLeafPad - 1) / kLeafPad * kLeafPad;
    int rc;
    if ((rc = ensure(leaves_s, (size_t)cpad * dp * sizeof(TG)))) return rc;
    if ((rc = ensure(lnorm, (size_t)cpad * sizeof(TG)))) return rc;
    if ((rc = ensure(pvar, (size_t)cpad * 8))) return rc;
    if ((rc = ensure(pmean, (size_t)cpad * 8))) return rc;
    if ((rc = ensure(grow_key, (size_t)cpad * 8))) return rc;
    const size_t wgs = (size_t)(cpad / 64);  // (at most: 64 leaves per workgroup is the smallest tile)
    if ((rc = ensure(one_partial, wgs * nseg * kArgmaxPartialBytes))) return rc;
    if ((rc = ensure(one_ppos, wgs * nseg * 8))) return rc;
    if (one_ctl.p == nullptr) {
      if ((rc = ensure(one_ctl, 64))) return rc;
      HIPCHECK(hipMemsetAsync(one_ctl.p, 0, 64, st()));
    }
    one.total = total;
    one.nseg = nseg;
    one.d = d;
    one.ls = ls_dev();
    one.leaves_s = leaves_s.p;
    one.lnorm = lnorm.p;
    one.key = as<int64_t>(grow_key);
    one.fin = LeafFinalize{as<double>(pvar), as<double>(pmean), 1, cpad, kp.variance, kp.noise, kp.mean_c, acq.varsigma,
                           as<double>(omean), as<double>(ovar), as<double>(oucb), lnorm.p, sizeof(TG) == 8}.with(acq);
    one.partial = one_partial.p;
    one.ppos = as<int64_t>(one_ppos);
    one.ticket = static_cast<unsigned*>(one_ctl.p);
    one.fallback = static_cast<unsigned*>(one_ctl.p) + 1;
    one.out_vals = as<double>(ovals);
    one.host_vals = result_host(plan, call, nseg);
    one.done_token = arm_token(call, true, nseg);  // (the last-arriving workgroup's thread 0 writes every host record, then the token)
    const TG* xsp;
    const TG* xnr;
    if constexpr (sizeof(TG) == 8) {
      xsp = as<double>(xs_p64);
      xnr = as<double>(xnorm64);
    } else {
      xsp = as<float>(xs_p32);
      xnr = as<float>(xnorm32);
    }
    if ((rc = ensure_tile_events(1))) return rc;
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->tile_ev[0], st()));
    rc = launch_leaf_tiles_one<TP, TG>(st(), as<TP>(linv_p), xsp, xnr, as<TP>(alpha), as<double>(pvar), as<double>(pmean),
                                      npad, dp / 4, cpad, kp, one);
    if (rc == 2) {
      call.one_launch_declined();
      return 2;
    }
    if (rc) return launch_status();
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->tile_ev[1], st()));
    call.tiles_recorded(plan.timed ? 1 : 0);
    call.enqueued(BestKind::OneLaunch, nseg, mode);
    return launch_status();
  }
  int try_one_launch(const BestPlan& plan, BestCall& call, OneLaunch& one, int64_t total, int nseg, const AcqSpec& acq, int mode) {
    if (!small_calls || !one_launch || !plan.one_launch || total <= 0 || total > kSmallBestMaxRows || nseg > 16) return 2;
    if (npad != 128 && npad != 256) return 2;
    // measured (tools/micro/one_dbg.py, float64, same box; wall us per best_ucb_grow call, one | three launches):
    // N = 52 / 162 rows 56.3 | 54.1, N = 100 / 1458 rows 61.0 | 59.8, N = 128 / 13122 rows 91.5 | 88.6, N = 256 / 4374 rows
    // 78.4 | 85.7 -- the two agent-scope fences of the last-arriver fold cost what the two launch boundaries they replace
    // cost; the single launch only pays at N_pad = 256
    if (npad == 128 && !one_launch_everywhere) return 2;
    if (math_in_use() != GPSO_MATH_NATIVE) return 2;
    if (ensure_linv_p() != GPSO_OK || res.linv_p != Copy::Valid) return 2;
    if (leaf_tiles_nbi<TP>(npad, dp / 4) != 1) return 2;
    if constexpr (kFloatPredict) {
      if (!gen_double()) {
        int rc = ensure_generation_inputs();
        if (rc) return rc;
        return try_one_launch_t<float>(plan, call, one, total, nseg, acq, mode);
      }
    }
    return try_one_launch_t<double>(plan, call, one, total, nseg, acq, mode);
  }

  // ---- screened calls (screen.hpp, screen.hip) ----------------------------------------------------------
  // The result of a best-UCB call is one record, and the tile kernel spends N^2 flops per leaf on the variance of every leaf.
  // A leaf's mean costs N D.  So: the mean pass (every leaf's mean, the tile kernel's bits), the screen (a leaf survives unless
  // its ucb at zero variance share lies below T' = the largest mean's), the tile kernel on the survivors' compact list, the
  // keyed arg-max over it -- whose last kernel accepts the record or asks for the general sequence (finish_best returns 1).
  // Where: one segment, the reference's rule with a finite varsigma >= 0, float leaves on the device in one chunk, the default
  // float kernels (fp16 split, fp16 contraction, fused step), m above the small calls' limit (GPSO_OPT_SCREEN = 2: any m),
  // and no refusal on this posterior so far.  The survivors' launch has room for as many leaf tiles as fill one round of the
  // chip: CUs / row blocks (at least one) -- more survivors than that is a refusal too.
  // probe: gpso_screen_probe asks -- whatever the option, the batch size and earlier refusals say
  bool screen_applies(int xs_dtype, int64_t m, int nseg, const AcqSpec& acq, bool probe = false) const {
    if (!kFloatPredict || nseg != 1 || m <= 0 || m > kLeafChunk) return false;
    if (!probe && (screen_mode == 0 || res.screen_refused || (screen_mode == 1 && m <= kSmallBestMaxRows))) return false;
    if (acq.kind != GPSO_ACQ_UCB_VAR || acq.latent != 0 || !std::isfinite(acq.varsigma) || acq.varsigma < 0.0) return false;
    if (xs_dtype != GPSO_F32 || !fuse_prep || gen_double() || split_variant != GPSO_SPLIT_KERNEL_AUTO) return false;
    if (!(bf16_usable() && res.linv_b == Copy::Valid && bf16_fits(false))) return false;
    return f16_split() && c16_in_use(false);
  }
  int64_t screen_cap_rows(int64_t mpad) const {
    const int nbi = (int)(npad / 256);
    return std::min<int64_t>(mpad, (int64_t)std::max(1, ctx->cu_count / nbi) * kLeafPad);
  }
  // the mean pass and the screen of a batch of float leaves on the device; probe: also every leaf's ub and flag -> screen_cols
  int enqueue_screen(const void* dev, int64_t m, const AcqSpec& acq, bool probe) {
    if constexpr (kFloatPredict) {
      int rc;
      if ((rc = ensure_generation_inputs())) return rc;
      const int nbi = (int)(npad / 256);
      const int64_t mpad = (m + kLeafPad - 1) / kLeafPad * kLeafPad;
      const int64_t cap = screen_cap_rows(mpad);
      if ((rc = ensure(pmean, (size_t)nbi * mpad * 8))) return rc;
      if ((rc = ensure(pvar, (size_t)nbi * mpad * 8))) return rc;
      if ((rc = ensure(screen_my, (size_t)mpad * 8))) return rc;
      if ((rc = ensure(screen_bmax, (size_t)(mpad / 128) * 8))) return rc;
      if ((rc = ensure(screen_cnt, (size_t)kScreenMaxParts * 8))) return rc;
      if ((rc = ensure(screen_rows, (size_t)cap * d * 4))) return rc;
      if ((rc = ensure(grow_key, (size_t)cap * 8))) return rc;
      if ((rc = ensure_keep(screen_ctl, 64))) return rc;
      if (probe && (rc = ensure(screen_cols, (size_t)2 * m * 8))) return rc;
      hipStream_t s = st();
      LeafMeanLaunch a;
      a.xs_h16 = xs_h16.p; a.alpha = as<float>(alpha); a.c16_scale = as<float>(c16_scal);
      a.raw.x = static_cast<const float*>(dev); a.raw.ls = ls_dev(); a.raw.m = m; a.raw.d = d;
      a.part_mean = as<double>(pmean);
      a.npad = npad; a.mpad = mpad; a.m = m; a.n_rows = n; a.dp4 = dp / 4; a.mean_c = kp.mean_c;
      a.my = as<double>(screen_my); a.block_max = as<double>(screen_bmax);
      ScreenLaunch b;
      a.nblk_out = &b.nblk;
      a.row_loop = row_loop; a.cu_count = ctx->cu_count; a.splits_out = &ctx->last_count[3];
      if ((rc = launch_leaf_mean(s, kp, a))) return launch_status();
      b.m = m;
      b.variance = kp.variance; b.noise = kp.noise; b.varsigma = acq.varsigma;
      b.raw = static_cast<const float*>(dev); b.d = d; b.cap = cap; b.counts = as<int64_t>(screen_cnt);
      b.my = as<double>(screen_my); b.block_max = as<double>(screen_bmax); b.key = as<int64_t>(grow_key);
      b.rows_out = as<float>(screen_rows); b.ctl = as<int64_t>(screen_ctl); b.probe = probe ? as<double>(screen_cols) : nullptr;
      launch_screen(s, b);
      return launch_status();
    } else {
      return ctx->fail(GPSO_E_STATE, "internal: a screened call on a double-predict context");
    }
  }
  // gpso_screen_probe: the mean pass and the screen alone; every leaf's my, ub and survive flag, and what the call would see
  int screen_probe(const void* xs, int xs_dtype, int xs_mem, int64_t m, double varsigma, double* my, double* ub, double* flag,
                   double* info) override {
    int rc = check_predict_args(xs, xs_dtype, xs_mem, m);
    if (rc) return rc;
    const AcqSpec acq(varsigma);
    if (!screen_applies(xs_dtype, m, 1, acq, true))
      return ctx->fail(GPSO_E_STATE, "gpso_screen_probe: no screened call on this context, batch or varsigma (float leaves in one chunk, "
                                     "the fp16 split with the fp16 contraction and the fused step, a finite varsigma >= 0)");
    const void* dev = nullptr;
    if ((rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
    if ((rc = enqueue_screen(dev, m, acq, true))) return rc;
    hipStream_t s = st();
    int64_t ctl[3] = {0, 0, 0};
    if (my) HIPCHECK(hipMemcpyAsync(my, screen_my.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    if (ub) HIPCHECK(hipMemcpyAsync(ub, screen_cols.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    if (flag) HIPCHECK(hipMemcpyAsync(flag, as<double>(screen_cols) + m, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(ctl, screen_ctl.p, 24, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if ((rc = launch_status())) return rc;
    probe_listed = false;
    probe_key.resize((size_t)ctl[0]);
    probe_rows.resize((size_t)ctl[0] * d);
    if (ctl[0] > 0) {
      HIPCHECK(hipMemcpyAsync(probe_key.data(), grow_key.p, (size_t)ctl[0] * 8, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipMemcpyAsync(probe_rows.data(), screen_rows.p, (size_t)ctl[0] * d * 4, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
    }
    probe_listed = true;
    if (info) {
      info[0] = (double)ctl[1];
      std::memcpy(&info[1], &ctl[2], 8);
      info[2] = (double)screen_cap_rows((m + kLeafPad - 1) / kLeafPad * kLeafPad);
    }
    return GPSO_OK;
  }
  // gpso_screen_list: the compact list the last gpso_screen_probe left -- the survivors' indices and raw rows
  int screen_list(int64_t max_rows, int64_t* key, float* rows, int64_t* live) override {
    if (!probe_listed) return ctx->fail(GPSO_E_STATE, "gpso_screen_list: no gpso_screen_probe on this context yet");
    if (max_rows < 0 || (max_rows > 0 && (!key || !rows))) return ctx->fail(GPSO_E_ARG, "gpso_screen_list: NULL output or max_rows < 0");
    const int64_t have = (int64_t)probe_key.size();
    if (live) *live = have;
    const int64_t rows_n = std::min(max_rows, have);
    if (rows_n > 0) {
      std::memcpy(key, probe_key.data(), (size_t)rows_n * 8);
      std::memcpy(rows, probe_rows.data(), (size_t)rows_n * d * 4);
    }
    return GPSO_OK;
  }
  // the whole screened call; the record (and the verdict) on their way to ovals and pinned host memory
  int enqueue_best_screened(const BestPlan& plan, BestCall& call, const void* dev, int64_t m, const AcqSpec& acq) {
    int rc;
    hipStream_t s = st();
    const int64_t mpad = (m + kLeafPad - 1) / kLeafPad * kLeafPad;
    const int64_t cap = screen_cap_rows(mpad);
    if ((rc = ensure(best_pos, (size_t)kArgmaxBlocks * 8))) return rc;
    if ((rc = ensure_tile_events(1))) return rc;
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->tile_ev[0], s));
    ctx->last_count[5] = ctx->last_count[6] = 0;  // (the mean pass parks nothing)
    if ((rc = enqueue_screen(dev, m, acq, false))) return rc;
    LeafFinalize fin{};
    TileSpan span{plan.timed, true};
    if ((rc = score_device_leaves(screen_rows.p, GPSO_F32, cap, acq, true, as<double>(omean), as<double>(ovar), as<double>(oucb),
                                  span, as<int64_t>(screen_ctl), &fin)))
      return rc;
    call.tiles_recorded(span.pairs);
    if (fin.part_var == nullptr) return ctx->fail(GPSO_E_STATE, "internal: the survivors of a screened call were not deferred");
    // (float generation: a NaN coordinate reaches the partial sums by itself, as it does in the unscreened call, whose fused
    // prologue leaves no norms to look at -- the record keeps that NaN's bits, not the finalize stage's own)
    fin.lnorm = nullptr;
    double* host = result_host(plan, call, 1);
    // (the survivors' list as a keyed one of a single segment: no analytic slots, every row in the appended tail, key = the
    // leaf's index in the caller's batch -- the arg-max ranks and tie-breaks on it)
    launch_keyed_argmax(s, as<double>(omean), as<double>(ovar), as<double>(oucb), as<int64_t>(grow_key), m, 0, 1,
                        as<int64_t>(screen_ctl), argmax_blocks(cap, 1), best.p, as<int64_t>(best_pos), as<double>(ovals), &fin,
                        host, arm_token(call, true, 1), as<int64_t>(screen_ctl), cap);
    call.screened(dev, GPSO_F32, m, acq);  // (what a re-run takes: the caller keeps device leaves untouched until the record is read)
    ctx->last_count[0] = ctx->last_count[1] = m;
    return launch_status();
  }

  // per segment (mean, var, ucb, bit-cast index relative to the segment start) -> ovals; seg_off: host,
  // nseg + 1 entries over [0, m]
  // plan.screen: the caller can run the call again should a screened one be refused (device leaves, finish_best's verdict read)
  int enqueue_best_leaves(const BestPlan& plan, BestCall& call, const void* dev, int xs_dtype, int64_t m, const int64_t* seg_off,
                          int nseg, const AcqSpec& acq) {
    int rc;
    call = BestCall::begun(plan);
    if (!plan.is_rerun) ctx->last_count[7] = 0, ctx->last_count[8] = kScreenNone;
    hipStream_t s = st();
    if ((rc = ensure(omean, (size_t)m * 8))) return rc;
    if ((rc = ensure(ovar, (size_t)m * 8))) return rc;
    if ((rc = ensure(oucb, (size_t)m * 8))) return rc;
    if ((rc = ensure(segoff, (size_t)(nseg + 1) * 8))) return rc;
    if ((rc = ensure(best, (size_t)nseg * kArgmaxBlocks * kArgmaxPartialBytes))) return rc;
    if ((rc = ensure(ovals, (size_t)group_payload_doubles(nseg) * 8))) return rc;
    std::vector<int64_t> so;
    if ((rc = checked_segments(m, seg_off, nseg, so, "M"))) return rc;
    if (so != segoff_cache) {  // the segmentation rarely changes between calls: upload only then
      HIPCHECK(hipMemcpyAsync(segoff.p, so.data(), (size_t)(nseg + 1) * 8, hipMemcpyHostToDevice, s));
      HIPCHECK(hipStreamSynchronize(s));
      segoff_cache = so;
    }
    if (plan.screen && screen_applies(xs_dtype, m, nseg, acq)) return enqueue_best_screened(plan, call, dev, m, acq);
    if (m > 0) {  // one launch for the whole call where it applies
      OneLaunch one{};
      one.mode = 2;
      one.raw = dev;
      one.raw_f64 = xs_dtype == GPSO_F64 ? 1 : 0;
      one.seg_off = as<int64_t>(segoff);
      if ((rc = try_one_launch(plan, call, one, m, nseg, acq, 0)) != 2) {
        ctx->last_count[0] = ctx->last_count[1] = m;
        return rc;
      }
    }
    LeafFinalize fin{};
    TileSpan span{plan.timed};
    if (m > 0)
      if ((rc = score_device_leaves(dev, xs_dtype, m, acq, true, as<double>(omean), as<double>(ovar), as<double>(oucb), span, nullptr, &fin))) return rc;
    call.tiles_recorded(span.pairs);
    // (round 4: the leaves of a one-chunk batch are finalised by the arg-max's first stage, and its second stage writes
    // the winners' records straight into the pinned host memory finish_best reads: two launches and a copy less per call)
    double* host = result_host(plan, call, nseg);
    const bool small = small_calls && fin.part_var != nullptr && m <= kSmallBestMaxRows && nseg <= 64;
    if (small) {
      // small batch: finalize and both arg-max stages in one launch of one workgroup
      SmallBest sb{};
      sb.fin = fin;
      sb.seg_off = as<int64_t>(segoff);
      sb.m = m;
      sb.nseg = nseg;
      sb.out_vals = as<double>(ovals);
      sb.host_vals = host;
      sb.done_token = arm_token(call, true, nseg);
      launch_small_best(s, sb, false);
    } else {
      launch_seg_argmax(s, as<double>(omean), as<double>(ovar), as<double>(oucb), as<int64_t>(segoff),
                        nseg, argmax_blocks(m, nseg), best.p, as<double>(ovals), fin.part_var ? &fin : nullptr, host,
                        arm_token(call, nseg == 1, nseg));
    }
    call.enqueued(small ? BestKind::Small : BestKind::General, nseg, 0);
    ctx->last_count[0] = ctx->last_count[1] = m;
    return launch_status();
  }

  // the reference rows [row_lo, row_hi) of the sub-tree under every box, de-duplicated (grow.hip), scored;
  // per segment (mean, var, ucb, bit-cast REFERENCE row index) -> ovals, live row count -> ovals[nseg*4]
  int enqueue_best_grow(const BestPlan& plan, BestCall& call, const double* bounds, int nseg, int depth, int64_t row_lo,
                        int64_t row_hi, const AcqSpec& acq) {
    if (!bounds) return ctx->fail(GPSO_E_ARG, "bounds must not be NULL");
    if (nseg < 1) return ctx->fail(GPSO_E_ARG, "nseg must be >= 1");
    if (depth < 0 || depth > 16) return ctx->fail(GPSO_E_ARG, "depth %d outside [0, 16]", depth);
    int rc;
    call = BestCall::begun(plan);
    TileSpan span{plan.timed};
    hipStream_t s = st();
    const int64_t rows = gpso_grow_rows(depth);
    const int64_t uniq = grow_unique_before(row_hi) - grow_unique_before(row_lo);
    const int64_t cap = (int64_t)nseg * (row_hi - row_lo);  // worst case: no centre child repeats its parent
    const size_t bb = (size_t)nseg * d * 2 * 8;
    const size_t ob = (size_t)cap * d * 8;
    if ((rc = ensure(leaves_raw, ob + bb))) return rc;
    if ((rc = ensure(grow_key, (size_t)std::max<int64_t>(cap, 1) * 8))) return rc;
    if ((rc = ensure_keep(live_cnt, 64))) return rc;
    if ((rc = ensure(omean, (size_t)cap * 8))) return rc;
    if ((rc = ensure(ovar, (size_t)cap * 8))) return rc;
    if ((rc = ensure(oucb, (size_t)cap * 8))) return rc;
    if ((rc = ensure(best, (size_t)nseg * kArgmaxBlocks * kArgmaxPartialBytes))) return rc;
    if ((rc = ensure(best_pos, (size_t)nseg * kArgmaxBlocks * 8))) return rc;
    if ((rc = ensure(ovals, (size_t)group_payload_doubles(nseg) * 8))) return rc;
    // Small calls (the optimiser's exploration levels: a few hundred to a few thousand rows) are launch-bound: boxes by
    // value, growth + input scaling in one launch, tiles, one-workgroup finalize + arg-max writing pinned host memory --
    // three launches and no copy operation instead of two copies in, five launches and a copy back
    if (small_calls && cap > 0 && cap <= kSmallBestMaxRows && nseg <= 64 && (size_t)nseg * d * 2 <= (size_t)kGrowBoxDoubles) {
      if (row_lo == 0 && row_hi == rows && plan.one_launch) {  // one launch for the whole call where it applies
        OneLaunch one{};
        one.mode = 1;
        std::memcpy(one.boxes.b, bounds, bb);
        one.depth = depth;
        one.rows = rows;
        one.uniq = uniq;
        if ((rc = try_one_launch(plan, call, one, (int64_t)nseg * uniq, nseg, acq, 1)) != 2) {
          ctx->last_count[1] = cap;
          return rc;
        }
      }
      const int64_t cpad = (cap + kLeafPad - 1) / kLeafPad * kLeafPad;
      const size_t tg = gen_double() ? 8 : 4;
      if ((rc = ensure(leaves_s, (size_t)cpad * dp * tg))) return rc;
      if ((rc = ensure(lnorm, (size_t)cpad * tg))) return rc;
      if (extra_cnt.p == nullptr) {
        if ((rc = ensure(extra_cnt, 64))) return rc;
        HIPCHECK(hipMemsetAsync(extra_cnt.p, 0, 64, s));
      }
      GrowBoxes gb;
      std::memcpy(gb.b, bounds, bb);
      unsigned long long* extra = static_cast<unsigned long long*>(extra_cnt.p);
      if constexpr (kFloatPredict) {
        if (!gen_double()) {
          if ((rc = ensure_generation_inputs())) return rc;
          launch_grow_unique_prep<float>(s, gb, nseg, d, dp, depth, row_lo, row_hi, ls_dev(), as<float>(leaves_s), as<float>(lnorm), as<int64_t>(grow_key), extra);
        }
      }
      if (gen_double())
        launch_grow_unique_prep<double>(s, gb, nseg, d, dp, depth, row_lo, row_hi, ls_dev(), as<double>(leaves_s), as<double>(lnorm), as<int64_t>(grow_key), extra);
      LeafFinalize fin{};
      if ((rc = score_device_leaves(nullptr, GPSO_F64, cap, acq, true, as<double>(omean), as<double>(ovar), as<double>(oucb), span, nullptr, &fin, true)))
        return rc;
      call.tiles_recorded(span.pairs);
      if (fin.part_var == nullptr) return ctx->fail(GPSO_E_STATE, "internal: small growth call was not deferred");
      SmallBest sb{};
      sb.fin = fin;
      sb.key = as<int64_t>(grow_key);
      sb.rows = rows;
      sb.uniq = uniq;
      sb.base = (int64_t)nseg * uniq;
      sb.extra = extra;
      sb.nseg = nseg;
      sb.out_vals = as<double>(ovals);
      sb.host_vals = result_host(plan, call, nseg);
      sb.done_token = arm_token(call, true, nseg);
      launch_small_best(s, sb, true);
      call.enqueued(BestKind::Small, nseg, 1);
      ctx->last_count[1] = cap;
      return launch_status();
    }
    double* bdev = reinterpret_cast<double*>(static_cast<char*>(leaves_raw.p) + ob);
    double* stage = ctx->pinned_stage((size_t)nseg * d * 2 + 1);
    if (!stage) return ctx->fail(GPSO_E_OOM, "pinned host staging");
    std::memcpy(stage, bounds, bb);
    const int64_t live0 = (int64_t)nseg * uniq;
    std::memcpy(stage + (size_t)nseg * d * 2, &live0, 8);
    HIPCHECK(hipMemcpyAsync(bdev, stage, bb, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(live_cnt.p, stage + (size_t)nseg * d * 2, 8, hipMemcpyHostToDevice, s));
    launch_grow_unique(s, bdev, nseg, d, depth, row_lo, row_hi, as<double>(leaves_raw), as<int64_t>(grow_key),
                       as<int64_t>(live_cnt));
    LeafFinalize fin{};
    if (cap > 0)
      if ((rc = score_device_leaves(leaves_raw.p, GPSO_F64, cap, acq, true, as<double>(omean), as<double>(ovar),
                                    as<double>(oucb), span, as<int64_t>(live_cnt), &fin)))
        return rc;
    call.tiles_recorded(span.pairs);
    double* host = result_host(plan, call, nseg);
    launch_keyed_argmax(s, as<double>(omean), as<double>(ovar), as<double>(oucb), as<int64_t>(grow_key), rows, uniq,
                        nseg, as<int64_t>(live_cnt), argmax_blocks(cap, nseg), best.p, as<int64_t>(best_pos), as<double>(ovals),
                        fin.part_var ? &fin : nullptr, host, arm_token(call, nseg == 1, nseg));
    call.enqueued(BestKind::General, nseg, 1);
    ctx->last_count[1] = cap;
    return launch_status();
  }

  // ---- group calls ---------------------------------------------------------------------------------------
  // Every rank takes part in every collective of a call, whatever happened in its local half: a rank whose half
  // fails (arguments, state, precision gate, allocation) still sends a payload -- no winners and its status in the
  // last slot (kernels.hpp: group_payload_doubles) -- the fold takes the worst status over the ranks, and EVERY rank
  // returns that code.  No rank is left inside a collective by a peer that returned early, and a posterior that
  // fails the precision self-test on the fitting rank makes the whole group return GPSO_E_PRECISION together.
  int ensure_group_buffers(int nseg, int world) {
    int rc;
    const size_t pd = (size_t)group_payload_doubles(nseg);
    if ((rc = ensure(ovals, pd * 8))) return rc;
    if ((rc = ensure(gath, (size_t)world * pd * 8))) return rc;
    if ((rc = ensure(ovals2, pd * 8))) return rc;
    return GPSO_OK;
  }
  // base (host, [world][nseg]): what is added to a rank's winner index to make it relative to the GLOBAL segment
  // start -- the offset of the rank's piece of the segment inside the segment
  static void segment_bases(int64_t m_global, const std::vector<int64_t>& so, int nseg, int world,
                            std::vector<int64_t>& base) {
    base.assign((size_t)world * nseg, 0);
    for (int r = 0; r < world; ++r) {
      int64_t rlo, rhi;
      shard_range(m_global, r, world, &rlo, &rhi);
      for (int i = 0; i < nseg; ++i) base[(size_t)r * nseg + i] = std::min(std::max(so[i], rlo), rhi) - so[i];
    }
  }
  // seg_off (host, nseg + 1 entries over [0, m], NULL: one segment), checked -> so
  int checked_segments(int64_t m, const int64_t* seg_off, int nseg, std::vector<int64_t>& so, const char* m_name = "the global M") {
    so.resize(nseg + 1);
    if (seg_off) {
      for (int i = 0; i <= nseg; ++i) so[i] = seg_off[i];
      if (so[0] != 0 || so[nseg] != m) return ctx->fail(GPSO_E_ARG, "seg_off must start at 0 and end at %s", m_name);
      for (int i = 0; i < nseg; ++i)
        if (so[i + 1] < so[i]) return ctx->fail(GPSO_E_ARG, "seg_off must be non-decreasing");
    } else {
      if (nseg != 1) return ctx->fail(GPSO_E_ARG, "seg_off == NULL requires nseg == 1");
      so[0] = 0;
      so[1] = m;
    }
    return GPSO_OK;
  }
  std::vector<int64_t> wbase_cache;  // what the device copy of the bases holds (they change with the batch shape only)
  int upload_base(const std::vector<int64_t>& base) {
    if (wbase.p != nullptr && base == wbase_cache) return GPSO_OK;
    wbase_cache.clear();
    int rc = ensure(wbase, base.size() * 8);
    if (rc) return rc;
    double* stage = ctx->pinned_stage(base.size());
    if (!stage) return ctx->fail(GPSO_E_OOM, "pinned host staging");
    std::memcpy(stage, base.data(), base.size() * 8);
    HIPCHECK(hipMemcpyAsync(wbase.p, stage, base.size() * 8, hipMemcpyHostToDevice, st()));
    wbase_cache = base;
    return GPSO_OK;
  }
  // local half of gpso_best_ucb_sharded for (rank, world): rows shard_range(m_global, rank, world) of the batch ->
  // this rank's per-segment winners in ovals (indices relative to the LOCAL piece of each segment), status slot 0
  // (plan: BestPlan::group_half -- the general sequences for leaves, the sequences with the append counter for grown calls)
  int sharded_local(const BestPlan& plan, BestCall& call, int rank, int world, const void* xs, int xs_dtype, int xs_mem, int64_t m_local, int64_t m_global,
                    const int64_t* seg_off, int nseg, double varsigma) {
    int rc = check_predict_args(xs, xs_dtype, xs_mem, m_local);
    if (rc) return rc;
    int64_t lo, hi;
    shard_range(m_global, rank, world, &lo, &hi);
    if (m_local != hi - lo)
      return ctx->fail(GPSO_E_ARG, "rank %d of %d must pass rows [%lld, %lld) of the %lld leaves (gpso_shard_range), got %lld rows",
                       rank, world, (long long)lo, (long long)hi, (long long)m_global, (long long)m_local);
    std::vector<int64_t> so, sl(nseg + 1);
    if ((rc = checked_segments(m_global, seg_off, nseg, so))) return rc;
    // local segmentation: the part of every global segment inside [lo, hi)
    for (int i = 0; i <= nseg; ++i) sl[i] = std::min(std::max(so[i], lo), hi) - lo;
    const void* dev = nullptr;
    if (m_local > 0 && (rc = stage_leaves(xs, xs_dtype, xs_mem, m_local, &dev))) return rc;
    return enqueue_best_leaves(plan, call, dev, xs_dtype, m_local, sl.data(), nseg, varsigma);
  }
  int sharded_local_grow(const BestPlan& plan, BestCall& call, int rank, int world, const double* bounds, int nseg, int depth, double varsigma) {
    if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "no posterior resident: call gpso_broadcast_posterior first");
    int rc = precision_gate();
    if (rc) return rc;
    int64_t lo, hi;
    shard_range(gpso_grow_rows(depth), rank, world, &lo, &hi);
    return enqueue_best_grow(plan, call, bounds, nseg, depth, lo, hi, varsigma);
  }
  // after the local half: on failure replace whatever it left in ovals by "no winner" rows and the status
  // (on success the arg-max kernels have written the status slot themselves: no host step on the fast path)
  int publish_local(int nseg, int local_rc) {
    if (local_rc == GPSO_OK) return GPSO_OK;
    const std::string keep = ctx->err;  // the local half's message
    hipStream_t s = st();
    const size_t pd = (size_t)group_payload_doubles(nseg);
    double* stage = ctx->pinned_stage(pd);  // (waits for the stream)
    if (!stage) return ctx->fail(GPSO_E_OOM, "pinned host staging");
    const int64_t none = -1;
    for (int i = 0; i < nseg; ++i) {
      stage[4 * i] = stage[4 * i + 1] = stage[4 * i + 2] = std::nan("");
      std::memcpy(&stage[4 * i + 3], &none, 8);
    }
    stage[4 * nseg] = 0.0;
    stage[4 * nseg + 1] = (double)local_rc;
    HIPCHECK(hipMemcpyAsync(ovals.p, stage, pd * 8, hipMemcpyHostToDevice, s));
    ctx->err = keep;
    return GPSO_OK;
  }
  // multi-GPU: all-gather every rank's payload and fold the winners with the arg-max rule on (ucb, global index)
  // and the statuses with min; base = wbase (uploaded before the local half) or none.  Result -> ovals2.
  int exchange_winners(const BestPlan& plan, BestCall& call, int nseg, bool with_base) {
    hipStream_t s = st();
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->ev[6], s));
    RCCLCHECK(RcclApi::get().AllGather(ovals.p, gath.p, (size_t)group_payload_doubles(nseg), ncclDouble, ctx->comm, s));
    enqueue_fold(plan, call, ctx->world, nseg, with_base, plan.timed);
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->ev[7], s));
    return launch_status();
  }
  // gath [world] payloads -> ovals2 and, straight from the kernel, the pinned memory finish_best reads
  void enqueue_fold(const BestPlan& plan, BestCall& call, int world, int nseg, bool with_base, bool collective_recorded) {
    double* host = result_host(plan, call, nseg);
    launch_reduce_winners(st(), as<double>(gath), with_base ? as<int64_t>(wbase) : nullptr, world, nseg, group_payload_doubles(nseg),
                          as<double>(ovals2), host, arm_token(call, nseg <= 64, nseg));
    call.folded(nseg, collective_recorded);
  }

  // Consumes the record: the host wait, then nseg x (mean, var, ucb, index) [+ the live row count] [+ the group's verdict]
  // out of the pinned memory the call's last kernel wrote.  done: a ticket's completion event (NULL: the whole stream).
  // call.mode 0: winners only; 1: + live count -> last_count[0]; 2: a folded group payload -- *verdict_out: the worst status
  // of the group (*who: its rank); outputs written only when that is GPSO_OK.  Returns 1: finish_or_rerun
  int finish_best(BestCall& in_flight, hipEvent_t done, int64_t* idx, double* mean, double* var, double* ucb,
                  int* verdict_out = nullptr, int64_t* who = nullptr) {
    const BestCall call = in_flight.consumed();
    hipStream_t s = st();
    const int nseg = call.nseg;
    double* vals = call.host;
    if (vals == nullptr) {  // (no pinned memory when the call was enqueued: a copy operation)
      if (!(vals = ctx->pinned_scratch((size_t)nseg * 4 + 2))) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
      HIPCHECK(hipMemcpyAsync(vals, call.mode == 2 ? ovals2.p : ovals.p, ((size_t)nseg * 4 + 2) * 8, hipMemcpyDeviceToHost, s));
      done = nullptr;
    }
    if (call.timed) HIPCHECK(hipEventRecord(ctx->ev[3], s));
    if (call.token != 0.0) HIPCHECK(ctx->wait_token(&vals[4 * nseg + 2], call.token, s));
    else if (done != nullptr) HIPCHECK(ctx->wait_event(done));
    else HIPCHECK(ctx->wait(s));
    int rc;
    if ((rc = launch_status())) return rc;
    collect_tile_ms(call.timed, call.tile_pairs);
    float ms = 0;
    if (call.timed && hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->last_ms[1] = ms;
    if (call.coll_timed && hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]) == hipSuccess) ctx->last_ms[3] = ms;
    // (a centre child does not repeat its parent: the caller re-runs)
    if (call.kind == BestKind::OneLaunch && vals[4 * nseg + 1] != 0.0) return 1;
    if (call.kind == BestKind::Screened) {
      ctx->last_count[0] = ctx->last_count[1] = call.screen.m;  // (a ticket: other calls have run since it was enqueued)
      if ((rc = screen_verdict(vals))) return rc;
    }
    if (call.mode == 2) {
      const int verdict = (int)vals[4 * nseg + 1];
      if (verdict_out) *verdict_out = verdict;
      if (who) std::memcpy(who, &vals[4 * nseg], 8);
      if (verdict != GPSO_OK) return GPSO_OK;  // (outputs untouched; the caller turns the verdict into its return value)
    }
    for (int i = 0; i < nseg; ++i) {  // (the one read-out: a ticket's end comes through here too)
      if (idx) std::memcpy(&idx[i], &vals[4 * i + 3], 8);
      if (mean) mean[i] = vals[4 * i];
      if (var) var[i] = vals[4 * i + 1];
      if (ucb) ucb[i] = vals[4 * i + 2];
    }
    if (call.mode == 1) std::memcpy(&ctx->last_count[0], &vals[4 * nseg], 8);
    return GPSO_OK;
  }
  // finish; where the call asks for the general sequence (a screened call was refused -- its posterior is not screened again
  // --, the one-launch kernel met a near-duplicate it has no slot for), enqueue it again under plan.rerun() and finish that
  template <typename Enqueue>
  int finish_or_rerun(const BestPlan& plan, BestCall& call, hipEvent_t done, Enqueue&& enqueue, int64_t* idx, double* mean,
                      double* var, double* ucb) {
    int rc = finish_best(call, done, idx, mean, var, ucb);
    if (rc != 1) return rc;
    if ((rc = enqueue(plan.rerun(), call))) return rc;
    return finish_best(call, nullptr, idx, mean, var, ucb);
  }
  // a screened call's record (one segment): the survivors' count and the last kernel's verdict -> the counters; a refusal ends
  // screening on this posterior and returns 1 -- the caller runs the call again, which then takes the general sequence
  int screen_verdict(const double* vals) {
    std::memcpy(&ctx->last_count[7], &vals[4], 8);
    const bool refused = vals[5] != 0.0;
    ctx->last_count[8] = refused ? kScreenRefused : kScreenAccepted;
    if (refused) res.screen_was_refused();
    return refused ? 1 : 0;
  }
  // the group's verdict as this rank's return value: its own failure keeps its own message
  int group_verdict(int verdict, int64_t who, int local_rc, const std::string& local_msg, const char* call) {
    if (verdict == GPSO_OK) return GPSO_OK;
    if (local_rc != GPSO_OK) {
      ctx->err = local_msg;
      return local_rc;
    }
    return ctx->fail(verdict, "%s: rank %lld of the group failed its half of the call with status %d (its message is "
                     "on that rank); every rank returns together", call, (long long)who, verdict);
  }

  int best_ucb(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
               const AcqSpec& acq, int64_t* idx, double* mean, double* var, double* ucb) override {
    ctx->tick_timing();
    int rc = check_predict_args(xs, xs_dtype, xs_mem, m);
    if (rc) return rc;
    if (nseg < 1) return ctx->fail(GPSO_E_ARG, "nseg must be >= 1");
    const BestPlan plan = BestPlan::synchronous(ctx->timing, xs_mem == GPSO_MEM_DEVICE);
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->ev[2], st()));
    const void* dev = nullptr;
    if (m > 0 && (rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
    auto enqueue = [&](const BestPlan& p, BestCall& c) { return enqueue_best_leaves(p, c, dev, xs_dtype, m, seg_off, nseg, acq); };
    BestCall call;
    if ((rc = enqueue(plan, call))) return rc;
    return finish_or_rerun(plan, call, nullptr, enqueue, idx, mean, var, ucb);
  }

  // ---- the non-blocking pair (round 5): gpso_best_ucb_begin / gpso_best_ucb_grow_begin enqueue a call and return a
  // ticket; gpso_best_ucb_end waits for THAT call and reads its records.  Two calls may be in flight: the device work of
  // the second is queued while the first still runs, so the GPU never idles over the host's round trip (pinned-memory
  // read, ctypes, Python: 42 us of a 0.77 ms step at C3, profiles/r04_step_timeline.txt).  Every call has its own pinned
  // result slot -- the arg-max kernels write their records there -- and a completion event; the device-side scratch is
  // shared and ordered by the stream.  The ticket (best_call.hpp: BestTicket) holds the enqueue's record until _end consumes
  // it.  BestPlan::ticket: no timing events, no one-launch kernel; a screened call carries what _end needs to run it again.
  int best_ucb_begin(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, const AcqSpec& acq,
                     const double* bounds, int depth) override {
    const bool grown = bounds != nullptr;
    if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "no posterior resident: call gpso_fit_eval / gpso_set_posterior first");
    if (nseg < 1 || (size_t)nseg * 4 + 3 > gpso_ctx::kSlotDoubles) return ctx->fail(GPSO_E_ARG, "nseg must be in [1, 1024] for an asynchronous call");
    int rc = grown ? precision_gate() : check_predict_args(xs, xs_dtype, xs_mem, m);
    if (rc) return rc;
    // any free slot (the round-robin one first): calls may be ended out of order, so after begin A, begin B, end B the free slot
    // is the one next_ticket does NOT name -- refuse only when both hold a call
    int k = ctx->next_ticket;
    if (ctx->tickets[k].in_use) k = (k + 1) % gpso_ctx::kSlots;
    if (ctx->tickets[k].in_use)
      return ctx->fail(GPSO_E_STATE, "two asynchronous best-UCB calls are already in flight: end one (gpso_best_ucb_end) first");
    if (ctx->slot_host == nullptr) {
      if (hipHostMalloc(reinterpret_cast<void**>(&ctx->slot_host), gpso_ctx::kSlots * gpso_ctx::kSlotDoubles * 8, hipHostMallocCoherent) != hipSuccess)
        return ctx->fail(GPSO_E_OOM, "pinned result slots");
      std::memset(ctx->slot_host, 0, gpso_ctx::kSlots * gpso_ctx::kSlotDoubles * 8);
      for (auto& t : ctx->tickets) HIPCHECK(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming));
    }
    const BestPlan plan = BestPlan::ticket(ctx->slot_host + (size_t)k * gpso_ctx::kSlotDoubles, xs_mem == GPSO_MEM_DEVICE);
    BestCall call;
    if (grown) {
      rc = enqueue_best_grow(plan, call, bounds, nseg, depth, 0, gpso_grow_rows(depth), acq);
    } else {
      const void* dev = nullptr;
      if (m > 0) rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev);
      if (rc == GPSO_OK) rc = enqueue_best_leaves(plan, call, dev, xs_dtype, m, seg_off, nseg, acq);
    }
    if (rc) return rc;
    if (xs_mem == GPSO_MEM_HOST && !grown && m > 0) HIPCHECK(hipStreamSynchronize(st()));  // (the caller's host leaves are free again on return)
    HIPCHECK(hipEventRecord(ctx->tickets[k].ev, st()));
    ctx->tickets[k].store(call);
    ctx->next_ticket = (k + 1) % gpso_ctx::kSlots;
    return k;
  }
  // (a refused screened call runs the general sequence now, behind whatever the stream still holds, untimed like every ticket)
  int best_ucb_end(int ticket, int64_t* idx, double* mean, double* var, double* ucb) override {
    if (ticket < 0 || ticket >= gpso_ctx::kSlots || !ctx->tickets[ticket].in_use)
      return ctx->fail(GPSO_E_ARG, "ticket %d names no asynchronous call in flight", ticket);
    BestCall call = ctx->tickets[ticket].take();
    const BestCall::Rerun sc = call.screen;
    auto again = [&](const BestPlan& p, BestCall& c) { return enqueue_best_leaves(p, c, sc.xs, sc.xs_dtype, sc.m, nullptr, 1, sc.acq); };
    return finish_or_rerun(BestPlan::ticket(call.host, true), call, ctx->tickets[ticket].ev, again, idx, mean, var, ucb);
  }

  int need_comm() {
    if (ctx->comm == nullptr) return ctx->fail(GPSO_E_STATE, "this context is not part of a group: call gpso_comm_init first");
    if (ctx->comm_aborted.load())
      return ctx->fail(GPSO_E_STATE, "the communicator of this context was aborted (gpso_comm_abort): gpso_comm_destroy + "
                                     "gpso_comm_init again before the next group call");
    return GPSO_OK;
  }

  // This rank's contiguous share of a batch of m_global leaves (rows shard_range(m_global, rank, world) of
  // it) -> the GLOBAL per-segment winners, identical on every rank and identical to gpso_best_ucb on the
  // whole batch.  seg_off (host, nseg + 1 entries over [0, m_global], NULL: one segment) is global.
  int best_ucb_sharded(const void* xs, int xs_dtype, int xs_mem, int64_t m_local, int64_t m_global,
                       const int64_t* seg_off, int nseg, double varsigma, int64_t* idx, double* mean,
                       double* var, double* ucb) override {
    ctx->tick_timing();
    int rc = need_comm();
    if (rc) return rc;
    // (arguments every rank passes alike fail alike: no collective has started yet)
    if (nseg < 1) return ctx->fail(GPSO_E_ARG, "nseg must be >= 1");
    if (m_global < 0) return ctx->fail(GPSO_E_ARG, "negative global leaf count");
    std::vector<int64_t> so, base;
    if ((rc = checked_segments(m_global, seg_off, nseg, so))) return rc;
    if ((rc = ensure_group_buffers(nseg, ctx->world))) return rc;
    const BestPlan plan = BestPlan::group_half(ctx->timing);
    BestCall call = BestCall::begun(plan);
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->ev[2], st()));
    segment_bases(m_global, so, nseg, ctx->world, base);
    int local = upload_base(base);
    if (local == GPSO_OK)
      local = sharded_local(plan, call, ctx->rank, ctx->world, xs, xs_dtype, xs_mem, m_local, m_global, seg_off, nseg, varsigma);
    return finish_group(plan, call, nseg, true, local, "gpso_best_ucb_sharded", idx, mean, var, ucb);
  }
  // behind the local half of a group call (grown: without bases): every rank publishes its payload, takes part in the
  // exchange, finishes the folded record and returns the group's verdict
  int finish_group(const BestPlan& plan, BestCall& call, int nseg, bool with_base, int local, const char* name, int64_t* idx,
                   double* mean, double* var, double* ucb) {
    const std::string local_msg = ctx->err;
    int rc, verdict = GPSO_OK;
    int64_t who = -1;
    if ((rc = publish_local(nseg, local))) return rc;
    if ((rc = exchange_winners(plan, call, nseg, with_base))) return rc;
    if ((rc = finish_best(call, nullptr, idx, mean, var, ucb, &verdict, &who))) return rc;
    if (!with_base) ctx->last_count[0] = -1;  // (grown: the local live count stays on the device, no second read-back)
    return group_verdict(verdict, who, local, local_msg, name);
  }

  // ------------------------------------------------------------------------------------------
  int grow_to_device(const double* bounds, int nseg, int d_, int depth, int64_t* rows_out) {
    if (!bounds) return ctx->fail(GPSO_E_ARG, "bounds must not be NULL");
    if (nseg < 1) return ctx->fail(GPSO_E_ARG, "nseg must be >= 1");
    if (d_ < 1 || d_ > kMaxD) return ctx->fail(GPSO_E_ARG, "input dimension %d outside [1, %d]", d_, kMaxD);
    if (depth < 0 || depth > 16) return ctx->fail(GPSO_E_ARG, "depth %d outside [0, 16]", depth);
    const int64_t rows = gpso_grow_rows(depth);
    *rows_out = rows;
    int rc;
    const size_t bb = (size_t)nseg * d_ * 2 * 8;
    const size_t ob = (size_t)nseg * rows * d_ * 8;
    // bounds live behind the generated rows in the same buffer
    if ((rc = ensure(leaves_raw, ob + bb))) return rc;
    double* bdev = reinterpret_cast<double*>(static_cast<char*>(leaves_raw.p) + ob);
    double* stage = ctx->pinned_stage((size_t)nseg * d_ * 2);
    if (!stage) return ctx->fail(GPSO_E_OOM, "pinned host staging");
    std::memcpy(stage, bounds, bb);
    HIPCHECK(hipMemcpyAsync(bdev, stage, bb, hipMemcpyHostToDevice, st()));
    launch_grow(st(), bdev, nseg, d_, depth, as<double>(leaves_raw));
    return launch_status();
  }

  int grow(const double* bounds, int nseg, int d_, int depth, double* out) override {
    if (!out) return ctx->fail(GPSO_E_ARG, "out must not be NULL");
    int64_t rows = 0;
    int rc = grow_to_device(bounds, nseg, d_, depth, &rows);
    if (rc) return rc;
    if (rows > 0)
      HIPCHECK(hipMemcpyAsync(out, leaves_raw.p, (size_t)nseg * rows * d_ * 8, hipMemcpyDeviceToHost, st()));
    HIPCHECK(hipStreamSynchronize(st()));
    return GPSO_OK;
  }

  // One exploration level: the sub-tree centres of every box are generated on the device WITHOUT the rows
  // that repeat an earlier row bit for bit (a centre child repeats its parent: 1/3 of the reference's
  // list, gpso/param_space.py:186-200), scored, and the winner is reported by its REFERENCE row index --
  // the result is what gp_eval_best_ucb(leaf.grow(depth)) returns (grow.hip: grow_unique_kernel).
  int best_ucb_grow(const double* bounds, int nseg, int depth, const AcqSpec& acq, int64_t* idx,
                    double* mean, double* var, double* ucb) override {
    ctx->tick_timing();
    if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "no posterior resident: call gpso_fit_eval / gpso_set_posterior first");
    int rc = precision_gate();
    if (rc) return rc;
    const BestPlan plan = BestPlan::synchronous(ctx->timing, false);
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->ev[2], st()));
    auto enqueue = [&](const BestPlan& p, BestCall& c) { return enqueue_best_grow(p, c, bounds, nseg, depth, 0, gpso_grow_rows(depth), acq); };
    BestCall call;
    if ((rc = enqueue(plan, call))) return rc;
    return finish_or_rerun(plan, call, nullptr, enqueue, idx, mean, var, ucb);
  }

  // The same on a group: every rank generates and scores the reference rows shard_range(rows, rank, world)
  // of every box (no leaf crosses a link: O(D) bytes in); the winners are all-gathered and folded on the
  // (ucb, reference row index) order.  Identical result on every rank, identical to gpso_best_ucb_grow.
  int best_ucb_grow_sharded(const double* bounds, int nseg, int depth, double varsigma, int64_t* idx,
                            double* mean, double* var, double* ucb) override {
    ctx->tick_timing();
    int rc = need_comm();
    if (rc) return rc;
    if (nseg < 1) return ctx->fail(GPSO_E_ARG, "nseg must be >= 1");
    if (depth < 0 || depth > 16) return ctx->fail(GPSO_E_ARG, "depth %d outside [0, 16]", depth);
    if ((rc = ensure_group_buffers(nseg, ctx->world))) return rc;
    const BestPlan plan = BestPlan::group_half(ctx->timing);
    BestCall call = BestCall::begun(plan);
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->ev[2], st()));
    const int local = sharded_local_grow(plan, call, ctx->rank, ctx->world, bounds, nseg, depth, varsigma);
    return finish_group(plan, call, nseg, false, local, "gpso_best_ucb_grow_sharded", idx, mean, var, ucb);
  }

  // ---- the two halves on their own, for an arbitrary (rank, world) and without a communicator: what a group of
  // `world` ranks computes can be replayed on ONE device, the all-gather replaced by the caller's concatenation ----
  int shard_winners(int rank, int world, const void* xs, int xs_dtype, int xs_mem, int64_t m_local, int64_t m_global,
                    const int64_t* seg_off, int nseg, double varsigma, double* payload) override {
    BestPlan plan;
    BestCall call;
    const int rc = half_begun(rank, world, nseg, payload, plan, call);
    if (rc) return rc;
    return payload_out(call, nseg, sharded_local(plan, call, rank, world, xs, xs_dtype, xs_mem, m_local, m_global, seg_off, nseg, varsigma), payload);
  }
  int shard_winners_grow(int rank, int world, const double* bounds, int nseg, int depth, double varsigma,
                         double* payload) override {
    BestPlan plan;
    BestCall call;
    const int rc = half_begun(rank, world, nseg, payload, plan, call);
    if (rc) return rc;
    return payload_out(call, nseg, sharded_local_grow(plan, call, rank, world, bounds, nseg, depth, varsigma), payload);
  }
  // what the two share in front of the half: the arguments, the buffers, the half's plan, the call's first event
  int half_begun(int rank, int world, int nseg, const double* payload, BestPlan& plan, BestCall& call) {
    ctx->tick_timing();
    if (!payload) return ctx->fail(GPSO_E_ARG, "payload must not be NULL");
    if (world < 1 || rank < 0 || rank >= world) return ctx->fail(GPSO_E_ARG, "rank %d / world %d", rank, world);
    if (nseg < 1) return ctx->fail(GPSO_E_ARG, "nseg must be >= 1");
    const int rc = ensure_group_buffers(nseg, world);
    if (rc) return rc;
    plan = BestPlan::group_half(ctx->timing);
    call = BestCall::begun(plan);
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->ev[2], st()));
    return GPSO_OK;
  }
  // consumes the half's record: the payload is copied from the device, whatever the half's last kernel wrote to pinned memory
  int payload_out(BestCall& in_flight, int nseg, int local, double* payload) {
    const BestCall call = in_flight.consumed();
    const std::string local_msg = ctx->err;
    int rc = publish_local(nseg, local);
    if (rc) return rc;
    const size_t pd = (size_t)group_payload_doubles(nseg);
    HIPCHECK(hipMemcpyAsync(payload, ovals.p, pd * 8, hipMemcpyDeviceToHost, st()));
    HIPCHECK(hipStreamSynchronize(st()));
    collect_tile_ms(call.timed, call.tile_pairs);
    ctx->err = local_msg;
    return local;  // (the payload carries the same status in its last slot)
  }
  // gathered [world][group_payload_doubles(nseg)] (host, rank order) -> the group's result.  m_global >= 0: payloads
  // of gpso_shard_winners (indices relative to local segment pieces: the bases are added); < 0: of
  // gpso_shard_winners_grow (global reference row indices)
  int fold_winners(const double* gathered, int world, int64_t m_global, const int64_t* seg_off, int nseg, int64_t* idx,
                   double* mean, double* var, double* ucb) override {
    ctx->tick_timing();
    if (!gathered) return ctx->fail(GPSO_E_ARG, "gathered must not be NULL");
    if (world < 1 || nseg < 1) return ctx->fail(GPSO_E_ARG, "world %d / nseg %d", world, nseg);
    int rc = ensure_group_buffers(nseg, world);
    if (rc) return rc;
    hipStream_t s = st();
    const BestPlan plan = BestPlan::synchronous(ctx->timing, false);
    if (plan.timed) HIPCHECK(hipEventRecord(ctx->ev[2], s));
    const bool with_base = m_global >= 0;
    if (with_base) {
      std::vector<int64_t> so, base;
      if ((rc = checked_segments(m_global, seg_off, nseg, so))) return rc;
      segment_bases(m_global, so, nseg, world, base);
      if ((rc = upload_base(base))) return rc;
    }
    const int pd = group_payload_doubles(nseg);
    HIPCHECK(hipMemcpyAsync(gath.p, gathered, (size_t)world * pd * 8, hipMemcpyHostToDevice, s));
    BestCall call = BestCall::begun(plan);
    enqueue_fold(plan, call, world, nseg, with_base, false);
    if ((rc = launch_status())) return rc;
    int64_t who = -1;
    int verdict = GPSO_OK;
    if ((rc = finish_best(call, nullptr, idx, mean, var, ucb, &verdict, &who))) return rc;
    if (verdict != GPSO_OK)
      return ctx->fail(verdict, "gpso_fold_winners: the payload of rank %lld carries status %d", (long long)who, verdict);
    return GPSO_OK;
  }

  // Make the posterior resident on `root` resident on every rank of the group: a 48-byte header (shape,
  // arithmetic options and the root's status), checked on every rank and agreed with an all-reduce(min) so that
  // either all ranks go on or all return the same code; the receivers' allocation is agreed the same way; then
  // ONE RCCL broadcast of the contiguous range of the posterior arena this posterior uses (posterior_span), straight
  // out of / into the library's device memory, on the context's stream.  A posterior that fails the precision self-test on the root is NOT sent:
  // every rank returns GPSO_E_PRECISION (the root is the only rank that can test it -- it holds the targets).
  int agree_min(int64_t* hd_slot, int64_t* host_slot, int64_t mine, int64_t* agreed) {
    RcclApi& R = RcclApi::get();
    hipStream_t s = st();
    *host_slot = mine;
    HIPCHECK(hipMemcpyAsync(hd_slot, host_slot, 8, hipMemcpyHostToDevice, s));
    RCCLCHECK(R.AllReduce(hd_slot, hd_slot, 1, ncclInt64, ncclMin, ctx->comm, s));
    HIPCHECK(hipMemcpyAsync(host_slot, hd_slot, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    *agreed = *host_slot;
    return GPSO_OK;
  }
  int broadcast_posterior(int root) override {
    int rc = need_comm();
    if (rc) return rc;
    RcclApi& R = RcclApi::get();
    if (root < 0 || root >= ctx->world) return ctx->fail(GPSO_E_ARG, "root %d outside the group of %d", root, ctx->world);
    hipStream_t s = st();
    const bool is_root = ctx->rank == root;
    if ((rc = ensure(bhdr, 128))) return rc;
    int64_t* hd = as<int64_t>(bhdr);
    int64_t* host = reinterpret_cast<int64_t*>(ctx->pinned_scratch(8));
    if (!host) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    int64_t mine = GPSO_OK;  // this rank's status of the call so far
    std::string why;
    if (is_root) {
      // still take part in the collectives below when something is wrong: every rank must leave together
      if (!res.has_post()) {
        mine = ctx->fail(GPSO_E_STATE, "gpso_broadcast_posterior: the root has no posterior resident");
      } else if ((rc = decide_generation()) != GPSO_OK) {
        mine = rc;
      } else if (can_selftest()) {
        if ((rc = selftest_with_fallback()) != GPSO_OK) mine = rc;  // (settles GPSO_MATH_AUTO)
        else if (!st_pass()) mine = precision_gate();                // GPSO_E_PRECISION with the measured errors
      }
      why = ctx->err;
    }
    // the predict math the posterior travels with (under GPSO_MATH_AUTO the root's self-test has chosen)
    // (bit 12: GPSO_MATH_AUTO -- its split buffer has room for three planes whatever the rung, so the option itself must agree)
    const int64_t my_opts = (int64_t)(res.math_native_fallback ? GPSO_MATH_NATIVE : res.math) | ((int64_t)math_auto << 12) | ((int64_t)ctx->dtype << 16);
    // the ONE range of the root's posterior arena that travels (offset and length are the same on every rank: the
    // arena's layout depends on the shape and the types only)
    void* span_ptr = nullptr;
    int64_t span_off = 0, span_bytes = 0;
    if (is_root && mine == GPSO_OK && (rc = posterior_span(&span_ptr, &span_off, &span_bytes)) != GPSO_OK) {
      mine = rc;
      why = ctx->err;
    }
    if (is_root) {
      host[0] = n; host[1] = d; host[2] = my_opts; host[3] = mine; host[4] = host[5] = 0; host[6] = span_off; host[7] = span_bytes;
      HIPCHECK(hipMemcpyAsync(hd, host, 64, hipMemcpyHostToDevice, s));
    }
    RCCLCHECK(R.Broadcast(hd, hd, 64, ncclChar, root, ctx->comm, s));
    HIPCHECK(hipMemcpyAsync(host, hd, 64, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    const int64_t rn = host[0], rd = host[1], ropts = host[2], root_status = host[3];
    span_off = host[6];
    span_bytes = host[7];
    if (!is_root && root_status == GPSO_OK) {
      const int64_t rmath = ropts & 0xfff, rauto = (ropts >> 12) & 1, rdtype = ropts >> 16;
      if (rdtype == (int64_t)ctx->dtype && math_auto && rauto &&
          (rmath == GPSO_MATH_F16X3 || rmath == GPSO_MATH_BF16X6 || rmath == GPSO_MATH_NATIVE)) {
        // the root's choice (its self-test ruled): the rung of the ladder, or the f32 MFMA kernel
        res.ladder_follows((int)rmath, kFloatPredict);
      } else if (rdtype != (int64_t)ctx->dtype || rmath != res.math || rauto != (int64_t)math_auto) {
        mine = ctx->fail(GPSO_E_ARG, "gpso_broadcast_posterior: dtype / predict math options differ from the root's");
        why = ctx->err;
      }
    }
    // agree: min over the ranks (slot 4 of the header block); the root's status counts on every rank
    int64_t agreed = 0;
    if ((rc = agree_min(hd + 4, host + 4, std::min<int64_t>(mine, root_status), &agreed))) return rc;
    if (agreed != GPSO_OK) {
      if (mine != GPSO_OK) {
        ctx->err = why;
        return (int)mine;
      }
      return ctx->fail((int)agreed, "gpso_broadcast_posterior: %s (status %d); every rank returns together",
                       root_status != GPSO_OK ? "the root cannot send its posterior" : "another rank of the group cannot take the root's posterior",
                       (int)agreed);
    }
    // receivers allocate; agreed again, so that an allocation failure leaves no rank inside the broadcasts
    mine = is_root ? GPSO_OK : alloc_posterior(rn, (int)rd);
    if (mine == GPSO_OK && !is_root) mine = posterior_span_at(span_off, span_bytes, &span_ptr);
    why = ctx->err;
    if ((rc = agree_min(hd + 5, host + 5, mine, &agreed))) return rc;
    if (agreed != GPSO_OK) {
      if (mine != GPSO_OK) {
        ctx->err = why;
        return (int)mine;
      }
      return ctx->fail((int)agreed, "gpso_broadcast_posterior: a rank of the group could not allocate the posterior (status %d)", (int)agreed);
    }
    RCCLCHECK(R.Broadcast(span_ptr, span_ptr, (size_t)span_bytes, ncclChar, root, ctx->comm, s));
    ctx->last_count[0] = ctx->last_count[1] = span_bytes;  // (gpso_last_count after a broadcast: the bytes that travelled)
    if (!is_root) {
      if ((rc = adopt_posterior())) return rc;  // (synchronises the stream)
    } else {
      HIPCHECK(ctx->wait(s));
    }
    return posterior_mark_synced();  // every rank: the group holds these n rows in this math at this scale
  }

  // ---- the peers of a group brought up to date after gpso_append: only what the appends wrote travels -----------------------
  int posterior_mark_synced() override {
    if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "no posterior resident");
    float scale = 0.0f;
    int rc = current_split_scale(&scale);
    if (rc) return rc;
    res.peers_hold(n, math_in_use(), scale);
    return GPSO_OK;
  }
  // the ranges (offsets into the posterior arena: the same on every context of this shape and type) that a peer holding the
  // posterior as of the last hand-off lacks; returns their number, 0 when the peer is up to date, and -- when rows do not
  // apply (another posterior since, another predict math, the fp16 scale crossed a power of two) -- ONE range: the whole span
  int posterior_dirty_ranges(int64_t* offsets, int64_t* nbytes, int cap) override {
    if (!offsets || !nbytes || cap < 10) return ctx->fail(GPSO_E_ARG, "need room for 10 ranges");
    void* span_ptr = nullptr;
    int64_t span_off = 0, span_bytes = 0;
    int rc = posterior_span(&span_ptr, &span_off, &span_bytes);  // (settles the arithmetic choices, builds pending pieces)
    if (rc) return rc;
    float scale = 0.0f;
    if ((rc = current_split_scale(&scale))) return rc;
    if (!rows_apply(scale)) {
      offsets[0] = span_off;
      nbytes[0] = span_bytes;
      return 1;
    }
    if (res.sync_n == n) return 0;
    std::vector<std::pair<int64_t, int64_t>> rr;
    rows_ranges(res.sync_n, rr);
    for (size_t i = 0; i < rr.size(); ++i) {
      offsets[i] = rr[i].first;
      nbytes[i] = rr[i].second;
    }
    return (int)rr.size();
  }
  // Collective.  Returns GPSO_OK when only rows travelled, 1 when the whole range did (any rank that cannot take rows -- it
  // never received this posterior, holds another shape / math / scale -- makes every rank take the whole), < 0 on error;
  // gpso_last_count(ctx, 0) = the bytes that travelled.  Same header / verdict protocol as gpso_broadcast_posterior.
  int broadcast_posterior_rows(int root) override {
    int rc = need_comm();
    if (rc) return rc;
    RcclApi& R = RcclApi::get();
    if (root < 0 || root >= ctx->world) return ctx->fail(GPSO_E_ARG, "root %d outside the group of %d", root, ctx->world);
    hipStream_t s = st();
    const bool is_root = ctx->rank == root;
    if ((rc = ensure(bhdr, 256))) return rc;
    int64_t* hd = as<int64_t>(bhdr);
    int64_t* host = reinterpret_cast<int64_t*>(ctx->pinned_scratch(32));
    if (!host) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    // the root says what it can offer: rows since n_base in (math, scale), or nothing but the whole range (n_base = -1; also
    // when anything is wrong on the root: the full call then reports it on every rank)
    int64_t n_base = -1, n_now = 0, mth = 0, scale_bits = 0;
    if (is_root) {
      void* span_ptr = nullptr;
      int64_t span_off = 0, span_bytes = 0;
      float scale = 0.0f;
      if (res.has_post() && posterior_span(&span_ptr, &span_off, &span_bytes) == GPSO_OK && current_split_scale(&scale) == GPSO_OK &&
          rows_apply(scale) && !(can_selftest() && !st_pass())) {
        n_base = res.sync_n;
        n_now = n;
        mth = math_in_use();
        scale_bits = (int64_t)__builtin_bit_cast(unsigned, scale);
      }
      host[0] = n_base; host[1] = n_now; host[2] = mth; host[3] = scale_bits; host[4] = npad; host[5] = dp; host[6] = host[7] = 0;
      HIPCHECK(hipMemcpyAsync(hd, host, 64, hipMemcpyHostToDevice, s));
    }
    RCCLCHECK(R.Broadcast(hd, hd, 64, ncclChar, root, ctx->comm, s));
    HIPCHECK(hipMemcpyAsync(host, hd, 64, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    n_base = host[0]; n_now = host[1]; mth = host[2]; scale_bits = host[3];
    const int64_t r_npad = host[4], r_dp = host[5];
    // can THIS rank take rows?  (the peers' record is what the last hand-off left on them)
    int64_t mine = 1;
    if (n_base < 0) mine = 0;
    else if (!is_root)
      mine = (res.has_post() && arena.p != nullptr && res.sync_n == n_base && n == n_base && npad == r_npad && dp == r_dp && math_in_use() == (int)mth &&
              (int64_t)__builtin_bit_cast(unsigned, res.sync_scale) == scale_bits && n_now <= npad) ? 1 : 0;
    int64_t agreed = 0;
    if ((rc = agree_min(hd + 8, host + 8, mine, &agreed))) return rc;
    if (agreed != 1) {
      rc = broadcast_posterior(root);
      return rc == GPSO_OK ? 1 : rc;
    }
    int64_t moved = 0;
    if (n_now > n_base) {
      const int64_t n_keep = n;
      n = n_now;  // (rows_ranges describes the posterior of n_now rows)
      std::vector<std::pair<int64_t, int64_t>> rr;
      rows_ranges(n_base, rr);
      n = n_keep;
      char* base = static_cast<char*>(arena.p);
      RCCLCHECK(R.GroupStart());
      for (const auto& r : rr) {
        RCCLCHECK(R.Broadcast(base + r.first, base + r.first, (size_t)r.second, ncclChar, root, ctx->comm, s));
        moved += r.second;
      }
      RCCLCHECK(R.GroupEnd());
    }
    ctx->last_count[0] = ctx->last_count[1] = moved;
    if (!is_root) {
      n = n_now;
      if ((rc = adopt_posterior())) return rc;  // (reads the hyper block that just arrived; synchronises the stream)
    } else {
      HIPCHECK(ctx->wait(s));
    }
    return posterior_mark_synced();
  }

  // ------------------------------------------------------------------------------------------
  int get_matrix(int which, double* out) override {
    if (!out) return ctx->fail(GPSO_E_ARG, "out must not be NULL");
    const TF* src = nullptr;
    int lower = 1;
    switch (which) {
      case GPSO_MAT_CHOL:
        if (!res.chol_valid) return ctx->fail(GPSO_E_STATE, "no factor resident");
        if (res.variational()) return ctx->fail(GPSO_E_STATE, "a VGP predictive has no Cholesky factor of its own (GPSO_MAT_LINV holds C = R L^-1)");
        src = as<TF>(Lf);
        break;
      case GPSO_MAT_LINV:
        if (!res.chol_valid) return ctx->fail(GPSO_E_STATE, "no factor resident");
        src = as<TF>(linv);
        break;
      case GPSO_MAT_KINV:
        if (!res.have_kinv) return ctx->fail(GPSO_E_STATE, "Kinv only exists after gpso_fit_eval with grad");
        src = as<TF>(kinvb);
        lower = 2;
        break;
      default:
        return ctx->fail(GPSO_E_ARG, "unknown matrix id %d", which);
    }
    int rc = ensure(getter_tmp, (size_t)n * n * 8);
    if (rc) return rc;
    launch_convert_out<TF>(st(), src, npad, as<double>(getter_tmp), n, n, lower);
    HIPCHECK(hipMemcpyAsync(out, getter_tmp.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, st()));
    HIPCHECK(hipStreamSynchronize(st()));
    return GPSO_OK;
  }

  int get_vector(int which, double* out) override {
    if (!out) return ctx->fail(GPSO_E_ARG, "out must not be NULL");
    if (which == GPSO_VEC_NOISE_DIAG) {  // a property of the data, not of a posterior: the host mirror, or zeros
      if (!res.have_data) return ctx->fail(GPSO_E_STATE, "GPSO_VEC_NOISE_DIAG needs training data (gpso_set_data)");
      if (res.have_s) std::memcpy(out, s_host.data(), (size_t)n * 8);
      else std::memset(out, 0, (size_t)n * 8);
      return GPSO_OK;
    }
    if (!res.has_post() || !res.chol_valid) return ctx->fail(GPSO_E_STATE, "no fitted posterior resident");
    if (which == GPSO_VEC_WHITE && res.variational()) return ctx->fail(GPSO_E_STATE, "a VGP predictive has no whitened targets");
    const TF* src = (which == GPSO_VEC_ALPHA) ? as<TF>(alpha_f) : (which == GPSO_VEC_WHITE) ? as<TF>(white) : nullptr;
    if (!src) return ctx->fail(GPSO_E_ARG, "unknown vector id %d", which);
    int rc = ensure(getter_tmp, (size_t)n * 8);
    if (rc) return rc;
    launch_convert_out<TF>(st(), src, npad, as<double>(getter_tmp), 1, n, 0);
    HIPCHECK(hipMemcpyAsync(out, getter_tmp.p, (size_t)n * 8, hipMemcpyDeviceToHost, st()));
    HIPCHECK(hipStreamSynchronize(st()));
    return GPSO_OK;
  }

  // hyper | packed L^-1 | scaled inputs (double: plain, MFMA fragments, norms) | alpha [| bf16 pieces].
  // The generation inputs always travel in double; a receiver derives the float copies itself when the sender's choice is
  // float generation.  settle the posterior's arithmetic choices (generation, GPSO_MATH_AUTO's rung) and write them into
  // slot 7 of the hyper block, which travels (resident.hpp: handoff_word)
  // (span_only: the flag describes the contiguous range of posterior_span -- the packed L^-1 is part of it only when the
  // posterior runs the f32 / f64 MFMA kernel; otherwise every buffer travels)
  int settle_and_flag(bool span_only) {
    if (!res.has_post()) return GPSO_OK;
    int rc = decide_generation();
    if (rc) return rc;
    if (can_selftest() && (rc = selftest_with_fallback())) return rc;  // settles GPSO_MATH_AUTO
    const bool with_linv_p = !span_only || math_in_use() == GPSO_MATH_NATIVE;
    if (with_linv_p && (rc = ensure_linv_p())) return rc;
    double* flag = ctx->pinned_scratch(256) + 120;  // (a slot neither the read-backs nor set_theta use)
    *flag = res.handoff_word(gen_double(), bf16_usable(), with_linv_p);
    HIPCHECK(hipMemcpyAsync(as<double>(hyper) + 7, flag, 8, hipMemcpyHostToDevice, st()));
    HIPCHECK(hipStreamSynchronize(st()));  // callers copy these buffers on streams of their own
    return GPSO_OK;
  }
  int posterior_buffers(void** ptrs, int64_t* nbytes, int cap) override {
    if (npad == 0) return ctx->fail(GPSO_E_STATE, "no problem shape yet");
    if (cap < 7) return ctx->fail(GPSO_E_ARG, "need room for 7 buffers");
    int rc = settle_and_flag(false);
    if (rc) return rc;
    const size_t s = sizeof(TP);
    int k = 0;
    ptrs[k] = hyper.p;   nbytes[k++] = (int64_t)(kHyperHeader + kMaxD) * 8;
    ptrs[k] = linv_p.p;  nbytes[k++] = (int64_t)(packed_linv_elems(npad) * s);
    ptrs[k] = xs64.p;    nbytes[k++] = (int64_t)(npad * dp * 8);
    ptrs[k] = xs_p64.p;  nbytes[k++] = (int64_t)(npad * dp * 8);
    ptrs[k] = xnorm64.p; nbytes[k++] = (int64_t)(npad * 8);
    ptrs[k] = alpha.p;   nbytes[k++] = (int64_t)(npad * s);
    // the 16-bit pieces of L^-1 travel when the mode is on -- a sender whose pieces were never built (a posterior it
    // adopted itself, math switched afterwards) still sends the buffer, so that both sides of a hand-off list the
    // same buffers, and says so in the hyper block (bit 4 of slot 7 clear): the receivers then run the f32 kernel
    if (bf16_usable()) {
      ptrs[k] = linv_b.p; nbytes[k++] = (int64_t)split_bytes();
    }
    return k;
  }
  // The ONE contiguous range of the posterior arena the resident posterior uses (what gpso_broadcast_posterior sends):
  // *offset = its distance from the arena's start -- the same on every context of the same shape and type.
  int posterior_span(void** ptr, int64_t* offset, int64_t* nbytes) override {
    if (npad == 0 || arena.p == nullptr) return ctx->fail(GPSO_E_STATE, "no problem shape yet");
    if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "no posterior resident");
    int rc = settle_and_flag(true);
    if (rc) return rc;
    if (math_in_use() == GPSO_MATH_NATIVE && res.linv_p != Copy::Valid)
      return ctx->fail(GPSO_E_STATE, "this context received its posterior without the packed L^-1 and cannot pass it on for the f32 kernel");
    size_t off, bytes;
    posterior_range(&off, &bytes);
    if (ptr) *ptr = static_cast<char*>(arena.p) + off;
    if (offset) *offset = (int64_t)off;
    if (nbytes) *nbytes = (int64_t)bytes;
    return GPSO_OK;
  }
  // where a span (offset, nbytes) announced by a peer lands in THIS context's arena (after gpso_alloc_posterior)
  int posterior_span_at(int64_t offset, int64_t nbytes, void** ptr) override {
    if (arena.p == nullptr) return ctx->fail(GPSO_E_STATE, "gpso_alloc_posterior first");
    if (offset < 0 || nbytes <= 0 || offset % 256 != 0 || (size_t)offset + (size_t)nbytes > arena.bytes)
      return ctx->fail(GPSO_E_ARG, "posterior span [%lld, +%lld) does not fit this context's arena of %zu bytes (different "
                       "dtype / shape on the sender?)", (long long)offset, (long long)nbytes, arena.bytes);
    *ptr = static_cast<char*>(arena.p) + offset;
    return GPSO_OK;
  }
  // 64-bit fingerprint of the predict-ready posterior (the buffers gpso_posterior_buffers lists, the parts in use):
  // two contexts that ran the same deterministic fit hold the same value -- what a group that REPLICATES the fit on
  // every rank compares instead of broadcasting ("measure both")
  DevBuf hash_out;
  int posterior_hash(uint64_t* out) override {
    if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "no posterior resident");
    int rc = settle_and_flag(true);
    if (rc) return rc;
    if ((rc = ensure(hash_out, 8))) return rc;
    hipStream_t s = st();
    HIPCHECK(hipMemsetAsync(hash_out.p, 0, 8, s));
    const size_t sp = sizeof(TP);
    uint64_t salt = 1;
    auto add = [&](const void* p_, size_t bytes) { launch_hash_words(s, p_, bytes / 8, salt++, static_cast<unsigned long long*>(hash_out.p)); };
    add(hyper.p, (size_t)(kHyperHeader + kMaxD) * 8);
    add(xs64.p, (size_t)npad * dp * 8);
    add(xs_p64.p, (size_t)npad * dp * 8);
    add(xnorm64.p, (size_t)npad * 8);
    add(alpha.p, (size_t)npad * sp / 8 * 8);
    if (math_in_use() != GPSO_MATH_NATIVE) {
      if (f16_split()) add(f16_scale(), 8);
      add(split_planes(), (size_t)nsplit() * npad * npad * 2);
    } else {
      add(linv_p.p, packed_linv_elems(npad) * sp);
    }
    uint64_t* host = reinterpret_cast<uint64_t*>(ctx->pinned_scratch(8));
    if (!host) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    HIPCHECK(hipMemcpyAsync(host, hash_out.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx->wait(s));
    if ((rc = launch_status())) return rc;
    *out = host[0];
    return GPSO_OK;
  }

  int alloc_posterior(int64_t n_, int d_) override {
    int rc = refuse_if_async("gpso_alloc_posterior");
    if (rc) return rc;
    rc = shape(n_, d_);
    if (rc) return rc;
    res.shape_allocated();
    return GPSO_OK;
  }

  int adopt_posterior() override {
    if (npad == 0) return ctx->fail(GPSO_E_STATE, "gpso_alloc_posterior first");
    double* h = ctx->pinned_scratch(kHyperHeader + kMaxD);
    if (!h) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
    HIPCHECK(hipMemcpyAsync(h, hyper.p, (size_t)(kHyperHeader + kMaxD) * 8, hipMemcpyDeviceToHost, st()));
    HIPCHECK(hipStreamSynchronize(st()));
    // (a posterior EXTENDED by gpso_append on the sender arrives with more rows than the buffers were announced for: the
    // layout is a function of the padded size, which an in-place append cannot change)
    const int64_t hn = (int64_t)h[0];
    if ((int)h[1] != d || hn < n || hn > npad)
      return ctx->fail(GPSO_E_ARG, "received posterior is for n=%lld d=%d, buffers were sized for n=%lld d=%d",
                       (long long)h[0], (int)h[1], (long long)n, d);
    n = hn;
    kp.kernel = (int)h[2];
    n_ls = (int)h[3];
    kp.variance = h[4];
    kp.noise = h[5];
    kp.mean_c = h[6];
    ls_host.assign(h + kHyperHeader, h + kHyperHeader + n_ls);
    res.adopted((int)h[7], kFloatPredict, math_auto, gen_mode, npad);
    return GPSO_OK;
  }
};

}  // namespace

// ---- the optimiser's vector u -> theta -> the engine, and the gradient back (theta.hpp) --------------------------------------
// theta (theta.hpp) from the optimiser's vector u, or why not.  lik_floor: what stands in front of the softplus of slot n_ls + 1
static int theta_of_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed, double lik_floor,
                      Theta* th) {
  switch (theta_from_u(kernel, u, n_ls, train_mean != 0, mean_c_fixed, lik_floor, th)) {
    case ThetaDecode::NullU: return ctx->fail(GPSO_E_ARG, "u must not be NULL");
    case ThetaDecode::NlsRange: return ctx->fail(GPSO_E_ARG, "n_ls=%d outside [1, %d]", n_ls, kGradMaxLs);
    case ThetaDecode::Ok: break;
  }
  return GPSO_OK;
}
constexpr double kGaussianFloor = 1.0e-6;  // gpflow.likelihoods.Gaussian DEFAULT_VARIANCE_LOWER_BOUND
// the VGP's and the SVGP's likelihood parameter: the Gaussian variance (1e-6 + softplus) or the Student-t scale (softplus,
// GPflow's positive())
static double vlik_floor(const gpso_ctx* ctx) { return ctx->eng->vlik_kind == GPSO_LIK_STUDENT_T ? 0.0 : kGaussianFloor; }
// what the evaluations in u share behind their guards: decode, optional copy-out, engine call, chain rule.  eval(th, g): the
// engine call, g the constrained gradient (NULL: none); want_g: a gradient is computed although grad_u is NULL (the moving-Z
// calls' grad_z)
template <typename Eval>
static int eval_in_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed, double lik_floor,
                     double* grad_u, bool want_g, double* theta_out, Eval eval) {
  Theta th;
  double g[kGradMaxLs + 3];
  int rc = theta_of_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, lik_floor, &th);
  if (rc) return rc;
  if (theta_out) theta_copy_out(th, theta_out);
  rc = eval(th, (grad_u || want_g) ? g : nullptr);
  if (rc != GPSO_OK || !grad_u) return rc;
  grad_to_u(u, n_ls, train_mean != 0, g, grad_u);
  return GPSO_OK;
}

// ==============================================================================================
extern "C" {

int gpso_create(gpso_ctx** out, int device, int dtype) {
  if (!out) {
    g_create_error = "out must not be NULL";
    return GPSO_E_ARG;
  }
  *out = nullptr;
  if (dtype != GPSO_F64 && dtype != GPSO_F32 && dtype != GPSO_MIXED) {
    g_create_error = "dtype must be GPSO_F64, GPSO_F32 or GPSO_MIXED";
    return GPSO_E_ARG;
  }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) {
    g_create_error = std::string("no HIP device available: ") + hipGetErrorString(e);
    return GPSO_E_HIP;
  }
  if (device < 0 || device >= count) {
    g_create_error = "device index out of range";
    return GPSO_E_ARG;
  }
  DeviceGuard guard(device);  // the caller's current device is restored on return
  if (!guard.ok) {
    g_create_error = "hipSetDevice failed";
    return GPSO_E_HIP;
  }
  gpso_ctx* ctx = new gpso_ctx();
  ctx->device = device;
  ctx->dtype = dtype;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->cu_count = cus;
  ContextPool::Set pooled;
  if (ContextPool::get().take(device, pooled)) {  // a destroyed context's stream, events and pinned buffers
    ctx->own_stream = pooled.stream;
    ctx->ev_wait = pooled.ev_wait;
    for (int i = 0; i < 8; ++i) ctx->ev[i] = pooled.ev[i];
    ctx->pinned = pooled.pinned;
    ctx->pinned_doubles = pooled.pinned_doubles;
    ctx->stage = pooled.stage;
    ctx->stage_doubles = pooled.stage_doubles;
    if (ctx->pinned) std::memset(ctx->pinned, 0, ctx->pinned_doubles * 8);
    ctx->stream = ctx->own_stream;
  } else {
  if ((e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess) {
    g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e);
    delete ctx;
    return GPSO_E_HIP;
  }
  ctx->stream = ctx->own_stream;
  if ((e = hipEventCreateWithFlags(&ctx->ev_wait, hipEventDisableTiming)) != hipSuccess) {
    g_create_error = std::string("hipEventCreate: ") + hipGetErrorString(e);
    gpso_destroy(ctx);
    return GPSO_E_HIP;
  }
  for (auto& ev : ctx->ev)
    if ((e = hipEventCreate(&ev)) != hipSuccess) {
      g_create_error = std::string("hipEventCreate: ") + hipGetErrorString(e);
      gpso_destroy(ctx);
      return GPSO_E_HIP;
    }
  }
  if (dtype == GPSO_F64)
    ctx->eng = new EngineT<double, double>(ctx);
  else if (dtype == GPSO_F32)
    ctx->eng = new EngineT<float, float>(ctx);
  else
    ctx->eng = new EngineT<double, float>(ctx);
  *out = ctx;
  return GPSO_OK;
}

void gpso_destroy(gpso_ctx* ctx) {
  if (!ctx) return;
  DeviceGuard guard(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->comm && !ctx->comm_aborted) (void)RcclApi::get().CommDestroy(ctx->comm);
  delete ctx->eng;
  for (auto& ev : ctx->tile_ev) (void)hipEventDestroy(ev);
  if (ctx->side_stream) (void)hipStreamSynchronize(ctx->side_stream);
  if (ctx->inv_stream) (void)hipStreamSynchronize(ctx->inv_stream);
  for (hipEvent_t e : {ctx->ev_col, ctx->ev_chain, ctx->ev_panel, ctx->ev_inv})
    if (e) (void)hipEventDestroy(e);
  if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
  if (ctx->inv_stream) (void)hipStreamDestroy(ctx->inv_stream);
  if (ctx->slot_host) (void)hipHostFree(ctx->slot_host);
  for (auto& t : ctx->tickets)
    if (t.ev) (void)hipEventDestroy(t.ev);
  // stream, events and pinned buffers go to the pool when they are complete and the pool has room (ContextPool)
  bool complete = ctx->own_stream != nullptr && ctx->ev_wait != nullptr;
  for (auto& ev : ctx->ev) complete = complete && ev != nullptr;
  ContextPool::Set give;
  if (complete) {
    (void)hipStreamSynchronize(ctx->own_stream);
    give.stream = ctx->own_stream;
    give.ev_wait = ctx->ev_wait;
    for (int i = 0; i < 8; ++i) give.ev[i] = ctx->ev[i];
    give.pinned = ctx->pinned;
    give.pinned_doubles = ctx->pinned_doubles;
    give.stage = ctx->stage;
    give.stage_doubles = ctx->stage_doubles;
  }
  if (!complete || !ContextPool::get().give(ctx->device, give)) {
    for (auto& ev : ctx->ev)
      if (ev) (void)hipEventDestroy(ev);
    if (ctx->ev_wait) (void)hipEventDestroy(ctx->ev_wait);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->stage) (void)hipHostFree(ctx->stage);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  }
  delete ctx;
}

const char* gpso_last_error(const gpso_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

// every entry point runs on the context's device and puts the caller's current device back on return
#define ENTER()                                                              \
  if (!ctx) return GPSO_E_ARG;                                               \
  DeviceGuard guard_(ctx->device);                                           \
  if (!guard_.ok) return ctx->fail(GPSO_E_HIP, "hipSetDevice(%d) failed", ctx->device); \
  gpso::g_launch_error.clear();

int gpso_set_stream(gpso_ctx* ctx, void* hip_stream) {
  ENTER();
  (void)hipStreamSynchronize(ctx->stream);
  ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
  return GPSO_OK;
}

int gpso_synchronize(gpso_ctx* ctx) {
  ENTER();
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  return GPSO_OK;
}

int gpso_set_option(gpso_ctx* ctx, int option, int value) {
  ENTER();
  return ctx->eng->set_option(option, value);
}

int gpso_set_option_f64(gpso_ctx* ctx, int option, double value) {
  ENTER();
  return ctx->eng->set_option_f64(option, value);
}

int gpso_wait_stream(gpso_ctx* ctx, void* producer_stream) {
  ENTER();
  hipStream_t prod = static_cast<hipStream_t>(producer_stream);
  if (prod == ctx->stream) return GPSO_OK;
  if (hipStreamQuery(prod) == hipSuccess) return GPSO_OK;  // nothing pending there: nothing to wait for (one call, no event)
  HIPCHECK(hipEventRecord(ctx->ev_wait, prod));
  HIPCHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_wait, 0));
  return GPSO_OK;
}

int gpso_precision_info(gpso_ctx* ctx, double* out) {
  ENTER();
  if (!out) return ctx->fail(GPSO_E_ARG, "out must not be NULL");
  return ctx->eng->precision_info(out);
}

int gpso_set_data(gpso_ctx* ctx, const double* X, const double* y, int64_t n, int d) {
  ENTER();
  return ctx->eng->set_data(X, y, n, d);
}

int gpso_fit_eval(gpso_ctx* ctx, int kernel, const double* lengthscales, int n_ls, double variance,
                  double noise, double mean_c, double* nlml, double* grad) {
  ENTER();
  Theta th;
  if (lengthscales) theta_from_parts(kernel, lengthscales, n_ls, variance, noise, mean_c, &th);
  return ctx->eng->fit_eval(lengthscales ? &th : nullptr, nlml, grad);
}

int gpso_fit_eval_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                    double* nlml, double* grad_u, double* theta_out) {
  ENTER();
  return eval_in_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, kGaussianFloor, grad_u, false, theta_out,
                   [&](const Theta& th, double* g) { return ctx->eng->fit_eval(&th, nlml, g); });
}

int gpso_loo(gpso_ctx* ctx, double* mean, double* var, double* lpd, double* loss) {
  ENTER();
  return ctx->eng->loo(mean, var, lpd, loss);
}

int gpso_fit_eval_loo(gpso_ctx* ctx, int kernel, const double* lengthscales, int n_ls, double variance, double noise,
                      double mean_c, double* loss, double* grad, double* nlml) {
  ENTER();
  Theta th;
  if (lengthscales) theta_from_parts(kernel, lengthscales, n_ls, variance, noise, mean_c, &th);
  return ctx->eng->fit_eval_loo(lengthscales ? &th : nullptr, loss, grad, nlml);
}

int gpso_fit_eval_loo_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                        double* loss, double* grad_u, double* theta_out, double* nlml) {
  ENTER();
  return eval_in_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, kGaussianFloor, grad_u, false, theta_out,
                   [&](const Theta& th, double* g) { return ctx->eng->fit_eval_loo(&th, loss, g, nlml); });
}

int gpso_fit_batch_max(gpso_ctx* ctx) {
  ENTER();
  return ctx->eng->fit_batch_max();
}

int gpso_fit_eval_u_batch(gpso_ctx* ctx, int kernel, const double* U, int b, int n_ls, int train_mean,
                          double mean_c_fixed, double* loss, double* grad_u, int* status, int64_t* pivot) {
  ENTER();
  if (!U || !loss || !status) return ctx->fail(GPSO_E_ARG, "U, loss and status must not be NULL");
  if (n_ls < 1 || n_ls > kGradMaxLs) return ctx->fail(GPSO_E_ARG, "n_ls=%d outside [1, %d]", n_ls, kGradMaxLs);
  int rc = ctx->eng->fit_eval_batch_check(kernel, b, n_ls);
  if (rc) return rc;
  const int nu = n_ls + 2 + (train_mean ? 1 : 0), H = n_ls + 3;
  // the transforms of gpso_fit_eval_u, entry by entry; an entry the single call would refuse for its values (a
  // lengthscale or a variance that is not positive: NaN included) is not launched and reports GPSO_E_ARG as there
  std::vector<double> th((size_t)b * H), g((size_t)b * H), f((size_t)b);
  std::vector<int> slot((size_t)b), info((size_t)b);
  int nv = 0, first_bad = -1;
  for (int e = 0; e < b; ++e) {
    Theta t;
    (void)theta_from_u(kernel, U + (size_t)e * nu, n_ls, train_mean != 0, mean_c_fixed, kGaussianFloor, &t);
    theta_copy_out(t, th.data() + (size_t)nv * H);
    // (the kernel id and n_ls passed the check above: with D := n_ls only the values are left to refuse)
    slot[e] = theta_refusal(t, n_ls, false) ? -1 : nv++;
  }
  if (nv > 0 && (rc = ctx->eng->fit_eval_batch(kernel, th.data(), nv, n_ls, f.data(), grad_u ? g.data() : nullptr, info.data())))
    return rc;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int e = 0; e < b; ++e) {
    const int v = slot[e];
    const bool fine = v >= 0 && info[v] == INT_MAX;
    status[e] = fine ? GPSO_OK : (v < 0 ? GPSO_E_ARG : GPSO_E_NOTPD);
    if (pivot) pivot[e] = (v >= 0 && !fine) ? info[v] : -1;
    loss[e] = fine ? f[v] : nan;
    if (!fine && first_bad < 0) first_bad = e;
    if (!grad_u) continue;
    double* gu = grad_u + (size_t)e * nu;
    if (fine) grad_to_u(U + (size_t)e * nu, n_ls, train_mean != 0, g.data() + (size_t)v * H, gu);
    else
      for (int k = 0; k < nu; ++k) gu[k] = nan;
  }
  if (first_bad >= 0) {
    if (slot[first_bad] < 0)
      (void)ctx->fail(GPSO_E_ARG, "batch entry %d: a lengthscale or the kernel variance is not positive", first_bad);
    else
      (void)ctx->fail(GPSO_E_NOTPD, "batch entry %d: K + noise*I is not positive definite: Cholesky failed at pivot %d",
                      first_bad, info[slot[first_bad]]);
  }
  return GPSO_OK;
}

int gpso_set_noise_diag(gpso_ctx* ctx, const double* s, int64_t n) {
  ENTER();
  return ctx->eng->set_noise_diag(s, n);
}

int gpso_append(gpso_ctx* ctx, const double* Xnew, const double* ynew, int64_t k, double* nlml) {
  ENTER();
  return ctx->eng->append(Xnew, ynew, nullptr, k, nlml);
}

int gpso_append_noise(gpso_ctx* ctx, const double* Xnew, const double* ynew, const double* snew, int64_t k, double* nlml) {
  ENTER();
  return ctx->eng->append(Xnew, ynew, snew, k, nlml);
}

// the variational and sparse families model ONE noise variance: a context that carries per-point noise is refused by
// every entry point of theirs that computes, instead of having the vector silently ignored
static int refuse_noise_diag(gpso_ctx* ctx) {
  if (!ctx->eng->has_noise_diag()) return GPSO_OK;
  return ctx->fail(GPSO_E_ARG, "a per-point noise vector is set on this context (gpso_set_noise_diag): the VGP, SGPR, SVGP and "
                               "inducing-point entry points have one shared noise variance and would ignore it -- clear it "
                               "with gpso_set_noise_diag(ctx, NULL, n) first");
}

int gpso_set_posterior(gpso_ctx* ctx, const double* X, const double* L, const double* alpha,
                       int64_t n, int d, int kernel, const double* lengthscales, int n_ls,
                       double variance, double noise, double mean_c) {
  ENTER();
  if (!lengthscales) return ctx->fail(GPSO_E_ARG, "NULL argument");  // (with X, L and alpha: the engine's first check)
  Theta th;
  theta_from_parts(kernel, lengthscales, n_ls, variance, noise, mean_c, &th);
  return ctx->eng->set_posterior(X, L, alpha, n, d, th);
}

// ---- variational GP --------------------------------------------------------------------------------------------
int gpso_vgp_set_likelihood(gpso_ctx* ctx, int kind, double df, int n_gh, const double* gh_x, const double* gh_w) {
  ENTER();
  return ctx->eng->vgp_set_likelihood(kind, df, n_gh, gh_x, gh_w);
}

int gpso_vgp_set_q(gpso_ctx* ctx, const double* mu, const double* S, int64_t n) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  if ((mu == nullptr) != (S == nullptr)) return ctx->fail(GPSO_E_ARG, "mu and S: both or neither");
  return ctx->eng->vgp_set_q(mu, S, n);
}

int gpso_vgp_extend_q(gpso_ctx* ctx) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  return ctx->eng->vgp_extend_q();
}

int gpso_vgp_get_q(gpso_ctx* ctx, double* mu, double* S) {
  ENTER();
  return ctx->eng->vgp_get_q(mu, S);
}

int gpso_vgp_natgrad(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                     double gamma) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  Theta th;
  int rc = theta_of_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), &th);
  if (rc) return rc;
  return ctx->eng->vgp_natgrad(th, gamma);
}

int gpso_vgp_elbo_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                    double* loss, double* grad_u, double* theta_out) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  if (!loss) return ctx->fail(GPSO_E_ARG, "loss must not be NULL");
  return eval_in_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), grad_u, false, theta_out,
                   [&](const Theta& th, double* g) { return ctx->eng->vgp_elbo(th, loss, g); });
}

int gpso_vgp_posterior(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  Theta th;
  int rc = theta_of_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), &th);
  if (rc) return rc;
  return ctx->eng->vgp_posterior(th);
}

// ---- sparse GP regression on inducing points ---------------------------------------------------------------------
int gpso_sgpr_set_inducing(gpso_ctx* ctx, const double* Z, int64_t m) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  return ctx->eng->sgpr_set_inducing(Z, m);
}

int gpso_sgpr_select_inducing(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int64_t m, int64_t* idx_out) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  Theta th;
  int rc = theta_of_u(ctx, kernel, u, n_ls, 0, 0.0, kGaussianFloor, &th);
  if (rc) return rc;
  return ctx->eng->sgpr_select_inducing(th, m, idx_out);
}

int gpso_sgpr_get_inducing(gpso_ctx* ctx, double* Z, int64_t* m, int64_t* n_data) {
  ENTER();
  return ctx->eng->sgpr_get_inducing(Z, m, n_data);
}

int gpso_sgpr_get_factor(gpso_ctx* ctx, int which, double* out) {
  ENTER();
  return ctx->eng->sgpr_get_factor(which, out);
}

int gpso_sgpr_bound_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                      double* loss, double* grad_u, double* theta_out) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  if (!loss) return ctx->fail(GPSO_E_ARG, "loss must not be NULL");
  return eval_in_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, kGaussianFloor, grad_u, false, theta_out,
                   [&](const Theta& th, double* g) { return ctx->eng->sgpr_bound(th, loss, g); });
}

int gpso_sgpr_posterior(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                        double* delta_out) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  Theta th;
  int rc = theta_of_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, kGaussianFloor, &th);
  if (rc) return rc;
  return ctx->eng->sgpr_posterior(th, delta_out);
}

// ---- sparse variational GP on inducing points (theta from u as the VGP's: vlik_floor) ------------------------------------
int gpso_svgp_init_q(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                     double noise_variance) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  Theta th{};
  if (!(noise_variance > 0.0)) return ctx->eng->svgp_init_q(th, 0.0);  // the prior
  int rc = theta_of_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), &th);
  if (rc) return rc;
  return ctx->eng->svgp_init_q(th, noise_variance);
}

int gpso_svgp_set_q(gpso_ctx* ctx, const double* mu, const double* S, int64_t m) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  if ((mu == nullptr) != (S == nullptr)) return ctx->fail(GPSO_E_ARG, "mu and S: both or neither");
  return ctx->eng->svgp_set_q(mu, S, m);
}

int gpso_svgp_get_q(gpso_ctx* ctx, double* mu, double* S) {
  ENTER();
  return ctx->eng->svgp_get_q(mu, S);
}

int gpso_svgp_natgrad(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                      double gamma) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  Theta th;
  int rc = theta_of_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), &th);
  if (rc) return rc;
  return ctx->eng->svgp_natgrad(th, gamma);
}

int gpso_svgp_elbo_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                     double* loss, double* grad_u, double* theta_out) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  if (!loss) return ctx->fail(GPSO_E_ARG, "loss must not be NULL");
  return eval_in_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), grad_u, false, theta_out,
                   [&](const Theta& th, double* g) { return ctx->eng->svgp_elbo(th, loss, g); });
}

int gpso_svgp_posterior(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                        double* delta_out) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  Theta th;
  int rc = theta_of_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), &th);
  if (rc) return rc;
  return ctx->eng->svgp_posterior(th, delta_out);
}

// ---- the sparse models at a moving Z ------------------------------------------------------------------------------------
int gpso_sgpr_move_inducing(gpso_ctx* ctx, const double* Z) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  return ctx->eng->sgpr_move_inducing(Z);
}

int gpso_sgpr_bound_uz(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                       const double* Z, double* loss, double* grad_u, double* grad_z, double* theta_out) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  if (!loss) return ctx->fail(GPSO_E_ARG, "loss must not be NULL");
  return eval_in_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, kGaussianFloor, grad_u, grad_z != nullptr, theta_out,
                   [&](const Theta& th, double* g) { return ctx->eng->sgpr_bound_z(th, Z, loss, g, grad_z); });
}

int gpso_svgp_elbo_uz(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                      const double* Z, double* loss, double* grad_u, double* grad_z, double* theta_out) {
  ENTER();
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  if (!loss) return ctx->fail(GPSO_E_ARG, "loss must not be NULL");
  return eval_in_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), grad_u, grad_z != nullptr, theta_out,
                   [&](const Theta& th, double* g) { return ctx->eng->svgp_elbo_z(th, Z, loss, g, grad_z); });
}

int gpso_predict(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double* mean,
                 double* var, int out_mem) {
  ENTER();
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "bad out_mem %d", out_mem);
  return ctx->eng->predict(xs, xs_dtype, xs_mem, m, mean, var, out_mem);
}

int gpso_predict_grad(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double* mean, double* var,
                      double* dmean, double* dvar, int out_mem) {
  ENTER();
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "bad out_mem %d", out_mem);
  return ctx->eng->predict_grad(xs, xs_dtype, xs_mem, m, mean, var, dmean, dvar, out_mem);
}

int gpso_predict_joint(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, double* mean,
                       double* cov, int out_mem) {
  ENTER();
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "bad out_mem %d", out_mem);
  return ctx->eng->predict_joint(xs, xs_dtype, xs_mem, m, diag_add, mean, cov, out_mem);
}

int gpso_sample_joint(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, const double* z,
                      int64_t s, double* samples, int64_t* best_idx, double* best_val) {
  ENTER();
  return ctx->eng->sample_joint(xs, xs_dtype, xs_mem, m, diag_add, z, s, samples, best_idx, best_val);
}

int gpso_paths_draw(gpso_ctx* ctx, const double* omega, const double* phase, int64_t f, const double* w, const double* eps,
                    int64_t s) {
  ENTER();
  return ctx->eng->paths_draw(omega, phase, f, w, eps, s);
}

int gpso_paths_draw_q(gpso_ctx* ctx, const double* omega, const double* phase, int64_t f, const double* w, const double* eps,
                      int64_t s) {
  ENTER();
  return ctx->eng->paths_draw_q(omega, phase, f, w, eps, s);
}

int gpso_paths_eval(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
                    double* values, int out_mem, int64_t* best_idx, double* best_val) {
  ENTER();
  return ctx->eng->paths_eval(xs, xs_dtype, xs_mem, m, seg_off, nseg, values, out_mem, best_idx, best_val);
}

int gpso_cross_cov(gpso_ctx* ctx, const void* xa, int xs_dtype, int xs_mem, int64_t m, const double* xb, int b, double* cov,
                   int out_mem) {
  ENTER();
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "bad out_mem %d", out_mem);
  return ctx->eng->cross_cov(xa, xs_dtype, xs_mem, m, xb, b, cov, out_mem);
}

int gpso_paths_info(gpso_ctx* ctx, int64_t* s, int64_t* f) {
  ENTER();
  if (!s || !f) return ctx->fail(GPSO_E_ARG, "s and f must not be NULL");
  ctx->eng->paths_info(s, f);
  return GPSO_OK;
}

int gpso_best_ucb(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m,
                  const int64_t* seg_off, int nseg, double varsigma, int64_t* idx, double* mean,
                  double* var, double* ucb) {
  ENTER();
  return ctx->eng->best_ucb(xs, xs_dtype, xs_mem, m, seg_off, nseg, varsigma, idx, mean, var, ucb);
}

int gpso_best_ucb_begin(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
                        double varsigma) {
  ENTER();
  return ctx->eng->best_ucb_begin(xs, xs_dtype, xs_mem, m, seg_off, nseg, varsigma, nullptr, 0);
}

int gpso_best_ucb_grow_begin(gpso_ctx* ctx, const double* bounds, int nseg, int depth, double varsigma) {
  ENTER();
  if (!bounds) return ctx->fail(GPSO_E_ARG, "bounds must not be NULL");
  return ctx->eng->best_ucb_begin(nullptr, GPSO_F64, GPSO_MEM_DEVICE, 0, nullptr, nseg, varsigma, bounds, depth);
}

int gpso_best_ucb_end(gpso_ctx* ctx, int ticket, int64_t* idx, double* mean, double* var, double* ucb) {
  ENTER();
  return ctx->eng->best_ucb_end(ticket, idx, mean, var, ucb);
}

int64_t gpso_grow_rows(int depth) {
  int64_t rows = 0, w = 1;
  for (int j = 0; j < depth; ++j) {
    rows += w;
    w *= 3;
  }
  return rows;
}

int gpso_grow(gpso_ctx* ctx, const double* bounds, int nseg, int d, int depth, double* out_coords) {
  ENTER();
  return ctx->eng->grow(bounds, nseg, d, depth, out_coords);
}

int gpso_best_ucb_grow(gpso_ctx* ctx, const double* bounds, int nseg, int depth, double varsigma,
                       int64_t* idx, double* mean, double* var, double* ucb) {
  ENTER();
  return ctx->eng->best_ucb_grow(bounds, nseg, depth, varsigma, idx, mean, var, ucb);
}

// ---- acquisition functions (acq.hpp) ----------------------------------------------------------
// NULL when the record is usable, else what is wrong with it
static const char* acq_refusal(const gpso_acq* a, bool mes = false /* the call can hand the kind its maxima */) {
  if (!a) return "acq must not be NULL";
  if (a->kind == GPSO_ACQ_MES) return mes ? nullptr : "GPSO_ACQ_MES needs its maxima: this call cannot see them";
  if (a->kind < GPSO_ACQ_UCB_VAR || a->kind > GPSO_ACQ_PI) return "unknown acquisition kind";
  const bool ucb = a->kind == GPSO_ACQ_UCB_VAR || a->kind == GPSO_ACQ_UCB_STD;
  if (ucb && !std::isfinite(a->varsigma)) return "varsigma must be finite";
  if (!ucb && !std::isfinite(a->incumbent)) return "incumbent must be finite";
  if (!ucb && !std::isfinite(a->xi)) return "xi must be finite";
  return nullptr;
}
static gpso::AcqSpec acq_spec(const gpso_acq* a) { return gpso::AcqSpec(a->kind, a->latent != 0, a->varsigma, a->incumbent, a->xi); }
// ... of a call on a context: GPSO_ACQ_MES reads the context's resident maxima
static gpso::AcqSpec acq_spec(const gpso_ctx* ctx, const gpso_acq* a) {
  if (a->kind != GPSO_ACQ_MES) return acq_spec(a);
  return gpso::AcqSpec(a->kind, a->latent != 0, 0.0, 0.0, 0.0, ctx->eng->maxima_dev, ctx->eng->maxima_k);
}
static gpso::AcqSpec mes_spec_host(const double* ystar, int k, int latent) {
  return gpso::AcqSpec(GPSO_ACQ_MES, latent != 0, 0.0, 0.0, 0.0, ystar, k);
}
static bool maxima_usable(const double* ystar, int k) {
  if (!ystar || k < 1 || k > GPSO_ACQ_MAX_MAXIMA) return false;
  for (int i = 0; i < k; ++i)
    if (!std::isfinite(ystar[i])) return false;
  return true;
}
#define ACQ_ENTER()                                                                    \
  ENTER();                                                                             \
  if (const char* why = acq_refusal(acq, true)) return ctx->fail(GPSO_E_ARG, "%s", why); \
  if (acq->kind == GPSO_ACQ_MES && ctx->eng->maxima_k == 0)                            \
  return ctx->fail(GPSO_E_STATE, "GPSO_ACQ_MES without maxima on this context: gpso_acq_set_maxima first")

int gpso_best_acq(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
                  const gpso_acq* acq, int64_t* idx, double* mean, double* var, double* value) {
  ACQ_ENTER();
  return ctx->eng->best_ucb(xs, xs_dtype, xs_mem, m, seg_off, nseg, acq_spec(ctx, acq), idx, mean, var, value);
}

int gpso_best_acq_begin(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
                        const gpso_acq* acq) {
  ACQ_ENTER();
  return ctx->eng->best_ucb_begin(xs, xs_dtype, xs_mem, m, seg_off, nseg, acq_spec(ctx, acq), nullptr, 0);
}

int gpso_best_acq_grow(gpso_ctx* ctx, const double* bounds, int nseg, int depth, const gpso_acq* acq, int64_t* idx,
                       double* mean, double* var, double* value) {
  ACQ_ENTER();
  return ctx->eng->best_ucb_grow(bounds, nseg, depth, acq_spec(ctx, acq), idx, mean, var, value);
}

int gpso_best_acq_grow_begin(gpso_ctx* ctx, const double* bounds, int nseg, int depth, const gpso_acq* acq) {
  ACQ_ENTER();
  if (!bounds) return ctx->fail(GPSO_E_ARG, "bounds must not be NULL");
  return ctx->eng->best_ucb_begin(nullptr, GPSO_F64, GPSO_MEM_DEVICE, 0, nullptr, nseg, acq_spec(ctx, acq), bounds, depth);
}

int gpso_acq_values(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_acq* acq, double* mean,
                    double* var, double* value, int out_mem) {
  ACQ_ENTER();
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "bad out_mem %d", out_mem);
  return ctx->eng->acq_values(xs, xs_dtype, xs_mem, m, acq_spec(ctx, acq), mean, var, value, out_mem);
}

int gpso_best_batch(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_acq* acq, double obs_noise, int q,
                    int64_t* idx, double* mean, double* var, double* value, int* n_picked, double* var_after, int out_mem) {
  ACQ_ENTER();
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "bad out_mem %d", out_mem);
  return ctx->eng->best_batch(xs, xs_dtype, xs_mem, m, acq_spec(ctx, acq), obs_noise, q, idx, mean, var, value, n_picked, var_after, out_mem);
}

int gpso_batch_greedy_host(const gpso_acq* acq, const double* mean, const double* s2, const double* cov, double noise, double obs_noise,
                           int64_t m, int q, int64_t* idx, double* var, double* value, int* n_picked, double* var_after) {
  if (acq_refusal(acq) != nullptr || m < 1 || q < 1 || q > gpso::kBatchMaxPicks || m > gpso::kBatchMaxCells / q || !mean || !s2 || !cov ||
      !idx || !n_picked || noise != noise || !(obs_noise >= 0.0) || obs_noise - obs_noise != 0.0)
    return GPSO_E_ARG;
  return gpso::batch_greedy_host(acq_spec(acq), mean, s2, cov, noise, obs_noise, m, q, idx, var, value, n_picked, var_after);
}

int gpso_batch_greedy_mes_host(const double* ystar, int k, int latent, const double* mean, const double* s2, const double* cov,
                               double noise, double obs_noise, int64_t m, int q, int64_t* idx, double* var, double* value,
                               int* n_picked, double* var_after) {
  if (!maxima_usable(ystar, k) || m < 1 || q < 1 || q > gpso::kBatchMaxPicks || m > gpso::kBatchMaxCells / q || !mean || !s2 || !cov ||
      !idx || !n_picked || noise != noise || !(obs_noise >= 0.0) || obs_noise - obs_noise != 0.0)
    return GPSO_E_ARG;
  return gpso::batch_greedy_host(mes_spec_host(ystar, k, latent), mean, s2, cov, noise, obs_noise, m, q, idx, var, value, n_picked,
                                 var_after);
}

int gpso_acq_set_maxima(gpso_ctx* ctx, const double* ystar, int k) {
  ENTER();
  return ctx->eng->set_maxima(ystar, k);
}

int gpso_acq_get_maxima(gpso_ctx* ctx, double* ystar, int* k) {
  if (!ctx) return GPSO_E_ARG;
  if (!k) return ctx->fail(GPSO_E_ARG, "k must not be NULL");
  *k = ctx->eng->maxima_k;
  if (ystar) std::memcpy(ystar, ctx->eng->maxima_host, (size_t)*k * 8);
  return GPSO_OK;
}

int gpso_acq_mes_eval_host(const double* ystar, int k, int latent, const double* mean, const double* var, double noise, int64_t n,
                           double* out) {
  if (!maxima_usable(ystar, k) || n < 0 || (n > 0 && (!mean || !var || !out)) || noise != noise) return GPSO_E_ARG;
  gpso::acq_eval_host(mes_spec_host(ystar, k, latent), mean, var, noise, (long long)n, out);
  return GPSO_OK;
}

int gpso_acq_math_host(int fn, const double* x, int64_t n, double* out) {
  if (n < 0 || (n > 0 && (!x || !out))) return GPSO_E_ARG;
  return gpso::acq_math_host(fn, x, (long long)n, out) == 0 ? GPSO_OK : GPSO_E_ARG;
}

int gpso_max_logcdf(gpso_ctx* ctx, const double* mean, const double* var, int mem, int64_t m, double var_sub, const double* y, int g,
                    double* logcdf, int64_t* n_used) {
  ENTER();
  return ctx->eng->max_logcdf(mean, var, mem, m, var_sub, y, g, logcdf, n_used);
}

int gpso_max_logcdf_host(const double* mean, const double* var, int64_t m, double var_sub, const double* y, int g, double* logcdf,
                         int64_t* n_used) {
  if (!mean || !var || !y || !logcdf || m < 1 || g < 1 || g > kMaxCdfThresholds || var_sub != var_sub) return GPSO_E_ARG;
  for (int i = 0; i < g; ++i)
    if (y[i] != y[i]) return GPSO_E_ARG;
  long long used = 0;
  gpso::max_logcdf_host(mean, var, (long long)m, var_sub, y, g, logcdf, &used);
  if (n_used) *n_used = used;
  return GPSO_OK;
}

int gpso_screen_probe(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double varsigma, double* my, double* ub,
                      double* flag, double* info) {
  ENTER();
  return ctx->eng->screen_probe(xs, xs_dtype, xs_mem, m, varsigma, my, ub, flag, info);
}

int gpso_screen_list(gpso_ctx* ctx, int64_t max_rows, int64_t* key, float* rows, int64_t* live) {
  ENTER();
  return ctx->eng->screen_list(max_rows, key, rows, live);
}

int gpso_screen_eval_host(const double* my, const double* v, double variance, double noise, double varsigma, int64_t n,
                          double* ucb, double* ub) {
  if (n < 0 || (n > 0 && !my)) return GPSO_E_ARG;
  gpso::screen_eval_host(my, v, variance, noise, varsigma, (long long)n, ucb, ub);
  return GPSO_OK;
}

double gpso_screen_threshold_host(double max_my, double noise, double varsigma) {
  return gpso::screen_threshold_host(max_my, noise, varsigma);
}

int gpso_screen_survives_host(double my, double ub, double threshold) { return gpso::screen_survives_host(my, ub, threshold); }

int gpso_screen_accepts_host(double u_star, double threshold, int64_t count, int64_t cap) {
  return gpso::screen_accepts_host(u_star, threshold, (long long)count, (long long)cap);
}

int gpso_screen_partition_host(int64_t m, int parts, int w, int64_t* lo, int64_t* hi) {
  if (m < 0 || parts < 1 || w < 0 || w >= parts || !lo || !hi) return GPSO_E_ARG;
  long long a = 0, b = 0;
  gpso::screen_partition_host((long long)m, parts, w, &a, &b);
  *lo = a;
  *hi = b;
  return GPSO_OK;
}

int gpso_screen_parts_host(int64_t m) { return gpso::screen_parts_host((long long)m); }

int gpso_acq_eval_host(const gpso_acq* acq, const double* mean, const double* var, double noise, int64_t n, double* out) {
  if (acq_refusal(acq) != nullptr || n < 0 || (n > 0 && (!mean || !var || !out)) || noise != noise) return GPSO_E_ARG;
  gpso::acq_eval_host(acq_spec(acq), mean, var, noise, (long long)n, out);
  return GPSO_OK;
}

int64_t gpso_padded_n(const gpso_ctx* ctx) {
  return ctx ? ctx->eng->padded_n() : 0;
}

int gpso_problem_shape(const gpso_ctx* ctx, int64_t* n, int* d) {
  if (!ctx) return GPSO_E_ARG;
  int64_t nn = 0;
  int dd = 0;
  ctx->eng->problem_shape(&nn, &dd);
  if (n) *n = nn;
  if (d) *d = dd;
  return GPSO_OK;
}

int gpso_get_matrix(gpso_ctx* ctx, int which, double* out) {
  ENTER();
  return ctx->eng->get_matrix(which, out);
}

int gpso_get_vector(gpso_ctx* ctx, int which, double* out) {
  ENTER();
  return ctx->eng->get_vector(which, out);
}

int gpso_posterior_buffers(gpso_ctx* ctx, void** ptrs, int64_t* nbytes, int cap) {
  ENTER();
  if (!ptrs || !nbytes) return ctx->fail(GPSO_E_ARG, "NULL argument");
  return ctx->eng->posterior_buffers(ptrs, nbytes, cap);
}

int gpso_posterior_span(gpso_ctx* ctx, void** ptr, int64_t* offset, int64_t* nbytes) {
  ENTER();
  return ctx->eng->posterior_span(ptr, offset, nbytes);
}

int gpso_posterior_span_at(gpso_ctx* ctx, int64_t offset, int64_t nbytes, void** ptr) {
  ENTER();
  if (!ptr) return ctx->fail(GPSO_E_ARG, "ptr must not be NULL");
  return ctx->eng->posterior_span_at(offset, nbytes, ptr);
}

int gpso_posterior_hash(gpso_ctx* ctx, uint64_t* out) {
  ENTER();
  if (!out) return ctx->fail(GPSO_E_ARG, "out must not be NULL");
  return ctx->eng->posterior_hash(out);
}

int gpso_alloc_posterior(gpso_ctx* ctx, int64_t n, int d) {
  ENTER();
  return ctx->eng->alloc_posterior(n, d);
}

int gpso_adopt_posterior(gpso_ctx* ctx) {
  ENTER();
  return ctx->eng->adopt_posterior();
}

double gpso_last_ms(gpso_ctx* ctx, int what) {
  if (!ctx || what < 0 || what > 3) return -1.0;
  return ctx->last_ms[what];
}

// ---- multi-GPU group --------------------------------------------------------------------------
int gpso_comm_unique_id(void* out) {
  if (!out) return GPSO_E_ARG;
  RcclApi& R = RcclApi::get();
  if (!R.ok) {
    g_create_error = R.load_error;
    return GPSO_E_RCCL;
  }
  ncclUniqueId id;
  const ncclResult_t r = R.GetUniqueId(&id);
  if (r != ncclSuccess) {
    g_create_error = std::string("ncclGetUniqueId: ") + R.GetErrorString(r);
    return GPSO_E_RCCL;
  }
  static_assert(sizeof(id) == GPSO_UNIQUE_ID_BYTES, "unique id size");
  std::memcpy(out, &id, sizeof(id));
  return GPSO_OK;
}

int gpso_comm_init(gpso_ctx* ctx, int rank, int world, const void* unique_id) {
  ENTER();
  if (!unique_id) return ctx->fail(GPSO_E_ARG, "unique_id must not be NULL");
  if (world < 1 || rank < 0 || rank >= world) return ctx->fail(GPSO_E_ARG, "rank %d / world %d", rank, world);
  if (ctx->comm) return ctx->fail(GPSO_E_STATE, "the context already belongs to a group%s (gpso_comm_destroy first)",
                                  ctx->comm_aborted.load() ? " whose communicator was aborted" : "");
  RcclApi& R = RcclApi::get();
  if (!R.ok) return ctx->fail(GPSO_E_RCCL, "%s", R.load_error.c_str());
  ncclUniqueId id;
  std::memcpy(&id, unique_id, sizeof(id));
  RCCLCHECK(R.CommInitRank(&ctx->comm, world, id, rank));
  ctx->rank = rank;
  ctx->world = world;
  return GPSO_OK;
}

int gpso_comm_destroy(gpso_ctx* ctx) {
  ENTER();
  if (ctx->comm && !ctx->comm_aborted) {
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    RCCLCHECK(RcclApi::get().CommDestroy(ctx->comm));
  }
  ctx->comm = nullptr;
  ctx->comm_aborted = false;
  ctx->rank = 0;
  ctx->world = 1;
  return GPSO_OK;
}

int gpso_comm_info(const gpso_ctx* ctx, int* rank, int* world) {
  if (!ctx) return GPSO_E_ARG;
  if (rank) *rank = ctx->rank;
  if (world) *world = ctx->world;
  return ctx->comm ? 1 : 0;
}

void gpso_shard_range(int64_t m, int rank, int world, int64_t* lo, int64_t* hi) {
  int64_t a = 0, b = 0;
  if (world >= 1 && rank >= 0 && rank < world && m >= 0) shard_range(m, rank, world, &a, &b);
  if (lo) *lo = a;
  if (hi) *hi = b;
}

int gpso_broadcast_posterior(gpso_ctx* ctx, int root) {
  ENTER();
  return ctx->eng->broadcast_posterior(root);
}

int gpso_broadcast_posterior_rows(gpso_ctx* ctx, int root) {
  ENTER();
  return ctx->eng->broadcast_posterior_rows(root);
}

int gpso_posterior_dirty_ranges(gpso_ctx* ctx, int64_t* offsets, int64_t* nbytes, int cap) {
  ENTER();
  return ctx->eng->posterior_dirty_ranges(offsets, nbytes, cap);
}

int gpso_posterior_mark_synced(gpso_ctx* ctx) {
  ENTER();
  return ctx->eng->posterior_mark_synced();
}

int gpso_best_ucb_sharded(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m_local,
                          int64_t m_global, const int64_t* seg_off, int nseg, double varsigma, int64_t* idx,
                          double* mean, double* var, double* ucb) {
  ENTER();
  return ctx->eng->best_ucb_sharded(xs, xs_dtype, xs_mem, m_local, m_global, seg_off, nseg, varsigma, idx, mean,
                                    var, ucb);
}

int gpso_best_ucb_grow_sharded(gpso_ctx* ctx, const double* bounds, int nseg, int depth, double varsigma,
                               int64_t* idx, double* mean, double* var, double* ucb) {
  ENTER();
  return ctx->eng->best_ucb_grow_sharded(bounds, nseg, depth, varsigma, idx, mean, var, ucb);
}

int gpso_shard_winners(gpso_ctx* ctx, int rank, int world, const void* xs, int xs_dtype, int xs_mem,
                       int64_t m_local, int64_t m_global, const int64_t* seg_off, int nseg, double varsigma,
                       double* payload) {
  ENTER();
  return ctx->eng->shard_winners(rank, world, xs, xs_dtype, xs_mem, m_local, m_global, seg_off, nseg, varsigma, payload);
}

int gpso_shard_winners_grow(gpso_ctx* ctx, int rank, int world, const double* bounds, int nseg, int depth,
                            double varsigma, double* payload) {
  ENTER();
  return ctx->eng->shard_winners_grow(rank, world, bounds, nseg, depth, varsigma, payload);
}

int gpso_fold_winners(gpso_ctx* ctx, const double* gathered, int world, int64_t m_global, const int64_t* seg_off,
                      int nseg, int64_t* idx, double* mean, double* var, double* ucb) {
  ENTER();
  return ctx->eng->fold_winners(gathered, world, m_global, seg_off, nseg, idx, mean, var, ucb);
}

int gpso_group_payload_doubles(int nseg) { return nseg < 0 ? 0 : gpso::group_payload_doubles(nseg); }

// Callable from ANOTHER thread than the one blocked inside a group call of this context: it only touches the
// communicator (ncclCommAbort makes the collective kernels in flight exit, so the blocked call returns an error).
int gpso_comm_abort(gpso_ctx* ctx) {
  if (!ctx) return GPSO_E_ARG;
  ncclComm_t c = ctx->comm;
  if (c == nullptr) return GPSO_OK;
  RcclApi& R = RcclApi::get();
  if (!R.ok || R.CommAbort == nullptr) return GPSO_E_RCCL;
  if (ctx->comm_aborted.exchange(true)) return GPSO_OK;  // (already aborted: the handle is gone)
  return R.CommAbort(c) == ncclSuccess ? GPSO_OK : GPSO_E_RCCL;
}

int64_t gpso_last_count(gpso_ctx* ctx, int what) {
  if (!ctx || what < 0 || what > 8) return -1;
  return what == 4 ? g_dev_bytes_held.load(std::memory_order_relaxed) : ctx->last_count[what];
}

const char* gpso_version(void) { return "gpso-hip 0.5.0 (gfx950)"; }

}  // extern "C"
