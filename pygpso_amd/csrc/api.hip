// C-ABI of libgpso_hip.so (see include/gpso_hip.h): context, device memory, call sequencing.
// No torch, no BLAS/solver libraries: every kernel launched here is hand-written (predict.hip,
// fit.hip, grow.hip).
#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>
#include <set>
#include <utility>

#include "engine_core.hpp"

using namespace gpso;
using namespace gpso::host;

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

// launcher-side errors (hipFuncSetAttribute, unsupported GEMM shapes) + the HIP launch status
int host::EngineCore::launch_status() {
  HIPCHECK(hipGetLastError());
  if (!g_launch_error.empty()) {
    const std::string msg = g_launch_error;
    g_launch_error.clear();
    return ctx->fail(GPSO_E_HIP, "%s", msg.c_str());
  }
  return GPSO_OK;
}

}  // namespace gpso

namespace {

thread_local std::string g_create_error;

// contiguous share [lo, hi) of m items for `rank` of `world`: global order is preserved across ranks
inline void shard_range(int64_t m, int rank, int world, int64_t* lo, int64_t* hi) {
  const int64_t base = m / world, extra = m % world;
  *lo = rank * base + std::min<int64_t>(rank, extra);
  *hi = *lo + base + (rank < extra ? 1 : 0);
}

}  // namespace

namespace gpso::host {
namespace {

// TF: fit type (Gram, Cholesky, L^-1, alpha);  TP: predict / apply type.
//   GPSO_F64   -> EngineT<double, double>
//   GPSO_F32   -> EngineT<float, float>
//   GPSO_MIXED -> EngineT<double, float>
template <typename TF, typename TP>
struct EngineT : EngineCore {
  explicit EngineT(gpso_ctx* c) : EngineCore(c, sizeof(TF), sizeof(TP) == 4) {
    check = sizeof(TP) == 4;  // float predict arithmetic: self-test on by default
    // default tolerances: a double factor with a float apply measures 1e-6 .. 3e-5 (bf16x3) -> 1e-4; an
    // all-float engine is a 1e-4-class instrument already at noise 1e-3 -> 1e-3
    tol_var = tol_mean = (sizeof(TF) == 4) ? 1.0e-3 : 1.0e-4;
  }
  static constexpr bool kFloatPredict = sizeof(TP) == 4;
  static constexpr int kAutoFirst = kFloatPredict ? GPSO_MATH_F16X3 : GPSO_MATH_NATIVE;
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
  // A best-UCB call in flight (best_call.hpp): the entry point's plan goes down, the enqueue's record comes back.
  using BestPlan = gpso::BestPlan; using BestCall = gpso::BestCall; using BestKind = gpso::BestKind;
  // the pinned memory the call's last kernel -- about to be launched -- writes nseg records to, and the token behind them
  double* result_host(const BestPlan& plan, BestCall& call, int nseg) { return call.writes_host(plan.slot ? plan.slot : ctx->pinned_scratch((size_t)nseg * 4 + 3)); }
  double arm_token(BestCall& call, bool single_workgroup, int nseg) { return call.arm_token(single_workgroup, nseg, ctx->next_token()); }
  // -> where the fit's pass leaves the maximum, nullptr when the fp16 split does not apply to this posterior
  float* f16_max_for_fit() {
    f16_handed_at = nullptr;
    if constexpr (!kFloatPredict) return nullptr;
    if (!f16_split() || !bf16_usable()) return nullptr;
    if (ensure(linv_b, split_bytes()) != GPSO_OK || ensure(amax_rows, (size_t)npad * 4) != GPSO_OK) return nullptr;
    f16_handed_at = f16_scale();
    return f16_scale();
  }

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
  // the typed step of EngineCore::install_predictive: the predict-ready copies of what the install left in linv and alpha_f
  int pack_predictive(hipStream_t s) override {
    launch_pack_linv<TF, TP>(s, as<TF>(linv), n, npad, as<TP>(linv_p));
    launch_convert_vec<TF, TP>(s, as<TF>(alpha_f), as<TP>(alpha), npad);
    return pack_bf16();
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
      case GPSO_OPT_SURVIVOR_TILE:
        if (value < 0 || value > 2)
          return ctx->fail(GPSO_E_ARG, "survivor tile: 0 (narrow for a screened call's survivors), 1 (wide everywhere) or 2 (narrow wherever the default kernels run)");
        survivor_tile = value;
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

  // ---- batched evaluation (multi-start hyper-parameter search): fit.hip small_fit_batch_kernel; EngineCore checks the call ----
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
    if ((rc = pack_predictive(s))) return rc;
    HIPCHECK(hipStreamSynchronize(s));  // the caller's host buffers are free again on return
    if ((rc = launch_status())) return rc;
    res.installed();
    return GPSO_OK;
  }

  // ------------------------------------------------------------------------------------------
  // leaves already on the device as raw coordinates (dtype xs_dtype) -> mean/var(/ucb) device arrays.
  // TG = generation type (double unless the context is float-predict with GPSO_GEN_F32).
  // defer (nullable): the caller's arg-max can finalise the leaves itself (launch_seg_argmax / launch_keyed_argmax with
  // a LeafFinalize) -- when the batch is ONE chunk the finalize launch is skipped and *defer says what to finalise;
  // otherwise defer->part_var stays NULL and the leaves are finalised here as before
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
          // GPSO_OPT_SURVIVOR_TILE = 2: the narrow tile for float leaves whatever the call (the launcher keeps the wide kernel
          // outside the default family)
          if (survivor_tile == 2 && xs_dtype == GPSO_F32) a.tile = LeafTile::Narrow;
          a.splits_out = &ctx->last_count[3]; a.tile_out = &ctx->last_count[9];
          a.park_bytes = park_bytes; a.park_scratch = &EngineT::park_cb; a.park_owner = this; a.park_out = &ctx->last_count[5];
          if (span.open && m_live_c != nullptr && span.narrow_max > 0) {
            // A screened call's survivors (m_live_c: the screen's control block).  A few hundred leaves are a chain on a handful
            // of CUs under the wide tile and spread over four times as many under the narrow one; near the room's edge the wide
            // tile is the faster one.  Only the device knows the count: where both can happen both launches are enqueued, each
            // behind the live-row word the compaction left for ITS tile -- the other one's is zero, and it leaves at once.
            const bool both = span.narrow_max < mp;
            a.tile = LeafTile::Narrow;
            if (both) a.m_live = m_live_c + kScreenCtlNarrow;
            rc = launch_leaf_tiles_bf16<TG>(s, kp, a, split_variant);
            if (rc == 0 && both) {
              a.tile = LeafTile::Wide;
              a.m_live = m_live_c + kScreenCtlWide;
              rc = launch_leaf_tiles_bf16<TG>(s, kp, a, split_variant);
            }
          } else {
            rc = launch_leaf_tiles_bf16<TG>(s, kp, a, split_variant);
          }
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

  int score_device_leaves(const void* xs_dev, int xs_dtype, int64_t m, const AcqSpec& acq, bool want_ucb, double* mean_dev,
                          double* var_dev, double* ucb_dev, TileSpan& span, const int64_t* m_live = nullptr,
                          LeafFinalize* defer = nullptr, bool prepared = false) override {
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
  // called at the top of every predict-type entry point
  int precision_gate() override {
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

  // ---- best-UCB sequencing: enqueue the local work (winners stay on the device, no host wait) ->
  //      [multi-GPU: all-gather + fold] -> one read-back ------------------------------------------------
  // ---- one-launch small calls (predict.hip: leaf_tiles_v2_one_kernel) -------------------------------------------------
  // Applies when the native tile kernel runs this posterior with ONE row block (N_pad = 128 or 256) and the batch is
  // small.  Returns 0 when the call was enqueued (records on their way to ovals and pinned host memory), 2 when it does
  // not apply -- the caller goes on with the next-best sequence --, or a negative status.  mode: finish_best's read-back
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
  // GPSO_OPT_SURVIVOR_TILE for a survivors' launch with room for cap rows: 1 -- no count takes the narrow tile, 2 -- every count,
  // 0 -- the counts the makespan model gives it (screen.hpp)
  int64_t survivor_narrow_rows(int64_t cap) const {
    if (survivor_tile == 1) return 0;
    if (survivor_tile == 2) return cap;
    return survivor_narrow_max((int)(npad / 256), ctx->cu_count, cap);
  }
  int enqueue_screen(const void* dev, int64_t m, const AcqSpec& acq, bool probe, int64_t narrow_max = 0) {
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
      b.raw = static_cast<const float*>(dev); b.d = d; b.cap = cap; b.narrow_max = narrow_max; b.counts = as<int64_t>(screen_cnt);
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
    const int64_t narrow_max = survivor_narrow_rows(cap);
    if ((rc = enqueue_screen(dev, m, acq, false, narrow_max))) return rc;
    LeafFinalize fin{};
    TileSpan span{plan.timed, true, 0, narrow_max};
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
    call.screened(dev, GPSO_F32, m, acq, narrow_max);  // (what a re-run takes: the caller keeps device leaves untouched until the record is read)
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
      if ((rc = screen_verdict(call, vals))) return rc;
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
  int screen_verdict(const BestCall& call, const double* vals) {
    std::memcpy(&ctx->last_count[7], &vals[4], 8);
    ctx->last_count[9] = ctx->last_count[7] <= call.narrow_max ? 64 : 256;  // (the tile this count's survivors' launch ran)
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
  // 64-bit fingerprint of the predict-ready posterior (the buffers gpso_posterior_buffers lists, the parts in use):
  // two contexts that ran the same deterministic fit hold the same value -- what a group that REPLICATES the fit on
  // every rank compares instead of broadcasting ("measure both")
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
}  // namespace gpso::host

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
// the Bernoulli kind is the dense VGP's alone: the sparse family refuses it whole, it does not half-serve it
static int refuse_bernoulli_sparse(gpso_ctx* ctx, const char* who) {
  if (ctx->eng->vlik_kind != GPSO_LIK_BERNOULLI) return GPSO_OK;
  return ctx->fail(GPSO_E_ARG, "%s: GPSO_LIK_BERNOULLI is served by the dense variational GP (gpso_vgp_*) only, not by the sparse family", who);
}
int gpso_svgp_init_q(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                     double noise_variance) {
  ENTER();
  if (int rcb = refuse_bernoulli_sparse(ctx, "gpso_svgp_init_q")) return rcb;
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  Theta th{};
  if (!(noise_variance > 0.0)) return ctx->eng->svgp_init_q(th, 0.0);  // the prior
  int rc = theta_of_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), &th);
  if (rc) return rc;
  return ctx->eng->svgp_init_q(th, noise_variance);
}

int gpso_svgp_set_q(gpso_ctx* ctx, const double* mu, const double* S, int64_t m) {
  ENTER();
  if (int rcb = refuse_bernoulli_sparse(ctx, "gpso_svgp_set_q")) return rcb;
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  if ((mu == nullptr) != (S == nullptr)) return ctx->fail(GPSO_E_ARG, "mu and S: both or neither");
  return ctx->eng->svgp_set_q(mu, S, m);
}

int gpso_svgp_get_q(gpso_ctx* ctx, double* mu, double* S) {
  ENTER();
  if (int rcb = refuse_bernoulli_sparse(ctx, "gpso_svgp_get_q")) return rcb;
  return ctx->eng->svgp_get_q(mu, S);
}

int gpso_svgp_natgrad(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                      double gamma) {
  ENTER();
  if (int rcb = refuse_bernoulli_sparse(ctx, "gpso_svgp_natgrad")) return rcb;
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  Theta th;
  int rc = theta_of_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), &th);
  if (rc) return rc;
  return ctx->eng->svgp_natgrad(th, gamma);
}

int gpso_svgp_elbo_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                     double* loss, double* grad_u, double* theta_out) {
  ENTER();
  if (int rcb = refuse_bernoulli_sparse(ctx, "gpso_svgp_elbo_u")) return rcb;
  if (int rcs = refuse_noise_diag(ctx)) return rcs;
  if (!loss) return ctx->fail(GPSO_E_ARG, "loss must not be NULL");
  return eval_in_u(ctx, kernel, u, n_ls, train_mean, mean_c_fixed, vlik_floor(ctx), grad_u, false, theta_out,
                   [&](const Theta& th, double* g) { return ctx->eng->svgp_elbo(th, loss, g); });
}

int gpso_svgp_posterior(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                        double* delta_out) {
  ENTER();
  if (int rcb = refuse_bernoulli_sparse(ctx, "gpso_svgp_posterior")) return rcb;
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
  if (int rcb = refuse_bernoulli_sparse(ctx, "gpso_svgp_elbo_uz")) return rcb;
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

// ---- the hyper-parameter ensemble (ensemble.hpp) -------------------------------------------------
int gpso_ensemble_max(gpso_ctx* ctx) { return ctx ? ctx->eng->ensemble_max() : 0; }

int gpso_ensemble_push(gpso_ctx* ctx) {
  ENTER();
  return ctx->eng->ensemble_push();
}

int gpso_ensemble_clear(gpso_ctx* ctx) {
  ENTER();
  return ctx->eng->ensemble_clear();
}

int gpso_ensemble_info(gpso_ctx* ctx, int* k, double* theta) {
  if (!ctx) return GPSO_E_ARG;
  return ctx->eng->ensemble_info(k, theta);
}

int gpso_ensemble_best_acq(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
                           const gpso_acq* acq, int64_t* idx, double* mean_mix, double* var_mix, double* value) {
  ENTER();
  if (acq && acq->kind == GPSO_ACQ_MES)
    return ctx->fail(GPSO_E_ARG, "gpso_ensemble_best_acq: GPSO_ACQ_MES is not integrated over an ensemble: its maxima belong to one theta");
  if (const char* why = acq_refusal(acq)) return ctx->fail(GPSO_E_ARG, "gpso_ensemble_best_acq: %s", why);
  return ctx->eng->ensemble_best_acq(xs, xs_dtype, xs_mem, m, seg_off, nseg, acq_spec(acq), idx, mean_mix, var_mix, value);
}

int gpso_ensemble_acq_values(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_acq* acq, double* mean_mix,
                             double* var_mix, double* value, double* member_mean, double* member_var, int out_mem) {
  ENTER();
  if (acq && acq->kind == GPSO_ACQ_MES)
    return ctx->fail(GPSO_E_ARG, "gpso_ensemble_acq_values: GPSO_ACQ_MES is not integrated over an ensemble: its maxima belong to one theta");
  if (const char* why = acq_refusal(acq)) return ctx->fail(GPSO_E_ARG, "gpso_ensemble_acq_values: %s", why);
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "gpso_ensemble_acq_values: bad out_mem %d", out_mem);
  return ctx->eng->ensemble_acq_values(xs, xs_dtype, xs_mem, m, acq_spec(acq), mean_mix, var_mix, value, member_mean, member_var, out_mem);
}

int gpso_ensemble_fold_host(const gpso_acq* acq, const double* member_mean, const double* member_var, const double* noise, int k, int64_t m,
                            double* mean_mix, double* var_mix, double* value) {
  if (acq_refusal(acq) != nullptr || !member_mean || !member_var || k < 1 || k > gpso::kEnsembleMax || m < 1) return GPSO_E_ARG;
  if (acq->latent != 0 && acq->kind != GPSO_ACQ_UCB_VAR && !noise) return GPSO_E_ARG;
  if (!mean_mix && !var_mix && !value) return GPSO_E_ARG;
  gpso::ensemble_fold_host(acq_spec(acq), member_mean, member_var, noise, k, m, mean_mix, var_mix, value);
  return GPSO_OK;
}

// ---- outcome constraints (constraints.hpp) -------------------------------------------------------
int gpso_constraint_max(gpso_ctx* ctx) { return ctx ? ctx->eng->constraint_max() : 0; }

int gpso_constraint_push(gpso_ctx* ctx, gpso_ctx* src, double threshold, int sense) {
  ENTER();
  if (!src) return ctx->fail(GPSO_E_ARG, "gpso_constraint_push: src must not be NULL");
  return ctx->eng->constraint_push(*src->eng, threshold, sense);
}

int gpso_constraint_clear(gpso_ctx* ctx) {
  ENTER();
  return ctx->eng->constraint_clear();
}

int gpso_constraint_info(gpso_ctx* ctx, int* k, double* theta, double* threshold, int* sense) {
  if (!ctx) return GPSO_E_ARG;
  return ctx->eng->constraint_info(k, theta, threshold, sense);
}

// what the constrained calls refuse about their two records before the engine looks at the context
static const char* constrained_refusal(const gpso_acq* acq, const gpso_cspec* cspec) {
  if (acq && acq->kind == GPSO_ACQ_MES) return "GPSO_ACQ_MES is not served under constraints";
  if (const char* why = acq_refusal(acq)) return why;
  if (!cspec) return "cspec must not be NULL";
  if (cspec->mode != GPSO_CON_WEIGHT && cspec->mode != GPSO_CON_GATE && cspec->mode != GPSO_CON_FEASIBILITY) return "unknown cspec.mode";
  if (cspec->log_pof_min != cspec->log_pof_min || cspec->log_pof_min > 0.0) return "cspec.log_pof_min must be a log-probability (<= 0; -inf: no gate)";
  if (cspec->mode == GPSO_CON_WEIGHT && (acq->kind == GPSO_ACQ_UCB_VAR || acq->kind == GPSO_ACQ_UCB_STD))
    return "a UCB kind is signed and cannot be weighted by a probability: use GPSO_CON_GATE, or EI / log-EI / PI";
  return nullptr;
}
static gpso::ConSpec con_spec(const gpso_cspec* c) {
  gpso::ConSpec s;
  s.mode = c->mode;
  s.log_pof_min = c->log_pof_min;
  return s;
}

int gpso_constrained_best_acq(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
                              const gpso_acq* acq, const gpso_cspec* cspec, int64_t* idx, double* mean, double* var, double* value,
                              double* logpof) {
  ENTER();
  if (const char* why = constrained_refusal(acq, cspec)) return ctx->fail(GPSO_E_ARG, "gpso_constrained_best_acq: %s", why);
  return ctx->eng->constrained_best_acq(xs, xs_dtype, xs_mem, m, seg_off, nseg, acq_spec(acq), con_spec(cspec), idx, mean, var, value, logpof);
}

int gpso_constrained_acq_values(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_acq* acq,
                                const gpso_cspec* cspec, double* mean, double* var, double* value, double* logpof, double* member_mean,
                                double* member_var, int out_mem) {
  ENTER();
  if (const char* why = constrained_refusal(acq, cspec)) return ctx->fail(GPSO_E_ARG, "gpso_constrained_acq_values: %s", why);
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "gpso_constrained_acq_values: bad out_mem %d", out_mem);
  return ctx->eng->constrained_acq_values(xs, xs_dtype, xs_mem, m, acq_spec(acq), con_spec(cspec), mean, var, value, logpof, member_mean,
                                          member_var, out_mem);
}

int gpso_constrained_fold_host(const gpso_acq* acq, const gpso_cspec* cspec, const double* mean, const double* var, double noise,
                               const double* member_mean, const double* member_var, const double* member_noise, const double* threshold,
                               const int* sense, int k, int64_t m, double* value, double* logpof) {
  if (constrained_refusal(acq, cspec) != nullptr || !member_mean || !member_var || !member_noise || !threshold || !sense || k < 1 ||
      k > gpso::kConstraintsMax || m < 1 || noise != noise || (!value && !logpof))
    return GPSO_E_ARG;
  if (cspec->mode != GPSO_CON_FEASIBILITY && (!mean || !var)) return GPSO_E_ARG;
  double thr[gpso::kConstraintsMax], sn[gpso::kConstraintsMax];
  for (int i = 0; i < k; ++i) {
    if ((sense[i] != 1 && sense[i] != -1) || !std::isfinite(threshold[i]) || member_noise[i] != member_noise[i]) return GPSO_E_ARG;
    thr[i] = threshold[i];
    sn[i] = (double)sense[i];
  }
  gpso::constrained_fold_host(acq_spec(acq), con_spec(cspec), mean, var, noise, member_mean, member_var, member_noise, thr, sn, k, (long long)m,
                              value, logpof);
  return GPSO_OK;
}

int gpso_constrained_success_fold_host(const gpso_acq* acq, const gpso_cspec* cspec, const double* mean, const double* var, double noise,
                                       const double* member_mean, const double* member_var, const double* member_noise,
                                       const double* threshold, const int* sense, int k, int64_t m, const double* success_mean,
                                       const double* success_var, double* value, double* logpof) {
  if (constrained_refusal(acq, cspec) != nullptr || !success_mean || !success_var || k < 0 || k > gpso::kConstraintsMax || m < 1 ||
      noise != noise || (!value && !logpof))
    return GPSO_E_ARG;
  if (k > 0 && (!member_mean || !member_var || !member_noise || !threshold || !sense)) return GPSO_E_ARG;
  if (cspec->mode != GPSO_CON_FEASIBILITY && (!mean || !var)) return GPSO_E_ARG;
  double thr[gpso::kConstraintsMax] = {}, sn[gpso::kConstraintsMax] = {};
  for (int i = 0; i < k; ++i) {
    if ((sense[i] != 1 && sense[i] != -1) || !std::isfinite(threshold[i]) || member_noise[i] != member_noise[i]) return GPSO_E_ARG;
    thr[i] = threshold[i];
    sn[i] = (double)sense[i];
  }
  gpso::constrained_success_fold_host(acq_spec(acq), con_spec(cspec), mean, var, noise, member_mean, member_var, member_noise, thr, sn, k,
                                      (long long)m, success_mean, success_var, value, logpof);
  return GPSO_OK;
}

// ---- bi-objective search (ehvi.hpp) ---------------------------------------------------------------------
// what the EHVI calls refuse about their two records before the engine looks at the context
static const char* ehvi_refusal(const gpso_ehvi* e, const gpso_cspec* cspec) {
  if (!e) return "ehvi must not be NULL";
  if (const char* why = gpso::ehvi_front_refusal(e->p, e->front, e->ref)) return why;
  if (!cspec) return nullptr;
  if (cspec->mode == GPSO_CON_FEASIBILITY) return "GPSO_CON_FEASIBILITY ranks by logpof alone: gpso_constrained_best_acq / gpso_constrained_acq_values serve it";
  if (cspec->mode != GPSO_CON_WEIGHT && cspec->mode != GPSO_CON_GATE) return "unknown cspec.mode";
  if (cspec->log_pof_min != cspec->log_pof_min || cspec->log_pof_min > 0.0) return "cspec.log_pof_min must be a log-probability (<= 0; -inf: no gate)";
  return nullptr;
}
static gpso::EhviSpec ehvi_spec(const gpso_ehvi* e, const gpso_cspec* cspec) {
  gpso::EhviSpec s;
  s.member = e->member;
  s.latent = e->latent != 0 ? 1 : 0;
  s.p = e->p;
  gpso::ehvi_strips(e->p, e->front, e->ref, s.xa, s.xh);
  s.has_con = cspec != nullptr;
  if (cspec) s.con = con_spec(cspec);
  return s;
}

int gpso_ehvi_values(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_ehvi* ehvi, const gpso_cspec* cspec,
                     double* value, double* logpof, double* mean, double* var, int out_mem) {
  ENTER();
  if (const char* why = ehvi_refusal(ehvi, cspec)) return ctx->fail(GPSO_E_ARG, "gpso_ehvi_values: %s", why);
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "gpso_ehvi_values: bad out_mem %d", out_mem);
  return ctx->eng->ehvi_values(xs, xs_dtype, xs_mem, m, ehvi_spec(ehvi, cspec), value, logpof, mean, var, out_mem);
}

int gpso_best_ehvi(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, const gpso_ehvi* ehvi,
                   const gpso_cspec* cspec, int64_t* idx, double* value, double* logpof, double* mean, double* var) {
  ENTER();
  if (const char* why = ehvi_refusal(ehvi, cspec)) return ctx->fail(GPSO_E_ARG, "gpso_best_ehvi: %s", why);
  return ctx->eng->best_ehvi(xs, xs_dtype, xs_mem, m, seg_off, nseg, ehvi_spec(ehvi, cspec), idx, value, logpof, mean, var);
}

int gpso_ehvi_fold_host(const gpso_ehvi* ehvi, const gpso_cspec* cspec, const double* mean1, const double* var1, double noise1,
                        const double* mean2, const double* var2, double noise2, const double* other_mean, const double* other_var,
                        const double* other_noise, const double* threshold, const int* sense, int k, int64_t m, const double* success_mean,
                        const double* success_var, double* value, double* logpof) {
  if (ehvi_refusal(ehvi, cspec) != nullptr || !mean1 || !var1 || !mean2 || !var2 || noise1 != noise1 || noise2 != noise2 || k < 0 ||
      k > gpso::kConstraintsMax - 1 || m < 1 || (!value && !logpof) || (success_mean == nullptr) != (success_var == nullptr))
    return GPSO_E_ARG;
  if (k > 0 && (!other_mean || !other_var || !other_noise || !threshold || !sense)) return GPSO_E_ARG;
  double thr[gpso::kConstraintsMax] = {}, sn[gpso::kConstraintsMax] = {};
  for (int i = 0; i < k; ++i) {
    if ((sense[i] != 1 && sense[i] != -1) || !std::isfinite(threshold[i]) || other_noise[i] != other_noise[i]) return GPSO_E_ARG;
    thr[i] = threshold[i];
    sn[i] = (double)sense[i];
  }
  const gpso::EhviSpec s = ehvi_spec(ehvi, cspec);
  gpso::ehvi_fold_host(s.latent, s.p, s.xa, s.xh, s.has_con, s.con, mean1, var1, noise1, mean2, var2, noise2, other_mean, other_var, other_noise,
                       thr, sn, k, (long long)m, success_mean, success_var, value, logpof);
  return GPSO_OK;
}

// ---- failed evaluations (success.hpp) ----------------------------------------------------------------
int gpso_success_prob_host(const double* mean, const double* var, int64_t n, double* logprob, double* prob) {
  if (!mean || !var || n < 1 || (!logprob && !prob)) return GPSO_E_ARG;
  gpso::success_prob_host(mean, var, (long long)n, logprob, prob);
  return GPSO_OK;
}

int gpso_predict_prob(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double* prob, double* logprob, double* mean,
                      double* var, int out_mem) {
  ENTER();
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "gpso_predict_prob: bad out_mem %d", out_mem);
  return ctx->eng->predict_prob(xs, xs_dtype, xs_mem, m, prob, logprob, mean, var, out_mem);
}

int gpso_success_push(gpso_ctx* ctx, gpso_ctx* src) {
  ENTER();
  if (!src) return ctx->fail(GPSO_E_ARG, "gpso_success_push: src must not be NULL");
  return ctx->eng->success_push(*src->eng);
}

int gpso_success_clear(gpso_ctx* ctx) {
  ENTER();
  return ctx->eng->success_clear();
}

int gpso_success_info(gpso_ctx* ctx, int* present, int64_t* n, double* theta) {
  ENTER();
  return ctx->eng->success_info(present, n, theta);
}

int gpso_batch_greedy_host(const gpso_acq* acq, const double* mean, const double* s2, const double* cov, double noise, double obs_noise,
                           int64_t m, int q, int64_t* idx, double* var, double* value, int* n_picked, double* var_after) {
  if (acq_refusal(acq) != nullptr || m < 1 || q < 1 || q > gpso::kBatchMaxPicks || m > gpso::kBatchMaxCells / q || !mean || !s2 || !cov ||
      !idx || !n_picked || noise != noise || !(obs_noise >= 0.0) || obs_noise - obs_noise != 0.0)
    return GPSO_E_ARG;
  return gpso::batch_greedy_host(acq_spec(acq), mean, s2, cov, noise, obs_noise, m, q, idx, var, value, n_picked, var_after);
}

// ---- Monte-Carlo batch acquisition over the path draws (mcbatch.hpp) --------------------------------------
int gpso_paths_best_batch(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_mcacq* acq, const double* incumbent_s,
                          const double* pending, int b, int q, int64_t* idx, double* gain, double* batch_value, int* n_picked, double* gain0,
                          int out_mem) {
  ENTER();
  if (!acq) return ctx->fail(GPSO_E_ARG, "gpso_paths_best_batch: acq must not be NULL");
  return ctx->eng->paths_best_batch(xs, xs_dtype, xs_mem, m, acq->kind, acq->xi, acq->incumbent, incumbent_s, pending, b, q, idx, gain,
                                    batch_value, n_picked, gain0, out_mem);
}

int gpso_paths_batch_host(const gpso_mcacq* acq, const double* values, int64_t s, int64_t m, int b, const double* incumbent_s, int q,
                          int64_t* idx, double* gain, double* batch_value, int* n_picked, double* gain0) {
  if (!acq || !values || !idx || !n_picked || s < 1 || s > gpso::kMcMaxDraws || m < 1 || q < 1 || q > gpso::kMcMaxPicks || b < 0 ||
      b > gpso::kMcMaxPending || m + b > gpso::kMcMaxCells / s || gpso::mc_refusal(acq->kind, acq->xi, acq->incumbent, incumbent_s, s) != nullptr)
    return GPSO_E_ARG;
  std::vector<double> bars((size_t)s, acq->incumbent);
  if (incumbent_s) std::memcpy(bars.data(), incumbent_s, (size_t)s * 8);
  return gpso::mc_batch_host(acq->kind, acq->xi, values, m + b, (int)s, m, b, bars.data(), q, idx, gain, batch_value, n_picked, gain0);
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

int64_t gpso_survivor_narrow_max_host(int row_blocks, int cus, int64_t room) {
  if (row_blocks < 1 || cus < 1 || room < 0) return GPSO_E_ARG;
  return gpso::survivor_narrow_max(row_blocks, cus, room);
}

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
  if (!ctx || what < 0 || what > 9) return -1;
  return what == 4 ? g_dev_bytes_held.load(std::memory_order_relaxed) : ctx->last_count[what];
}

const char* gpso_version(void) { return "gpso-hip 0.5.0 (gfx950)"; }

}  // extern "C"
