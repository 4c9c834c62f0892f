// The engine behind a context, without its types: everything a context keeps -- shape, residency record,
// hyper-parameters, every buffer and option -- and every helper and call that touches no typed buffer.  Members are defined here
// (inline), in engine_points.hip and in engine_variational.hip.  What launches a kernel instantiated on the fit type TF or the
// predict type TP is a pure virtual here and an override in api.hip's EngineT<TF, TP>.
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>

#include "batch.hpp"
#include "constraints.hpp"
#include "context.hpp"
#include "devbuf.hpp"
#include "ehvi.hpp"
#include "ensemble.hpp"
#include "mcbatch.hpp"
#include "resident.hpp"
#include "screen.hpp"

namespace gpso::host {

struct EngineCore {
  gpso_ctx* ctx;
  // what the core needs to know of EngineT<TF, TP>: bytes of a fit-type element, and whether the predict type is float
  const size_t fit_elem;
  const bool float_predict;
  size_t pred_elem() const { return float_predict ? 4 : 8; }
  EngineCore(gpso_ctx* c, size_t fit_elem_, bool float_predict_) : ctx(c), fit_elem(fit_elem_), float_predict(float_predict_) {}
  virtual ~EngineCore() {}

  // problem
  int64_t n = 0, npad = 0;
  int d = 0, dp = 0;
  // which of the buffers below mean something (resident.hpp: the record and its transitions, its only writers)
  gpso::Resident res{float_predict ? GPSO_MATH_F16X3 : GPSO_MATH_NATIVE};
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
  bool has_noise_diag() const { return res.have_s; }
  int fit_overlap = 2;              // GPSO_OPT_FIT_OVERLAP (bit 0 look-ahead, bit 1 overlapped inverse: the default): two-level double fits overlap chains, updates and the inverse (0: sequential, round 5)
  int fit_planes_mode = 2;          // GPSO_OPT_FIT_BF16_SYRK: 0 f32 MFMA | 1 bf16 pieces (6 MFMAs per product) | 2 fp16 pieces (3) where representable
  // predict math, the OPTION (what the posterior uses: res.math).  GPSO_MATH_AUTO walks the ladder fp16 split (3 MFMAs per
  // product) -> bf16x6 -> f32 MFMA kernel, one rung down each time the posterior's self-test fails on it (selftest_with_fallback)
  bool math_auto = float_predict;
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
  int contraction = GPSO_CONTRACTION_AUTO;     // GPSO_OPT_CONTRACTION
  // the x.x* contraction of the fp16-split kernel runs on the fp16 pipe under float generation (D_pad + 1 slots in at most
  // two chunks of 32: every D this library accepts).  Measured in one process on one posterior (tools/c16_check.py,
  // profiles/r04_c16_check.jsonl), fp16 pipe against the f32 instruction: D = 6 +4 %, 12 +8 %, 20 +17 %, 33 +28 %, 40 +30 %
  bool c16_in_use(bool gen64) const {
    if (!float_predict || gen64 || res.c16_fallback || !f16_split() || contraction == GPSO_CONTRACTION_F32 || leaf_c16_chunks(dp / 4) > 2) return false;
    return leaf_bf16_lds_bytes(2, dp / 4, 4, true) <= 160 * 1024;
  }
  bool small_calls = true, one_launch = true, one_launch_everywhere = false;  // GPSO_OPT_SMALL_CALLS
  bool fuse_prep = true;  // GPSO_OPT_FUSED_PREP: float leaves are scaled in the fp16-contraction kernel's prologue (same bits)
  int64_t single_level_max = -1;  // < 0: library default
  bool fused_small = true;        // GPSO_OPT_FIT_FUSED_SMALL
  std::vector<int64_t> segoff_cache;  // what the device copy of seg_off currently holds
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
  // GPSO_OPT_SURVIVOR_TILE: 0 the narrow tile for the survivors' launch of a screened call, 1 wide everywhere, 2 narrow wherever
  // the default family runs on float device leaves (tests)
  int survivor_tile = GPSO_SURVIVOR_TILE_DEFAULT;
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
  // gpso_paths_best_batch (mcbatch.hip): scaled points of a chunk and their norms, the raw pending rows, the S x ld value matrix
  // (grow-only; gpso_paths_eval's pe_* buffers and the path set are not touched), the live flags, the blocks' maxima, the
  // state words, host-bound round-0 gains
  DevBuf mc_ts, mc_norm, mc_praw, mc_vals, mc_live, mc_bmax, mc_state, mc_g0;
  // precision self-test
  bool check = false;
  bool can_selftest() const { return check && res.st_have && res.have_data; }  // (posteriors from outside carry no targets)
  double tol_var = 1.0e-4, tol_mean = 1.0e-4;
  double st_vals[6] = {0, 0, 0, 0, 0, 0};
  DevBuf st_mean, st_var, st_out;

  int64_t padded_n() const { return npad; }
  void problem_shape(int64_t* n_out, int* d_out) const {
    *n_out = n;
    *d_out = d;
  }

  // generation type actually used by the resident posterior
  bool gen_double() const { return !float_predict || !res.gen_eff32; }
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
  bool bf16_usable() const { return res.split_usable(float_predict, npad); }
  DevBuf one_ctl, one_partial, one_ppos;  // the one-launch small calls (EngineT::try_one_launch)
  DevBuf hash_out;                       // gpso_posterior_hash
  int math_in_use() const {
    return (bf16_usable() && res.linv_b == Copy::Valid && bf16_fits(gen_double())) ? res.math : GPSO_MATH_NATIVE;
  }

  int set_option_f64(int option, double value) {
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

  int launch_status();  // (api.hip, beside the launchers' error slot)

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
    const int64_t pad = (float_predict && n > kPadN) ? 2 * kPadN : kPadN;
    npad = (n + pad - 1) / pad * pad;
    dp = (d + 3) / 4 * 4;
    int rc;
    // (room for the padded size: gpso_append adds rows in place)
    if ((rc = ensure(x64, (size_t)npad * d * 8))) return rc;
    if ((rc = ensure(y64, (size_t)npad * 8))) return rc;
    if ((rc = carve_posterior())) return rc;
    if (float_predict) {
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
  bool split_slot_exists() const { return float_predict && npad % 256 == 0; }
  int carve_posterior() {
    if (arena.p != nullptr && arena_npad == npad && arena_dp == dp) return GPSO_OK;
    const size_t b_linv = up256(packed_linv_elems(npad) * pred_elem());
    const size_t b_hyper = up256((size_t)(kHyperHeader + kMaxD) * 8);
    const size_t b_xs = up256((size_t)npad * dp * 8);
    const size_t b_norm = up256((size_t)npad * 8);
    const size_t b_alpha = up256((size_t)npad * pred_elem());
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
    if (!(float_predict && f16_split() && bf16_usable() && res.linv_b == Copy::Valid)) return GPSO_OK;
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
    rel(alpha, 0, (size_t)npad * pred_elem());  // alpha_1 += R^T a_2: every entry moved
    if (math_in_use() != GPSO_MATH_NATIVE) {
      rel(linv_b, 0, 256);  // the scale slot
      for (int s_ = 0; s_ < nsplit(); ++s_)  // plane s: tile row rt at ((s npad16 + rt) npad 32) bytes behind the slot
        rel(linv_b, 256 + ((size_t)s_ * npad16 + rt0) * npad * 32, (size_t)(rt1 + 1 - rt0) * npad * 32);
    } else {
      const size_t t0 = (size_t)rt0 * (rt0 + 1) / 2, t1 = (size_t)(rt1 + 1) * (rt1 + 2) / 2;  // tiles row-major over the triangle
      rel(linv_p, t0 * 256 * pred_elem(), (t1 - t0) * 256 * pred_elem());
    }
  }
  // can the peers be brought up to date by rows?  (root side; scale = current_split_scale)
  bool rows_apply(float scale) const {
    return res.has_post() && res.sync_n >= 0 && res.sync_n <= n && res.sync_math == math_in_use() && scale == res.sync_scale &&
           (res.sync_n == n || res.sync_n / 16 <= (n - 1) / 16);
  }

  int ensure_fit_buffers() {
    int rc;
    const size_t s = fit_elem;
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
    res.reset_generation(float_predict, math_auto, gen_mode);
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
  int set_data(const double* X, const double* y, int64_t n_, int d_) { return put_rows(X, y, n_, d_, false); }
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
  int set_noise_diag(const double* sv, int64_t n_) {
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

  // entries one launch of a batched evaluation may hold for the resident data: one workgroup per CU where the one-launch fit
  // applies, else none
  int fit_batch_max() { return (res.have_data && fused_small && small_fit_eligible(n, dp)) ? kSmallBatchMax : 0; }

  // everything a batched call is refused for, before anything is touched
  int fit_eval_batch_check(int kernel, int b, int n_ls_) {
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

  // are the tile kernel's event pairs recorded, and how many were (collect_tile_ms).  open: the survivors of a screened call -- the
  // pair's first event stands in front of the mean pass already, and the split launch's counters keep describing that pass
  // narrow_max (open): survivor counts up to this take the narrow tile (screen.hpp: survivor_narrow_max; what the compaction was told)
  struct TileSpan { bool timed; bool open = false; int pairs = 0; int64_t narrow_max = 0; };
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
  // the families that read a float64 factor (engine_points.hip, engine_variational.hip) on a float fit: refused in the
  // call's own words, never read as a format (who: the entry point's name in front of them, where two share the words)
  int need_double_fit(const char* text, const char* who = "") { return fit_elem == 8 ? GPSO_OK : ctx->fail(GPSO_E_ARG, "%s%s", who, text); }
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

  // seg_off of a best-UCB / best-acquisition call (host, nseg + 1 entries over [0, m], NULL: one segment), checked -> so
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
  int check_predict_args(const void* xs, int xs_dtype, int xs_mem, int64_t m) {
    if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "no posterior resident: call gpso_fit_eval / gpso_set_posterior first");
    if (m < 0) return ctx->fail(GPSO_E_ARG, "negative leaf count");
    int rc = check_points(xs, xs_dtype, xs_mem, m);
    return rc ? rc : precision_gate();
  }

  // gpso_screen_list: the compact list the last gpso_screen_probe left -- the survivors' indices and raw rows
  int screen_list(int64_t max_rows, int64_t* key, float* rows, int64_t* live) {
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
  // where a span (offset, nbytes) announced by a peer lands in THIS context's arena (after gpso_alloc_posterior)
  int posterior_span_at(int64_t offset, int64_t nbytes, void** ptr) {
    if (arena.p == nullptr) return ctx->fail(GPSO_E_STATE, "gpso_alloc_posterior first");
    if (offset < 0 || nbytes <= 0 || offset % 256 != 0 || (size_t)offset + (size_t)nbytes > arena.bytes)
      return ctx->fail(GPSO_E_ARG, "posterior span [%lld, +%lld) does not fit this context's arena of %zu bytes (different "
                       "dtype / shape on the sender?)", (long long)offset, (long long)nbytes, arena.bytes);
    *ptr = static_cast<char*>(arena.p) + offset;
    return GPSO_OK;
  }

  int alloc_posterior(int64_t n_, int d_) {
    int rc = refuse_if_async("gpso_alloc_posterior");
    if (rc) return rc;
    rc = shape(n_, d_);
    if (rc) return rc;
    res.shape_allocated();
    return GPSO_OK;
  }

  // ---- the point calls on the dense double factor, and the untyped calls of MES (engine_points.hip) ----
  // GPSO_ACQ_MES: the sampled maxima a context keeps for the epilogues (the caller's numbers: nothing here drops them)
  int set_maxima(const double* ystar, int k);
  double maxima_host[GPSO_ACQ_MAX_MAXIMA] = {};
  int maxima_k = 0;
  const double* maxima_dev = nullptr;
  int max_logcdf(const double* mean, const double* var, int mem, int64_t m, double var_sub, const double* y, int g, double* logcdf, int64_t* n_used);
  int predict_grad(const void* xs, int xs_dtype, int xs_mem, int64_t m, double* mean, double* var, double* dmean, double* dvar, int out_mem);
  int joint_enqueue(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, double* mean_dev, double* cov_dev, int64_t ldc, bool pad_identity);
  int joint_check(const char* what, const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add);
  int predict_joint(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, double* mean, double* cov, int out_mem);
  int sample_joint(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, const double* z, int64_t s, double* samples, int64_t* best_idx, double* best_val);
  int paths_draw_impl(bool variational, const char* who, const double* omega, const double* phase, int64_t f, const double* w, const double* eps, int64_t s);
  int paths_draw(const double* omega, const double* phase, int64_t f, const double* w, const double* eps, int64_t s) {
    return paths_draw_impl(false, "gpso_paths_draw", omega, phase, f, w, eps, s);
  }
  int paths_draw_q(const double* omega, const double* phase, int64_t f, const double* w, const double* eps, int64_t s) {
    return paths_draw_impl(true, "gpso_paths_draw_q", omega, phase, f, w, eps, s);
  }
  int paths_eval(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, double* values, int out_mem, int64_t* best_idx, double* best_val);
  void paths_info(int64_t* s_out, int64_t* f_out) const {
    *s_out = res.paths_valid ? pth.s : 0;
    *f_out = res.paths_valid ? pth.f : 0;
  }
  int cross_cov(const void* xa, int xs_dtype, int xs_mem, int64_t m, const double* xb, int b, double* cov, int out_mem);
  int best_batch(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, double obs_noise, int q, int64_t* idx, double* mean, double* var, double* value, int* n_picked, double* var_after, int out_mem);
  int paths_best_batch(const void* xs, int xs_dtype, int xs_mem, int64_t m, int kind, double xi, double incumbent, const double* incumbent_s, const double* pending, int b, int q, int64_t* idx, double* gain, double* batch_value, int* n_picked, double* gain0, int out_mem);

  // ---- the hyper-parameter ensemble (ensemble.hpp, ensemble.hip).  The members' copies -- kEnsembleMax
  // slots each of the hyper block, the scaled rows, the dense double L^-1 and alpha -- belong to the ensemble and to nothing
  // else: no fit, hand-off, hash or path set reads them.  res.ensemble says whether they describe the resident data; ens_k
  // counts them while it does.  Then the calls' workspaces: the members' columns [K][m], the three folded columns, the
  // segment offsets, the arg-max's partials and records
  DevBuf ens_hyper, ens_xs, ens_linv, ens_alpha;
  DevBuf ens_mean, ens_var, ens_mix, ens_seg, ens_part, ens_out;
  int ens_k = 0, ens_d = 0, ens_dp = 0, ens_kernel = 0;
  int64_t ens_n = 0;
  std::vector<double> ens_theta;  // [ens_k][kEnsembleTheta]: what gpso_ensemble_info reports
  static constexpr int64_t kEnsHyperStride = kHyperHeader + kMaxD;
  int ensemble_count() const { return res.ensemble ? ens_k : 0; }
  int ensemble_max() const { return (fit_elem == 8 && res.have_data && n <= kEnsembleMaxN) ? kEnsembleMax : 0; }
  int ensemble_push();
  int ensemble_clear();
  int ensemble_info(int* k, double* theta) const;
  int ensemble_refusals(const char* who, const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq);
  int ensemble_enqueue(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, hipStream_t* s);
  int ensemble_acq_values(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, double* mean_mix, double* var_mix,
                          double* value, double* member_mean, double* member_var, int out_mem);
  int ensemble_best_acq(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, const AcqSpec& acq,
                        int64_t* idx, double* mean_mix, double* var_mix, double* value);

  // ---- outcome constraints (constraints.hpp, constraints.hip).  The set's copies -- kConstraintsMax
  // slots each of a constraint model's hyper block, scaled rows, dense double L^-1 and alpha -- belong to the set and to
  // nothing else: no fit, hand-off, hash, path set or ensemble reads them.  The set is the CONTEXT's, not its data's: the
  // members have targets of their own, so res.constraints survives new data and refits and ends with gpso_constraint_clear
  // and gpso_alloc_posterior; con_k, written by a push alone, counts the members while it holds (constraint_count()).  Then the calls' workspaces: the columns [1 + J][m]
  // (row 0: the objective's), value and logpof [2][m], the segment offsets, the arg-max's partials and records, the
  // winners' logpof
  DevBuf con_hyper, con_xs, con_linv, con_alpha;
  DevBuf con_mean, con_var, con_val, con_seg, con_part, con_out, con_win;
  int con_k = 0, con_d = 0, con_dp = 0, con_kernel = 0;
  int64_t con_n = 0;
  std::vector<double> con_theta;  // [con_k][kEnsembleTheta]: what gpso_constraint_info reports
  double con_thr[kConstraintsMax] = {}, con_sense[kConstraintsMax] = {};
  int constraint_count() const { return res.constraints ? con_k : 0; }
  // (a push depends on src, not on this context's data: a context without data yet can be given members.  Data of more than
  // kEnsembleMaxN rows cannot be the objective of a constrained call, so the answer is 0 there)
  int constraint_max() const { return (fit_elem == 8 && (!res.have_data || n <= kEnsembleMaxN)) ? kConstraintsMax : 0; }
  int constraint_push(EngineCore& src, double threshold, int sense);
  int constraint_clear();
  int constraint_info(int* k, double* theta, double* threshold, int* sense) const;
  int constrained_refusals(const char* who, const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, const ConSpec& con);
  int constrained_columns(const void* xs, int xs_dtype, int xs_mem, int64_t m, hipStream_t* s);
  int constrained_enqueue(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, const ConSpec& con, hipStream_t* s);
  int constrained_acq_values(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, const ConSpec& con, double* mean,
                             double* var, double* value, double* logpof, double* member_mean, double* member_var, int out_mem);
  int constrained_best_acq(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, const AcqSpec& acq,
                           const ConSpec& con, int64_t* idx, double* mean, double* var, double* value, double* logpof);

  // ---- bi-objective search (ehvi.hpp, ehvi.hip).  Nothing resident of its own: objective 2 is a member
  // of the constraint set, the columns are the constrained calls' (constrained_columns), value and logpof land in con_val and
  // the winners' three extra columns (objective 2's mean and variance, logpof) in con_win [3][nseg]
  int ehvi_refusals(const char* who, const void* xs, int xs_dtype, int xs_mem, int64_t m, const EhviSpec& e);
  int ehvi_enqueue(const void* xs, int xs_dtype, int xs_mem, int64_t m, const EhviSpec& e, hipStream_t* s);
  int ehvi_values(const void* xs, int xs_dtype, int xs_mem, int64_t m, const EhviSpec& e, double* value, double* logpof, double* mean,
                  double* var, int out_mem);
  int best_ehvi(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, const EhviSpec& e, int64_t* idx,
                double* value, double* logpof, double* mean, double* var);

  // ---- failed evaluations (success.hpp).  The success member: ONE slot of the four copies a constraint
  // member has, of a Bernoulli-installed classifier posterior (res.bernoulli on its context) with an N and a kernel of its own.
  // Its lifetime is the constraint set's (res.success); while it is resident the constrained calls add its log-probability to
  // logpof as the last term, and serve J = 0.  suc_mean / suc_var / suc_val: gpso_predict_prob's columns and its two outputs
  DevBuf suc_hyper, suc_xs, suc_linv, suc_alpha;
  DevBuf suc_mean, suc_var, suc_val;
  int suc_d = 0, suc_dp = 0, suc_kernel = 0;
  int64_t suc_n = 0;
  double suc_theta[kEnsembleTheta] = {};  // what gpso_success_info reports
  bool success_present() const { return res.success; }
  int predict_prob(const void* xs, int xs_dtype, int xs_mem, int64_t m, double* prob, double* logprob, double* mean, double* var, int out_mem);
  int success_push(EngineCore& src);
  int success_clear();
  int success_info(int* present, int64_t* n_out, double* theta) const;

  // ---- the variational and sparse families (engine_variational.hip says what each buffer holds) ----
  DevBuf vq_mu, vq_S, vA, vB, vC, vvec, vsmall;  // the VGP: q(v) = N(mu, S S^T), three matrices, the vectors, the sums and verdicts
  int64_t vq_n = -1, vq_npad = -1;  // shape q was made for (another shape: q restarts at the prior)
  DevBuf vgh, vlvec;  // a general scalar likelihood: the Gauss-Hermite rule and the quadrature's per-point vectors
  int vlik_kind = GPSO_LIK_GAUSSIAN;  // the VGP's likelihood (GPSO_LIK_*): what slot n_ls + 1 of u means
  double vlik_df = 0.0;
  int vlik_n_gh = 0;
  DevBuf sgX, sgY, sgXs, sgXn, sgKuf, sgA, sgW, sgPart, sgM1, sgM2, sgM3, sgvecN, sgvecM, sgsmall, sggpart, sgidx;  // the SGPR
  DevBuf sgZpart, sgZg;  // the moving-Z evaluations' slice partials and dF/dZ [M x D] (inducing.hip)
  std::vector<double> sg_xh;  // host mirror of the training inputs (the rows greedy selection gathers Z from)
  int64_t sg_n = 0, sg_npad = 0;
  DevBuf svq_mu, svq_S, svB, svD, svvecN;  // the SVGP: q over the M inducing values, S^T A, A diag(a), the N-vectors
  int64_t svq_m = -1, svq_mpad = -1;  // the rows q was made for (-1: none; the next call starts q at the prior)
  double* vvec_at(int k) const { return as<double>(vvec) + (size_t)k * npad; }
  double* lvec_at(int k) const { return as<double>(vlvec) + (size_t)k * npad; }
  double* sgn_at(int k) const { return as<double>(sgvecN) + (size_t)k * sg_npad; }
  double* sgm_at(int k) const { return as<double>(sgvecM) + (size_t)k * npad; }
  double* svn_at(int k) const { return as<double>(svvecN) + (size_t)k * sg_npad; }
  int* vinfo() const;
  double vlik_const(double p) const;
  void vgp_quadrature(const double* L, double* A, double p, double mean_c);
  int vgp_set_likelihood(int kind, double df, int n_gh, const double* gh_x, const double* gh_w);
  int vgp_begin(bool sparse = false /* the rows are inducing points: the SGPR's factors go too */);
  void vgp_prior();
  int vgp_chol(double* A, double* Lout, double* Linv, int* info, double pad_diag);
  int vgp_factor(const Theta& th);
  int vgp_finish(double** out, Post kind = Post::Vgp);
  void vgp_reset_info();
  int vgp_set_q(const double* mu, const double* S, int64_t n_);
  int vgp_extend_q();
  int vgp_get_q(double* mu, double* S);
  int vgp_natural_update(const double* qmu, const double* qS, double gamma, double* mu_out, double* S_out);
  int vgp_natgrad(const Theta& th, double gamma);
  int vgp_elbo(const Theta& th, double* loss, double* grad);
  int vgp_shifted_root(double* delta_out, bool sigma_ready = false /* K already holds Sigma (the SGPR install: B^-1) */,
                       const double* qS = nullptr /* the root of Sigma when it is not the VGP's (the SVGP's q) */);
  int vgp_posterior(const Theta& th);
  int install_predictive(Post kind);
  int sgpr_need_f64() { return need_double_fit("SGPR needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context"); }
  int sgpr_stash();
  int sgpr_set_inducing(const double* Z, int64_t m);
  int sgpr_select_inducing(const Theta& th, int64_t m, int64_t* idx_out);
  int sgpr_get_inducing(double* Z, int64_t* m_out, int64_t* n_data_out);
  int sgpr_get_factor(int which, double* out);
  int sgpr_factor(const Theta& th, const char* who);
  int sgpr_bound_impl(const Theta& th, double* loss, double* grad, double* grad_z, const char* who);
  int sgpr_bound(const Theta& th, double* loss, double* grad) { return sgpr_bound_impl(th, loss, grad, nullptr, "gpso_sgpr_bound_u"); }
  int sgpr_posterior(const Theta& th, double* delta_out);
  int sparse_nsplit() const;
  int sparse_workspace(bool svgp);
  int svgp_need_z(const char* who);
  void svgp_prior();
  int svgp_q();
  int svgp_begin(const Theta& th, const char* who, bool rect);
  void svgp_pointwise(double variance, double p, double mean_c, bool want_v, bool gauss);
  void svgp_adat(double* aat, double* lam);
  int svgp_step(const Theta& th, double gamma, bool conj, const char* who);
  int svgp_natgrad(const Theta& th, double gamma) { return svgp_step(th, gamma, false, "gpso_svgp_natgrad"); }
  // s2 > 0: the conjugate start at that noise variance (th.lik is not read); else the prior (th is not read)
  int svgp_init_q(const Theta& th, double s2);
  int svgp_set_q(const double* mu, const double* S, int64_t m);
  int svgp_get_q(double* mu, double* S);
  int svgp_elbo_impl(const Theta& th, double* loss, double* grad, double* grad_z, const char* who);
  int svgp_elbo(const Theta& th, double* loss, double* grad) { return svgp_elbo_impl(th, loss, grad, nullptr, "gpso_svgp_elbo_u"); }
  int svgp_posterior(const Theta& th, double* delta_out);
  // ... and at a moving Z (inducing.hip): Z (nullable) replaces the resident inducing rows in place
  int inducing_buffers();
  int inducing_args(const char* who, const double* Z);
  int inducing_put(const double* Z);
  int sgpr_move_inducing(const double* Z);
  int sgpr_bound_z(const Theta& th, const double* Z, double* loss, double* grad, double* grad_z);
  int svgp_elbo_z(const Theta& th, const double* Z, double* loss, double* grad, double* grad_z);

  // ---- typed: overridden by EngineT<TF, TP> (api.hip).  First the hooks the calls above reach typed code through
  // (DESIGN.md 3.5 names the launch that forces each), then the entry points that stayed with their types ----
  virtual int pack_predictive(hipStream_t s) = 0;  // install_predictive: linv_p, alpha and the split pieces from linv / alpha_f
  virtual int score_device_leaves(const void* xs_dev, int xs_dtype, int64_t m, const AcqSpec& acq, bool want_ucb, double* mean_dev, double* var_dev, double* ucb_dev, TileSpan& span, const int64_t* m_live = nullptr, LeafFinalize* defer = nullptr, bool prepared = false) = 0;
  virtual int precision_gate() = 0;  // called at the top of every predict-type entry point
  // theta crosses this interface as one Theta (theta.hpp): lik is the noise variance, the likelihood's variance or its scale.
  // (gpso_fit_eval / gpso_fit_eval_loo: th is NULL when the caller passed no lengthscales -- refused where it always was)
  virtual int fit_eval(const Theta* th, double* nlml, double* grad) = 0;
  virtual int set_posterior(const double* X, const double* L, const double* alpha, int64_t n, int d, const Theta& th) = 0;
  // leave-one-out predictive of the resident fitted posterior / one evaluation of the LOO-CV objective (loo.hip)
  virtual int loo(double* mean, double* var, double* lpd, double* loss) = 0;
  virtual int fit_eval_loo(const Theta* th, double* loss, double* grad, double* nlml) = 0;
  virtual int fit_eval_batch(int kernel, const double* th, int nv, int n_ls, double* loss, double* grad, int* info) = 0;
  virtual int append(const double* Xnew, const double* ynew, const double* snew, int64_t k, double* nlml) = 0;
  virtual int predict(const void* xs, int xs_dtype, int xs_mem, int64_t m, double* mean, double* var, int out_mem) = 0;
  // mean, var and the acquisition column of every leaf (each output nullable)
  virtual int acq_values(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, double* mean, double* var, double* value, int out_mem) = 0;
  virtual int best_ucb(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, const AcqSpec& acq, int64_t* idx, double* mean, double* var, double* ucb) = 0;
  virtual int best_ucb_begin(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, const AcqSpec& acq, const double* bounds, int depth) = 0;
  virtual int best_ucb_end(int ticket, int64_t* idx, double* mean, double* var, double* ucb) = 0;
  virtual int screen_probe(const void* xs, int xs_dtype, int xs_mem, int64_t m, double varsigma, double* my, double* ub, double* flag, double* info) = 0;
  virtual int grow(const double* bounds, int nseg, int d, int depth, double* out) = 0;
  virtual int best_ucb_grow(const double* bounds, int nseg, int depth, const AcqSpec& acq, int64_t* idx, double* mean, double* var, double* ucb) = 0;
  virtual int get_matrix(int which, double* out) = 0;
  virtual int get_vector(int which, double* out) = 0;
  virtual int posterior_buffers(void** ptrs, int64_t* nbytes, int cap) = 0;
  virtual int posterior_span(void** ptr, int64_t* offset, int64_t* nbytes) = 0;
  virtual int posterior_hash(uint64_t* out) = 0;
  virtual int adopt_posterior() = 0;
  virtual int set_option(int option, int value) = 0;
  virtual int precision_info(double* out) = 0;
  virtual int broadcast_posterior(int root) = 0;
  virtual int broadcast_posterior_rows(int root) = 0;
  virtual int posterior_dirty_ranges(int64_t* offsets, int64_t* nbytes, int cap) = 0;
  virtual int posterior_mark_synced() = 0;
  virtual int best_ucb_sharded(const void* xs, int xs_dtype, int xs_mem, int64_t m_local, int64_t m_global, const int64_t* seg_off, int nseg, double varsigma, int64_t* idx, double* mean, double* var, double* ucb) = 0;
  virtual int best_ucb_grow_sharded(const double* bounds, int nseg, int depth, double varsigma, int64_t* idx, double* mean, double* var, double* ucb) = 0;
  // the two halves of the sharded calls for an arbitrary (rank, world), without a communicator
  virtual int shard_winners(int rank, int world, const void* xs, int xs_dtype, int xs_mem, int64_t m_local, int64_t m_global, const int64_t* seg_off, int nseg, double varsigma, double* payload) = 0;
  virtual int shard_winners_grow(int rank, int world, const double* bounds, int nseg, int depth, double varsigma, double* payload) = 0;
  virtual int fold_winners(const double* gathered, int world, int64_t m_global, const int64_t* seg_off, int nseg, int64_t* idx, double* mean, double* var, double* ucb) = 0;
};

}  // namespace gpso::host
