// EngineCore's calls that evaluate the resident posterior at points the caller gives and read the dense double factor for it
// (DESIGN.md sections 7h-7n: predict_grad, the joint predictive, pathwise draws, cross-covariance, batch selection), and the two
// untyped calls of max-value entropy search.  No typed buffer is touched here: a float fit is refused by need_double_fit.
#include <climits>
#include <cstddef>
#include <vector>

#include "engine_core.hpp"

namespace gpso::host {

// GPSO_ACQ_MES reads its maxima from this buffer (acq.hpp); no call of this context but the next set_maxima touches it
int EngineCore::set_maxima(const double* ystar, int k) {
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
int EngineCore::max_logcdf(const double* mean, const double* var, int mem, int64_t m, double var_sub, const double* y, int g, double* logcdf,
               int64_t* n_used) {
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

// ---- mean, var and their gradients in the test points (predict_grad.hip).  Reads the dense fit-type
// factor, alpha_f, xs64 and the hyper block and writes buffers of its own only: the posterior, its packed copies and the
// self-test's verdicts stay as they are.  M is worked off in chunks of kPredictGradChunk, so the workspace is a few
// N_pad x chunk doubles whatever M is
int EngineCore::predict_grad(const void* xs, int xs_dtype, int xs_mem, int64_t m, double* mean, double* var, double* dmean, double* dvar,
                 int out_mem) {
  if (int rcd = need_double_fit("gpso_predict_grad needs a GPSO_F64 or GPSO_MIXED context (the dense factor in double)")) return rcd;
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
int EngineCore::joint_enqueue(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, double* mean_dev,
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
int EngineCore::joint_check(const char* what, const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add) {
  if (m < 1 || m > kPredictGradChunk)
    return ctx->fail(GPSO_E_ARG, "%s takes 1 to %lld test points (m=%lld): the joint covariance of more is out of scope", what,
                     (long long)kPredictGradChunk, (long long)m);
  int rc = check_points(xs, xs_dtype, xs_mem, m);
  if (rc) return rc;
  if (!(diag_add == diag_add) || diag_add - diag_add != 0.0) return ctx->fail(GPSO_E_ARG, "diag_add must be finite");
  return need_dense_factor(what);
}

int EngineCore::predict_joint(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, double* mean, double* cov,
                  int out_mem) {
  if (int rcd = need_double_fit("gpso_predict_joint needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)")) return rcd;
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
int EngineCore::sample_joint(const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add, const double* z, int64_t ns,
                 double* samples, int64_t* best_idx, double* best_val) {
  if (int rcd = need_double_fit("gpso_sample_joint needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)")) return rcd;
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
// the draw of a variational posterior: v = beta + Lu^-T (Q eps - Lu^-1 Phi(Zr) w^T) from what the
// install left in Lf (Lu), alpha_f (beta) and vq_S / svq_S / sgM2 (Q); Lu^-1 is rebuilt from Lf into vA (vB: the copy of
// Lu with a unit diagonal on the padding, work: scratch) -- three buffers the install has finished with
int EngineCore::paths_draw_impl(bool variational, const char* who, const double* omega, const double* phase, int64_t f, const double* w,
                    const double* eps, int64_t ns) {
  if (int rcd = need_double_fit(" needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)", who)) return rcd;
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
int EngineCore::paths_eval(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, double* values, int out_mem,
               int64_t* best_idx, double* best_val) {
  if (int rcd = need_double_fit("gpso_paths_eval needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)")) return rcd;
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

// ---- latent cross-covariance and greedy batch selection (batch.hip).  Both calls read the dense
// fit-type factor, the scaled rows and the hyper block -- gpso_best_batch also whatever gpso_acq_values reads -- and write
// buffers of their own only: the posterior, its packed copies, the self-test's verdicts and a resident path set stay as they are
int EngineCore::cross_cov(const void* xa, int xs_dtype, int xs_mem, int64_t m, const double* xb, int b, double* cov, int out_mem) {
  if (int rcd = need_double_fit("gpso_cross_cov needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)")) return rcd;
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
int EngineCore::best_batch(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, double obs_noise, int q, int64_t* idx,
               double* mean, double* var, double* value, int* n_picked, double* var_after, int out_mem) {
  if (int rcd = need_double_fit("gpso_best_batch needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)")) return rcd;
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

// ---- Monte-Carlo batch acquisition over the path draws (mcbatch.hip).  Stage A is gpso_paths_eval's
// kernel over the call's own chunk buffers, writing the S x ld value matrix (candidates, then the pending points from column
// roundup(m, 64) on); then the q rounds back to back, the end rules decided on the device, one wait.  Reads the path set and
// what gpso_paths_eval reads; writes buffers of its own only
int EngineCore::paths_best_batch(const void* xs, int xs_dtype, int xs_mem, int64_t m, int kind, double xi, double incumbent,
                                 const double* incumbent_s, const double* pending, int b, int q, int64_t* idx, double* gain,
                                 double* batch_value, int* n_picked, double* gain0, int out_mem) {
  if (int rcd = need_double_fit("gpso_paths_best_batch needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)")) return rcd;
  ctx->tick_timing();
  if (m < 1) return ctx->fail(GPSO_E_ARG, "gpso_paths_best_batch needs at least one leaf (m=%lld)", (long long)m);
  if (q < 1 || q > kMcMaxPicks) return ctx->fail(GPSO_E_ARG, "gpso_paths_best_batch picks 1 to %d leaves (q=%d)", kMcMaxPicks, q);
  if (b < 0 || b > kMcMaxPending) return ctx->fail(GPSO_E_ARG, "gpso_paths_best_batch takes 0 to %d pending points (b=%d)", kMcMaxPending, b);
  if (b > 0 && !pending) return ctx->fail(GPSO_E_ARG, "pending must not be NULL with b=%d", b);
  if (!xs) return ctx->fail(GPSO_E_ARG, "xs must not be NULL");
  if (!idx || !n_picked) return ctx->fail(GPSO_E_ARG, "idx and n_picked must not be NULL");
  int rc = check_points(xs, xs_dtype, xs_mem, m);
  if (rc) return rc;
  if (out_mem != GPSO_MEM_HOST && out_mem != GPSO_MEM_DEVICE) return ctx->fail(GPSO_E_ARG, "bad out_mem %d", out_mem);
  if (!res.paths_valid)
    return ctx->fail(GPSO_E_STATE, "no path set resident for this posterior: call gpso_paths_draw (every fit, append, new data, noise vector, install and hand-off ends the set)");
  if ((rc = refuse_if_async("gpso_paths_best_batch"))) return rc;
  const int64_t ns = pth.s;
  if (const char* why = mc_refusal(kind, xi, incumbent, incumbent_s, ns)) return ctx->fail(GPSO_E_ARG, "gpso_paths_best_batch: %s", why);
  if (m + b > kMcMaxCells / ns)
    return ctx->fail(GPSO_E_ARG, "gpso_paths_best_batch: S * (m + b) above 2^26 (S=%lld, m=%lld, b=%d)", (long long)ns, (long long)m, b);
  const int64_t mall = (m + 63) / 64 * 64, chunk = std::min<int64_t>(kPathsChunk, mall), ldv = mall + (b > 0 ? 64 : 0);
  const int64_t nblk = mc_round_blocks(m);
  if ((rc = ensure(mc_ts, (size_t)chunk * dp * 8))) return rc;
  if ((rc = ensure(mc_norm, (size_t)chunk * 8))) return rc;
  if ((rc = ensure(mc_vals, (size_t)ns * ldv * 8))) return rc;
  if ((rc = ensure(mc_live, (size_t)m))) return rc;
  if ((rc = ensure(mc_bmax, (size_t)nblk * 16))) return rc;
  if ((rc = ensure(mc_state, sizeof(McState)))) return rc;
  if (b > 0 && (rc = ensure(mc_praw, (size_t)kMcMaxPending * d * 8))) return rc;
  const bool g0_host = gain0 && out_mem == GPSO_MEM_HOST;
  if (g0_host && (rc = ensure(mc_g0, (size_t)m * 8))) return rc;
  constexpr size_t kRecordBytes = offsetof(McState, bar);
  McState* host = reinterpret_cast<McState*>(ctx->pinned_scratch(sizeof(McState) / 8 + 1));
  if (!host) return ctx->fail(GPSO_E_OOM, "pinned host scratch");
  std::vector<double> bars((size_t)ns, incumbent);
  if (incumbent_s) std::memcpy(bars.data(), incumbent_s, (size_t)ns * 8);
  hipStream_t s;
  if ((rc = points_begin(&s))) return rc;
  const void* dev = nullptr;
  if ((rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
  McState* state = static_cast<McState*>(mc_state.p);
  HIPCHECK(hipMemsetAsync(state, 0, sizeof(McState), s));
  HIPCHECK(hipMemcpyAsync(state->bar, bars.data(), (size_t)ns * 8, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemsetAsync(mc_live.p, 1, (size_t)m, s));
  double* V = as<double>(mc_vals);
  PathsEvalLaunch g;
  g.ts = as<double>(mc_ts); g.xs = as<double>(xs64); g.omega = as<double>(pth.omega); g.phase = as<double>(pth.phase);
  g.W = as<double>(pth.w); g.VT = as<double>(pth.vt);
  g.n = n; g.npad = npad; g.s = ns; g.f = pth.f; g.ldw = pth.ldw; g.dp = dp; g.kp = kp; g.ldo = ldv;
  for (int64_t off = 0; off < m; off += chunk) {
    const int64_t mc = std::min(chunk, m - off), mpad = (mc + 63) / 64 * 64;
    prep_points<double>(s, dev, xs_dtype, off, mc, mpad, nullptr, as<double>(mc_ts), as<double>(mc_norm));
    g.m = mc;
    g.out = V + off;  // (columns off .. off + mpad: below mall, so inside the row)
    if (launch_paths_eval(s, g) != 0) return launch_status();
    if ((rc = launch_status())) return rc;
  }
  if (b > 0) {  // the pending points: b more columns by the same kernel, from column mall on
    HIPCHECK(hipMemcpyAsync(mc_praw.p, pending, (size_t)b * d * 8, hipMemcpyHostToDevice, s));
    prep_points<double>(s, mc_praw.p, GPSO_F64, 0, b, 64, nullptr, as<double>(mc_ts), as<double>(mc_norm));
    g.m = b;
    g.out = V + mall;
    if (launch_paths_eval(s, g) != 0) return launch_status();
  }
  if (ctx->timing) HIPCHECK(hipEventRecord(ctx->ev[0], s));  // (stage A ends here: gpso_last_ms(ctx, 0) is the rounds alone)
  McLaunch r;
  r.st = state; r.V = V; r.ld = ldv; r.m = m; r.pcol = mall; r.s = (int)ns; r.b = b; r.kind = kind; r.xi = xi;
  r.live = static_cast<unsigned char*>(mc_live.p);
  r.bmax_v = as<double>(mc_bmax);
  r.bmax_i = reinterpret_cast<int64_t*>(r.bmax_v + nblk);
  if (launch_mc_init(s, r) != 0) return launch_status();
  double* g0_dev = !gain0 ? nullptr : g0_host ? as<double>(mc_g0) : gain0;
  for (int t = 0; t < q; ++t) launch_mc_round(s, r, t, g0_dev);
  if ((rc = launch_status())) return rc;
  HIPCHECK(hipMemcpyAsync(host, state, kRecordBytes, hipMemcpyDeviceToHost, s));
  if (g0_host) HIPCHECK(hipMemcpyAsync(gain0, g0_dev, (size_t)m * 8, hipMemcpyDeviceToHost, s));
  if ((rc = points_end(s, m))) return rc;
  float rounds_ms = 0;
  if (ctx->timing && hipEventElapsedTime(&rounds_ms, ctx->ev[0], ctx->ev[3]) == hipSuccess) ctx->last_ms[0] = rounds_ms;
  *n_picked = host->n_picked;
  for (int t = 0; t < host->n_picked; ++t) {
    idx[t] = host->idx[t];
    if (gain) gain[t] = host->gain[t];
    if (batch_value) batch_value[t] = host->value[t];
  }
  return GPSO_OK;
}

// ---- the hyper-parameter ensemble (ensemble.hip).  A push copies what a point call reads of the
// resident posterior -- device to device, on the context's stream, nothing computed -- into slots that only the integrated
// calls read; those read nothing of the resident posterior, so a refit at another theta between them changes no bit of theirs.
// Every call here leaves the posterior, its packed copies, the hyper block, gpso_posterior_hash and a path set as they are
int EngineCore::ensemble_push() {
  if (int rcd = need_double_fit("gpso_ensemble_push needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double)")) return rcd;
  if (!res.has_post()) return ctx->fail(GPSO_E_STATE, "gpso_ensemble_push: no posterior resident: call gpso_fit_eval first");
  if (res.post != Post::Fitted || !res.chol_valid || !res.have_data)
    return ctx->fail(GPSO_E_STATE, "gpso_ensemble_push needs an exact-GP posterior fitted with targets on this context (gpso_set_data + gpso_fit_eval): "
                                   "a variational, installed or adopted posterior is no member of an ensemble");
  if (n > kEnsembleMaxN) return ctx->fail(GPSO_E_ARG, "gpso_ensemble_push: N=%lld above the ensemble's %d (gpso_ensemble_max = 0)", (long long)n, kEnsembleMaxN);
  int rc = refuse_if_async("gpso_ensemble_push");
  if (rc) return rc;
  const int k = ensemble_count();
  if (k >= kEnsembleMax) return ctx->fail(GPSO_E_STATE, "gpso_ensemble_push: the ensemble is full (%d members: GPSO_ENSEMBLE_MAX)", kEnsembleMax);
  if (k > 0 && (n != ens_n || d != ens_d || kp.kernel != ens_kernel))
    return ctx->fail(GPSO_E_STATE, "gpso_ensemble_push: the resident posterior (N=%lld, D=%d, kernel %d) disagrees with the ensemble's members "
                                   "(N=%lld, D=%d, kernel %d): gpso_ensemble_clear first", (long long)n, d, kp.kernel, (long long)ens_n, ens_d, ens_kernel);
  // (k == 0: the slots may be re-allocated for another D_pad, nothing in them is kept; k > 0: the shape is the same, nothing grows)
  const size_t b_xs = (size_t)npad * dp * 8, b_linv = (size_t)npad * npad * 8, b_alpha = (size_t)npad * 8, b_hyper = (size_t)kEnsHyperStride * 8;
  if ((rc = ensure(ens_hyper, kEnsembleMax * b_hyper))) return rc;
  if ((rc = ensure(ens_xs, kEnsembleMax * b_xs))) return rc;
  if ((rc = ensure(ens_linv, kEnsembleMax * b_linv))) return rc;
  if ((rc = ensure(ens_alpha, kEnsembleMax * b_alpha))) return rc;
  hipStream_t s = st();
  HIPCHECK(hipMemcpyAsync(static_cast<char*>(ens_hyper.p) + k * b_hyper, hyper.p, b_hyper, hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(static_cast<char*>(ens_xs.p) + k * b_xs, xs64.p, b_xs, hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(static_cast<char*>(ens_linv.p) + k * b_linv, linv.p, b_linv, hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(static_cast<char*>(ens_alpha.p) + k * b_alpha, alpha_f.p, b_alpha, hipMemcpyDeviceToDevice, s));
  if (k == 0) {
    ens_n = n; ens_d = d; ens_dp = dp; ens_kernel = kp.kernel;
    ens_theta.clear();
  }
  ens_theta.resize((size_t)(k + 1) * kEnsembleTheta);
  double* row = &ens_theta[(size_t)k * kEnsembleTheta];
  expand_ls(ls_host.data(), n_ls, row);
  row[kMaxD] = kp.variance; row[kMaxD + 1] = kp.noise; row[kMaxD + 2] = kp.mean_c;
  ens_k = k + 1;
  res.ensemble_pushed();
  return k;
}

int EngineCore::ensemble_clear() {
  int rc = refuse_if_async("gpso_ensemble_clear");
  if (rc) return rc;
  ens_k = 0;
  res.ensemble_cleared();
  return GPSO_OK;
}

int EngineCore::ensemble_info(int* k, double* theta) const {
  if (!k) return ctx->fail(GPSO_E_ARG, "k must not be NULL");
  *k = ensemble_count();
  if (theta && *k > 0) std::memcpy(theta, ens_theta.data(), (size_t)*k * kEnsembleTheta * 8);
  return GPSO_OK;
}

// what both integrated calls refuse, before anything is allocated or enqueued
int EngineCore::ensemble_refusals(const char* who, const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq) {
  if (int rcd = need_double_fit(" needs a GPSO_F64 or GPSO_MIXED context -- dtype=\"float64\" or \"mixed\" -- (the members' factors are double)", who)) return rcd;
  const int k = ensemble_count();
  if (k == 0)
    return ctx->fail(GPSO_E_STATE, "%s: no ensemble resident for this data: gpso_ensemble_push after a fit (new data, an append, a noise vector, "
                                   "an install and a hand-off end the ensemble)", who);
  if (acq.kind == GPSO_ACQ_MES) return ctx->fail(GPSO_E_ARG, "%s: GPSO_ACQ_MES is not integrated over an ensemble: its maxima belong to one theta", who);
  if (m < 1) return ctx->fail(GPSO_E_ARG, "%s needs at least one leaf (m=%lld)", who, (long long)m);
  if (m > ((int64_t)1 << 28) / k) return ctx->fail(GPSO_E_ARG, "%s: k * m above 2^28 (k=%d, m=%lld)", who, k, (long long)m);
  int rc = check_points(xs, xs_dtype, xs_mem, m);
  if (rc) return rc;
  return refuse_if_async(who);
}

// ... and what both enqueue behind their refusals: the workspaces, the members' columns (stage 1) and the fold (stage 2).  On
// return the stream is open (points_begin), ens_mean / ens_var hold [K][m] and ens_mix the three folded columns
int EngineCore::ensemble_enqueue(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, hipStream_t* s) {
  ctx->tick_timing();
  const int k = ensemble_count();
  int rc;
  if ((rc = ensure(ens_mean, (size_t)k * m * 8))) return rc;
  if ((rc = ensure(ens_var, (size_t)k * m * 8))) return rc;
  if ((rc = ensure(ens_mix, (size_t)3 * m * 8))) return rc;
  if ((rc = points_begin(s))) return rc;
  const void* dev = nullptr;
  if ((rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
  EnsembleMembersLaunch g;
  g.hyper = as<double>(ens_hyper); g.xs = as<double>(ens_xs); g.linv = as<double>(ens_linv); g.alpha = as<double>(ens_alpha);
  g.hyper_stride = kEnsHyperStride; g.leaves = dev; g.leaves_f64 = xs_dtype == GPSO_F64 ? 1 : 0; g.m = m; g.ld = m;
  g.n = (int)ens_n; g.npad = kPadN; g.d = ens_d; g.dp = ens_dp; g.kernel = ens_kernel; g.k = k;
  g.mean = as<double>(ens_mean); g.var = as<double>(ens_var);
  if (launch_ensemble_members(*s, g) != 0) return launch_status();
  double* mix = as<double>(ens_mix);
  launch_ensemble_fold(*s, acq, g.mean, g.var, g.hyper, kEnsHyperStride, k, m, m, mix, mix + m, mix + 2 * m);
  return launch_status();
}

int EngineCore::ensemble_acq_values(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, double* mean_mix, double* var_mix,
                                    double* value, double* member_mean, double* member_var, int out_mem) {
  int rc = ensemble_refusals("gpso_ensemble_acq_values", xs, xs_dtype, xs_mem, m, acq);
  if (rc) return rc;
  if (!mean_mix && !var_mix && !value && !member_mean && !member_var)
    return ctx->fail(GPSO_E_ARG, "gpso_ensemble_acq_values: every output is NULL");
  hipStream_t s;
  if ((rc = ensemble_enqueue(xs, xs_dtype, xs_mem, m, acq, &s))) return rc;
  const hipMemcpyKind kind = out_mem == GPSO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  const double* mix = as<double>(ens_mix);
  const size_t col = (size_t)m * 8, cols = (size_t)ensemble_count() * col;
  if (mean_mix) HIPCHECK(hipMemcpyAsync(mean_mix, mix, col, kind, s));
  if (var_mix) HIPCHECK(hipMemcpyAsync(var_mix, mix + m, col, kind, s));
  if (value) HIPCHECK(hipMemcpyAsync(value, mix + 2 * m, col, kind, s));
  if (member_mean) HIPCHECK(hipMemcpyAsync(member_mean, ens_mean.p, cols, kind, s));
  if (member_var) HIPCHECK(hipMemcpyAsync(member_var, ens_var.p, cols, kind, s));
  return points_end(s, m);
}

// the folded columns feed the arg-max gpso_best_acq's general route runs (launch_seg_argmax): its segments (checked_segments,
// that route's check), its first maximum, its NaN-wins rule.  One read-back of nseg records
int EngineCore::ensemble_best_acq(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, const AcqSpec& acq,
                                  int64_t* idx, double* mean_mix, double* var_mix, double* value) {
  int rc = ensemble_refusals("gpso_ensemble_best_acq", xs, xs_dtype, xs_mem, m, acq);
  if (rc) return rc;
  if (!idx) return ctx->fail(GPSO_E_ARG, "gpso_ensemble_best_acq: idx must not be NULL");
  if (nseg < 1 || nseg > 1024) return ctx->fail(GPSO_E_ARG, "gpso_ensemble_best_acq: nseg=%d outside [1, 1024]", nseg);
  std::vector<int64_t> so;
  if ((rc = checked_segments(m, seg_off, nseg, so, "M"))) return rc;
  const int nblk = argmax_blocks(m, nseg);
  if ((rc = ensure(ens_seg, (size_t)(nseg + 1) * 8))) return rc;
  if ((rc = ensure(ens_part, (size_t)nseg * kArgmaxBlocks * kArgmaxPartialBytes))) return rc;
  if ((rc = ensure(ens_out, (size_t)(nseg * 4 + 2) * 8))) return rc;
  hipStream_t s;
  if ((rc = ensemble_enqueue(xs, xs_dtype, xs_mem, m, acq, &s))) return rc;
  HIPCHECK(hipMemcpyAsync(ens_seg.p, so.data(), (size_t)(nseg + 1) * 8, hipMemcpyHostToDevice, s));
  const double* mix = as<double>(ens_mix);
  launch_seg_argmax(s, mix, mix + m, mix + 2 * m, as<int64_t>(ens_seg), nseg, nblk, ens_part.p, as<double>(ens_out));
  if ((rc = launch_status())) return rc;
  std::vector<double> rec((size_t)nseg * 4);
  HIPCHECK(hipMemcpyAsync(rec.data(), ens_out.p, rec.size() * 8, hipMemcpyDeviceToHost, s));
  if ((rc = points_end(s, m))) return rc;
  for (int i = 0; i < nseg; ++i) {
    if (mean_mix) mean_mix[i] = rec[(size_t)i * 4];
    if (var_mix) var_mix[i] = rec[(size_t)i * 4 + 1];
    if (value) value[i] = rec[(size_t)i * 4 + 2];
    int64_t w;
    std::memcpy(&w, &rec[(size_t)i * 4 + 3], 8);
    idx[i] = w;
  }
  return GPSO_OK;
}

// ---- outcome constraints (constraints.hip).  A push copies what a point call reads of the posterior
// resident on `src` -- this context or another on the same device -- into the next slot of THIS context's set: device to
// device, nothing computed.  The constrained calls read the objective from the context's own buffers (a K = 1 launch of the
// ensemble's stage 1: no copy, whatever was refitted) and the members from the set.  Every call here leaves both posteriors,
// their packed copies, the hyper blocks, gpso_posterior_hash, a path set and an ensemble as they are
namespace {
// the ensemble's rule (section 7q) on the context `e`, in the words of the call `who`; what: whose posterior is meant
int member_refusal(gpso_ctx* report, EngineCore& e, const char* who, const char* what) {
  if (e.fit_elem != 8)
    return report->fail(GPSO_E_ARG, "%s needs GPSO_F64 or GPSO_MIXED contexts -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double): %s is GPSO_F32", who, what);
  if (!e.res.has_post()) return report->fail(GPSO_E_STATE, "%s: no posterior resident on %s: call gpso_fit_eval first", who, what);
  if (e.res.post != Post::Fitted || !e.res.chol_valid || !e.res.have_data)
    return report->fail(GPSO_E_STATE, "%s needs an exact-GP posterior fitted with targets on %s (gpso_set_data + gpso_fit_eval): a variational, "
                                      "sparse, installed or adopted posterior is neither an objective nor a constraint model", who, what);
  if (e.n > kEnsembleMaxN) return report->fail(GPSO_E_ARG, "%s: N=%lld on %s above the constraint set's %d", who, (long long)e.n, what, kEnsembleMaxN);
  return GPSO_OK;
}
}  // namespace

int EngineCore::constraint_push(EngineCore& src, double threshold, int sense) {
  const char* who = "gpso_constraint_push";
  if (src.ctx->device != ctx->device)
    return ctx->fail(GPSO_E_ARG, "%s: src lives on device %d, ctx on device %d: a member is copied device to device on one device", who, src.ctx->device, ctx->device);
  if (fit_elem != 8) return ctx->fail(GPSO_E_ARG, "%s needs GPSO_F64 or GPSO_MIXED contexts -- dtype=\"float64\" or \"mixed\": ctx is GPSO_F32", who);
  if (sense != 1 && sense != -1) return ctx->fail(GPSO_E_ARG, "%s: sense=%d is neither +1 (feasible where c <= threshold) nor -1 (c >= threshold)", who, sense);
  if (!std::isfinite(threshold)) return ctx->fail(GPSO_E_ARG, "%s: the threshold must be finite", who);
  int rc = member_refusal(ctx, src, who, "src");
  if (rc) return rc;
  if ((rc = refuse_if_async(who))) return rc;
  if (src.ctx->slots_busy() != 0)
    return ctx->fail(GPSO_E_STATE, "%s while %d asynchronous best-UCB call(s) are open on src: gpso_best_ucb_end them first", who, src.ctx->slots_busy());
  const int k = constraint_count();
  if (k >= kConstraintsMax) return ctx->fail(GPSO_E_STATE, "%s: the set is full (%d members: GPSO_CONSTRAINTS_MAX)", who, kConstraintsMax);
  if (k > 0 && (src.n != con_n || src.d != con_d || src.kp.kernel != con_kernel))
    return ctx->fail(GPSO_E_STATE, "%s: the posterior on src (N=%lld, D=%d, kernel %d) disagrees with the set's members (N=%lld, D=%d, kernel %d): "
                                   "gpso_constraint_clear first", who, (long long)src.n, src.d, src.kp.kernel, (long long)con_n, con_d, con_kernel);
  // (k == 0: the slots may be re-allocated for another D_pad, nothing in them is kept; k > 0: the shape is the same, nothing grows)
  const size_t b_xs = (size_t)src.npad * src.dp * 8, b_linv = (size_t)src.npad * src.npad * 8, b_alpha = (size_t)src.npad * 8,
               b_hyper = (size_t)kEnsHyperStride * 8;
  if ((rc = ensure(con_hyper, kConstraintsMax * b_hyper))) return rc;
  if ((rc = ensure(con_xs, kConstraintsMax * b_xs))) return rc;
  if ((rc = ensure(con_linv, kConstraintsMax * b_linv))) return rc;
  if ((rc = ensure(con_alpha, kConstraintsMax * b_alpha))) return rc;
  hipStream_t s = st();
  const bool other = src.st() != s;
  if (other) HIPCHECK(hipStreamSynchronize(src.st()));  // what src's fit enqueued is in its buffers
  HIPCHECK(hipMemcpyAsync(static_cast<char*>(con_hyper.p) + k * b_hyper, src.hyper.p, b_hyper, hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(static_cast<char*>(con_xs.p) + k * b_xs, src.xs64.p, b_xs, hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(static_cast<char*>(con_linv.p) + k * b_linv, src.linv.p, b_linv, hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(static_cast<char*>(con_alpha.p) + k * b_alpha, src.alpha_f.p, b_alpha, hipMemcpyDeviceToDevice, s));
  if (other) HIPCHECK(hipStreamSynchronize(s));  // (src may be refitted the moment this returns: the copies have left it)
  if (k == 0) {
    con_n = src.n; con_d = src.d; con_dp = src.dp; con_kernel = src.kp.kernel;
    con_theta.clear();
  }
  con_theta.resize((size_t)(k + 1) * kEnsembleTheta);
  double* row = &con_theta[(size_t)k * kEnsembleTheta];
  expand_ls(src.ls_host.data(), src.n_ls, row);
  row[kMaxD] = src.kp.variance; row[kMaxD + 1] = src.kp.noise; row[kMaxD + 2] = src.kp.mean_c;
  con_thr[k] = threshold;
  con_sense[k] = (double)sense;
  con_k = k + 1;
  res.constraint_pushed();
  return k;
}

int EngineCore::constraint_clear() {
  int rc = refuse_if_async("gpso_constraint_clear");
  if (rc) return rc;
  con_k = 0;
  res.constraints_cleared();
  return GPSO_OK;
}

int EngineCore::constraint_info(int* k, double* theta, double* threshold, int* sense) const {
  if (!k) return ctx->fail(GPSO_E_ARG, "k must not be NULL");
  *k = constraint_count();
  if (theta && *k > 0) std::memcpy(theta, con_theta.data(), (size_t)*k * kEnsembleTheta * 8);
  for (int i = 0; i < *k; ++i) {
    if (threshold) threshold[i] = con_thr[i];
    if (sense) sense[i] = (int)con_sense[i];
  }
  return GPSO_OK;
}

// what both constrained calls refuse, before anything is allocated or enqueued
int EngineCore::constrained_refusals(const char* who, const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, const ConSpec& con) {
  if (acq.kind == GPSO_ACQ_MES) return ctx->fail(GPSO_E_ARG, "%s: GPSO_ACQ_MES is not served under constraints", who);
  if (con.mode != GPSO_CON_WEIGHT && con.mode != GPSO_CON_GATE && con.mode != GPSO_CON_FEASIBILITY)
    return ctx->fail(GPSO_E_ARG, "%s: cspec.mode=%d is none of GPSO_CON_WEIGHT, GPSO_CON_GATE, GPSO_CON_FEASIBILITY", who, con.mode);
  if (con.log_pof_min != con.log_pof_min || con.log_pof_min > 0.0)
    return ctx->fail(GPSO_E_ARG, "%s: cspec.log_pof_min must be a log-probability (<= 0; -inf: no gate)", who);
  if (con.mode == GPSO_CON_WEIGHT && (acq.kind == GPSO_ACQ_UCB_VAR || acq.kind == GPSO_ACQ_UCB_STD))
    return ctx->fail(GPSO_E_ARG, "%s: a UCB kind is signed and cannot be weighted by a probability: use GPSO_CON_GATE, or EI / log-EI / PI", who);
  int rc = member_refusal(ctx, *this, who, "ctx (the objective)");
  if (rc) return rc;
  const int k = constraint_count();
  const bool suc = success_present();
  if (k == 0 && !suc) return ctx->fail(GPSO_E_STATE, "%s: no constraint set on this context: gpso_constraint_push first (gpso_alloc_posterior ends a set)", who);
  if (ensemble_count() > 0)
    return ctx->fail(GPSO_E_STATE, "%s: a hyper-parameter ensemble is resident on this context: constraints are not integrated over it "
                                   "(gpso_ensemble_clear first)", who);
  if (suc && d != suc_d)
    return ctx->fail(GPSO_E_STATE, "%s: the objective has D=%d, the success member D=%d: the member is stale, gpso_success_clear and push "
                                   "a classifier of these inputs", who, d, suc_d);
  if (k > 0 && (n != con_n || d != con_d || kp.kernel != con_kernel))
    return ctx->fail(GPSO_E_STATE, "%s: the objective (N=%lld, D=%d, kernel %d) no longer has the shape of the set's members (N=%lld, D=%d, "
                                   "kernel %d): the set is stale, gpso_constraint_clear and push models of the new rows",
                     who, (long long)n, d, kp.kernel, (long long)con_n, con_d, con_kernel);
  if (m < 1) return ctx->fail(GPSO_E_ARG, "%s needs at least one leaf (m=%lld)", who, (long long)m);
  if (m > ((int64_t)1 << 28) / (k + 1 + (suc ? 1 : 0))) return ctx->fail(GPSO_E_ARG, "%s: (J + 1) * m above 2^28 (J=%d, m=%lld)", who, k, (long long)m);
  if ((rc = check_points(xs, xs_dtype, xs_mem, m))) return rc;
  return refuse_if_async(who);
}

// ... and what both enqueue behind their refusals, in two stages.  The column stage (constrained_columns): the workspaces and
// stage 1 -- one launch for the objective on the context's own buffers, one for the J members; with a success member (section
// 7s) one more K = 1 launch, with the member's own n and kernel, writes row 1 + J.  On return the stream is open
// (points_begin) and con_mean / con_var hold [1 + J (+ 1)][m] with the objective in row 0; con_val [2][m] is allocated.  The
// EHVI calls (section 7t) run the same stage and fold the columns differently
int EngineCore::constrained_columns(const void* xs, int xs_dtype, int xs_mem, int64_t m, hipStream_t* s) {
  ctx->tick_timing();
  const int k = constraint_count();
  const bool suc = success_present();
  const size_t rows = (size_t)k + 1 + (suc ? 1 : 0);
  int rc;
  if ((rc = ensure(con_mean, rows * m * 8))) return rc;
  if ((rc = ensure(con_var, rows * m * 8))) return rc;
  if ((rc = ensure(con_val, (size_t)2 * m * 8))) return rc;
  if ((rc = points_begin(s))) return rc;
  const void* dev = nullptr;
  if ((rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
  EnsembleMembersLaunch g;
  g.hyper = as<double>(hyper); g.xs = as<double>(xs64); g.linv = as<double>(linv); g.alpha = as<double>(alpha_f);
  g.hyper_stride = kEnsHyperStride; g.leaves = dev; g.leaves_f64 = xs_dtype == GPSO_F64 ? 1 : 0; g.m = m; g.ld = m;
  g.n = (int)n; g.npad = kPadN; g.d = d; g.dp = dp; g.kernel = kp.kernel; g.k = 1;
  g.mean = as<double>(con_mean); g.var = as<double>(con_var);
  if (launch_ensemble_members(*s, g) != 0) return launch_status();
  EnsembleMembersLaunch c = g;
  c.hyper = as<double>(con_hyper); c.xs = as<double>(con_xs); c.linv = as<double>(con_linv); c.alpha = as<double>(con_alpha);
  c.n = (int)con_n; c.d = con_d; c.dp = con_dp; c.kernel = con_kernel; c.k = k;
  c.mean = g.mean + m; c.var = g.var + m;
  if (k > 0 && launch_ensemble_members(*s, c) != 0) return launch_status();
  EnsembleMembersLaunch u = g;
  if (suc) {
    u.hyper = as<double>(suc_hyper); u.xs = as<double>(suc_xs); u.linv = as<double>(suc_linv); u.alpha = as<double>(suc_alpha);
    u.n = (int)suc_n; u.d = suc_d; u.dp = suc_dp; u.kernel = suc_kernel; u.k = 1;
    u.mean = g.mean + (int64_t)(k + 1) * m; u.var = g.var + (int64_t)(k + 1) * m;
    if (launch_ensemble_members(*s, u) != 0) return launch_status();
  }
  return launch_status();
}

// ... and the fold (stage 2) over those columns: con_val holds value [m] then logpof [m]; the fold reads the success member's
// row last
int EngineCore::constrained_enqueue(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, const ConSpec& con, hipStream_t* s) {
  int rc = constrained_columns(xs, xs_dtype, xs_mem, m, s);
  if (rc) return rc;
  const int k = constraint_count();
  double *cm = as<double>(con_mean), *cv = as<double>(con_var);
  ConFoldLaunch f;
  f.acq = acq; f.con = con;
  f.obj_mean = cm; f.obj_var = cv; f.obj_hyper = as<double>(hyper);
  f.cmean = cm + m; f.cvar = cv + m; f.chyper = as<double>(con_hyper); f.hyper_stride = kEnsHyperStride;
  for (int i = 0; i < k; ++i) { f.thr[i] = con_thr[i]; f.sense[i] = con_sense[i]; }
  f.nj = k; f.ld = m; f.m = m;
  if (success_present()) { f.smean = cm + (int64_t)(k + 1) * m; f.svar = cv + (int64_t)(k + 1) * m; }
  f.value = as<double>(con_val); f.logpof = f.value + m;
  launch_constrained_fold(*s, f);
  return launch_status();
}

int EngineCore::constrained_acq_values(const void* xs, int xs_dtype, int xs_mem, int64_t m, const AcqSpec& acq, const ConSpec& con, double* mean,
                                       double* var, double* value, double* logpof, double* member_mean, double* member_var, int out_mem) {
  int rc = constrained_refusals("gpso_constrained_acq_values", xs, xs_dtype, xs_mem, m, acq, con);
  if (rc) return rc;
  if (!mean && !var && !value && !logpof && !member_mean && !member_var)
    return ctx->fail(GPSO_E_ARG, "gpso_constrained_acq_values: every output is NULL");
  hipStream_t s;
  if ((rc = constrained_enqueue(xs, xs_dtype, xs_mem, m, acq, con, &s))) return rc;
  const hipMemcpyKind kind = out_mem == GPSO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  const double *cm = as<double>(con_mean), *cv = as<double>(con_var), *val = as<double>(con_val);
  // (the member columns: the J constraints', then the success member's where one is resident)
  const size_t col = (size_t)m * 8, cols = ((size_t)constraint_count() + (success_present() ? 1 : 0)) * col;
  if (mean) HIPCHECK(hipMemcpyAsync(mean, cm, col, kind, s));
  if (var) HIPCHECK(hipMemcpyAsync(var, cv, col, kind, s));
  if (value) HIPCHECK(hipMemcpyAsync(value, val, col, kind, s));
  if (logpof) HIPCHECK(hipMemcpyAsync(logpof, val + m, col, kind, s));
  if (member_mean) HIPCHECK(hipMemcpyAsync(member_mean, cm + m, cols, kind, s));
  if (member_var) HIPCHECK(hipMemcpyAsync(member_var, cv + m, cols, kind, s));
  return points_end(s, m);
}

// the objective's columns and the folded value feed the arg-max gpso_best_acq's general route runs (launch_seg_argmax): its
// segments (checked_segments, that route's check), its first maximum, its NaN-wins rule; a gather picks the winners' logpof.
// One read-back of nseg records and nseg doubles
int EngineCore::constrained_best_acq(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, const AcqSpec& acq,
                                     const ConSpec& con, int64_t* idx, double* mean, double* var, double* value, double* logpof) {
  int rc = constrained_refusals("gpso_constrained_best_acq", xs, xs_dtype, xs_mem, m, acq, con);
  if (rc) return rc;
  if (!idx) return ctx->fail(GPSO_E_ARG, "gpso_constrained_best_acq: idx must not be NULL");
  if (nseg < 1 || nseg > 1024) return ctx->fail(GPSO_E_ARG, "gpso_constrained_best_acq: nseg=%d outside [1, 1024]", nseg);
  std::vector<int64_t> so;
  if ((rc = checked_segments(m, seg_off, nseg, so, "M"))) return rc;
  const int nblk = argmax_blocks(m, nseg);
  if ((rc = ensure(con_seg, (size_t)(nseg + 1) * 8))) return rc;
  if ((rc = ensure(con_part, (size_t)nseg * kArgmaxBlocks * kArgmaxPartialBytes))) return rc;
  if ((rc = ensure(con_out, (size_t)(nseg * 4 + 2) * 8))) return rc;
  if ((rc = ensure(con_win, (size_t)nseg * 8))) return rc;
  hipStream_t s;
  if ((rc = constrained_enqueue(xs, xs_dtype, xs_mem, m, acq, con, &s))) return rc;
  HIPCHECK(hipMemcpyAsync(con_seg.p, so.data(), (size_t)(nseg + 1) * 8, hipMemcpyHostToDevice, s));
  const double* val = as<double>(con_val);
  launch_seg_argmax(s, as<double>(con_mean), as<double>(con_var), val, as<int64_t>(con_seg), nseg, nblk, con_part.p, as<double>(con_out));
  launch_constrained_gather(s, val + m, as<int64_t>(con_seg), as<double>(con_out), nseg, as<double>(con_win));
  if ((rc = launch_status())) return rc;
  std::vector<double> rec((size_t)nseg * 5);
  HIPCHECK(hipMemcpyAsync(rec.data(), con_out.p, (size_t)nseg * 4 * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(rec.data() + (size_t)nseg * 4, con_win.p, (size_t)nseg * 8, hipMemcpyDeviceToHost, s));
  if ((rc = points_end(s, m))) return rc;
  for (int i = 0; i < nseg; ++i) {
    if (mean) mean[i] = rec[(size_t)i * 4];
    if (var) var[i] = rec[(size_t)i * 4 + 1];
    if (value) value[i] = rec[(size_t)i * 4 + 2];
    if (logpof) logpof[i] = rec[(size_t)nseg * 4 + i];
    int64_t w;
    std::memcpy(&w, &rec[(size_t)i * 4 + 3], 8);
    idx[i] = w;
  }
  return GPSO_OK;
}

// ---- bi-objective search (ehvi.hpp, ehvi.hip).  What both EHVI calls refuse, before anything is
// allocated or enqueued: the constrained calls' state rules (in those calls' words, under this call's name), then a set that
// holds no constraint model at all, then objective 2's index.  The record itself -- the front, the reference point, cspec --
// was checked by the C-ABI entry
int EngineCore::ehvi_refusals(const char* who, const void* xs, int xs_dtype, int xs_mem, int64_t m, const EhviSpec& e) {
  int rc = constrained_refusals(who, xs, xs_dtype, xs_mem, m, AcqSpec(GPSO_ACQ_EI, e.latent, 0.0, 0.0, 0.0), e.has_con ? e.con : ConSpec());
  if (rc) return rc;
  const int k = constraint_count();
  if (k == 0)
    return ctx->fail(GPSO_E_STATE, "%s: no constraint set on this context: objective 2 is a member of the set (gpso_constraint_push its model "
                                   "first; a success member alone is no objective)", who);
  if (e.member < 0 || e.member >= k) return ctx->fail(GPSO_E_ARG, "%s: member=%d outside [0, %d): objective 2 is a member of the set", who, e.member, k);
  return GPSO_OK;
}

// the constrained calls' column stage, then the EHVI fold: con_val holds value [m] then logpof [m]
int EngineCore::ehvi_enqueue(const void* xs, int xs_dtype, int xs_mem, int64_t m, const EhviSpec& e, hipStream_t* s) {
  int rc = constrained_columns(xs, xs_dtype, xs_mem, m, s);
  if (rc) return rc;
  const int k = constraint_count();
  double *cm = as<double>(con_mean), *cv = as<double>(con_var);
  EhviFoldLaunch f;
  std::memcpy(f.xa, e.xa, sizeof(f.xa));
  std::memcpy(f.xh, e.xh, sizeof(f.xh));
  f.p = e.p; f.latent = e.latent; f.has_con = e.has_con ? 1 : 0; f.con = e.con;
  f.obj_mean = cm; f.obj_var = cv; f.obj_hyper = as<double>(hyper);
  f.cmean = cm + m; f.cvar = cv + m; f.chyper = as<double>(con_hyper); f.hyper_stride = kEnsHyperStride;
  f.member = e.member;
  for (int i = 0; i < k; ++i) {
    if (i == e.member) continue;
    f.oidx[f.nother] = i; f.othr[f.nother] = con_thr[i]; f.osense[f.nother] = con_sense[i];
    ++f.nother;
  }
  if (success_present()) { f.smean = cm + (int64_t)(k + 1) * m; f.svar = cv + (int64_t)(k + 1) * m; }
  f.ld = m; f.m = m;
  f.value = as<double>(con_val); f.logpof = f.value + m;
  launch_ehvi_fold(*s, f);
  return launch_status();
}

int EngineCore::ehvi_values(const void* xs, int xs_dtype, int xs_mem, int64_t m, const EhviSpec& e, double* value, double* logpof, double* mean,
                            double* var, int out_mem) {
  int rc = ehvi_refusals("gpso_ehvi_values", xs, xs_dtype, xs_mem, m, e);
  if (rc) return rc;
  if (!value && !logpof && !mean && !var) return ctx->fail(GPSO_E_ARG, "gpso_ehvi_values: every output is NULL");
  hipStream_t s;
  if ((rc = ehvi_enqueue(xs, xs_dtype, xs_mem, m, e, &s))) return rc;
  const hipMemcpyKind kind = out_mem == GPSO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  const double *cm = as<double>(con_mean), *cv = as<double>(con_var), *val = as<double>(con_val);
  const size_t col = (size_t)m * 8;
  const int64_t row2 = (int64_t)(1 + e.member) * m;  // objective 2's row of the columns
  if (value) HIPCHECK(hipMemcpyAsync(value, val, col, kind, s));
  if (logpof) HIPCHECK(hipMemcpyAsync(logpof, val + m, col, kind, s));
  if (mean) {
    HIPCHECK(hipMemcpyAsync(mean, cm, col, kind, s));
    HIPCHECK(hipMemcpyAsync(mean + m, cm + row2, col, kind, s));
  }
  if (var) {
    HIPCHECK(hipMemcpyAsync(var, cv, col, kind, s));
    HIPCHECK(hipMemcpyAsync(var + m, cv + row2, col, kind, s));
  }
  return points_end(s, m);
}

// the arg-max of the constrained calls (launch_seg_argmax: its segments, its first maximum, its NaN-wins rule) over the EHVI
// fold's value; the gather runs once per extra winner column -- objective 2's mean and variance, logpof
int EngineCore::best_ehvi(const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg, const EhviSpec& e, int64_t* idx,
                          double* value, double* logpof, double* mean, double* var) {
  int rc = ehvi_refusals("gpso_best_ehvi", xs, xs_dtype, xs_mem, m, e);
  if (rc) return rc;
  if (!idx) return ctx->fail(GPSO_E_ARG, "gpso_best_ehvi: idx must not be NULL");
  if (nseg < 1 || nseg > 1024) return ctx->fail(GPSO_E_ARG, "gpso_best_ehvi: nseg=%d outside [1, 1024]", nseg);
  std::vector<int64_t> so;
  if ((rc = checked_segments(m, seg_off, nseg, so, "M"))) return rc;
  const int nblk = argmax_blocks(m, nseg);
  if ((rc = ensure(con_seg, (size_t)(nseg + 1) * 8))) return rc;
  if ((rc = ensure(con_part, (size_t)nseg * kArgmaxBlocks * kArgmaxPartialBytes))) return rc;
  if ((rc = ensure(con_out, (size_t)(nseg * 4 + 2) * 8))) return rc;
  if ((rc = ensure(con_win, (size_t)3 * nseg * 8))) return rc;
  hipStream_t s;
  if ((rc = ehvi_enqueue(xs, xs_dtype, xs_mem, m, e, &s))) return rc;
  HIPCHECK(hipMemcpyAsync(con_seg.p, so.data(), (size_t)(nseg + 1) * 8, hipMemcpyHostToDevice, s));
  const double *cm = as<double>(con_mean), *cv = as<double>(con_var), *val = as<double>(con_val);
  const int64_t row2 = (int64_t)(1 + e.member) * m;
  double* win = as<double>(con_win);
  launch_seg_argmax(s, cm, cv, val, as<int64_t>(con_seg), nseg, nblk, con_part.p, as<double>(con_out));
  launch_constrained_gather(s, cm + row2, as<int64_t>(con_seg), as<double>(con_out), nseg, win);
  launch_constrained_gather(s, cv + row2, as<int64_t>(con_seg), as<double>(con_out), nseg, win + nseg);
  launch_constrained_gather(s, val + m, as<int64_t>(con_seg), as<double>(con_out), nseg, win + 2 * nseg);
  if ((rc = launch_status())) return rc;
  std::vector<double> rec((size_t)nseg * 7);
  HIPCHECK(hipMemcpyAsync(rec.data(), con_out.p, (size_t)nseg * 4 * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(rec.data() + (size_t)nseg * 4, con_win.p, (size_t)nseg * 3 * 8, hipMemcpyDeviceToHost, s));
  if ((rc = points_end(s, m))) return rc;
  const double* w3 = rec.data() + (size_t)nseg * 4;
  for (int i = 0; i < nseg; ++i) {
    if (mean) { mean[i] = rec[(size_t)i * 4]; mean[nseg + i] = w3[i]; }
    if (var) { var[i] = rec[(size_t)i * 4 + 1]; var[nseg + i] = w3[nseg + i]; }
    if (value) value[i] = rec[(size_t)i * 4 + 2];
    if (logpof) logpof[i] = w3[2 * nseg + i];
    int64_t w;
    std::memcpy(&w, &rec[(size_t)i * 4 + 3], 8);
    idx[i] = w;
  }
  return GPSO_OK;
}

// ---- failed evaluations: the success probability and the success member (success.hpp) -----------------
namespace {
// a Bernoulli-installed classifier posterior within the ensemble's rule (section 7q) on `e`, in the words of the call `who`
int bernoulli_refusal(gpso_ctx* report, EngineCore& e, const char* who, const char* what) {
  if (e.fit_elem != 8)
    return report->fail(GPSO_E_ARG, "%s needs GPSO_F64 or GPSO_MIXED contexts -- dtype=\"float64\" or \"mixed\" -- (the dense factor in double): %s is GPSO_F32", who, what);
  if (!e.res.has_post()) return report->fail(GPSO_E_STATE, "%s: no posterior resident on %s: call gpso_vgp_posterior under GPSO_LIK_BERNOULLI first", who, what);
  if (e.res.post != Post::Vgp || !e.res.bernoulli || !e.res.chol_valid)
    return report->fail(GPSO_E_STATE, "%s needs a variational GP installed under GPSO_LIK_BERNOULLI on %s (gpso_vgp_set_likelihood + gpso_vgp_posterior): "
                                      "any other posterior has no success probability", who, what);
  if (e.n > kEnsembleMaxN) return report->fail(GPSO_E_ARG, "%s: N=%lld on %s above %d", who, (long long)e.n, what, kEnsembleMaxN);
  return GPSO_OK;
}
}  // namespace

// P(success) at m points of the Bernoulli install resident here: stage 1 of the ensemble with K = 1 on the context's own
// buffers (the LATENT mean and variance: the install's noise slot is 0), then one thread per point of success.hpp's map
int EngineCore::predict_prob(const void* xs, int xs_dtype, int xs_mem, int64_t m, double* prob, double* logprob, double* mean, double* var,
                             int out_mem) {
  const char* who = "gpso_predict_prob";
  int rc = bernoulli_refusal(ctx, *this, who, "ctx");
  if (rc) return rc;
  if (!prob && !logprob && !mean && !var) return ctx->fail(GPSO_E_ARG, "%s: every output is NULL", who);
  if (m < 1) return ctx->fail(GPSO_E_ARG, "%s needs at least one point (m=%lld)", who, (long long)m);
  if (m > ((int64_t)1 << 28)) return ctx->fail(GPSO_E_ARG, "%s: m above 2^28 (m=%lld)", who, (long long)m);
  if ((rc = check_points(xs, xs_dtype, xs_mem, m))) return rc;
  if ((rc = refuse_if_async(who))) return rc;
  ctx->tick_timing();
  if ((rc = ensure(suc_mean, (size_t)m * 8))) return rc;
  if ((rc = ensure(suc_var, (size_t)m * 8))) return rc;
  if ((rc = ensure(suc_val, (size_t)2 * m * 8))) return rc;
  hipStream_t s;
  if ((rc = points_begin(&s))) return rc;
  const void* dev = nullptr;
  if ((rc = stage_leaves(xs, xs_dtype, xs_mem, m, &dev))) return rc;
  EnsembleMembersLaunch g;
  g.hyper = as<double>(hyper); g.xs = as<double>(xs64); g.linv = as<double>(linv); g.alpha = as<double>(alpha_f);
  g.hyper_stride = kEnsHyperStride; g.leaves = dev; g.leaves_f64 = xs_dtype == GPSO_F64 ? 1 : 0; g.m = m; g.ld = m;
  g.n = (int)n; g.npad = kPadN; g.d = d; g.dp = dp; g.kernel = kp.kernel; g.k = 1;
  g.mean = as<double>(suc_mean); g.var = as<double>(suc_var);
  if (launch_ensemble_members(s, g) != 0) return launch_status();
  double* val = as<double>(suc_val);
  launch_success_map(s, g.mean, g.var, m, val, val + m);
  if ((rc = launch_status())) return rc;
  const hipMemcpyKind kind = out_mem == GPSO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  const size_t col = (size_t)m * 8;
  if (logprob) HIPCHECK(hipMemcpyAsync(logprob, val, col, kind, s));
  if (prob) HIPCHECK(hipMemcpyAsync(prob, val + m, col, kind, s));
  if (mean) HIPCHECK(hipMemcpyAsync(mean, g.mean, col, kind, s));
  if (var) HIPCHECK(hipMemcpyAsync(var, g.var, col, kind, s));
  return points_end(s, m);
}

// the four copies gpso_constraint_push makes, into the one slot of the success member: device to device, nothing computed
int EngineCore::success_push(EngineCore& src) {
  const char* who = "gpso_success_push";
  if (src.ctx->device != ctx->device)
    return ctx->fail(GPSO_E_ARG, "%s: src lives on device %d, ctx on device %d: a member is copied device to device on one device", who, src.ctx->device, ctx->device);
  if (fit_elem != 8) return ctx->fail(GPSO_E_ARG, "%s needs GPSO_F64 or GPSO_MIXED contexts -- dtype=\"float64\" or \"mixed\": ctx is GPSO_F32", who);
  int rc = bernoulli_refusal(ctx, src, who, "src");
  if (rc) return rc;
  if (res.have_data && src.d != d)
    return ctx->fail(GPSO_E_ARG, "%s: the classifier on src has D=%d, the data on ctx D=%d", who, src.d, d);
  if ((rc = refuse_if_async(who))) return rc;
  if (src.ctx->slots_busy() != 0)
    return ctx->fail(GPSO_E_STATE, "%s while %d asynchronous best-UCB call(s) are open on src: gpso_best_ucb_end them first", who, src.ctx->slots_busy());
  const size_t b_xs = (size_t)src.npad * src.dp * 8, b_linv = (size_t)src.npad * src.npad * 8, b_alpha = (size_t)src.npad * 8,
               b_hyper = (size_t)kEnsHyperStride * 8;
  if ((rc = ensure(suc_hyper, b_hyper))) return rc;
  if ((rc = ensure(suc_xs, b_xs))) return rc;
  if ((rc = ensure(suc_linv, b_linv))) return rc;
  if ((rc = ensure(suc_alpha, b_alpha))) return rc;
  hipStream_t s = st();
  const bool other = src.st() != s;
  if (other) HIPCHECK(hipStreamSynchronize(src.st()));  // what src's install enqueued is in its buffers
  HIPCHECK(hipMemcpyAsync(suc_hyper.p, src.hyper.p, b_hyper, hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(suc_xs.p, src.xs64.p, b_xs, hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(suc_linv.p, src.linv.p, b_linv, hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(suc_alpha.p, src.alpha_f.p, b_alpha, hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipStreamSynchronize(s));  // (src may be retrained the moment this returns: the copies have left it)
  suc_n = src.n; suc_d = src.d; suc_dp = src.dp; suc_kernel = src.kp.kernel;
  expand_ls(src.ls_host.data(), src.n_ls, suc_theta);
  suc_theta[kMaxD] = src.kp.variance; suc_theta[kMaxD + 1] = src.kp.noise; suc_theta[kMaxD + 2] = src.kp.mean_c;
  res.success_pushed();
  return GPSO_OK;
}

int EngineCore::success_clear() {
  int rc = refuse_if_async("gpso_success_clear");
  if (rc) return rc;
  res.success_cleared();
  return GPSO_OK;
}

int EngineCore::success_info(int* present, int64_t* n_out, double* theta) const {
  if (!present) return ctx->fail(GPSO_E_ARG, "present must not be NULL");
  *present = success_present() ? 1 : 0;
  if (n_out) *n_out = *present ? suc_n : 0;
  if (theta && *present) std::memcpy(theta, suc_theta, sizeof(suc_theta));
  return GPSO_OK;
}

}  // namespace gpso::host
