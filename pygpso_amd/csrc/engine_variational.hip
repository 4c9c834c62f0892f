// EngineCore's variational and sparse families: VGP, SGPR, SVGP and the sparse models at a moving Z (DESIGN.md sections 7a-7d).
// Every buffer is read as double; a float fit is refused by need_double_fit.  The one typed step, the predict-ready copies of
// an installed predictive, is EngineT's pack_predictive.
#include <climits>
#include <vector>

#include "engine_core.hpp"

namespace gpso::host {

// ---- variational GP (GPflow 2 VGP, whitened, Gaussian likelihood) ----------------------------
// q(v) = N(mu, S S^T) lives here beside the training data: vq_mu [N_pad], vq_S [N_pad^2] (lower; identity on the padding).
// Every product is a whole-matrix float64 GEMM (launch_dgemm), every factorisation the fit's launch_potrf; the calls leave
// the fit's buffers (K, Lf, linv, work) holding VGP intermediates, so they invalidate any GPR posterior first.
constexpr double kVgpJitter = 1.0e-6;  // GPflow's default_jitter, in the K of the ELBO and of the predictive
enum { kVgpR = 0, kVgpFvar = 1, kVgpSrow = 2, kVgpH = 3, kVgpH2 = 4, kVgpZero = 5, kVgpVecs = 6 };
// vsmall: [0, 6) the -ELBO sums, [8, 8 + kGradMaxLs + 3) the gradient (launch_gradient: n_ls + 3 doubles), then the four
// int verdicts of the factorisations (Gram, Lambda, Sigma, I - Sigma) in two doubles of their own
constexpr int kVgpGradAt = 8, kVgpInfoAt = kVgpGradAt + kGradMaxLs + 3, kVgpSmall = kVgpInfoAt + 2;
static_assert(kVgpGradAt >= 6 && kVgpInfoAt >= kVgpGradAt + kGradMaxLs + 3, "vsmall layout: sums, gradient and verdicts overlap");
int* EngineCore::vinfo() const { return reinterpret_cast<int*>(as<double>(vsmall) + kVgpInfoAt); }
// a general scalar likelihood (vlik_kind != GPSO_LIK_GAUSSIAN): df, the Gauss-Hermite rule on the device (vgh: [0, 64)
// nodes x sqrt(2), [64, 128) weights / sqrt(pi)) and the per-point vectors of the quadrature (vlvec)
enum { kLikM = 0, kLikV = 1, kLikGm = 2, kLikA = 3, kLikT = 4, kLikVe = 5, kLikDve = 6, kLikMu = 7, kLikVecs = 8 };
// the f-free part of log p(y | f) at the likelihood parameter p (Student-t: the scale; Gaussian: the variance)
double EngineCore::vlik_const(double p) const {
  if (vlik_kind == GPSO_LIK_BERNOULLI) return 0.0;  // (log Phi(s f) has no f-free part and no parameter)
  if (vlik_kind == GPSO_LIK_STUDENT_T)
    return std::lgamma(0.5 * (vlik_df + 1.0)) - std::lgamma(0.5 * vlik_df) -
           0.5 * (std::log(p * p) + std::log(vlik_df) + std::log(M_PI));
  return -0.5 * (std::log(2.0 * M_PI) + std::log(p));
}
// m = L mu + c, v = rownorm(L S) (A := L S), then the quadrature at q: gm, a, t, VE, dVE/dp
void EngineCore::vgp_quadrature(const double* L, double* A, double p, double mean_c) {
  hipStream_t s = st();
  launch_vgp_gemv(s, L, false, as<double>(vq_mu), 0.0, 1.0, mean_c, nullptr, lvec_at(kLikM), n, npad);
  launch_dgemm(s, L, false, as<double>(vq_S), false, A, npad, 1.0, 0.0);
  launch_vgp_rownorm(s, A, lvec_at(kLikV), n, npad);
  launch_vgp_quad(s, as<double>(y64), lvec_at(kLikM), lvec_at(kLikV), as<double>(vgh), vlik_n_gh, vlik_kind, p, vlik_df,
                  vlik_const(p), mean_c, lvec_at(kLikGm), lvec_at(kLikA), lvec_at(kLikT), lvec_at(kLikVe),
                  lvec_at(kLikDve), n, npad);
}

int EngineCore::vgp_set_likelihood(int kind, double df, int n_gh, const double* gh_x, const double* gh_w) {
  if (int rcd = need_double_fit("the variational GP needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context")) return rcd;
  if (kind != GPSO_LIK_GAUSSIAN && kind != GPSO_LIK_STUDENT_T && kind != GPSO_LIK_GAUSSIAN_GH && kind != GPSO_LIK_BERNOULLI)
    return ctx->fail(GPSO_E_ARG, "unknown likelihood kind %d", kind);
  if (kind != GPSO_LIK_GAUSSIAN) {
    if (n_gh < 1 || n_gh > 64) return ctx->fail(GPSO_E_ARG, "n_gh=%d outside [1, 64]", n_gh);
    if (!gh_x || !gh_w) return ctx->fail(GPSO_E_ARG, "gh_x / gh_w must not be NULL");
    if (kind == GPSO_LIK_STUDENT_T && !(df > 2.0))
      return ctx->fail(GPSO_E_ARG, "Student-t df=%g: need df > 2 (a finite predictive variance)", df);
    if (kind == GPSO_LIK_BERNOULLI && df != 0.0)
      return ctx->fail(GPSO_E_ARG, "Bernoulli df=%g: the kind has no parameter, pass df = 0", df);
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

int EngineCore::vgp_begin(bool sparse) {
  if (int rcd = need_double_fit("the variational GP needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context")) return rcd;
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
void EngineCore::vgp_prior() {
  (void)hipMemsetAsync(vq_mu.p, 0, (size_t)npad * 8, st());
  launch_vgp_pad_identity(st(), as<double>(vq_S), 0, npad, nullptr);
  vq_n = n;
  vq_npad = npad;
}
// A (destroyed: lower triangle read, identity padding) = Lout Lout^T; Linv = Lout^-1.  Both leave as clean lower triangles:
// zero above the diagonal, pad_diag on the diagonal of the padding, zero elsewhere on it
int EngineCore::vgp_chol(double* A, double* Lout, double* Linv, int* info, double pad_diag) {
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
int EngineCore::vgp_factor(const Theta& th) {
  int rc = set_theta(th.with_lik(kVgpJitter));
  if (rc) return rc;
  if ((rc = scale_inputs())) return rc;
  launch_gram<double>(st(), as<double>(xs64), as<double>(xnorm64), n, npad, dp, kp, as<double>(K), vinfo() + 0);
  return vgp_chol(as<double>(K), as<double>(Lf), as<double>(linv), vinfo() + 0, 0.0);
}
// wait for the stream, then the verdicts of the factorisations (out: host copy of vsmall)
// (kind: whose factorisations these are -- the names in a failure's message)
int EngineCore::vgp_finish(double** out, Post kind) {
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
void EngineCore::vgp_reset_info() {
  for (int q = 0; q < 4; ++q) launch_vgp_pad_identity(st(), nullptr, 0, 0, vinfo() + q);  // (INT_MAX; no matrix)
}

int EngineCore::vgp_set_q(const double* mu, const double* S, int64_t n_) {
  if (int rcd = need_double_fit("the variational GP needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context")) return rcd;
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
int EngineCore::vgp_extend_q() {
  if (int rcd = need_double_fit("the variational GP needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context")) return rcd;
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
int EngineCore::vgp_get_q(double* mu, double* S) {
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
int EngineCore::vgp_natural_update(const double* qmu, const double* qS, double gamma, double* mu_out, double* S_out) {
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
int EngineCore::vgp_natgrad(const Theta& th, double gamma) {
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
int EngineCore::vgp_elbo(const Theta& th, double* loss, double* grad) {
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
      grad[n_ls + 1] = vlik_kind == GPSO_LIK_BERNOULLI ? 0.0 : -host[1];  // (no parameter: exactly 0.0, not -0.0)
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
int EngineCore::vgp_shifted_root(double* delta_out, bool sigma_ready, const double* qS) {
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
int EngineCore::vgp_posterior(const Theta& th) {
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
    // the likelihood's variance in the predictive: scale^2 df / (df - 2) (Student-t, closed form) or s2; + delta k**.
    // Bernoulli: 0 -- the install serves the LATENT mean and variance (log-concave: delta is 0), gpso_predict_prob maps them
    const double noise = vlik_kind == GPSO_LIK_BERNOULLI ? 0.0
                         : vlik_kind == GPSO_LIK_STUDENT_T ? s2 * s2 * vlik_df / (vlik_df - 2.0) : s2;
    if ((rc = set_theta(th.with_lik(noise + shift * th.variance)))) return rc;
  }
  if ((rc = install_predictive(Post::Vgp))) return rc;
  if (vlik_kind == GPSO_LIK_BERNOULLI) res.bernoulli_installed();
  return GPSO_OK;
}
// what the three variational installs share once linv holds C and alpha_f holds beta: the predict-ready copies, the
// factorisations' verdicts, and the posterior's kind
int EngineCore::install_predictive(Post kind) {
  hipStream_t s = st();
  int rc;
  double* host;
  if (!(rc = pack_predictive(s))) rc = vgp_finish(&host, kind);
  res.variational_ready(kind, rc == GPSO_OK);
  return rc;
}

// ---- sparse GP regression on inducing points (GPflow 2 SGPR, Gaussian likelihood, Z fixed) --------
// gpso_sgpr_set_inducing / gpso_sgpr_select_inducing move the training data (N rows) into buffers of their own (sgX raw,
// sgY) and make Z the context's resident rows (n = M): Kuu, its factor and everything M x M then run through the fit's
// buffers and kernels at size M_pad exactly as the VGP's do at N_pad, the installed predictive is a posterior over the M
// rows Z that every predict path serves, and the rectangular [M_pad x N_pad] work lives in sgKuf / sgA / sgW.
enum { kSgE = 0, kSgW = 1, kSgT = 2, kSgVecsN = 3 };
enum { kSgAe = 0, kSgCv = 1, kSgMu = 2, kSgAvec = 3, kSgRows = 4, kSgZero = 5, kSgVecsM = 6 };
constexpr int kSgGradAt = 16, kSgSmall = kSgGradAt + kGradMaxLs + 1;
// the resident rows are the caller's data: keep them as the SGPR's training set
int EngineCore::sgpr_stash() {
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

int EngineCore::sgpr_set_inducing(const double* Z, int64_t m) {
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

int EngineCore::sgpr_select_inducing(const Theta& th, int64_t m, int64_t* idx_out) {
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

int EngineCore::sgpr_get_inducing(double* Z, int64_t* m_out, int64_t* n_data_out) {
  if (!res.sg_have || !res.sg_have_z) return ctx->fail(GPSO_E_STATE, "no inducing points set (gpso_sgpr_set_inducing / gpso_sgpr_select_inducing)");
  if (m_out) *m_out = n;
  if (n_data_out) *n_data_out = sg_n;
  if (Z) std::memcpy(Z, x_host.data(), (size_t)n * d * 8);
  return GPSO_OK;
}

// the intermediates of the last successful gpso_sgpr_bound_u, for checks against a reference
int EngineCore::sgpr_get_factor(int which, double* out) {
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
int EngineCore::sgpr_factor(const Theta& th, const char* who) {
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

// grad_z (nullable, with grad): also d(-F)/dZ [M * D], from the weights the theta gradient has just formed
int EngineCore::sgpr_bound_impl(const Theta& th, double* loss, double* grad, double* grad_z, const char* who) {
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
int EngineCore::sgpr_posterior(const Theta& th, double* delta_out) {
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
enum { kSvM = 0, kSvV = 1, kSvGm = 2, kSvA = 3, kSvT = 4, kSvVe = 5, kSvDve = 6, kSvVecsN = 7 };
// the long-K products A A^T (SGPR) and A diag(a) A^T (SVGP) are split along N into this many fixed-order partial products
int EngineCore::sparse_nsplit() const {
  int ns = 1;
  while (ns < 16 && sg_npad % (256 * ns) == 0 && sg_npad / (2 * ns) >= 512) ns *= 2;
  return ns;
}
// the rectangular [M_pad x N_pad] and square [M_pad^2] work of an evaluation at the resident M and N.  Each family asks
// for its own third rectangle(s) and N-vectors only: sgW / sgvecN the SGPR, svB / svD / svvecN the SVGP
int EngineCore::sparse_workspace(bool svgp) {
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

int EngineCore::svgp_need_z(const char* who) {
  int rc = sgpr_need_f64();
  if (rc) return rc;
  if (!res.sg_have || !res.sg_have_z)
    return ctx->fail(GPSO_E_STATE, "%s needs the data and the inducing points: gpso_set_data, then gpso_sgpr_set_inducing or gpso_sgpr_select_inducing", who);
  return GPSO_OK;
}
void EngineCore::svgp_prior() {
  (void)hipMemsetAsync(svq_mu.p, 0, (size_t)npad * 8, st());
  launch_vgp_pad_identity(st(), as<double>(svq_S), 0, npad, nullptr);
  svq_m = n;
  svq_mpad = npad;
}
// q's buffers at the resident M; the prior when q was made for other rows
int EngineCore::svgp_q() {
  int rc;
  if (svq_m == n && svq_mpad == npad) return GPSO_OK;
  if ((rc = ensure(svq_mu, (size_t)npad * 8))) return rc;
  if ((rc = ensure(svq_S, (size_t)npad * npad * 8))) return rc;
  svgp_prior();
  return GPSO_OK;
}

// Lu (Lf), Lu^-1 (linv) at theta; rect: also Kuf (sgKuf) and A = Lu^-1 Kuf (sgA).  The verdict of Kuu in vinfo() 0
int EngineCore::svgp_begin(const Theta& th, const char* who, bool rect) {
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
void EngineCore::svgp_pointwise(double variance, double p, double mean_c, bool want_v, bool gauss) {
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
void EngineCore::svgp_adat(double* aat, double* lam) {
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
int EngineCore::svgp_step(const Theta& th, double gamma, bool conj, const char* who) {
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

int EngineCore::svgp_init_q(const Theta& th, double s2) {
  if (s2 > 0.0) return svgp_step(th.with_lik(s2), 1.0, true, "gpso_svgp_init_q");
  int rc = svgp_need_z("gpso_svgp_init_q");
  if (rc || (rc = vgp_begin()) || (rc = svgp_q())) return rc;
  svgp_prior();
  HIPCHECK(ctx->wait(st()));
  return launch_status();
}

int EngineCore::svgp_set_q(const double* mu, const double* S, int64_t m) {
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

int EngineCore::svgp_get_q(double* mu, double* S) {
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
// grad_z (nullable, with grad): also d(-ELBO)/dZ [M * D] at fixed q (whitened: q stays valid while Z moves; the k_diag
// term does not depend on Z)
int EngineCore::svgp_elbo_impl(const Theta& th, double* loss, double* grad, double* grad_z, const char* who) {
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
int EngineCore::svgp_posterior(const Theta& th, double* delta_out) {
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
int EngineCore::inducing_buffers() {
  int rc = ensure(sgZpart, (size_t)(inducing_slices(npad, sg_npad) + 1) * npad * (dp + 1) * 8);
  if (rc) return rc;
  return ensure(sgZg, (size_t)n * d * 8);
}
int EngineCore::inducing_args(const char* who, const double* Z) {
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
int EngineCore::inducing_put(const double* Z) {
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

int EngineCore::sgpr_move_inducing(const double* Z) {
  if (!Z) return ctx->fail(GPSO_E_ARG, "Z must not be NULL");
  int rc = inducing_args("gpso_sgpr_move_inducing", Z);
  if (rc) return rc;
  return inducing_put(Z);
}

int EngineCore::sgpr_bound_z(const Theta& th, const double* Z, double* loss, double* grad, double* grad_z) {
  int rc = inducing_args("gpso_sgpr_bound_uz", Z);
  if (rc || (rc = theta_status(theta_refusal(th, d, true), "noise variance"))) return rc;
  if (Z && (rc = inducing_put(Z))) return rc;
  return sgpr_bound_impl(th, loss, grad, grad_z, "gpso_sgpr_bound_uz");
}

int EngineCore::svgp_elbo_z(const Theta& th, const double* Z, double* loss, double* grad, double* grad_z) {
  int rc = inducing_args("gpso_svgp_elbo_uz", Z);
  if (rc || (rc = theta_status(theta_refusal(th, d, true), "likelihood parameter"))) return rc;
  if (Z && (rc = inducing_put(Z))) return rc;
  return svgp_elbo_impl(th, loss, grad, grad_z, "gpso_svgp_elbo_uz");
}

}  // namespace gpso::host
