// The hyper-parameters on their way from the optimiser's unconstrained vector u to the engine and back: the one decoder, the
// one validator and the one chain rule of every training entry point.  Host side only, no HIP; api.hip is the one file of
// the library that includes this (tools/theta_check.cpp compiles it on its own).  pygpso_amd/model.py's _softplus1 and
// _sigmoid are the Python twins of the two transforms and must agree with them bit for bit.
#pragma once
#include <cmath>

namespace gpso {

constexpr int kThetaMaxLs = 64;  // = kGradMaxLs of kernels.hpp (api.hip asserts it)

// GPflow-2's parameter transforms, bit for bit what numpy computes for them on the host
// side of the reference's optimiser loop: softplus(u) = logaddexp(0, u) in numpy's own case split (libm log1p / exp),
// sigmoid(u) = (1 + tanh(u / 2)) / 2.
inline double gpso_softplus(double u) {
  if (u == 0.0) return 0.693147180559945309417232121458176568;  // log 2
  if (u < 0.0) return 0.0 + std::log1p(std::exp(u));
  if (u > 0.0) return u + std::log1p(std::exp(-u));
  return u;  // NaN
}
inline double gpso_sigmoid(double u) { return 0.5 * (1.0 + std::tanh(0.5 * u)); }

// theta = (lengthscales..., kernel variance, likelihood parameter, mean).  lik is whatever slot n_ls + 1 means to the
// caller: the noise variance, the Gaussian likelihood's variance or the Student-t scale
struct Theta {
  int kernel, n_ls;
  double ls[kThetaMaxLs];
  double variance, lik, mean_c;
  // the same kernel at another value of the last-but-one slot (what a family writes into the hyper block: a jitter, a
  // predictive variance)
  Theta with_lik(double value) const {
    Theta t = *this;
    t.lik = value;
    return t;
  }
};

enum class ThetaDecode { Ok, NullU, NlsRange };

// u[n_ls + 2 (+ 1 with train_mean)] -> theta.  lik_floor: 1e-6 for a Gaussian variance (gpflow.likelihoods.Gaussian's
// DEFAULT_VARIANCE_LOWER_BOUND), 0.0 for the Student-t scale (GPflow's positive())
inline ThetaDecode theta_from_u(int kernel, const double* u, int n_ls, bool train_mean, double mean_c_fixed, double lik_floor,
                                Theta* th) {
  if (!u) return ThetaDecode::NullU;
  if (n_ls < 1 || n_ls > kThetaMaxLs) return ThetaDecode::NlsRange;
  th->kernel = kernel;
  th->n_ls = n_ls;
  for (int k = 0; k < n_ls; ++k) th->ls[k] = gpso_softplus(u[k]);
  th->variance = gpso_softplus(u[n_ls]);
  th->lik = lik_floor + gpso_softplus(u[n_ls + 1]);
  th->mean_c = train_mean ? u[n_ls + 2] : mean_c_fixed;
  return ThetaDecode::Ok;
}
// ... and from constrained values as a caller passes them (ls not NULL).  n_ls is kept as given, for the validator to
// refuse; no more than kThetaMaxLs lengthscales are read
inline void theta_from_parts(int kernel, const double* ls, int n_ls, double variance, double lik, double mean_c, Theta* th) {
  th->kernel = kernel;
  th->n_ls = n_ls;
  for (int k = 0; k < n_ls && k < kThetaMaxLs; ++k) th->ls[k] = ls[k];
  th->variance = variance;
  th->lik = lik;
  th->mean_c = mean_c;
}

// theta_out[n_ls + 3] = (ls..., variance, lik, mean)
inline void theta_copy_out(const Theta& th, double* theta_out) {
  for (int k = 0; k < th.n_ls; ++k) theta_out[k] = th.ls[k];
  theta_out[th.n_ls] = th.variance;
  theta_out[th.n_ls + 1] = th.lik;
  theta_out[th.n_ls + 2] = th.mean_c;
}

// chain rule: d/du = d/dtheta * sigmoid(u) for the softplus-transformed parameters, identity for the mean.
// g[n_ls + 3] -> grad_u[n_ls + 2 (+ 1 with train_mean)]
inline void grad_to_u(const double* u, int n_ls, bool train_mean, const double* g, double* grad_u) {
  for (int k = 0; k < n_ls + 2; ++k) grad_u[k] = g[k] * gpso_sigmoid(u[k]);
  if (train_mean) grad_u[n_ls + 2] = g[n_ls + 2];
}

// What the engine cannot use, in the order it is looked for.  index / value: what the message names -- the kernel id,
// n_ls, or the lengthscale's position and the offending value
enum class ThetaRule { None, Lik, Kernel, Nls, Lengthscale, Variance };
struct ThetaRefusal {
  ThetaRule rule;
  int index;
  double value;
  explicit operator bool() const { return rule != ThetaRule::None; }
};

// the kernel id, then n_ls against the D of the resident rows
inline ThetaRefusal theta_shape_refusal(int kernel, int n_ls, int d) {
  if (kernel < 0 || kernel > 3) return {ThetaRule::Kernel, kernel, 0.0};
  if (!(n_ls == 1 || n_ls == d) || n_ls > kThetaMaxLs) return {ThetaRule::Nls, n_ls, 0.0};
  return {ThetaRule::None, 0, 0.0};
}
// check_lik: the likelihood parameter must be positive too, and is looked at first.  NaN is refused wherever it stands
inline ThetaRefusal theta_refusal(const Theta& th, int d, bool check_lik) {
  if (check_lik && !(th.lik > 0.0)) return {ThetaRule::Lik, 0, th.lik};
  if (const ThetaRefusal r = theta_shape_refusal(th.kernel, th.n_ls, d)) return r;
  for (int k = 0; k < th.n_ls; ++k)
    if (!(th.ls[k] > 0.0)) return {ThetaRule::Lengthscale, k, th.ls[k]};
  if (!(th.variance > 0.0)) return {ThetaRule::Variance, 0, th.variance};
  return {ThetaRule::None, 0, 0.0};
}

}  // namespace gpso
