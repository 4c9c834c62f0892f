// Failed evaluations: a GP classifier of "the evaluation returned a finite score", a whitened VGP under
// the Bernoulli likelihood with the exact probit link (GPSO_LIK_BERNOULLI), whose install serves the LATENT mean and variance
// of f.  This header holds what turns one point's latent (mean, var) into the probability of success,
//     P(success) = integral Phi(f) N(f; mean, var) df = Phi(mean / sqrt(1 + var)),
// as ONE text for the device (success.hip: success_map_kernel and the fold's last term) and the host
// (gpso_success_prob_host).  Built with contraction off, as constraints.hpp is.
//
//   success_log_prob(mean, var) = acq_log_ncdf(mean / sqrt(1 + max(var, 0)), 0)      a NaN in: NaN out
//   the probability             = acq_exp of it
#pragma once
#include "acq.hpp"

namespace gpso {

GPSO_ACQ_HD inline double success_log_prob(double mean, double var) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (mean != mean || var != var) return __builtin_nan("");
  const double v = var > 0.0 ? var : 0.0;
  return acq_log_ncdf(mean / sqrt(1.0 + v), 0.0);
}

GPSO_ACQ_HD inline double success_prob_of_log(double logprob) { return acq_exp(logprob); }

// host loop of gpso_success_prob_host (success.hip: built without contraction, like the device map); outputs nullable
void success_prob_host(const double* mean, const double* var, long long n, double* logprob, double* prob);

}  // namespace gpso
