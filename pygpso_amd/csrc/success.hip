// Failed evaluations (success.hpp holds the probit map, constraints.hpp the fold and the launch records).
//
// con_success_fold_kernel: con_fold_kernel (constraints.hip) with a success member's latent columns in the launch record:
// one thread per leaf, constrained_success_fold_leaf -- the J constraints' terms in index order, then the member's
// log-probability of success as the LAST term; J = 0: that term alone.  Coalesced column reads and stores, nothing shared
// between threads: no atomics, and a leaf's bits depend neither on its slot nor on the batch.
// success_map_kernel: one thread per point, the probit map of gpso_predict_prob.
// A translation unit of its own: constraints.hip then compiles to the code it had without this feature.
// Compiled with -ffp-contract=off; every fused multiply-add is written out.
#include "constraints.hpp"
#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void con_success_fold_kernel(ConFoldLaunch g) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= g.m) return;
  double noise[kConstraintsMax];
  for (int i = 0; i < g.nj; ++i) noise[i] = g.chyper[(int64_t)i * g.hyper_stride + 5];
  double value, logpof;
  constrained_success_fold_leaf(g.acq, g.con, g.obj_mean[j], g.obj_var[j], g.obj_hyper[5], g.cmean, g.cvar, noise, g.thr, g.sense, g.nj, g.ld,
                                j, g.smean[j], g.svar[j], &value, &logpof);
  g.value[j] = value;
  g.logpof[j] = logpof;
}

// one thread per point, nothing shared: the probit map of a Bernoulli install's latent columns (success.hpp); outputs nullable
__global__ __launch_bounds__(kThreads) void success_map_kernel(const double* __restrict__ mean, const double* __restrict__ var, int64_t m,
                                                               double* __restrict__ logprob, double* __restrict__ prob) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const double lp = success_log_prob(mean[j], var[j]);
  if (logprob != nullptr) logprob[j] = lp;
  if (prob != nullptr) prob[j] = success_prob_of_log(lp);
}

}  // namespace

void success_prob_host(const double* mean, const double* var, long long n, double* logprob, double* prob) {
  for (long long j = 0; j < n; ++j) {
    const double lp = success_log_prob(mean[j], var[j]);
    if (logprob) logprob[j] = lp;
    if (prob) prob[j] = success_prob_of_log(lp);
  }
}

void constrained_success_fold_host(const AcqSpec& a, const ConSpec& c, const double* mean, const double* var, double noise, const double* cmean,
                                   const double* cvar, const double* cnoise, const double* thr, const double* sense, int nj, long long m,
                                   const double* smean, const double* svar, double* value, double* logpof) {
  for (long long j = 0; j < m; ++j) {
    double v, lp;
    constrained_success_fold_leaf(a, c, mean ? mean[j] : 0.0, var ? var[j] : 0.0, noise, cmean, cvar, cnoise, thr, sense, nj, (int64_t)m,
                                  (int64_t)j, smean[j], svar[j], &v, &lp);
    if (value) value[j] = v;
    if (logpof) logpof[j] = lp;
  }
}

void launch_constrained_success_fold(hipStream_t st, const ConFoldLaunch& g) {
  hipLaunchKernelGGL(con_success_fold_kernel, dim3((unsigned)((g.m + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, g);
}

void launch_success_map(hipStream_t st, const double* mean, const double* var, int64_t m, double* logprob, double* prob) {
  hipLaunchKernelGGL(success_map_kernel, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, mean, var, m, logprob, prob);
}

}  // namespace gpso
