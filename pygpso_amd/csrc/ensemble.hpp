// The hyper-parameter ensemble: K posteriors of the same data, one per sample theta_k of p(theta | y),
// and the integrated acquisition of Snoek, Larochelle & Adams (2012) over them.  This header holds the fold -- what turns the
// K members' (mean_k, var_k) of one leaf into the mixture moments and the value the arg-max ranks by -- as ONE text for the
// device (ensemble.hip: ens_fold_kernel) and the host (gpso_ensemble_fold_host), and the launch records of ensemble.hip.
//
//   a_k      = acq.hpp's map on (mean_k, s2_k), s2_k = var_k, or var_k - noise_k for a latent kind (UCB_VAR never does)
//   UCB_VAR, UCB_STD, EI, PI:  value = (sum_k a_k) / K           terms in index order, one division
//   LOGEI:   value = mx + log(sum_k exp(l_k - mx)) - log K,  mx = max_k l_k      (acq_exp / acq_log: the header's own, so that
//            host and device agree);  -inf if every member is -inf
//   a NaN member: NaN.   MES is refused by every caller: its maxima belong to one theta
//   mean_mix = (sum_k m_k) / K,   var_mix = (sum_k (v_k + (m_k - mean_mix)^2)) / K      two passes, index order
//   K = 1: the member's own three numbers, bit for bit (x / 1.0 == x; the LOGEI form is skipped)
// Columns are [K][ld]: member k's value of leaf j at col[k * ld + j].
#pragma once
#include <cstdint>

#include "acq.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace gpso {

constexpr int kEnsembleMax = 32;      // GPSO_ENSEMBLE_MAX
constexpr int kEnsembleMaxN = 128;    // one row block of the factor: the one-launch fit's range
constexpr int kEnsembleTheta = 48 + 3;  // gpso_ensemble_info: 48 lengthscales, variance, noise, mean_c

// the three numbers of leaf j.  noise[k]: member k's noise variance (read by the latent kinds only)
GPSO_ACQ_HD inline void ensemble_fold_leaf(const AcqSpec& a, const double* mean, const double* var, const double* noise, int k,
                                           int64_t ld, int64_t j, double* mean_mix, double* var_mix, double* value) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double kk = (double)k;
  // (every sum starts at its first term, not at 0.0: K = 1 hands the member's bits through, a -0.0 included)
  double sm = mean[j];
  for (int i = 1; i < k; ++i) sm += mean[i * ld + j];
  const double mm = sm / kk;
  double sv = 0.0;
  for (int i = 0; i < k; ++i) {
    const double dm = mean[i * ld + j] - mm;
    const double sq = dm * dm;
    const double term = var[i * ld + j] + sq;
    sv = i == 0 ? term : sv + term;
  }
  *mean_mix = mm;
  *var_mix = sv / kk;
  const bool latent = a.latent && a.kind != GPSO_ACQ_UCB_VAR;
  auto member = [&](int i) { return acq_value<false>(a, mean[i * ld + j], latent ? var[i * ld + j] - noise[i] : var[i * ld + j]); };
  if (a.kind != GPSO_ACQ_LOGEI || k == 1) {
    double s = member(0);
    for (int i = 1; i < k; ++i) s += member(i);
    *value = s / kk;
    return;
  }
  // log of the mean EI.  Two passes over the members' values (at most kEnsembleMax of them)
  double l[kEnsembleMax];
  double mx = -__builtin_inf();
  bool nan = false;
  for (int i = 0; i < k; ++i) {
    l[i] = member(i);
    nan = nan || l[i] != l[i];
    if (l[i] > mx) mx = l[i];
  }
  if (nan) {
    *value = __builtin_nan("");
    return;
  }
  if (mx == -__builtin_inf() || mx == __builtin_inf()) {  // (every member -inf; or one +inf: no caller comes near)
    *value = mx;
    return;
  }
  double s = 0.0;
  for (int i = 0; i < k; ++i) s += acq_exp(l[i] - mx);
  *value = (mx + acq_log(s)) - acq_log(kk);
}

// host loop of gpso_ensemble_fold_host (ensemble.hip: built without contraction, like the device fold)
void ensemble_fold_host(const AcqSpec& a, const double* member_mean, const double* member_var, const double* noise, int k, long long m,
                        double* mean_mix, double* var_mix, double* value);

#if defined(__HIPCC__)
// ---- ensemble.hip ------------------------------------------------------------------------------------------------------
// Stage 1: grid (ceil(m / 64), K), 256 threads: member k's (mean, var) of 64 raw leaves -> mean[k * ld + j], var[k * ld + j].
// Member k's copies sit at hyper + k * hyper_stride etc.; every member has the shape (n, npad = 128, dp) and the kernel kind
struct EnsembleMembersLaunch {
  const double* hyper = nullptr;  // [K][hyper_stride]: the hyper blocks (slot 4 variance, 5 noise, 6 mean_c, 8.. lengthscales)
  const double* xs = nullptr;     // [K][npad * dp] scaled rows
  const double* linv = nullptr;   // [K][npad * npad] dense double L^-1 (read where j <= i < n only)
  const double* alpha = nullptr;  // [K][npad]
  int64_t hyper_stride = 0;
  const void* leaves = nullptr;  // raw leaves [m][d], float or double
  int leaves_f64 = 0;
  int64_t m = 0, ld = 0;
  int n = 0, npad = 0, d = 0, dp = 0, kernel = 0, k = 0;
  double* mean = nullptr;  // [K][ld]
  double* var = nullptr;
};
int launch_ensemble_members(hipStream_t st, const EnsembleMembersLaunch& g);
// Stage 2: one launch over the leaves: ensemble_fold_leaf of every leaf.  noise_at: where member k's noise variance lies,
// hyper + k * hyper_stride + 5.  The outputs are nullable
void launch_ensemble_fold(hipStream_t st, const AcqSpec& a, const double* mean, const double* var, const double* hyper, int64_t hyper_stride,
                          int k, int64_t ld, int64_t m, double* mean_mix, double* var_mix, double* value);
#endif

}  // namespace gpso
