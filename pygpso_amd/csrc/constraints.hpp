// Outcome constraints: J exact-GP posteriors of constrained outputs c_i(x) beside the objective's, and
// the constrained acquisition of Gardner et al. (2014) and Gelbart, Snoek & Adams (2014) over them.  This header holds the
// fold -- what turns one leaf's objective column (mean, var) and its J constraint columns into the probability of feasibility
// and the value the arg-max ranks by -- as ONE text for the device (constraints.hip: con_fold_kernel) and the host
// (gpso_constrained_fold_host), and the launch records of constraints.hip.
//
//   s2_i   = max(var_i - noise_i, 0)                 the LATENT variance: the constraint function, not a noisy reading of it
//   z_i    = sense_i (t_i - mean_i) / sqrt(s2_i)     acq_z_diff: the rounding of the difference is kept
//   lp_i   = acq_log_ncdf(z_i);   at s2_i = 0: 0 where sense_i (t_i - mean_i) >= 0, else -inf
//   logpof = sum_i lp_i           index order, starting at its first term;  a NaN anywhere: NaN
//   a0     = acq.hpp's map on the objective's (mean, var), or var - noise for a latent kind (UCB_VAR never does)
//   weight (0):       EI, PI: a0 acq_exp(logpof);  LOGEI: l0 + logpof;  -inf where logpof < log_pof_min   (no UCB kind)
//   gate (1):         a0 where logpof >= log_pof_min, else -inf; a0's own bits.  log_pof_min = -inf: no gate, a0 always
//   feasibility (2):  logpof
//   a NaN logpof gives a NaN value in every mode but the open gate.  MES is refused by every caller
// Columns are [J][ld]: constraint i's value of leaf j at col[i * ld + j].
#pragma once
#include <cstdint>

#include "acq.hpp"
#include "success.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef GPSO_CON_WEIGHT
#define GPSO_CON_WEIGHT 0
#define GPSO_CON_GATE 1
#define GPSO_CON_FEASIBILITY 2
#endif

namespace gpso {

constexpr int kConstraintsMax = 16;  // GPSO_CONSTRAINTS_MAX

struct ConSpec {
  int mode = GPSO_CON_GATE;
  double log_pof_min = -__builtin_inf();
};

// log P(sense (t - c) >= 0) under c ~ N(mean, var - noise)
GPSO_ACQ_HD inline double con_log_pof_term(double mean, double var, double noise, double thr, double sense) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (mean != mean || var != var) return __builtin_nan("");
  double s2 = var - noise;
  s2 = s2 > 0.0 ? s2 : 0.0;
  if (s2 == 0.0) {
    const double d = sense * (thr - mean);
    return d >= 0.0 ? 0.0 : -__builtin_inf();
  }
  double z, zl;
  acq_z_diff(thr, mean, s2, sqrt(s2), &z, &zl);
  return acq_log_ncdf(sense * z, sense * zl);
}

// what the mode makes of a leaf's logpof `lp` and the objective's (om, ov): the value the arg-max ranks by
GPSO_ACQ_HD inline void constrained_value_leaf(const AcqSpec& a, const ConSpec& c, double om, double ov, double onoise, double lp, double* value,
                                               double* logpof) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *logpof = lp;
  if (c.mode == GPSO_CON_FEASIBILITY) {
    *value = lp;
    return;
  }
  const bool latent = a.latent && a.kind != GPSO_ACQ_UCB_VAR;
  const double a0 = acq_value<false>(a, om, latent ? ov - onoise : ov);
  const double ninf = -__builtin_inf();
  if (c.mode == GPSO_CON_GATE) {
    if (c.log_pof_min == ninf) *value = a0;
    else if (lp != lp) *value = lp;
    else *value = lp >= c.log_pof_min ? a0 : ninf;
    return;
  }
  if (lp < c.log_pof_min) *value = ninf;
  else if (lp != lp) *value = lp;
  else if (a.kind == GPSO_ACQ_LOGEI) *value = a0 + lp;
  else *value = a0 * acq_exp(lp);
}

// the two numbers of leaf j.  (om, ov, onoise): the objective's predictive column entries and its noise variance;
// thr / sense / cnoise [J]: the members' thresholds, senses (+1: c <= t, -1: c >= t) and noise variances
GPSO_ACQ_HD inline void constrained_fold_leaf(const AcqSpec& a, const ConSpec& c, double om, double ov, double onoise, const double* cmean,
                                              const double* cvar, const double* cnoise, const double* thr, const double* sense, int nj,
                                              int64_t ld, int64_t j, double* value, double* logpof) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double lp = con_log_pof_term(cmean[j], cvar[j], cnoise[0], thr[0], sense[0]);
  for (int i = 1; i < nj; ++i) lp += con_log_pof_term(cmean[i * ld + j], cvar[i * ld + j], cnoise[i], thr[i], sense[i]);
  constrained_value_leaf(a, c, om, ov, onoise, lp, value, logpof);
}

// ... with a success member (success.hpp): its log-probability at the latent (smean, svar) of leaf j is
// the LAST term of logpof, behind the nj constraints in index order; nj = 0: it IS logpof (the sum starts at its first term)
GPSO_ACQ_HD inline void constrained_success_fold_leaf(const AcqSpec& a, const ConSpec& c, double om, double ov, double onoise,
                                                      const double* cmean, const double* cvar, const double* cnoise, const double* thr,
                                                      const double* sense, int nj, int64_t ld, int64_t j, double smean, double svar,
                                                      double* value, double* logpof) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double ls = success_log_prob(smean, svar);
  double lp = ls;
  if (nj > 0) {
    lp = con_log_pof_term(cmean[j], cvar[j], cnoise[0], thr[0], sense[0]);
    for (int i = 1; i < nj; ++i) lp += con_log_pof_term(cmean[i * ld + j], cvar[i * ld + j], cnoise[i], thr[i], sense[i]);
    lp += ls;
  }
  constrained_value_leaf(a, c, om, ov, onoise, lp, value, logpof);
}

// host loop of gpso_constrained_fold_host (constraints.hip: built without contraction, like the device fold)
void constrained_fold_host(const AcqSpec& a, const ConSpec& c, const double* mean, const double* var, double noise, const double* cmean,
                           const double* cvar, const double* cnoise, const double* thr, const double* sense, int nj, long long m,
                           double* value, double* logpof);
// ... and of gpso_constrained_success_fold_host (success.hip): smean / svar [m] the success member's latent columns; nj may be 0
void constrained_success_fold_host(const AcqSpec& a, const ConSpec& c, const double* mean, const double* var, double noise, const double* cmean,
                                   const double* cvar, const double* cnoise, const double* thr, const double* sense, int nj, long long m,
                                   const double* smean, const double* svar, double* value, double* logpof);

#if defined(__HIPCC__)
// ---- constraints.hip ---------------------------------------------------------------------------------------------------
// what the fold kernel reads of the set: per member its threshold, sense and where its noise variance lies (the hyper block's slot 5)
struct ConFoldLaunch {
  AcqSpec acq;
  ConSpec con;
  const double* obj_mean = nullptr;   // [m]
  const double* obj_var = nullptr;    // [m]
  const double* obj_hyper = nullptr;  // the objective's hyper block (slot 5: noise variance)
  const double* cmean = nullptr;      // [J][ld]
  const double* cvar = nullptr;
  const double* chyper = nullptr;     // [J][hyper_stride]
  int64_t hyper_stride = 0;
  double thr[kConstraintsMax] = {};
  double sense[kConstraintsMax] = {};
  int nj = 0;
  int64_t ld = 0, m = 0;
  double* value = nullptr;   // [m]
  double* logpof = nullptr;  // [m]
  // (behind everything section 7r's record holds, whose offsets stay what they were)
  const double* smean = nullptr;  // [m] the success member's latent columns (success.hpp); NULL: none, the fold of section 7r
  const double* svar = nullptr;
};
// one thread per leaf: constrained_fold_leaf, or constrained_success_fold_leaf where smean is set (nj may then be 0)
void launch_constrained_fold(hipStream_t st, const ConFoldLaunch& g);
// the winner's logpof per segment: out[i] = logpof[seg_off[i] + idx_i], idx_i read from launch_seg_argmax's records
// (rec[4 i + 3], a bit-cast int64; -1: an empty segment, NaN)
void launch_constrained_gather(hipStream_t st, const double* logpof, const int64_t* seg_off_dev, const double* rec, int nseg, double* out);
// ---- success.hip -------------------------------------------------------------------------------------------------------
// launch_constrained_fold's route where g.smean is set: constrained_success_fold_leaf, one thread per leaf
void launch_constrained_success_fold(hipStream_t st, const ConFoldLaunch& g);
// one thread per point: logprob[j] = success_log_prob(mean[j], var[j]), prob[j] = acq_exp of it
void launch_success_map(hipStream_t st, const double* mean, const double* var, int64_t m, double* logprob, double* prob);
#endif

}  // namespace gpso
