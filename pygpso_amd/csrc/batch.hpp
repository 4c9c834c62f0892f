// Greedy batch selection under hallucinated updates (GP-BUCB, "kriging believer"): the arithmetic of one row in one round.
// One restatement for the device (batch.hip: batch_col_kernel, batch_finish_kernel, batch_pick_kernel) and for the host
// (gpso_batch_greedy_host: the CPU tests), built like acq.hpp and screen.hpp.  DESIGN.md section 7n.
//
// Round t has picked p_t.  With Cov(., .) the LATENT posterior covariance of the resident posterior and G[s][.] the columns
// of the earlier rounds s < t:
//     c_t[j]      = Cov(j, p_t) - sum_{s < t} G[s][j] G[s][p_t]         (s in round order, one fused multiply-add each)
//     d_t         = c_t[p_t] + obs_noise                                 (c_t[p_t] from the pick's own latent variance)
//     G[t][j]     = c_t[j] / sqrt(d_t)
//     s2_{t+1}[j] = s2_t[j] - G[t][j]^2                                  (one fused multiply-add; the means do not move)
// s2 is the PREDICTIVE variance a leaf is ranked by; a kind with `latent` set reads s2 - noise (UCB_VAR never does: the
// finalize epilogue's rule).  The arg-max is numpy's: the first maximum, and a NaN beats every number.
#pragma once
#include <cmath>
#include <cstdint>

#include "acq.hpp"

namespace gpso {

constexpr int kBatchMaxPicks = 64;                    // q of gpso_best_batch, b of gpso_cross_cov
constexpr int64_t kBatchMaxCells = (int64_t)1 << 27;  // q * m: the doubles of G

// the value a live row is ranked by in the rounds after the first
template <bool WITH_MES = true>
GPSO_ACQ_HD inline double batch_score(const AcqSpec& a, double mean, double s2, double noise) {
  return acq_value<WITH_MES>(a, mean, (a.latent && a.kind != GPSO_ACQ_UCB_VAR) ? s2 - noise : s2);
}

// does (v, i) rank before (bv, bi)?  i < 0: no candidate; bi < 0: no holder yet.  A total order, so every merge tree gives
// the same winner
GPSO_ACQ_HD inline bool batch_beats(double v, int64_t i, double bv, int64_t bi) {
  if (i < 0) return false;
  if (bi < 0) return true;
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

// d_t from the pick's latent variance lv and gp[s] = G[s][p_t], s < t
GPSO_ACQ_HD inline double batch_pick_d(double lv, const double* gp, int t, double obs_noise) {
  double c = lv;
  for (int s = 0; s < t; ++s) c = fma(-gp[s], gp[s], c);
  return c + obs_noise;
}
// the stop test: a d that is not finite or not positive ends the batch after its pick
GPSO_ACQ_HD inline bool batch_d_usable(double d) { return d - d == 0.0 && d > 0.0; }

// G[t][j] from the raw latent covariance c = Cov(j, p_t); gj[s * stride] = G[s][j]
GPSO_ACQ_HD inline double batch_row_g(double c, const double* gj, int64_t stride, const double* gp, int t, double root_d) {
  for (int s = 0; s < t; ++s) c = fma(-gj[(int64_t)s * stride], gp[s], c);
  return c / root_d;
}
GPSO_ACQ_HD inline double batch_downdate(double s2, double g) { return fma(-g, g, s2); }

// the retire test.  Device: the row's scaled coordinates equal the pick's exactly (r2 from direct differences).  Host, which
// sees no coordinates: the row is the pick, or the covariance cannot tell them apart -- Cov(j, j), Cov(j, p) and Cov(p, p)
// are the same number, which a covariance built per distinct point and expanded gives for every repeated row
GPSO_ACQ_HD inline bool batch_same_point(double r2) { return r2 == 0.0; }
GPSO_ACQ_HD inline bool batch_same_point_cov(double cjj, double cjp, double cpp) { return cjj == cpp && cjp == cpp; }

// gpso_batch_greedy_host (batch.hip: built without contraction, like the kernels)
int batch_greedy_host(const AcqSpec& a, const double* mean, const double* s2, const double* cov, double noise, double obs_noise,
                      int64_t m, int q, int64_t* idx, double* var, double* value, int* n_picked, double* var_after);

}  // namespace gpso
