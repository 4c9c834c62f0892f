// Monte-Carlo batch acquisition over the resident path draws (qEI, qNoisyEI, qPI): the arithmetic of one row in one round.
// One restatement for the device (mcbatch.hip: mc_init_kernel, mc_round_kernel, mc_fold_kernel) and for the host
// (gpso_paths_batch_host: the CPU tests and the bit checks), built like batch.hpp and ehvi.hpp.  DESIGN.md section 7u.
//
// V[s][j] is the value of draw s < S at row j (draw-major, leading dimension ld), t[s] the draw's bar:
//     GPSO_MC_QEI   gain(j) = (1/S) sum_s max(V[s][j] - t[s] - x[s], 0)         s in draw order, in double, nothing fused, one
//                   division.  x[s] is xi until a pick (or a pending point) has cleared the draw's bar by more than xi, and 0
//                   from then on; after pick p  t[s] = max(t[s], V[s][p]) in a draw that is cleared (by this pick or before),
//                   and t[s] stays in a draw that is not.  At xi = 0 this is  max(V - t, 0)  and  t = max(t, V[p])  in every
//                   draw.  The margin is charged once per draw, so the gains of the picks add up to the batch's value
//                   (1/S) sum_s max over the picks of max(V[s][p] - t0[s] - xi, 0), and a copy of a pick gains exactly 0
//     GPSO_MC_QPI   gain(j) = (1/S) #{ s : not yet cleared, V[s][j] > t[s] + xi }   an integer count, one division; the bars
//                   stay, after pick p the draws it cleared are cleared
// A NaN among the terms of a row makes its gain a NaN (for QPI: a NaN anywhere in the row's column).  Pending columns are folded
// into the bars and flags before round 0 as picks are, in column order.  The arg-max is batch.hpp's batch_beats: the first
// maximum, and a NaN beats every number.
#pragma once
#include <cstdint>

#include "batch.hpp"

namespace gpso {

constexpr int kMcMaxPicks = 64;                      // q of gpso_paths_best_batch
constexpr int kMcMaxPending = 64;                    // b: pending columns
constexpr int kMcMaxDraws = 256;                     // S of a path set (kPathsMaxDraws)
constexpr int64_t kMcMaxCells = (int64_t)1 << 26;    // S * (m + b): the doubles of V
constexpr int kMcQei = 0, kMcQpi = 1;                // GPSO_MC_QEI, GPSO_MC_QPI

// one draw's term of a QEI gain: the improvement over the bar by more than the draw's margin x, a NaN kept
GPSO_ACQ_HD inline double mc_improvement(double v, double bar, double x) {
  const double d = v - bar - x;
  return d > 0.0 ? d : (d == d ? 0.0 : d);
}
// the margin of a draw: xi until the draw is cleared
GPSO_ACQ_HD inline double mc_margin(int cleared, double xi) { return cleared ? 0.0 : xi; }
// QEI: a pick (or a pending point) of value v in a draw.  A NaN moves nothing
GPSO_ACQ_HD inline void mc_apply_qei(double v, double xi, double* bar, int* cleared) {
  if (*cleared) {
    if (v > *bar) *bar = v;
  } else if (v - *bar - xi > 0.0) {
    *bar = v;
    *cleared = 1;
  }
}
// QPI: does the value clear the draw's bar?  thr = bar + xi; a NaN clears nothing
GPSO_ACQ_HD inline bool mc_clears(double v, double thr) { return v > thr; }
GPSO_ACQ_HD inline double mc_threshold(double bar, double xi) { return bar + xi; }

// gain of the column col[s * ld], s < S, under QEI: x[s] = mc_margin(cleared[s], xi)
GPSO_ACQ_HD inline __attribute__((always_inline)) double mc_gain_qei(const double* col, int64_t ld, const double* bar, const double* x, int s_n) {
  double sum = 0.0;
#pragma unroll 8
  for (int s = 0; s < s_n; ++s) sum = sum + mc_improvement(col[(int64_t)s * ld], bar[s], x[s]);
  return sum / (double)s_n;
}
// ... under QPI: thr[s] = mc_threshold(bar[s], xi), cleared[s] != 0 once a pick or a pending point has cleared it
GPSO_ACQ_HD inline __attribute__((always_inline)) double mc_gain_qpi(const double* col, int64_t ld, const double* thr, const int* cleared, int s_n) {
  int count = 0;
  bool nan = false;
#pragma unroll 8
  for (int s = 0; s < s_n; ++s) {
    const double v = col[(int64_t)s * ld];
    nan = nan || v != v;
    if (!cleared[s] && mc_clears(v, thr[s])) ++count;
  }
  return nan ? __builtin_nan("") : (double)count / (double)s_n;
}

// what a round does with the winner (gain g at row p >= 0) of its arg-max: 0 report it and go on, 1 report it and end, 2 end
// without reporting.  Round 0's pick is always reported; a later one only with a gain > 0; a NaN is reported and ends
GPSO_ACQ_HD inline int mc_verdict(int round, double g) {
  if (g != g) return 1;
  if (round > 0 && !(g > 0.0)) return 2;
  return 0;
}

// NULL when the record and the bars are usable, else what is wrong (both entry points)
inline const char* mc_refusal(int kind, double xi, double incumbent, const double* incumbent_s, int64_t s_n) {
  if (kind != kMcQei && kind != kMcQpi) return "unknown kind (GPSO_MC_QEI, GPSO_MC_QPI)";
  if (xi != xi) return "xi is NaN";
  if (incumbent_s) {
    for (int64_t s = 0; s < s_n; ++s)
      if (incumbent_s[s] != incumbent_s[s]) return "an incumbent_s entry is NaN";
  } else if (incumbent != incumbent) {
    return "incumbent is NaN";
  }
  return nullptr;
}

// gpso_paths_batch_host (mcbatch.hip: built without contraction, like the kernels).  V [S][ld], rows 0 .. m - 1 the candidates,
// m .. m + b - 1 the pending columns; bar0 [S] the initial bars
int mc_batch_host(int kind, double xi, const double* V, int64_t ld, int s_n, int64_t m, int b, const double* bar0, int q, int64_t* idx,
                  double* gain, double* batch_value, int* n_picked, double* gain0);

}  // namespace gpso
