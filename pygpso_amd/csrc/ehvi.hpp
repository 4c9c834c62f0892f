// Bi-objective search: the exact expected hypervolume improvement of the pair (objective, one member of
// the constraint set) over a given Pareto front, weighted or gated by the probability of feasibility of the REMAINING members.
// This header holds the fold -- what turns one leaf's two objective columns (mean, var), the other members' columns and the
// success member's into the EHVI, logpof and the value the arg-max ranks by -- as ONE text for the device (ehvi.hip:
// ehvi_fold_kernel) and the host (gpso_ehvi_fold_host), and the launch record of ehvi.hip.  Maximisation.
//
//   front (a_k, b_k), k = 1 .. P <= 63: a strictly ascending, b strictly descending, every point strictly above (r1, r2)
//   a_0 = r1, a_{P+1} = +inf;  strip heights h_k = b_{k+1} (k < P), h_P = r2
//   Y_i ~ N(mu_i, s_i^2) independent; s_i^2 = max(var_i - noise_i, 0) (latent) or max(var_i, 0)
//   g(x) = E[(Y1 - x)+] = s1 H((mu1 - x) / s1),  e_k = E[(Y2 - h_k)+],  H(z) = phi(z) + z Phi(z);  s = 0: max(mu - x, 0)
//   EHVI = sum_{k=0..P} (g(a_k) - g(a_{k+1})) e_k,   g(+inf) = 0
// H is ehvi_h: the three pieces of acq_h (the body; acq_mills_p for -10 < z < -1; the far-tail series beyond) built from the
// written-out acq_exp / acq_erfc alone, so that a device value has its host twin's bits.  The z of a difference keeps both
// roundings (acq_z_diff).  The sum has a FIXED order: the P + 1 terms sit in slots 0 .. P of 64, the rest are +0.0, and for
// w = 32, 16, 8, 4, 2, 1: slot[i] += slot[i + w] (i < w); slot 0 is the EHVI.  The device runs the tree as six shuffle-down
// steps over the lanes of a wave, the host over an array.
//   a NaN mean or variance of either objective: NaN.  Otherwise a mean of -inf (either): +0.0; else a mean of +inf: +inf;
//   a variance that is not finite: NaN
//   logpof = sum over the members OTHER than objective 2 of con_log_pof_term, index order, from its first term; then
//            success_log_prob last where a success member is resident; no term at all: +0.0
//   no cspec: value = EHVI.   weight: EHVI acq_exp(logpof), -inf where logpof < log_pof_min.   gate: EHVI's own bits where
//   logpof >= log_pof_min, else -inf; log_pof_min = -inf: no gate.  The NaN rules are constrained_value_leaf's
#pragma once
#include <cstdint>

#include "constraints.hpp"

#ifndef GPSO_EHVI_FRONT_MAX
#define GPSO_EHVI_FRONT_MAX 63
#endif

namespace gpso {

constexpr int kEhviFrontMax = GPSO_EHVI_FRONT_MAX;
constexpr int kEhviSlots = kEhviFrontMax + 1;  // the strips of a front of 63 points: the lanes of a wave

// H(z + zl) = phi + z Phi
GPSO_ACQ_HD inline double ehvi_h(double z, double zl) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (z >= kAcqMidTail) {
    const double phi = kAcqInvSqrt2Pi * acq_exp_mhalf_sq_d(z, zl);
    const double Phi = acq_ncdf_d(z, zl);
    return fma(z, Phi, phi) + zl * Phi;
  }
  const double t = -z, tl = -zl;
  double hi, lo;
  acq_square(t, tl, &hi, &lo);
  const double e = acq_exp_mhalf_d(hi, lo);
  if (!(e > 0.0)) return 0.0;  // (phi has underflowed: H < phi)
  double q;  // H = phi(t) q
  if (z > kAcqFarTail) {
    q = acq_mills_p(t, tl) / (hi + lo);  // q = 1 - T R(T) = p / T^2, without the subtraction
  } else {
    const double r = (1.0 / hi) * (1.0 - lo / hi);  // 1 / (t + tl)^2
    double term = r;
    q = r;
    for (int k = 1; k < 48; ++k) {
      term *= -(double)(2 * k + 1) * r;
      q += term;
      if (!(fabs(term) > 1e-17 * q)) break;
    }
  }
  return (kAcqInvSqrt2Pi * e) * q;
}

// E[(Y - x)+] under Y ~ N(mean, s2), s = sqrt(s2); mean, s2 and x finite
GPSO_ACQ_HD inline double ehvi_excess(double mean, double s2, double s, double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (s == 0.0) {
    const double d = mean - x;
    return d > 0.0 ? d : 0.0;
  }
  double z, zl;
  acq_z_diff(mean, x, s2, s, &z, &zl);
  return s * ehvi_h(z, zl);
}

// what a leaf's strips share: the two objectives' means and the standard deviations the strips read; or the value the
// leaf has without any strip (`decided`)
struct EhviLeaf {
  double m1, v1, s1, m2, v2, s2;
  double early;
  bool decided;
};

GPSO_ACQ_HD inline EhviLeaf ehvi_leaf(int latent, double mean1, double var1, double noise1, double mean2, double var2, double noise2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  EhviLeaf l;
  l.m1 = mean1; l.m2 = mean2;
  double a = latent ? var1 - noise1 : var1, b = latent ? var2 - noise2 : var2;
  a = a > 0.0 ? a : (a != a ? a : 0.0);
  b = b > 0.0 ? b : (b != b ? b : 0.0);
  l.v1 = a; l.v2 = b;
  l.s1 = sqrt(a); l.s2 = sqrt(b);
  const double inf = __builtin_inf();
  l.decided = true;
  if (mean1 != mean1 || mean2 != mean2 || var1 != var1 || var2 != var2 || a != a || b != b) l.early = __builtin_nan("");
  else if (mean1 == -inf || mean2 == -inf) l.early = 0.0;
  else if (mean1 == inf || mean2 == inf) l.early = inf;
  else if (a == inf || b == inf) l.early = __builtin_nan("");
  else { l.early = 0.0; l.decided = false; }
  return l;
}

// strip k's two expectations: g(a_k) and e_k.  xa[k] = a_k (xa[0] = r1), xh[k] = h_k
GPSO_ACQ_HD inline double ehvi_strip_g(const EhviLeaf& l, double a) { return ehvi_excess(l.m1, l.v1, l.s1, a); }
GPSO_ACQ_HD inline double ehvi_strip_e(const EhviLeaf& l, double h) { return ehvi_excess(l.m2, l.v2, l.s2, h); }
// ... and its term, g_next = g(a_{k+1}) (0 for the last strip)
GPSO_ACQ_HD inline double ehvi_strip_term(double g, double g_next, double e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (g - g_next) * e;
}

// the strips of a front: xa / xh [kEhviSlots], slots above p are 0 and are not read
inline void ehvi_strips(int p, const double* front, const double* ref, double* xa, double* xh) {
  for (int k = 0; k < kEhviSlots; ++k) xa[k] = xh[k] = 0.0;
  xa[0] = ref[0];
  for (int k = 1; k <= p; ++k) xa[k] = front[2 * (k - 1)];
  for (int k = 0; k < p; ++k) xh[k] = front[2 * k + 1];
  xh[p] = ref[1];
}

// what a call asks for, behind its record's checks (api.hip): objective 2's index in the set, the strips, how logpof enters
struct EhviSpec {
  int member = 0, latent = 1, p = 0;
  double xa[kEhviSlots] = {};
  double xh[kEhviSlots] = {};
  bool has_con = false;
  ConSpec con;
};

// why a front is refused (NULL: it is served)
inline const char* ehvi_front_refusal(int p, const double* front, const double* ref) {
  if (p < 0 || p > kEhviFrontMax) return "p outside [0, 63] (GPSO_EHVI_FRONT_MAX)";
  if (p > 0 && front == nullptr) return "front must not be NULL where p > 0";
  if (!(ref[0] - ref[0] == 0.0) || !(ref[1] - ref[1] == 0.0)) return "the reference point must be finite";
  for (int k = 0; k < 2 * p; ++k)
    if (!(front[k] - front[k] == 0.0)) return "every front entry must be finite";
  for (int k = 0; k < p; ++k) {
    if (!(front[2 * k] > ref[0]) || !(front[2 * k + 1] > ref[1])) return "every front point must lie strictly above the reference point in both objectives";
    if (k > 0 && !(front[2 * k] > front[2 * k - 2])) return "the front's first objective must be strictly ascending";
    if (k > 0 && !(front[2 * k + 1] < front[2 * k - 1])) return "the front's second objective must be strictly descending";
  }
  return nullptr;
}

// the fixed order of the sum over an array of kEhviSlots terms (the device: six shuffle-down steps)
GPSO_ACQ_HD inline double ehvi_tree(double* slot) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int w = kEhviSlots / 2; w >= 1; w >>= 1)
    for (int i = 0; i < w; ++i) slot[i] += slot[i + w];
  return slot[0];
}

// the EHVI of one leaf, serially (the host; the device spreads the strips over lanes: ehvi.hip)
inline double ehvi_leaf_serial(const EhviLeaf& l, int p, const double* xa, const double* xh) {
  if (l.decided) return l.early;
  double g[kEhviSlots + 1], slot[kEhviSlots];
  for (int k = 0; k <= p; ++k) g[k] = ehvi_strip_g(l, xa[k]);
  g[p + 1] = 0.0;
  for (int k = 0; k < kEhviSlots; ++k) slot[k] = k <= p ? ehvi_strip_term(g[k], g[k + 1], ehvi_strip_e(l, xh[k])) : 0.0;
  return ehvi_tree(slot);
}

// what the record makes of a leaf's EHVI and logpof: the value the arg-max ranks by (has_con false: the EHVI itself)
GPSO_ACQ_HD inline double ehvi_value_leaf(bool has_con, const ConSpec& c, double ehvi, double lp) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!has_con) return ehvi;
  const double ninf = -__builtin_inf();
  if (c.mode == GPSO_CON_GATE) {
    if (c.log_pof_min == ninf) return ehvi;
    if (lp != lp) return lp;
    return lp >= c.log_pof_min ? ehvi : ninf;
  }
  if (lp < c.log_pof_min) return ninf;
  if (lp != lp) return lp;
  return ehvi * acq_exp(lp);
}

// host loop of gpso_ehvi_fold_host (ehvi.hip: built without contraction, like the device fold).  omean / ovar [k][m]: the
// members other than objective 2; smean / svar [m] nullable: the success member's latent columns
void ehvi_fold_host(int latent, int p, const double* xa, const double* xh, bool has_con, const ConSpec& c, const double* mean1,
                    const double* var1, double noise1, const double* mean2, const double* var2, double noise2, const double* omean,
                    const double* ovar, const double* onoise, const double* thr, const double* sense, int k, long long m,
                    const double* smean, const double* svar, double* value, double* logpof);

#if defined(__HIPCC__)
// ---- ehvi.hip ----------------------------------------------------------------------------------------------------------
// what the fold kernel reads: the strips (1 KB of kernel arguments), the columns [1 + J (+ 1)][ld] of the constrained calls'
// stage 1, and of the set per OTHER member its index, threshold and sense
struct EhviFoldLaunch {
  double xa[kEhviSlots] = {};
  double xh[kEhviSlots] = {};
  int p = 0, latent = 1, has_con = 0;
  ConSpec con;
  const double* obj_mean = nullptr;   // [m]
  const double* obj_var = nullptr;
  const double* obj_hyper = nullptr;  // the objective's hyper block (slot 5: noise variance)
  const double* cmean = nullptr;      // [J][ld]
  const double* cvar = nullptr;
  const double* chyper = nullptr;     // [J][hyper_stride]
  int64_t hyper_stride = 0;
  int member = 0;                     // objective 2's index in the set
  int nother = 0;                     // J - 1
  int oidx[kConstraintsMax] = {};     // the other members' indices, ascending
  double othr[kConstraintsMax] = {};
  double osense[kConstraintsMax] = {};
  const double* smean = nullptr;      // [m] the success member's latent columns; NULL: none
  const double* svar = nullptr;
  int64_t ld = 0, m = 0;
  double* value = nullptr;   // [m]
  double* logpof = nullptr;  // [m]
};
// a wave per leaf: lane k owns strip k, lane i < J - 1 (+ 1) a logpof term
void launch_ehvi_fold(hipStream_t st, const EhviFoldLaunch& g);
#endif

}  // namespace gpso
