// Acquisition maps: (mean, s^2) of one leaf -> the value the arg-max ranks by.  One restatement for the device epilogues
// (predict.hip: finalize_leaf, leaf_finalize_kernel) and for the host (gpso_acq_eval_host), in double, built from erfc,
// exp, log, sqrt and fma only -- what host libm and the device library both have.  DESIGN.md section 7l.
//
//   d = mean - incumbent - xi,  s = sqrt(max(s^2, 0)),  z = d / s          (maximisation)
//   UCB_VAR  mean + varsigma * s^2        (the reference's rule, gpso/gp_surrogate.py:326; product and sum rounded apart)
//   UCB_STD  mean + varsigma * s          (sqrt correctly rounded; product and sum rounded apart: numpy's bits)
//   EI       s * h(z),  h(z) = phi(z) + z Phi(z)
//   LOGEI    log EI, finite where EI underflows
//   PI       Phi(z)
//   s == 0:  EI = max(d, 0), LOGEI = log max(d, 0), PI = 1 | 1/2 | 0 by the sign of d.  A NaN mean or s^2: NaN.
//
// h(z) in three pieces:  z >= -1: phi + z Phi as written (the cancellation costs less than two bits);  -10 < z < -1:
// phi(z) * (1 + z Phi(z) / phi(z)) with Phi through erfc -- the bracket stays O(1/z^2) and phi's exponent is added in the
// log instead of underflowing;  z <= -10: phi(z) * sum_k (-1)^k (2k+1)!! / z^(2k+2), whose terms fall below 1e-17 of the
// sum before they start to grow.  z is carried as a pair (z, zl): the remainders of the square root and of the division
// are kept, because Phi and phi amplify a relative error of z by z^2 -- 1444 half-ulps at z = -38, where float64 EI dies.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GPSO_ACQ_HD __host__ __device__
#else
#define GPSO_ACQ_HD
#endif

#ifndef GPSO_ACQ_UCB_VAR
#define GPSO_ACQ_UCB_VAR 0
#define GPSO_ACQ_UCB_STD 1
#define GPSO_ACQ_EI 2
#define GPSO_ACQ_LOGEI 3
#define GPSO_ACQ_PI 4
#endif

namespace gpso {

// what a call ranks by; a plain varsigma converts to the reference's rule
struct AcqSpec {
  int kind = GPSO_ACQ_UCB_VAR;
  int latent = 0;
  double varsigma = 0, incumbent = 0, xi = 0;
  AcqSpec() = default;
  GPSO_ACQ_HD AcqSpec(double vs) : varsigma(vs) {}
  GPSO_ACQ_HD AcqSpec(int k, int l, double vs, double inc, double x) : kind(k), latent(l), varsigma(vs), incumbent(inc), xi(x) {}
};

constexpr double kAcqInvSqrt2Hi = 0.7071067811865476, kAcqInvSqrt2Lo = -4.833646656726457e-17;
constexpr double kAcqInvSqrt2Pi = 0.3989422804014327;
constexpr double kAcqHalfLog2Pi = 0.9189385332046728;
constexpr double kAcqMidTail = -1.0, kAcqFarTail = -10.0;  // where the pieces of h(z) join

// m + a * b with the product rounded on its own (numpy's two roundings), whatever the translation unit's contraction mode
GPSO_ACQ_HD inline double acq_mul_then_add(double m, double a, double b) {
#if defined(__clang__)  // (the library's compiler; another one that includes this for AcqSpec alone does not call the maps)
#pragma clang fp contract(off)
#endif
  const double prod = a * b;
  return m + prod;
}

// (t + tl)^2 as hi + lo
GPSO_ACQ_HD inline void acq_square(double t, double tl, double* hi, double* lo) {
  *hi = t * t;
  *lo = *hi < 1e300 ? fma(t, t, -*hi) + 2.0 * t * tl : 0.0;
}

// exp(-(hi + lo) / 2): the low part would cost |t|^2 ulps inside the exponential
GPSO_ACQ_HD inline double acq_exp_mhalf(double hi, double lo) {
  const double e = exp(-0.5 * hi);
  return e > 0.0 ? e * (1.0 - 0.5 * lo) : 0.0;
}

GPSO_ACQ_HD inline double acq_exp_mhalf_sq(double t, double tl) {
  double hi, lo;
  acq_square(t, tl, &hi, &lo);
  return acq_exp_mhalf(hi, lo);
}

// Phi(z + zl) = erfc(-(z + zl) / sqrt 2) / 2; the argument's low part enters through erfc'(x) / erfc(x) -> -2x
GPSO_ACQ_HD inline double acq_ncdf(double z, double zl) {
  const double x = -z * kAcqInvSqrt2Hi;
  double c = 0.5 * erfc(x);
  if (x > 1.0) {
    const double xl = fma(-z, kAcqInvSqrt2Hi, -x) - z * kAcqInvSqrt2Lo - zl * kAcqInvSqrt2Hi;
    c *= 1.0 - 2.0 * x * xl;
  }
  return c;
}

// s > 0: z = d / s as (z, zl) with s = sqrt(s2) -- both remainders kept
GPSO_ACQ_HD inline void acq_z(double d, double s2, double s, double* z, double* zl) {
  const double sl = fma(-s, s, s2) / (2.0 * s);  // sqrt(s2) = s + sl
  *z = d / s;
  const double r = (fma(-*z, s, d) - *z * sl) / s;
  *zl = (fabs(*z) <= 1e100 && r == r) ? r : 0.0;
}

// h(z + zl) = phi + z Phi, or its logarithm
GPSO_ACQ_HD inline double acq_h(double z, double zl, bool want_log) {
  if (z >= kAcqMidTail) {
    const double phi = kAcqInvSqrt2Pi * acq_exp_mhalf_sq(z, zl);
    const double Phi = acq_ncdf(z, zl);
    const double h = fma(z, Phi, phi) + zl * Phi;
    return want_log ? log(h) : h;
  }
  const double t = -z, tl = -zl;
  double hi, lo;
  acq_square(t, tl, &hi, &lo);
  double q;  // h = phi(t) * q
  if (z > kAcqFarTail) {
    const double e = acq_exp_mhalf(hi, lo);
    const double R = acq_ncdf(z, zl) / (kAcqInvSqrt2Pi * e);  // Mills' ratio Phi(-t) / phi(t)
    q = fma(-t, R, 1.0) - tl * R;
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
  if (want_log) return -0.5 * hi + ((log(q) - kAcqHalfLog2Pi) - 0.5 * lo);
  return kAcqInvSqrt2Pi * acq_exp_mhalf(hi, lo) * q;
}

// one leaf.  s2 is the variance the kind reads (predictive, or latent: the caller picks), clamped at 0 here
GPSO_ACQ_HD inline double acq_value(const AcqSpec& a, double mean, double s2) {
  if (a.kind == GPSO_ACQ_UCB_VAR) return acq_mul_then_add(mean, a.varsigma, s2);
  const double nan = __builtin_nan("");
  s2 = s2 < 0.0 ? 0.0 : s2;  // (a NaN stays a NaN)
  const double s = sqrt(s2);
  if (a.kind == GPSO_ACQ_UCB_STD) return acq_mul_then_add(mean, a.varsigma, s);
  if (a.kind != GPSO_ACQ_EI && a.kind != GPSO_ACQ_LOGEI && a.kind != GPSO_ACQ_PI) return nan;
  if (mean != mean || s2 != s2) return nan;
  const double d = (mean - a.incumbent) - a.xi;
  if (s == 0.0) {
    if (a.kind == GPSO_ACQ_PI) return d > 0.0 ? 1.0 : d < 0.0 ? 0.0 : 0.5;
    const double dp = d > 0.0 ? d : 0.0;
    return a.kind == GPSO_ACQ_EI ? dp : log(dp);
  }
  double z, zl;
  acq_z(d, s2, s, &z, &zl);
  if (a.kind == GPSO_ACQ_PI) return acq_ncdf(z, zl);
  if (a.kind == GPSO_ACQ_EI) return s * acq_h(z, zl, false);
  return log(s) + acq_h(z, zl, true);
}

// host loop of gpso_acq_eval_host (predict.hip: built without contraction, like the device epilogues)
void acq_eval_host(const AcqSpec& a, const double* mean, const double* var, double noise, long long n, double* out);

}  // namespace gpso
