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
//   MES      (1/K) sum_k t(g_k),  g_k = (y*_k - mean) / s,  t(g) = g phi(g) / (2 Phi(g)) - log Phi(g)     (section 7p)
//   s == 0:  EI = max(d, 0), LOGEI = log max(d, 0), PI = 1 | 1/2 | 0 by the sign of d, MES = 0.  A NaN mean or s^2: NaN.
//
// h(z) in three pieces:  z >= -1: phi + z Phi as written (the cancellation costs less than two bits);  -10 < z < -1:
// phi(z) * (1 + z Phi(z) / phi(z)) with Phi through erfc -- the bracket stays O(1/z^2) and phi's exponent is added in the
// log instead of underflowing;  z <= -10: phi(z) * sum_k (-1)^k (2k+1)!! / z^(2k+2), whose terms fall below 1e-17 of the
// sum before they start to grow.  z is carried as a pair (z, zl): the remainders of the square root and of the division
// are kept, because Phi and phi amplify a relative error of z by z^2 -- 1444 half-ulps at z = -38, where float64 EI dies.
//
// t(g) in the same three pieces (T = -g):  g >= -1: g phi / (2 Phi) - log Phi as written, -log Phi = -log1p(-Phi(-g)) for
// g > 0;  -10 < g < -1: Mills' ratio R = Phi(-T) / phi(T) and q = 1 - T R give -T^2 q / (2 (1 - q)) + log sqrt(2 pi) - log R
// -- the T^2 / 2 of both halves, each of which grows like T^2 / 2 while t grows like log T, has cancelled on paper; q itself
// comes as p / T^2 from a table of p = T^2 q (acq_mills_p) and R as (1 - q) / T, not from the subtraction 1 - T R;
// g <= -10: R = m / T, m = 1 + m1, m1 = sum_k (-1)^k (2k-1)!! / T^(2k) give (m1 T^2) / (2 m) + log sqrt(2 pi) + log T - log1p(m1).
// t and log Phi (acq_log_ncdf) call acq_exp / acq_log / acq_log1p / acq_erfc below, not the math library: see there.
// The K maxima y*_k are no part of the record: they arrive as a pointer and a count (device memory in a kernel, host
// memory in the host twins), are read in index order, and the sum is divided by K once.
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
#ifndef GPSO_ACQ_MES
#define GPSO_ACQ_MES 5
#endif

namespace gpso {

// what a call ranks by; a plain varsigma converts to the reference's rule
struct AcqSpec {
  int kind = GPSO_ACQ_UCB_VAR;
  int latent = 0;
  double varsigma = 0, incumbent = 0, xi = 0;
  const double* ystar = nullptr;  // GPSO_ACQ_MES: the K sampled maxima, in the memory of whoever evaluates the map
  int nystar = 0;
  AcqSpec() = default;
  GPSO_ACQ_HD AcqSpec(double vs) : varsigma(vs) {}
  GPSO_ACQ_HD AcqSpec(int k, int l, double vs, double inc, double x, const double* ys = nullptr, int nys = 0)
      : kind(k), latent(l), varsigma(vs), incumbent(inc), xi(x), ystar(ys), nystar(nys) {}
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

// ---- exp, log, log1p and erfc written out (GPSO_ACQ_MES and gpso_max_logcdf only) --------------------------------------
// A device value of these two has the bits of its host twin.  The host's and the device's math libraries agree on sqrt,
// fma, + - * / (all correctly rounded) and on nothing else: their erfc / exp / log / log1p differ in the last place on
// about one argument in ten.  So the maps of section 7p do not call them: the four functions below are built from
// + - * /, fma and the exponent bits alone, contraction off, and give the same bits wherever they are compiled.  The
// kinds of section 7l keep the library calls they had, and their bits.
//   acq_exp: x = k ln 2 + r, |r| <= ln 2 / 2; exp r = 1 + 2 r / (2 - c(r)) with the degree-5 rational remainder of FreeBSD's
//     e_exp.c (its constants; < 1 ulp).   acq_log: x = 2^k (1 + f), sqrt 1/2 < 1 + f < sqrt 2, s = f / (2 + f),
//     log(1 + f) = f - f^2/2 + s (f^2/2 + R(s^2)) with the degree-14 R of e_log.c (< 1 ulp).   acq_log1p: log(u) x / (u - 1),
//     u = 1 + x (Kahan's correction of the rounding of u).   acq_erfc, x >= 0: t = 2 / (2 + x), erfc x = t exp(-x^2) h(t)
//     with h = erfc(x) exp(x^2) / t in 32 Chebyshev coefficients over t in [0.045, 1] (x <= 42; fitted at 50 digits, the
//     first neglected coefficient is 1e-21 of h), summed by Clenshaw's recurrence; x^2 enters exp as hi + lo.  x < 0: 2 - erfc(-x).
//
// acq_exp and acq_log follow FreeBSD msun's e_exp.c and e_log.c (argument reduction, polynomial, constants), which carry:
//   ====================================================
//   Copyright (C) 1993 by Sun Microsystems, Inc. All rights reserved.  (e_exp.c: Copyright (C) 2004 by Sun Microsystems, Inc.)
//
//   Developed at SunSoft, a Sun Microsystems, Inc. business.
//   Permission to use, copy, modify, and distribute this
//   software is freely granted, provided that this notice
//   is preserved.
//   ====================================================
GPSO_ACQ_HD inline double acq_pow2(int k) { return __builtin_bit_cast(double, (long long)(k + 1023) << 52); }  // -1022 <= k <= 1023

GPSO_ACQ_HD inline double acq_exp(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (x != x) return x;
  if (x > 709.0) return __builtin_inf();  // (no caller comes near)
  if (x < -745.2) return 0.0;
  const int k = (int)(1.44269504088896338700e+00 * x + (x < 0.0 ? -0.5 : 0.5));
  const double hi = x - (double)k * 6.93147180369123816490e-01, lo = (double)k * 1.90821492927058770002e-10;
  const double r = hi - lo, t = r * r;
  const double c = r - t * (1.66666666666666019037e-01 + t * (-2.77777777770155933842e-03 + t * (6.61375632143793436117e-05 +
                       t * (-1.65339022054652515390e-06 + t * 4.13813679705723846039e-08))));
  const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
  if (k >= -1021) return y * acq_pow2(k);
  return (y * acq_pow2(k + 1000)) * acq_pow2(-1000);
}

GPSO_ACQ_HD inline double acq_log(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (x != x || x < 0.0) return __builtin_nan("");
  if (x == 0.0) return -__builtin_inf();
  if (x - x != 0.0) return x;  // +inf
  int k = 0;
  if (x < 2.2250738585072014e-308) {
    x *= 18014398509481984.0;  // 2^54
    k = -54;
  }
  long long bits = __builtin_bit_cast(long long, x);
  int hx = (int)(bits >> 32);
  k += (hx >> 20) - 1023;
  hx &= 0x000fffff;
  const int i = (hx + 0x95f64) & 0x100000;  // 1 + f in [sqrt 1/2, sqrt 2)
  bits = (bits & 0xffffffffLL) | ((long long)(hx | (i ^ 0x3ff00000)) << 32);
  k += i >> 20;
  const double f = __builtin_bit_cast(double, bits) - 1.0, dk = (double)k;
  const double s = f / (2.0 + f), z = s * s, w = z * z;
  const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
  const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 +
                         w * 1.479819860511658591e-01)));
  const double R = t2 + t1, hfsq = 0.5 * f * f;
  if (k == 0) return f - (hfsq - s * (hfsq + R));
  return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}

GPSO_ACQ_HD inline double acq_log1p(double x) {  // x > -1
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double u = 1.0 + x;
  if (u == 1.0) return x;
  return acq_log(u) * (x / (u - 1.0));
}

// c_0 / 2 + sum_{j < n} c_j T_j(u), Clenshaw's recurrence (the tables: tools/fit_acq_tables.py prints them, --check compares)
GPSO_ACQ_HD inline double acq_clenshaw(const double* c, int n, double u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double u2 = 2.0 * u;
  double b1 = 0.0, b2 = 0.0;
  for (int j = n - 1; j >= 1; --j) {
    const double b0 = (u2 * b1 - b2) + c[j];
    b2 = b1;
    b1 = b0;
  }
  return (u * b1 - b2) + 0.5 * c[0];
}

// q = 1 - T R(T) for 1 <= T <= 10, R = Phi(-T) / phi(T) Mills' ratio, WITHOUT the subtraction: p = T^2 q runs from 0.34 to
// 0.97 and is a table of its own in w = 1 / T, so q = p / T^2 keeps p's two ulps where 1 - T R loses a hundred times R's at
// T = 10.  Returns p at T = t + tl.
GPSO_ACQ_HD inline double acq_mills_p(double t, double tl) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  constexpr double kAcqCheb_mills[44] = {
      1.2590582095398533, -0.32343454401175287, 0.034232868735422674, 0.008168984092335197,
      -0.005614835996220959, 0.0017388309006036748, -0.0003173458726944125, -3.726855118921337e-07,
      2.797895497600536e-05, -1.3661749548116285e-05, 4.237449871648268e-06, -8.587184393834801e-07,
      3.058704611828805e-08, 7.078158135317123e-08, -4.16474512639731e-08, 1.550742273581508e-08,
      -4.1987985085999515e-09, 6.839545853586303e-10, 7.425788182949466e-11, -1.2030614803137767e-10,
      6.210318508488602e-11, -2.2862374867368012e-11, 6.389983543413183e-12, -1.142684805242962e-12,
      -7.144233753875302e-14, 1.8236773813298208e-13, -1.039377644952807e-13, 4.2137739480757257e-14,
      -1.3435981809434366e-14, 3.171064721315885e-15, -3.075709215449877e-16, -2.091610588322529e-16,
      1.7388325545988661e-16, -8.50733769730424e-17, 3.2464450532274104e-17, -9.972406409970374e-18,
      2.2335976915256967e-18, -1.409657394662482e-19, -2.0634643596810453e-19, 1.5605073414951393e-19,
      -7.60711866352171e-20, 2.96468291418711e-20, -9.495234488554746e-21, 2.3195930245520883e-21};
  const double w = (1.0 / t) * (1.0 - tl / t);
  return acq_clenshaw(kAcqCheb_mills, 44, (2.0 * w - 1.1) / 0.9);
}

GPSO_ACQ_HD inline double acq_erfc(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  constexpr double kAcqCheb_erfc[32] = {
      1.1761823897038282, 0.3495535717869262, 0.06052977235123217, 0.00290652989230148,
      -0.0009951844275379142, -0.00011592504883760251, 2.797601114802476e-05, 3.2210115897157735e-06,
      -1.1582093851762574e-06, -4.5598757353307946e-08, 5.2595691016857935e-08, -3.6802470813456498e-09,
      -2.0056674770803057e-09, 4.646329075317167e-10, 3.06543726495546e-11, -3.003876346669226e-11,
      3.773017728489039e-12, 9.893738075053656e-13, -4.2620186582036544e-13, 3.184770933190165e-14,
      1.9439435850401637e-14, -6.62135564743152e-15, 3.443747401814401e-16, 3.5720474426818335e-16,
      -1.1710888163531137e-16, 6.595769880282387e-18, 6.521938906174569e-18, -2.3359758943704535e-18,
      1.9967444593371766e-19, 1.158963749005648e-19, -5.0616667790251106e-20, 6.785899304808698e-21};
  if (x != x) return x;
  const double a = x < 0.0 ? -x : x;
  double r = 0.0;
  if (a < 40.0) {  // (beyond: exp(-a^2) is 0 long since)
    const double t = 2.0 / (2.0 + a);
    const double h = acq_clenshaw(kAcqCheb_erfc, 32, (2.0 * t - 1.045) / 0.955);
    const double hi = a * a, lo = fma(a, a, -hi);
    const double e = acq_exp(-hi);
    r = e > 0.0 ? (t * h) * (e * (1.0 - lo)) : 0.0;
  }
  return x < 0.0 ? 2.0 - r : r;
}

// acq_exp_mhalf, acq_exp_mhalf_sq and acq_ncdf over the functions above
GPSO_ACQ_HD inline double acq_exp_mhalf_d(double hi, double lo) {
  const double e = acq_exp(-0.5 * hi);
  return e > 0.0 ? e * (1.0 - 0.5 * lo) : 0.0;
}

GPSO_ACQ_HD inline double acq_exp_mhalf_sq_d(double t, double tl) {
  double hi, lo;
  acq_square(t, tl, &hi, &lo);
  return acq_exp_mhalf_d(hi, lo);
}

GPSO_ACQ_HD inline double acq_ncdf_d(double z, double zl) {
  const double x = -z * kAcqInvSqrt2Hi;
  double c = 0.5 * acq_erfc(x);
  if (x > 1.0) {
    const double xl = fma(-z, kAcqInvSqrt2Hi, -x) - z * kAcqInvSqrt2Lo - zl * kAcqInvSqrt2Hi;
    c *= 1.0 - 2.0 * x * xl;
  }
  return c;
}

// z = (y - mean) / s with the rounding of the difference kept as well: log Phi and t lose z^2 ulps to an ulp of z
GPSO_ACQ_HD inline void acq_z_diff(double y, double mean, double s2, double s, double* z, double* zl) {
  const double d = y - mean, bb = d - y;
  const double dl = (y - (d - bb)) + (-mean - bb);  // y - mean = d + dl exactly
  acq_z(d, s2, s, z, zl);
  const double r = dl / s;
  if (fabs(*z) <= 1e100 && r - r == 0.0) *zl += r;
}

// log1p(m1) + ... of the far tail: m1 = sum_{k>=1} (-1)^k (2k-1)!! r^k with r = 1 / T^2, stopped where acq_h stops
GPSO_ACQ_HD inline double acq_mills_m1(double r) {
  double term = 1.0, m1 = 0.0;
  for (int k = 1; k < 48; ++k) {
    term *= -(double)(2 * k - 1) * r;
    m1 += term;
    if (!(fabs(term) > 1e-17 * fabs(m1))) break;
  }
  return m1;
}

// log Phi(z + zl), finite down to where z^2 overflows: the pieces of acq_h
GPSO_ACQ_HD inline double acq_log_ncdf(double z, double zl) {
  if (z > 0.0) return acq_log1p(-acq_ncdf_d(-z, -zl));
  if (z >= kAcqMidTail) return acq_log(acq_ncdf_d(z, zl));
  const double t = -z, tl = -zl;
  double hi, lo;
  acq_square(t, tl, &hi, &lo);
  if (z > kAcqFarTail) {  // R = (1 - q) / T
    const double q = acq_mills_p(t, tl) / (hi + lo);
    return -0.5 * hi + (((acq_log1p(-q) - (acq_log(t) + tl / t)) - kAcqHalfLog2Pi) - 0.5 * lo);
  }
  if (!(hi < 1e300)) return -0.5 * hi;
  const double m1 = acq_mills_m1((1.0 / hi) * (1.0 - lo / hi));
  return -0.5 * hi + (((acq_log1p(m1) - (acq_log(t) + tl / t)) - kAcqHalfLog2Pi) - 0.5 * lo);
}

// t(g) = g phi(g) / (2 Phi(g)) - log Phi(g) at g = z + zl: what one sampled maximum adds to a leaf's MES value; >= 0
GPSO_ACQ_HD inline double acq_mes_term(double z, double zl) {
  if (z >= kAcqMidTail) {
    if (z > 40.0) return 0.0;  // (t < 1e-347; phi is 0 and an infinite z must not meet it)
    const double phi = kAcqInvSqrt2Pi * acq_exp_mhalf_sq_d(z, zl);
    const double Phi = acq_ncdf_d(z, zl);
    const double mlog = z > 0.0 ? -acq_log1p(-acq_ncdf_d(-z, -zl)) : -acq_log(Phi);
    return 0.5 * ((z * phi + zl * phi) / Phi) + mlog;
  }
  const double t = -z, tl = -zl;
  double hi, lo;
  acq_square(t, tl, &hi, &lo);
  const double logt = acq_log(t) + tl / t;
  if (z > kAcqFarTail) {  // -T^2 q / (2 (1 - q)) + log sqrt(2 pi) - log R with T^2 q = p and R = (1 - q) / T
    const double p = acq_mills_p(t, tl), q = p / (hi + lo);
    return -0.5 * p / (1.0 - q) + ((kAcqHalfLog2Pi + logt) - acq_log1p(-q));
  }
  if (!(hi < 1e300)) return (kAcqHalfLog2Pi - 0.5) + logt;
  const double r = (1.0 / hi) * (1.0 - lo / hi);  // 1 / (t + tl)^2
  const double m1 = acq_mills_m1(r);
  return 0.5 * (m1 / r) / (1.0 + m1) + ((kAcqHalfLog2Pi + logt) - acq_log1p(m1));
}

// GPSO_ACQ_MES of one leaf: the terms in index order, one division at the end
GPSO_ACQ_HD inline double acq_mes_value(const double* ystar, int k, double mean, double s2, double s) {
  if (s == 0.0) return 0.0;
  double sum = 0.0;
  for (int i = 0; i < k; ++i) {
    double z, zl;
    acq_z_diff(ystar[i], mean, s2, s, &z, &zl);
    sum += acq_mes_term(z, zl);
  }
  return sum / (double)k;
}

// one leaf.  s2 is the variance the kind reads (predictive, or latent: the caller picks), clamped at 0 here
// (WITH_MES false: an epilogue that is never handed GPSO_ACQ_MES does not carry its code)
template <bool WITH_MES = true>
GPSO_ACQ_HD inline double acq_value(const AcqSpec& a, double mean, double s2) {
  if (a.kind == GPSO_ACQ_UCB_VAR) return acq_mul_then_add(mean, a.varsigma, s2);
  const double nan = __builtin_nan("");
  s2 = s2 < 0.0 ? 0.0 : s2;  // (a NaN stays a NaN)
  const double s = sqrt(s2);
  if (a.kind == GPSO_ACQ_UCB_STD) return acq_mul_then_add(mean, a.varsigma, s);
  if (a.kind != GPSO_ACQ_EI && a.kind != GPSO_ACQ_LOGEI && a.kind != GPSO_ACQ_PI && !(WITH_MES && a.kind == GPSO_ACQ_MES)) return nan;
  if (mean != mean || s2 != s2) return nan;
  if (WITH_MES && a.kind == GPSO_ACQ_MES) return (a.ystar != nullptr && a.nystar > 0) ? acq_mes_value(a.ystar, a.nystar, mean, s2, s) : nan;
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
// gpso_acq_math_host (predict.hip): fn 0 acq_exp, 1 acq_log, 2 acq_log1p, 3 acq_erfc, 4 acq_mills_p; -1 for another fn
int acq_math_host(int fn, const double* x, long long n, double* out);
// host loop of gpso_max_logcdf_host (maxcdf.hip): sum over the rows without a NaN of log Phi((y_i - mean_j) / s_j), in row order
void max_logcdf_host(const double* mean, const double* var, long long m, double var_sub, const double* y, int g, double* logcdf,
                     long long* n_used);

}  // namespace gpso
