"""
Two restatements of max-value entropy search (pygpso_amd/csrc/acq.hpp: GPSO_ACQ_MES; csrc/maxcdf.hip), for the tests only:

* ``truth`` / ``truth_logcdf``        mpmath at 60 digits, evaluated on the float64 inputs exactly as they are
* ``restatement`` / ``restatement_logcdf``   float64 numpy / scipy: for the map a fresh writing of the three pieces of
  t(g) = g phi(g) / (2 Phi(g)) - log Phi(g)  (erfc, erfcx, log1p), for the sum ``math.fsum(scipy.special.log_ndtr(z))``

and the tolerance rule of tests/acq_oracle.py: the library stays within 8 x the restatement's own worst relative error
against truth on the grid below, floor 16 ulp.  The form built from ``scipy.special.log_ndtr`` is NOT the yardstick of the
map: it loses 5e4 ulp at g = -38, a tolerance derived from it would prove nothing.  For the sum the floor is
(16 + log2 m) ulp: m roundings of a sum of terms of one sign, on top of the terms' own error.

Errors are relative; below the normal range they are taken relative to the smallest normal number.
"""
import functools
import math
from fractions import Fraction

import mpmath as mp
import numpy as np
from scipy import special as sp

ULP = float(np.finfo(np.float64).eps)
GRID_G = (40.0, 12.0, 8.0, 3.0, 1.0, 0.5, 0.0, -0.5, -1.0, -1.0000001, -2.0, -5.0, -6.0, -9.999, -10.0, -12.0, -30.0, -38.0,
          -39.0, -1e2, -1e4, -1e6)
GRID_S = (1e-8, 1e-3, 1.0, 1e3)
_HALF_LOG_2PI = 0.9189385332046728

mp.mp.dps = 60


_SQRT2_MP = mp.sqrt(2)


def _log_ncdf_mp(g):
    """log Phi(g); above 0 through log1p of the upper tail, which 60 digits resolve no further than 1e-60 below 1."""
    if g > 0:
        return mp.log1p(-mp.erfc(g / _SQRT2_MP) / 2)
    return mp.log(mp.erfc(-g / _SQRT2_MP) / 2)


def _t_mp(g):
    phi = mp.exp(-g * g / 2) / mp.sqrt(2 * mp.pi)
    return g * phi / (2 * mp.exp(_log_ncdf_mp(g))) - _log_ncdf_mp(g)


def truth(ystar, mean, s2, s2_add=()):
    """mpmath MES values (mp.mpf, or mp.nan) for float64 arrays mean / s2 under the float64 maxima ``ystar``: the mean of
    t((y*_k - mean) / s).  ``s2_add``: float64 scalars or arrays added to s2 EXACTLY (the latent variance var - noise)."""
    ys = [mp.mpf(float(y)) for y in np.asarray(ystar, dtype=np.float64).reshape(-1)]
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    adds = [np.broadcast_to(np.asarray(a, dtype=np.float64), mean.shape) for a in s2_add]
    out = []
    for i, (m, v) in enumerate(zip(mean, np.asarray(s2, dtype=np.float64).reshape(-1))):
        if np.isnan(m) or np.isnan(v):
            out.append(mp.nan)
            continue
        m_, v_ = mp.mpf(float(m)), mp.mpf(float(v))
        for a in adds:
            v_ += mp.mpf(float(a[i]))
        v_ = max(v_, mp.mpf(0))
        if v_ == 0:
            out.append(mp.mpf(0))
            continue
        s = mp.sqrt(v_)
        out.append(sum(_t_mp((y - m_) / s) for y in ys) / len(ys))
    return out


def _t_np(g):
    """One term in float64: the three pieces, written fresh (scalar)."""
    g = np.float64(g)
    with np.errstate(all="ignore"):
        if g >= -1.0:
            if g > 40.0:
                return 0.0
            Phi = 0.5 * sp.erfc(-g / np.sqrt(2.0))
            g2 = g * g  # (and its rounding: at g = 12.000000000000002 half an ulp of 144 is 36 ulp of phi)
            g2l = float(Fraction(float(g)) ** 2 - Fraction(float(g2)))
            phi = np.exp(-0.5 * g2) * (1.0 - 0.5 * g2l) / np.sqrt(2.0 * np.pi)
            mlog = -np.log1p(-0.5 * sp.erfc(g / np.sqrt(2.0))) if g > 0 else -np.log(Phi)
            return float(0.5 * g * phi / Phi + mlog)
        t = -g
        if t < 10.0:
            R = np.sqrt(np.pi / 2.0) * sp.erfcx(t / np.sqrt(2.0))  # Mills' ratio
            q = 1.0 - t * R
            return float(-0.5 * t * t * q / (1.0 - q) + _HALF_LOG_2PI - np.log(R))
        r = 1.0 / (t * t)
        term, m1 = 1.0, 0.0
        for k in range(1, 48):
            term *= -(2 * k - 1) * r
            m1 += term
            if not abs(term) > 1e-17 * abs(m1):
                break
        return float(0.5 * (m1 / r) / (1.0 + m1) + _HALF_LOG_2PI + np.log(t) - np.log1p(m1))


def _gamma(y, m, v):
    """(g, gl): g = (y - m) / sqrt(v) in float64 and the remainder of that quotient, so that the restatement sees the gamma
    truth sees.  The roundings of the difference, of the square root and of the division are recovered exactly in rational
    arithmetic and carried to first order -- bookkeeping of the INPUT, not of the three pieces: without it the rows g = 12
    at s = 1e-8 and 1e-3 (y* = g s and s^2 are rounded there) charge the restatement g^2 = 144 half-ulps of its own
    division, 75 ulp on a term of 1e-31, and every bar derived from it is 8 times too wide."""
    F = Fraction
    s = float(np.sqrt(v))
    d = y - m
    dl = float(F(y) - F(m) - F(d))
    sl = float(F(v) - F(s) * F(s)) / (2.0 * s)
    g = d / s
    gl = (float(F(d) - F(g) * F(s)) - g * sl + dl) / s
    return g, gl


def _dt_np(g):
    """t'(g) = -(lam / 2) (1 + g^2 + g lam), lam = phi / Phi, for g > -1 (no cancellation there); below, |t'| < 1 / |g| and the
    remainder of g moves t by less than an ulp."""
    with np.errstate(all="ignore"):
        lam = np.exp(-0.5 * g * g) / np.sqrt(2.0 * np.pi) / (0.5 * sp.erfc(-g / np.sqrt(2.0)))
        return float(-0.5 * lam * (1.0 + g * g + g * lam))


def restatement(ystar, mean, s2):
    ys = np.asarray(ystar, dtype=np.float64).reshape(-1)
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    s2 = np.asarray(s2, dtype=np.float64).reshape(-1)
    out = np.empty_like(mean)
    for i, (m, v) in enumerate(zip(mean, s2)):
        if np.isnan(m) or np.isnan(v):
            out[i] = np.nan
            continue
        v = max(float(v), 0.0)
        if v == 0.0:
            out[i] = 0.0
            continue
        acc = 0.0
        for y in ys:
            g, gl = _gamma(float(y), float(m), v)
            term = _t_np(g)
            if -1.0 < g <= 40.0 and gl != 0.0:
                term += _dt_np(g) * gl
            acc += term
        out[i] = acc / len(ys)
    return out


def error(got, want):
    """Worst relative error of float64 ``got`` against the mpmath list ``want``; inf when a non-finite value is not
    matched exactly."""
    worst = 0.0
    for g, w in zip(np.asarray(got, dtype=np.float64).reshape(-1), want):
        g = float(g)
        if mp.isnan(w):
            e = 0.0 if np.isnan(g) else np.inf
        elif mp.isinf(w) or not np.isfinite(g):
            e = 0.0 if (mp.isinf(w) and g == float(w)) else np.inf
        elif abs(w) < mp.mpf(2) ** -1022:
            e = float(abs(mp.mpf(g) - w) / mp.mpf(2) ** -1022)
        else:
            e = float(abs(mp.mpf(g) - w) / abs(w))
        worst = max(worst, e)
    return worst


def grid():
    """(ystar [rows], mean, s2) of the fixed grid, K = 1 per row: g x s with mean 0 and y* = g * s exactly representable;
    then s = 0 on both sides of y* and on it; then NaN rows."""
    ystar, mean, s2 = [], [], []
    for g in GRID_G:
        for s in GRID_S:
            ystar.append(float(np.float64(g) * np.float64(s)))
            mean.append(0.0)
            s2.append(float(np.float64(s) * np.float64(s)))
    for m in (0.75, 0.0, -0.75):  # (y* = 0)
        ystar.append(0.0)
        mean.append(m)
        s2.append(0.0)
    for m, v in ((np.nan, 1.0), (0.0, np.nan)):
        ystar.append(0.5)
        mean.append(m)
        s2.append(v)
    return np.array(ystar), np.array(mean), np.array(s2)


@functools.lru_cache(maxsize=None)
def grid_truth():
    ystar, mean, s2 = grid()
    return tuple(truth([y], [m], [v])[0] for y, m, v in zip(ystar, mean, s2))


@functools.lru_cache(maxsize=None)
def tolerance():
    """(tolerance, the restatement's own worst error) on the grid."""
    ystar, mean, s2 = grid()
    got = [restatement([y], [m], [v])[0] for y, m, v in zip(ystar, mean, s2)]
    own = error(got, grid_truth())
    return max(8.0 * own, 16.0 * ULP), own


# ---- the law of the maximum ---------------------------------------------------------------------------------------------
def _rows(mean, var, var_sub):
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    v = np.asarray(var, dtype=np.float64).reshape(-1) - np.float64(var_sub)
    ok = ~(np.isnan(mean) | np.isnan(v))
    return mean[ok], np.maximum(v[ok], 0.0)


def truth_logcdf(mean, var, y, var_sub=0.0):
    """mpmath: [sum_j log Phi((y_i - mean_j) / s_j) for y_i in y] over the rows without a NaN, and their number.  (var -
    var_sub is the float64 difference: the library's input to the square root.)"""
    mean, v = _rows(mean, var, var_sub)
    ys = [mp.mpf(float(yi)) for yi in np.asarray(y, dtype=np.float64).reshape(-1)]
    out = [mp.mpf(0) for _ in ys]
    for m, s2 in zip(mean, v):
        m_, s = mp.mpf(float(m)), mp.sqrt(mp.mpf(float(s2)))
        for i, yi in enumerate(ys):
            d = yi - m_
            if s2 == 0.0:
                out[i] += mp.mpf(0) if d > 0 else mp.log(mp.mpf("0.5")) if d == 0 else mp.mpf("-inf")
            else:
                out[i] += _log_ncdf_mp(d / s)
    return out, len(mean)


def restatement_logcdf(mean, var, y, var_sub=0.0):
    mean, v = _rows(mean, var, var_sub)
    s = np.sqrt(v)
    out = []
    for yi in np.asarray(y, dtype=np.float64).reshape(-1):
        d = yi - mean
        with np.errstate(all="ignore"):
            terms = np.where(s > 0, sp.log_ndtr(d / np.where(s > 0, s, 1.0)), np.where(d > 0, 0.0, np.where(d == 0, np.log(0.5), -np.inf)))
        out.append(-np.inf if np.any(np.isneginf(terms)) else math.fsum(terms))
    return np.array(out), len(mean)


def truth_logcdf_sampled(mean, var, y, var_sub=0.0, n_exact=2000):
    """``truth_logcdf`` where 60 digits on every row would take minutes: ``n_exact`` rows spread over the batch at 60
    digits, the restatement's ``math.fsum`` (exactly rounded; its terms carry log_ndtr's error) for the others.  Returns
    (sums, rows used, the restatement's own worst error ON THE EXACT ROWS -- what the borrowed part may be off by)."""
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    var = np.asarray(var, dtype=np.float64).reshape(-1)
    pick = np.zeros(len(mean), dtype=bool)
    pick[np.unique(np.linspace(0, len(mean) - 1, n_exact).astype(int))] = True
    exact, n0 = truth_logcdf(mean[pick], var[pick], y, var_sub)
    own = error(restatement_logcdf(mean[pick], var[pick], y, var_sub)[0], exact)
    rest, n1 = restatement_logcdf(mean[~pick], var[~pick], y, var_sub)
    out = [e + (mp.mpf("-inf") if np.isneginf(r) else mp.mpf(float(r))) for e, r in zip(exact, rest)]
    return out, n0 + n1, own


def logcdf_tolerance(m, own=0.0):
    """8 x the restatement's own worst error (``own``), floor (16 + log2 m) ulp."""
    return max(8.0 * own, (16.0 + math.log2(max(m, 1))) * ULP)
