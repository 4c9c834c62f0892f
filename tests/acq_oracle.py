"""
Two restatements of the acquisition maps of pygpso_amd/csrc/acq.hpp, for the tests only:

* ``truth``      mpmath at 60 digits, evaluated on the float64 inputs exactly as they are (mean, s^2, incumbent, xi)
* ``yardstick``  plain float64 numpy / scipy of the same formulas (scipy.special.erfcx / log_ndtr / ndtr) -- what a
                 careful user would write; its own error against truth sets the tolerance the library is held to

and the tolerance rule: the library stays within 8 x the yardstick's worst error on the grid below, with a floor of 16 ulp
(another libm and a different join between the pieces, nothing more).  Errors are relative, for LOGEI absolute over
max(1, |value|).
"""
import functools

import mpmath as mp
import numpy as np
from scipy import special as sp

from tests.oracle_engine import OracleEngine
from tests.predict_grad_oracle import gpr_predict_grad

UCB_VAR, UCB_STD, EI, LOGEI, PI = 0, 1, 2, 3, 4
KINDS = {"ucb_std": UCB_STD, "ei": EI, "logei": LOGEI, "pi": PI}
ULP = float(np.finfo(np.float64).eps)
GRID_Z = (40.0, 8.0, 1.0, 0.0, -1.0, -5.0, -6.0, -30.0, -38.0, -39.0, -1e2, -1e4, -1e6)
GRID_S = (1e-8, 1e-3, 1.0, 1e3)

mp.mp.dps = 60


def truth(kind, mean, s2, varsigma=0.0, incumbent=0.0, xi=0.0, s2_add=()):
    """mpmath values (mp.mpf, or -inf / nan floats) for arrays of float64 mean / s2.  ``s2_add``: float64 scalars or arrays
    added to s2 EXACTLY (the latent variance var - noise, the ends of a rounding interval)."""
    out = []
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    adds = [np.broadcast_to(np.asarray(a, dtype=np.float64), mean.shape) for a in s2_add]
    for i, (m, v) in enumerate(zip(mean, np.asarray(s2, dtype=np.float64).reshape(-1))):
        if np.isnan(m) or np.isnan(v):
            out.append(mp.nan)
            continue
        m_, v_ = mp.mpf(float(m)), mp.mpf(float(v))
        for a in adds:
            v_ += mp.mpf(float(a[i]))
        v_ = max(v_, mp.mpf(0))
        s = mp.sqrt(v_)
        if kind == UCB_STD:
            out.append(m_ + mp.mpf(varsigma) * s)
            continue
        d = m_ - mp.mpf(incumbent) - mp.mpf(xi)
        if s == 0:
            if kind == PI:
                out.append(mp.mpf(1) if d > 0 else mp.mpf(0) if d < 0 else mp.mpf("0.5"))
            elif kind == EI:
                out.append(max(d, mp.mpf(0)))
            else:
                out.append(mp.log(d) if d > 0 else mp.mpf("-inf"))
            continue
        z = d / s
        Phi = mp.erfc(-z / mp.sqrt(2)) / 2
        if kind == PI:
            out.append(Phi)
            continue
        ei = s * (mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi) + z * Phi)
        out.append(ei if kind == EI else mp.log(ei))
    return out


def _log_h(z):
    """log(phi(z) + z Phi(z)) in float64: direct above -1, through erfcx below."""
    z = np.asarray(z, dtype=np.float64)
    out = np.empty_like(z)
    hi = z > -1.0
    zh = z[hi]
    with np.errstate(divide="ignore"):
        out[hi] = np.log(np.exp(-0.5 * zh * zh) / np.sqrt(2 * np.pi) + zh * sp.ndtr(zh))
        t = -z[~hi]
        out[~hi] = -0.5 * t * t - 0.5 * np.log(2 * np.pi) + np.log1p(-t * np.sqrt(np.pi / 2) * sp.erfcx(t / np.sqrt(2)))
    return out


def yardstick(kind, mean, s2, varsigma=0.0, incumbent=0.0, xi=0.0):
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    s = np.sqrt(np.maximum(np.asarray(s2, dtype=np.float64).reshape(-1), 0.0))
    if kind == UCB_STD:
        return mean + varsigma * s
    d = mean - incumbent - xi
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = d / s
        if kind == PI:
            out = np.where(z > -1.0, sp.ndtr(z), np.exp(sp.log_ndtr(z)))
            zero = np.where(d > 0, 1.0, np.where(d < 0, 0.0, 0.5))
        elif kind == EI:
            pdf, t = np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi), -z
            out = s * np.where(z > -1.0, pdf + z * sp.ndtr(z), pdf * (1.0 - t * np.sqrt(np.pi / 2) * sp.erfcx(t / np.sqrt(2))))
            zero = np.maximum(d, 0.0)
        else:
            out = np.log(s) + _log_h(np.where(s > 0, z, 0.0))
            zero = np.log(np.maximum(d, 0.0))
    return np.where(s > 0, out, zero)


def error(kind, got, want):
    """Worst error of float64 ``got`` against the mpmath list ``want`` under the rule of the module text; inf when a
    non-finite value is not matched exactly."""
    worst = 0.0
    for g, w in zip(np.asarray(got, dtype=np.float64).reshape(-1), want):
        g = float(g)
        if mp.isnan(w):
            e = 0.0 if np.isnan(g) else np.inf
        elif mp.isinf(w) or not np.isfinite(g):
            e = 0.0 if (mp.isinf(w) and g == float(w)) else np.inf
        elif kind == LOGEI:
            e = float(abs(mp.mpf(g) - w) / max(mp.mpf(1), abs(w)))
        elif abs(w) < mp.mpf(2) ** -1022:
            # below the normal range float64 is a fixed grid of spacing eps * 2^-1022: the error is taken relative to the
            # smallest normal number, which is what a relative error means on that grid
            e = float(abs(mp.mpf(g) - w) / mp.mpf(2) ** -1022)
        else:
            e = float(abs(mp.mpf(g) - w) / abs(w))
        worst = max(worst, e)
    return worst


def grid():
    """(mean, s2, incumbent) of the fixed grid: z x s with d = z * s exactly representable as the mean (incumbent 0), then
    s = 0 with d positive, zero and negative."""
    mean, s2 = [], []
    for z in GRID_Z:
        for s in GRID_S:
            mean.append(float(np.float64(z) * np.float64(s)))
            s2.append(float(np.float64(s) * np.float64(s)))
    for d in (0.75, 0.0, -0.75):
        mean.append(d)
        s2.append(0.0)
    return np.array(mean), np.array(s2), 0.0


@functools.lru_cache(maxsize=None)
def grid_truth(kind):
    mean, s2, inc = grid()
    return tuple(truth(kind, mean, s2, incumbent=inc))


@functools.lru_cache(maxsize=None)
def tolerance(kind):
    """(tolerance, the yardstick's own worst error) of a kind on the grid."""
    mean, s2, inc = grid()
    yard = error(kind, yardstick(kind, mean, s2, incumbent=inc), grid_truth(kind))
    return max(8.0 * yard, 16.0 * ULP), yard


def _host_maps(acq, mean, var, noise, incumbent):
    from pygpso_amd import HipGPEngine

    return HipGPEngine.acq_eval_host(acq, mean, var, noise, incumbent)


class AcqOracleEngine(OracleEngine):
    """The stand-in of tests/oracle_engine.py with the acquisition calls: the oracle posterior, then the LIBRARY's host maps
    (``gpso_acq_eval_host``) -- the device applies the same header to its own (mean, var)."""

    def acq_values(self, xs, acq, incumbent=None):
        xs = np.asarray(xs, dtype=np.float64)
        mean, var = self.predict(xs) if xs.shape[0] else (np.empty(0), np.empty(0))
        return mean, var, _host_maps(acq, mean, var, self.post.theta.noise, incumbent)

    def best_acq(self, xs, acq, seg_off=None, incumbent=None):
        xs = np.asarray(xs, dtype=np.float64)
        so = np.array([0, xs.shape[0]]) if seg_off is None else np.asarray(seg_off)
        mean, var, val = self.acq_values(xs, acq, incumbent)
        out = []
        for a, b in zip(so[:-1], so[1:]):
            i = int(np.argmax(val[a:b]))
            out.append((i, mean[a + i], var[a + i], val[a + i]))
        return tuple(np.array(c) for c in zip(*out))

    def best_acq_grow(self, bounds, depth, acq, incumbent=None):
        b = np.asarray(bounds, dtype=np.float64)
        b = b[None] if b.ndim == 2 else b
        coords = np.vstack(list(self.grow(b, depth)))
        return self.best_acq(coords, acq, np.arange(b.shape[0] + 1) * self.grow_rows(depth), incumbent)

    def predict_grad(self, xs, out=None):
        return gpr_predict_grad(self.post, np.asarray(xs, dtype=np.float64))
