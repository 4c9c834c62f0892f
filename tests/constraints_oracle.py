"""
Restatements for the outcome-constraint tests (pygpso_amd/csrc/constraints.hpp), independent of
pygpso_amd (but for ``host_logpof``, which asks the library, and the stand-in engine at the end, which applies the library's
host fold to the oracle's columns):

* ``truth_logpof``   mpmath at 60 digits on the float64 inputs exactly as they are: per constraint the latent variance
                     var - noise (clamped at 0), z = sense (t - mean) / s, log Phi(z) (tests/mes_oracle.py's ``_log_ncdf_mp``);
                     at s2 = 0 the term is 0 where sense (t - mean) >= 0 and -inf otherwise; the terms are summed exactly
* ``grid``           the fixed grid: z from 40 down to -1e6 (mes_oracle.GRID_G) times s in mes_oracle.GRID_S with mean 0 and
                     t = z s, once per sense; rows with a noise variance to subtract; s2 = 0 on both sides of the threshold and
                     on it, per sense; NaN rows.  For J > 1 member i is the grid rolled by 3 i rows
* ``tolerance``      the bound on logpof.  Not fixed here: ``log_ncdf_error`` MEASURES the worst relative error of the
                     library's log Phi (acq_log_ncdf, through gpso_constrained_fold_host with J = 1 in feasibility mode)
                     against truth on the grid; the bound is twice that, plus (J - 1) ulp for the ordered sum of J terms of
                     one sign, floor 16 ulp (mes_oracle.tolerance's floor)
* ``log_pof_numpy``  float64 numpy / scipy (log_ndtr): what a user would write; the loop tests read it

Measured when this file was written (the host entry, x86-64, 2026-10): log_ncdf_error() = 3.5e-16 (1.6 ulp, at z = 0),
so the bound is the floor, 16 ulp = 3.6e-15, at J = 1 and 2, and 18.2 ulp at J = 16; the library's own worst error on the
grid was 1.6 ulp at J = 1 and 2 and 2.2 ulp at J = 16.

Errors are relative; below the normal range they are taken relative to the smallest normal number (mes_oracle.error).
"""
import functools

import mpmath as mp
import numpy as np
from scipy import special as sp

from tests import mes_oracle
from tests.acq_oracle import AcqOracleEngine

ULP = mes_oracle.ULP
WEIGHT, GATE, FEASIBILITY = 0, 1, 2
_NOISE = 2.0 ** -10  # (added to s2 = 1 and s2 = 1e6 exactly: the latent variance the library subtracts back is s2)

mp.mp.dps = 60


def truth_logpof(cmean, cvar, cnoise, thr, sense):
    """mpmath log probability of feasibility [M] (mp.mpf, -inf or nan) from float64 member columns [J, M] and the members'
    noise variances, thresholds and senses [J]."""
    cmean, cvar = np.atleast_2d(np.asarray(cmean, dtype=np.float64)), np.atleast_2d(np.asarray(cvar, dtype=np.float64))
    out = []
    for j in range(cmean.shape[1]):
        total = mp.mpf(0)
        for i in range(cmean.shape[0]):
            m, v = float(cmean[i, j]), float(cvar[i, j])
            if np.isnan(m) or np.isnan(v) or mp.isnan(total):
                total = mp.nan
                continue
            s2 = max(mp.mpf(v) - mp.mpf(float(cnoise[i])), mp.mpf(0))
            d = mp.mpf(int(sense[i])) * (mp.mpf(float(thr[i])) - mp.mpf(m))
            if s2 == 0:
                total += mp.mpf(0) if d >= 0 else mp.mpf("-inf")
            else:
                total += mes_oracle._log_ncdf_mp(d / mp.sqrt(s2))
        out.append(total)
    return out


def log_pof_numpy(cmean, cvar, cnoise, thr, sense):
    """float64 [M]: sum_i log_ndtr(sense_i (t_i - mean_i) / s_i), the s2 = 0 rule included."""
    cmean, cvar = np.atleast_2d(np.asarray(cmean, dtype=np.float64)), np.atleast_2d(np.asarray(cvar, dtype=np.float64))
    total = np.zeros(cmean.shape[1])
    for i in range(cmean.shape[0]):
        s = np.sqrt(np.maximum(cvar[i] - cnoise[i], 0.0))
        d = sense[i] * (thr[i] - cmean[i])
        with np.errstate(all="ignore"):
            total = total + np.where(s > 0, sp.log_ndtr(d / np.where(s > 0, s, 1.0)), np.where(d >= 0, 0.0, -np.inf))
    return total


@functools.lru_cache(maxsize=None)
def _base_grid():
    mean, var, noise, thr, sense = [], [], [], [], []
    for sn in (1, -1):
        for g in mes_oracle.GRID_G:
            for s in mes_oracle.GRID_S:
                mean.append(0.0)
                var.append(float(np.float64(s) * np.float64(s)))
                noise.append(0.0)
                thr.append(float(sn * np.float64(g) * np.float64(s)))
                sense.append(sn)
            for s2 in (1.0, 1e6):  # a noise variance to subtract: var = s2 + noise exactly
                mean.append(0.25)
                var.append(s2 + _NOISE)
                noise.append(_NOISE)
                thr.append(float(0.25 + sn * np.float64(g) * np.sqrt(s2)))
                sense.append(sn)
        for m in (0.75, 0.0, -0.75):  # s2 = 0 (and a variance below the noise, clamped): t = 0 on both sides and on it
            for v, nz in ((0.0, 0.0), (1e-3, 2e-3)):
                mean.append(m)
                var.append(v)
                noise.append(nz)
                thr.append(0.0)
                sense.append(sn)
    for m, v in ((np.nan, 1.0), (0.0, np.nan)):
        mean.append(m)
        var.append(v)
        noise.append(0.0)
        thr.append(0.5)
        sense.append(1)
    return tuple(np.array(a) for a in (mean, var, noise, thr)) + (np.array(sense, dtype=np.int64),)


def grid(nj=1):
    """(cmean [J, M], cvar [J, M], cnoise [J, M], thr [J, M], sense [J, M]): PER-LEAF thresholds, senses and noise -- every
    leaf of the grid is a problem of its own (the host entry is called once per leaf with that leaf's [J] records)."""
    base = _base_grid()
    return tuple(np.array([np.roll(a, 3 * i) for i in range(nj)]) for a in base)


@functools.lru_cache(maxsize=None)
def grid_truth(nj=1):
    cm, cv, cn, th, sn = grid(nj)
    return tuple(truth_logpof(cm[:, j:j + 1], cv[:, j:j + 1], cn[:, j], th[:, j], sn[:, j])[0] for j in range(cm.shape[1]))


def host_logpof(nj=1):
    """The library's logpof on the grid, through the host entry (one call per leaf: its own thresholds and senses)."""
    from pygpso_amd import HipGPEngine, acquisition as A

    cm, cv, cn, th, sn = grid(nj)
    out = np.empty(cm.shape[1])
    zero = np.zeros(1)
    for j in range(cm.shape[1]):
        out[j] = HipGPEngine.constrained_fold_host(A.EI(), zero, zero + 1.0, 0.0, cm[:, j:j + 1], cv[:, j:j + 1], cn[:, j], th[:, j], sn[:, j],
                                                   mode="feasibility", incumbent=0.0)[1][0]
    return out


@functools.lru_cache(maxsize=None)
def log_ncdf_error():
    """The measured worst relative error of the library's log Phi against truth on the grid (J = 1)."""
    return mes_oracle.error(host_logpof(1), grid_truth(1))


def tolerance(nj=1):
    """(bound on logpof's relative error for J members, the measured error of log Phi)."""
    own = log_ncdf_error()
    return max(2.0 * own + (nj - 1) * ULP, 16.0 * ULP), own


# ---- the stand-in engine of the CPU loop tests ---------------------------------------------------------------------------
class ConstraintOracleEngine(AcqOracleEngine):
    """tests/acq_oracle.py's stand-in with the constraint calls: the oracle posteriors of the objective and of every pushed
    model, then the LIBRARY's host fold (``gpso_constrained_fold_host``) -- the device applies the same header to its own
    columns.  A push copies the source's posterior as it stands, as the device's does."""

    def __init__(self, dtype="float64", device=0):
        super().__init__(dtype, device)
        self._con = []  # (posterior, threshold, sense)

    def constraint_max(self):
        return 16 if self.n and self.n <= 128 else 0

    def constraint_push(self, src, threshold, sense):
        assert src.post is not None and len(self._con) < 16
        self._con.append((src.post, float(threshold), int(sense)))
        return len(self._con) - 1

    def constraint_clear(self):
        self._con = []

    def constraint_info(self):
        return len(self._con), None, np.array([c[1] for c in self._con]), np.array([c[2] for c in self._con], dtype=np.int64)

    def member_columns(self, xs):
        from oracle import gpr

        cols = [gpr.predict_y(p, xs) for p, _, _ in self._con]
        return np.array([c[0] for c in cols]), np.array([c[1] for c in cols])

    def constrained_acq_values(self, xs, acq, mode="gate", log_pof_min=-np.inf, incumbent=None, want_members=False):
        from pygpso_amd import HipGPEngine

        xs = np.asarray(xs, dtype=np.float64)
        assert self._con and all(p.X.shape == self.post.X.shape for p, _, _ in self._con)
        mean, var = self.predict(xs)
        mm, mv = self.member_columns(xs)
        val, lp = HipGPEngine.constrained_fold_host(acq, mean, var, self.post.theta.noise, mm, mv, [p.theta.noise for p, _, _ in self._con],
                                                    [c[1] for c in self._con], [c[2] for c in self._con], mode, log_pof_min, incumbent)
        return (mean, var, val, lp, mm, mv) if want_members else (mean, var, val, lp)

    def constrained_best_acq(self, xs, acq, mode="gate", log_pof_min=-np.inf, seg_off=None, incumbent=None):
        xs = np.asarray(xs, dtype=np.float64)
        so = np.array([0, xs.shape[0]]) if seg_off is None else np.asarray(seg_off)
        cols = self.constrained_acq_values(xs, acq, mode, log_pof_min, incumbent)
        out = []
        for a, b in zip(so[:-1], so[1:]):
            i = int(np.argmax(cols[2][a:b]))  # (a NaN wins, the first maximum on ties: np.argmax's rule too)
            out.append((i,) + tuple(c[a + i] for c in cols))
        return tuple(np.array(c) for c in zip(*out))
