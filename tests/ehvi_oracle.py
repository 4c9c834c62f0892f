"""
Oracle of the bi-objective calls, written independently of csrc/ehvi.hpp: numpy / scipy / mpmath, no tree,
no written-out exp or erfc, and the TRANSPOSED decomposition -- the strips run along objective 2 where the library's run along
objective 1.  Maximisation.

With the front (a_k, b_k), k = 1 .. P, a ascending and b descending, a_0 = r1, b_0 = +inf, b_{P+1} = r2 and
G_i(x) = E[(Y_i - x)+] = s_i psi((mu_i - x) / s_i), psi(z) = pdf(z) + z cdf(z):

    EHVI = sum_{k=0..P} (G_2(b_{k+1}) - G_2(b_k)) G_1(a_k),        G_2(+inf) = 0

(for Y_2 between b_{k+1} and b_k the front reaches a_k along objective 1).  ``hypervolume_brute`` is a union-of-rectangles
area over the grid the points span, and ``hvi_brute`` the growth one outcome adds: what EHVI is the expectation of.
"""
import mpmath as mp
import numpy as np
from scipy.stats import norm

from tests import constraints_oracle as co

ULP = 2.0 ** -52


# ---- brute force ---------------------------------------------------------------------------------------------------------
def hypervolume_brute(points, ref):
    """Area of the union of the rectangles [r1, x] x [r2, y] over the rows (x, y) of ``points`` strictly above ``ref``."""
    pts = np.reshape(np.asarray(points, dtype=np.float64), (-1, 2))
    r1, r2 = float(ref[0]), float(ref[1])
    pts = pts[(pts[:, 0] > r1) & (pts[:, 1] > r2)]
    if pts.shape[0] == 0:
        return 0.0
    xs = np.unique(np.concatenate([[r1], pts[:, 0]]))
    ys = np.unique(np.concatenate([[r2], pts[:, 1]]))
    area = 0.0
    for i in range(len(xs) - 1):
        for j in range(len(ys) - 1):
            if np.any((pts[:, 0] >= xs[i + 1]) & (pts[:, 1] >= ys[j + 1])):
                area += (xs[i + 1] - xs[i]) * (ys[j + 1] - ys[j])
    return float(area)


def front_brute(points):
    """(front rows sorted by f1, their indices) by the definition: a row stays unless another row dominates it; of equal rows
    the first stays."""
    pts = np.reshape(np.asarray(points, dtype=np.float64), (-1, 2))
    keep = []
    for i, p in enumerate(pts):
        dominated = any(np.all(q >= p) and np.any(q > p) for q in pts)
        repeated = any(np.array_equal(pts[k], p) for k in range(i))
        if not dominated and not repeated:
            keep.append(i)
    keep.sort(key=lambda i: pts[i, 0])
    return pts[keep], np.array(keep, dtype=np.int64)


def hvi_brute(y, front, ref):
    """The hypervolume the outcome ``y`` adds to ``front``."""
    f = np.reshape(np.asarray(front, dtype=np.float64), (-1, 2))
    return hypervolume_brute(np.vstack([f, np.reshape(y, (1, 2))]), ref) - hypervolume_brute(f, ref)


# ---- the EHVI, transposed ------------------------------------------------------------------------------------------------
def _excess(mean, s, x):
    """E[(Y - x)+], Y ~ N(mean, s^2), elementwise over mean / s [m]; x a scalar (+inf: 0)."""
    mean, s = np.asarray(mean, dtype=np.float64), np.asarray(s, dtype=np.float64)
    if np.isposinf(x):
        return np.zeros_like(mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (mean - x) / s
        g = s * (norm.pdf(z) + z * norm.cdf(z))
    return np.where(s > 0.0, g, np.maximum(mean - x, 0.0))


def sigmas(var1, noise1, var2, noise2, latent=True):
    v1 = np.asarray(var1, dtype=np.float64) - (noise1 if latent else 0.0)
    v2 = np.asarray(var2, dtype=np.float64) - (noise2 if latent else 0.0)
    return np.sqrt(np.maximum(v1, 0.0)), np.sqrt(np.maximum(v2, 0.0))


def ehvi_numpy(front, ref, mean1, s1, mean2, s2):
    """EHVI [m] of leaves with independent N(mean1, s1^2), N(mean2, s2^2) over ``front`` [P, 2] and ``ref``."""
    f = np.reshape(np.asarray(front, dtype=np.float64), (-1, 2))
    p = f.shape[0]
    a = np.concatenate([[ref[0]], f[:, 0]])             # a_0 .. a_P
    b = np.concatenate([[np.inf], f[:, 1], [ref[1]]])   # b_0 .. b_{P+1}
    total = np.zeros(np.shape(mean1), dtype=np.float64)
    for k in range(p + 1):
        total += (_excess(mean2, s2, b[k + 1]) - _excess(mean2, s2, b[k])) * _excess(mean1, s1, a[k])
    return total


def value_numpy(ehvi, logpof, mode=None, log_pof_min=-np.inf):
    if mode is None:
        return np.array(ehvi, dtype=np.float64)
    if mode == "gate":
        return np.where(logpof >= log_pof_min, ehvi, -np.inf) if log_pof_min > -np.inf else np.array(ehvi, dtype=np.float64)
    return np.where(logpof < log_pof_min, -np.inf, ehvi * np.exp(logpof))


def logpof_numpy(other_mean, other_var, other_noise, thr, sense, success_mean=None, success_var=None, m=None):
    """Sum of the other members' log Phi terms (tests/constraints_oracle.py) and the success member's probit term."""
    k = 0 if other_mean is None else np.shape(other_mean)[0]
    lp = np.zeros(m if k == 0 and success_mean is None else (np.shape(other_mean)[1] if k else np.shape(success_mean)[0]))
    if k:
        lp = lp + co.log_pof_numpy(np.asarray(other_mean), np.asarray(other_var), np.asarray(other_noise), np.asarray(thr), np.asarray(sense))
    if success_mean is not None:
        lp = lp + norm.logcdf(np.asarray(success_mean) / np.sqrt(1.0 + np.maximum(np.asarray(success_var), 0.0)))
    return lp


# ---- 60 digits -----------------------------------------------------------------------------------------------------------
def _mp_excess(mean, s, x):
    if s == 0:
        return max(mean - x, mp.mpf(0))
    z = (mean - x) / s
    return s * (mp.npdf(z) + z * mp.ncdf(z))


def ehvi_truth(front, ref, mean1, s2_1, mean2, s2_2):
    """One leaf at 60 digits, every input taken as the exact double it is (``s2_i`` the VARIANCES the strips read, their
    exact square roots the standard deviations) -> (EHVI, B): B = sum_k g(a_k) e_k, the sum BEFORE the subtraction of
    g(a_{k+1}) -- the size of what the strip differences are formed from, hence the scale of their rounding error."""
    with mp.workdps(60):
        return ehvi_truth_mp(front, ref, mp.mpf(float(mean1)), mp.sqrt(mp.mpf(float(s2_1))), mp.mpf(float(mean2)), mp.sqrt(mp.mpf(float(s2_2))))


def ehvi_truth_mp(front, ref, m1, d1, m2, d2):
    with mp.workdps(60):
        f = [(mp.mpf(float(x)), mp.mpf(float(y))) for x, y in np.reshape(np.asarray(front, dtype=np.float64), (-1, 2))]
        p = len(f)
        r1, r2 = mp.mpf(float(ref[0])), mp.mpf(float(ref[1]))
        a = [r1] + [x for x, _ in f]                  # a_0 .. a_P
        h = [f[k][1] for k in range(p)] + [r2]        # h_k = b_{k+1} (k < P), h_P = r2
        g = [_mp_excess(m1, d1, x) for x in a] + [mp.mpf(0)]
        e = [_mp_excess(m2, d2, y) for y in h]
        total = sum((g[k] - g[k + 1]) * e[k] for k in range(p + 1))
        scale = sum(g[k] * e[k] for k in range(p + 1))
        return total, scale


# ---- fronts and grids the tests share --------------------------------------------------------------------------------------
def make_front(p, seed=0, ref=(0.0, 0.0)):
    """A front of ``p`` points above ``ref`` on a convex-ish curve with uneven gaps: [p, 2], f1 ascending, f2 descending."""
    rng = np.random.default_rng([17, p, seed])
    if p == 0:
        return np.zeros((0, 2))
    t = np.sort(rng.uniform(0.05, 0.95, p))
    while np.any(np.diff(t) <= 0):
        t = np.sort(rng.uniform(0.05, 0.95, p))
    return np.column_stack([ref[0] + 2.0 * t, ref[1] + 1.5 * (1.0 - t ** 1.7)])


# ---- the stand-in engine of the CPU surrogate tests ------------------------------------------------------------------------
class EhviOracleEngine(co.ConstraintOracleEngine):
    """tests/constraints_oracle.py's stand-in with the EHVI calls: oracle posteriors for every column, then the LIBRARY's host
    fold (``gpso_ehvi_fold_host``), which the device applies to its own columns."""

    def ehvi_values(self, xs, member, front, ref, latent=True, mode=None, log_pof_min=-np.inf):
        from pygpso_amd import HipGPEngine

        xs = np.asarray(xs, dtype=np.float64)
        assert self._con and 0 <= member < len(self._con)
        mean, var = self.predict(xs)
        mm, mv = self.member_columns(xs)
        others = [i for i in range(len(self._con)) if i != member]
        val, lp = HipGPEngine.ehvi_fold_host(front, ref, mean, var, self.post.theta.noise, mm[member], mv[member], self._con[member][0].theta.noise,
                                             mm[others] if others else None, mv[others] if others else None,
                                             [self._con[i][0].theta.noise for i in others], [self._con[i][1] for i in others],
                                             [self._con[i][2] for i in others], latent=latent, mode=mode, log_pof_min=log_pof_min)
        return val, lp, np.array([mean, mm[member]]), np.array([var, mv[member]])

    def best_ehvi(self, xs, member, front, ref, latent=True, mode=None, log_pof_min=-np.inf, seg_off=None):
        xs = np.asarray(xs, dtype=np.float64)
        so = np.array([0, xs.shape[0]]) if seg_off is None else np.asarray(seg_off)
        val, lp, mean, var = self.ehvi_values(xs, member, front, ref, latent, mode, log_pof_min)
        idx = np.array([int(np.argmax(val[a:b])) for a, b in zip(so[:-1], so[1:])], dtype=np.int64)
        at = so[:-1] + idx
        return idx, val[at], lp[at], mean[:, at], var[:, at]


# ---- the accuracy grids (tests/test_ehvi_cpu.py; the GPU tests reuse the moderate tolerance) -------------------------------
GRID_P = (0, 1, 2, 31, 32, 63)
GRID_S = (1e-6, 1e-3, 0.03, 0.3, 1.0, 30.0, 1e3)
GRID_S_MIXED = ((1e-6, 1e3), (1e3, 1e-6), (0.03, 1.0))
GRID_OFF1 = (40.0, 10.0, 3.0, 1.0, 0.0, -1.0, -3.0, -10.0, -40.0)
GRID_OFF2 = (10.0, 0.0, -3.0, -40.0)
REF = (0.0, 0.0)
# the measured constants (tests/test_ehvi_cpu.py says how; DESIGN.md section 7t records them)
C_HOST_MEASURED = 5.521     # worst c of gpso_ehvi_fold_host on the full grid; allowed: twice it
C_HOST = 2.0 * C_HOST_MEASURED
C_ORACLE_MEASURED = 91.625  # worst c of ehvi_numpy itself on the moderate grid
C_VS_ORACLE = C_HOST + 4.0 * C_ORACLE_MEASURED  # host or device against ehvi_numpy: the two errors add, the oracle's with a margin of four
FLOOR = 2.0 ** -1000  # below it a double is in or near the subnormal range and carries fewer than 53 bits


MOD_S = ((0.5, 0.5), (1.0, 1.0), (0.5, 1.0))
MOD_OFF = (3.0, 1.0, 0.0, -1.0, -3.0)


def grid(p, moderate=False):
    """Leaves (mean1, s2_1, mean2, s2_2) [n] around ``make_front(p)``: the means from 40 standard deviations above to 40
    below a front point (P = 0: the reference corner), standard deviations from 1e-6 to 1e3, equal and mixed.  ``moderate``:
    offsets within 3 standard deviations of 0.5 or 1, where every strip's |z| stays below 6 (asserted) -- the range in which
    the plain double formulas of the numpy oracle hold."""
    f = make_front(p)
    anchor = f[p // 2] if p else np.array(REF)
    spairs = MOD_S if moderate else [(s, s) for s in GRID_S] + list(GRID_S_MIXED)
    rows = []
    for s1, s2 in spairs:
        for o1 in (MOD_OFF if moderate else GRID_OFF1):
            for o2 in (MOD_OFF if moderate else GRID_OFF2):
                rows.append((anchor[0] + o1 * s1, s1 * s1, anchor[1] + o2 * s2, s2 * s2))
    cols = tuple(np.array(c, dtype=np.float64) for c in zip(*rows))
    if moderate:
        a, h = np.concatenate([[REF[0]], f[:, 0]]), np.concatenate([f[:, 1], [REF[1]]])
        z1 = np.abs(cols[0][:, None] - a[None]) / np.sqrt(cols[1])[:, None]
        z2 = np.abs(cols[2][:, None] - h[None]) / np.sqrt(cols[3])[:, None]
        assert max(z1.max(), z2.max()) <= 6.0
    return f, cols


_TRUTH = {}


def grid_truth(p, moderate=False):
    """(EHVI, B) of ``grid(p)`` at 60 digits as lists of mpf; computed once."""
    key = (p, moderate)
    if key not in _TRUTH:
        f, (m1, v1, m2, v2) = grid(p, moderate)
        _TRUTH[key] = [ehvi_truth(f, REF, a, b, c, d) for a, b, c, d in zip(m1, v1, m2, v2)]
    return _TRUTH[key]


def worst_c(values, truth):
    """max over the leaves of |value - EHVI| / (2^-52 B + FLOOR): the error in units of the derived condition number."""
    with mp.workdps(60):
        return float(max(abs(mp.mpf(float(v)) - t) / (mp.mpf(ULP) * b + mp.mpf(FLOOR)) for v, (t, b) in zip(values, truth)))


def scale_numpy(front, ref, mean1, s1, mean2, s2):
    """B = sum_k g(a_k) e_k [m] in plain double: the scale the tolerances multiply."""
    f = np.reshape(np.asarray(front, dtype=np.float64), (-1, 2))
    a = np.concatenate([[ref[0]], f[:, 0]])
    h = np.concatenate([f[:, 1], [ref[1]]])
    return sum(_excess(mean1, s1, a[k]) * _excess(mean2, s2, h[k]) for k in range(f.shape[0] + 1))
