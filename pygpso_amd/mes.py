"""
Sampling the optimum's VALUE y* for max-value entropy search (Wang & Jegelka 2017), host side.

Two routes, both behind ``HipGPR.max_value_samples``:

* ``"paths"``: the maxima of K posterior functions over the candidate rows (``sample_paths`` + ``eval_paths``'s
  ``best_val``) -- joint draws, float64 and mixed engines.
* ``"gumbel"``: the candidates taken as independent, P(y* < y) = prod_j Phi((y - mean_j) / s_j).  Its logarithm at 64
  thresholds is one ``gpso_max_logcdf`` call; a Gumbel law  exp(-exp(-(y - a) / b))  is fitted to the 25 / 50 / 75 % points
  and sampled by inversion.  Every engine type; no random features.

Everything random comes from the host generator, as everywhere in this package.  Both routes clamp the samples from below
at the largest training target (``clamp_at``), as Wang & Jegelka do: the maximum of f is at least the best value seen, and
a sample below it would make the best leaf look certain to exceed y*.
"""
from __future__ import annotations

import numpy as np

GRID = 64  # thresholds per max-logcdf call (the call's limit)
_LOG_Q = np.log(np.array([0.25, 0.5, 0.75]))
_LL4, _LL2, _LL43 = float(np.log(np.log(4.0))), float(np.log(np.log(2.0))), float(np.log(np.log(4.0 / 3.0)))


def _crossing(y, logcdf, target):
    """Where the non-decreasing ``logcdf`` over the ascending grid ``y`` crosses ``target``, by linear interpolation in
    logcdf between the last point at or below it and the next one."""
    i = int(np.searchsorted(logcdf, target, side="right")) - 1
    i = min(max(i, 0), len(y) - 2)
    l0, l1 = logcdf[i], logcdf[i + 1]
    if not np.isfinite(l0) or l1 <= l0:
        return float(y[i + 1] if target > l0 else y[i])
    return float(y[i] + (y[i + 1] - y[i]) * (target - l0) / (l1 - l0))


def gumbel_fit(logcdf, lo, hi, max_widen=8):
    """Fit a Gumbel law to the maximum's distribution.  ``logcdf(y)``: log P(y* < y) at an ascending float64 array of at
    most 64 thresholds (``HipGPEngine.max_logcdf`` with the leaves bound).  A coarse grid of 64 thresholds over [lo, hi]
    brackets the quartiles -- widened by its own length, at most ``max_widen`` times, on the side that does not reach
    them --, a fine grid of 64 between the bracketing coarse points locates them.  Two calls where [lo, hi] holds the
    quartiles.  Returns (a, b, quantiles [3], spacing of the fine grid)."""
    lo, hi = float(lo), float(hi)
    if not (hi > lo):
        return lo, 0.0, np.array([lo, lo, lo]), 0.0
    for _ in range(max_widen + 1):
        coarse = np.linspace(lo, hi, GRID)
        lc = np.asarray(logcdf(coarse), dtype=np.float64)
        low_ok, high_ok = lc[0] <= _LOG_Q[0], lc[-1] >= _LOG_Q[2]
        if low_ok and high_ok:
            break
        span = hi - lo
        lo, hi = (lo if low_ok else lo - span), (hi if high_ok else hi + span)
    else:
        raise ValueError("gumbel_fit: the quartiles of the maximum's law were not bracketed")
    i0 = max(int(np.searchsorted(lc, _LOG_Q[0], side="right")) - 1, 0)
    i1 = min(int(np.searchsorted(lc, _LOG_Q[2], side="left")), GRID - 1)
    fine = np.linspace(coarse[i0], coarse[max(i1, i0 + 1)], GRID)
    lf = np.asarray(logcdf(fine), dtype=np.float64)
    y25, y50, y75 = (_crossing(fine, lf, t) for t in _LOG_Q)
    b = (y25 - y75) / (_LL43 - _LL4)
    a = y50 + b * _LL2
    return a, b, np.array([y25, y50, y75]), float(fine[1] - fine[0])


def gumbel_draw(a, b, k, rng):
    """``k`` draws of the Gumbel law (a, b) by inversion: a - b log(-log U), U uniform on (0, 1) from ``rng`` (a seed or a
    ``numpy.random.Generator``)."""
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    u = rng.random(int(k))
    u = np.clip(u, np.finfo(np.float64).tiny, 1.0 - np.finfo(np.float64).epsneg)
    return a - b * np.log(-np.log(u))


def clamp_at(samples, best_target):
    """The samples clamped from below at the largest training target."""
    return np.maximum(np.asarray(samples, dtype=np.float64), float(best_target))
