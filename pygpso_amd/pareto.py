"""
Bi-objective search (NOT in the reference): the host side of it -- Pareto fronts, their hypervolume,
a reference point and the thinning of a front that is longer than an EHVI call takes.  Plain numpy; MAXIMISATION of both
objectives, as everywhere in this package.

A *front* is an array [P, 2] of (f1, f2) rows with f1 strictly ascending and f2 strictly descending: the form
``gpso_ehvi.front`` takes.
"""
from __future__ import annotations

import warnings

import numpy as np

from . import _lib as L

FRONT_MAX = L.EHVI_FRONT_MAX


def _as_points(Y):
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[1] != 2:
        raise ValueError(f"expected outcomes of shape [n, 2], got {Y.shape}")
    if not np.all(np.isfinite(Y)):
        raise ValueError("outcomes must be finite")
    return Y


def pareto_front(Y):
    """The strict Pareto front of the rows of ``Y`` [n, 2] under maximisation -> (front [P, 2], rows [P]): the rows no other
    row dominates (>= in both objectives, > in one), sorted by f1 ascending (so f2 descends strictly), equal rows collapsed
    to the first of them; ``rows`` are their indices in ``Y``."""
    Y = _as_points(Y)
    n = Y.shape[0]
    if n == 0:
        return np.zeros((0, 2)), np.zeros(0, dtype=np.int64)
    order = np.lexsort((np.arange(n), -Y[:, 1], -Y[:, 0]))  # f1 descending, then f2 descending, then the first row
    keep, best = [], -np.inf
    for i in order:
        if Y[i, 1] > best:
            keep.append(i)
            best = Y[i, 1]
    rows = np.array(keep[::-1], dtype=np.int64)
    return Y[rows].copy(), rows


def hypervolume_2d(front, ref):
    """The area dominated by the rows of ``front`` [n, 2] (any point set: it need not be a front) and bounded below by the
    reference point ``ref``; rows not strictly above ``ref`` in both objectives add nothing."""
    Y = _as_points(np.reshape(np.asarray(front, dtype=np.float64), (-1, 2)))
    r = np.asarray(ref, dtype=np.float64).reshape(2)
    Y = Y[(Y[:, 0] > r[0]) & (Y[:, 1] > r[1])]
    f, _ = pareto_front(Y)
    if f.shape[0] == 0:
        return 0.0
    widths = np.diff(np.concatenate([[r[0]], f[:, 0]]))
    return float(np.sum(widths * (f[:, 1] - r[1])))


def default_reference(Y):
    """A reference point below the rows of ``Y`` [n, k]: per column the minimum minus 10 % of the column's range; a column
    of zero range subtracts 1."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[0] == 0:
        raise ValueError(f"expected outcomes of shape [n, k] with n >= 1, got {Y.shape}")
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    rng = hi - lo
    return lo - np.where(rng > 0.0, 0.1 * rng, 1.0)


def exclusive_hypervolumes(front, ref):
    """[P] the area only point k of ``front`` dominates: (a_k - a_{k-1}) (b_k - b_{k+1}) with a_0 = r1, b_{P+1} = r2."""
    f = _as_points(np.reshape(np.asarray(front, dtype=np.float64), (-1, 2)))
    r = np.asarray(ref, dtype=np.float64).reshape(2)
    return np.diff(np.concatenate([[r[0]], f[:, 0]])) * -np.diff(np.concatenate([f[:, 1], [r[1]]]))


def truncate_front(front, ref, max_points=FRONT_MAX):
    """``front`` [P, 2] (a front above ``ref``) with at most ``max_points`` points: while it is longer, the point of least
    exclusive hypervolume (the first of them) is dropped.  A front that had to be thinned dominates less than the full one,
    so the EHVI over it is an UPPER bound of the true one: the call warns."""
    f = _as_points(np.reshape(np.asarray(front, dtype=np.float64), (-1, 2))).copy()
    if max_points < 1:
        raise ValueError(f"max_points={max_points}: at least 1")
    if f.shape[0] > max_points:
        warnings.warn(f"the front has {f.shape[0]} points, an EHVI call takes {max_points}: the points of least exclusive "
                      "hypervolume are dropped, and the EHVI over the thinned front is an upper bound of the true one",
                      RuntimeWarning, stacklevel=2)
    while f.shape[0] > max_points:
        f = np.delete(f, int(np.argmin(exclusive_hypervolumes(f, ref))), axis=0)
    return f
