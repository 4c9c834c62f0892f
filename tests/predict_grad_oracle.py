"""float64 numpy/scipy restatement of the GP predictive's input gradients, in the manner of
``tests/loo_oracle.py``.  For a predictive (C, alpha, rows, theta) with mean = alpha^T k* + c and
var = variance - |C k*|^2 + noise, xs = x / l, r2_i = |xs* - xs_i|^2 from direct differences, k'_i = dk/dr2:

    v = C k*,  w = C^T v,  dk_i/dx*_d = 2 k'_i (xs*_d - xs_i,d) / l_d,
    dmean/dx*_d = sum_i alpha_i dk_i/dx*_d,   dvar/dx*_d = -2 sum_i w_i dk_i/dx*_d

A pair with r2 <= 1e-36 contributes zero to the gradients (exact for the squared exponential and the Matern-3/2 and -5/2,
the convention at the Matern-1/2's kink).

Test infrastructure: the kernel map and its derivative are ``oracle/gpr.py``'s.  Nothing here is imported by ``pygpso_amd``.
"""
import numpy as np
import scipy.linalg as sla

from oracle import gpr


def predictive_grad(C, alpha, rows, theta, Xs):
    """(mean[M], var[M], dmean[M, D], dvar[M, D]) of a generic predictive: C [n, n] (v = C k*), alpha [n], rows [n, D]."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    d = rows.shape[1]
    ls = np.broadcast_to(np.asarray(theta.lengthscales, dtype=np.float64), (d,)) if theta.lengthscales.shape[0] == 1 \
        else np.asarray(theta.lengthscales, dtype=np.float64)
    diff = (Xs / ls)[:, None, :] - (rows / ls)[None, :, :]  # [M, n, D]
    r2 = np.sum(diff * diff, axis=-1)
    K = gpr.kernel_from_r2(theta.kernel, r2, theta.variance)
    dK = np.where(r2 > 1e-36, gpr._dk_dr2(theta.kernel, r2, K, theta.variance), 0.0)
    V = K @ np.asarray(C).T  # row m: v = C k*
    W = V @ np.asarray(C)    # row m: w = C^T v
    mean = K @ alpha + theta.mean_c
    var = theta.variance - np.sum(V * V, axis=1) + theta.noise
    dmean = np.einsum("mn,mnd->md", 2.0 * dK * alpha[None, :], diff) / ls
    dvar = np.einsum("mn,mnd->md", -4.0 * dK * W, diff) / ls
    return mean, var, dmean, dvar


def linv_of(L):
    return sla.solve_triangular(L, np.eye(L.shape[0]), lower=True)


def gpr_predict_grad(post, Xs):
    """The exact GP's: ``post`` from ``oracle.gpr.posterior`` (or ``tests.hetero_oracle.posterior``: same members)."""
    return predictive_grad(linv_of(post.L), post.alpha, post.X, post.theta, Xs)


def central_differences(f, Xs, h=1.0e-6):
    """d f / d x by central differences: f maps [M, D] points to a tuple of [M] arrays; returns one [M, D] array per entry."""
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    m, d = Xs.shape
    outs = None
    for k in range(d):
        e = np.zeros(d)
        e[k] = h
        up, dn = f(Xs + e), f(Xs - e)
        if outs is None:
            outs = [np.empty((m, d)) for _ in up]
        for o, a, b in zip(outs, up, dn):
            o[:, k] = (a - b) / (2.0 * h)
    return outs


def projected_gradient(x, g_ascent, lower, upper):
    """Largest component of the projected gradient of a MAXIMISATION at x in the box: the ascent direction clipped where a
    bound is active (what L-BFGS-B's pgtol test looks at, for the minimised negative)."""
    step = np.clip(x + g_ascent, lower, upper) - x
    return float(np.max(np.abs(step))) if step.size else 0.0


def polish_problem():
    """The polish tests' problem: 30 seeded points of the unit square scored by the toy objective of ``tests/helpers.py``
    over its bounds, and four cells of the 3 x 3 grid of the square -- each search starts at its cell's centre and is held
    inside it, as a polish of one leaf would be.  Returns (coords [30, 2], scores [30], starts [4, 2], box [4, 2, 2])."""
    from tests.helpers import rotated_peaks

    coords = np.random.default_rng(5).random((30, 2))
    scores = np.array([rotated_peaks((-3.0 + 8.0 * c[0], -3.0 + 6.0 * c[1])) for c in coords])
    cells = [(0, 0), (1, 1), (2, 1), (1, 2)]
    box = np.array([[[i / 3.0, (i + 1) / 3.0], [j / 3.0, (j + 1) / 3.0]] for i, j in cells])
    return coords, scores, box.mean(axis=2), box
