"""float64 numpy restatement of the exact GP's leave-one-out predictive and LOO-CV objective (Rasmussen & Williams
5.4.2), in the manner of ``tests/hetero_oracle.py``.  With K_y = k(X, X) + diag(noise + s_i), alpha = K_y^-1 (y - c) and
kappa_i = (K_y^-1)_ii:

    mean_-i = y_i - alpha_i / kappa_i,  var_-i = 1 / kappa_i,  lpd_i = (log kappa_i - alpha_i^2 / kappa_i - log 2pi) / 2
    F = -sum lpd_i
    dF/dtheta_j = sum_ab W_ab dK_y,ab / dtheta_j,  W = K_y^-1 diag(c) K_y^-1 - (h alpha^T + alpha h^T) / 2,
    c_i = (1 + alpha_i^2 / kappa_i) / (2 kappa_i),  g_i = alpha_i / kappa_i,  h = K_y^-1 g;  dF/dnoise = tr W,  dF/dc = -sum h

``loo_brute`` is the definition itself: N refits without point i.

Test infrastructure: the Gram and derivative functions are ``oracle/gpr.py``'s, so r^2 has the fit's GEMM form
(``direct_r2=True``: r^2 from direct differences instead -- exactly 0 on the diagonal -- for the Matern-1/2, whose
sqrt amplifies the GEMM form's 1e-16 residue there to 1e-8).  Nothing here is imported by ``pygpso_amd``.
"""
import math

import numpy as np
import scipy.linalg as sla

from oracle import gpr

LOG_2PI = math.log(2.0 * math.pi)


def sqdist(X, X2, lengthscales, direct_r2=False):
    if not direct_r2:
        return gpr.scaled_sqdist(X, X2, lengthscales)
    ls = np.asarray(lengthscales, dtype=np.float64)
    A = np.asarray(X, dtype=np.float64) / ls
    B = A if X2 is None else np.asarray(X2, dtype=np.float64) / ls
    diff = A[:, None, :] - B[None, :, :]
    return np.sum(diff * diff, axis=-1)


def k_y(theta, X, s, direct_r2=False):
    """(K_y, r2, K): K_y = K + diag(noise + s)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    r2 = sqdist(X, None, theta.lengthscales, direct_r2)
    K = gpr.kernel_from_r2(theta.kernel, r2, theta.variance)
    Ky = K.copy()
    Ky[np.diag_indices(X.shape[0])] += theta.noise + np.asarray(s, dtype=np.float64).reshape(-1)
    return Ky, r2, K


def spd_inverse(Ky):
    """K_y^-1 = L^-T L^-1 through the Cholesky factor, as the fit forms it."""
    Linv = sla.solve_triangular(np.linalg.cholesky(Ky), np.eye(Ky.shape[0]), lower=True)
    return Linv.T @ Linv


def zeros_if_none(s, n):
    return np.zeros(n) if s is None else np.asarray(s, dtype=np.float64).reshape(-1)


def loo_closed(theta, X, y, s=None, direct_r2=False):
    """(mean, var, lpd, loss) from alpha and diag(K_y^-1)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    Ky, _, _ = k_y(theta, X, zeros_if_none(s, y.shape[0]), direct_r2)
    Kinv = spd_inverse(Ky)
    alpha = sla.cho_solve(sla.cho_factor(Ky, lower=True), y - theta.mean_c)
    kap = np.diag(Kinv)
    mean = y - alpha / kap
    var = 1.0 / kap
    lpd = 0.5 * np.log(kap) - 0.5 * alpha * alpha / kap - 0.5 * LOG_2PI
    return mean, var, lpd, float(-np.sum(lpd))


def loo_brute(theta, X, y, s=None, direct_r2=False):
    """The definition: for every i, the GP fitted to all points but i predicts y_i (variance: latent + noise + s_i)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.shape[0]
    s = zeros_if_none(s, n)
    Ky, _, _ = k_y(theta, X, s, direct_r2)
    mean, var = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        Kr = Ky[np.ix_(keep, keep)]
        k = Ky[keep, i]
        sol = sla.cho_solve(sla.cho_factor(Kr, lower=True), np.column_stack([y[keep] - theta.mean_c, k]))
        mean[i] = theta.mean_c + k @ sol[:, 0]
        var[i] = Ky[i, i] - k @ sol[:, 1]
    lpd = -0.5 * np.log(var) - 0.5 * (y - mean) ** 2 / var - 0.5 * LOG_2PI
    return mean, var, lpd, float(-np.sum(lpd))


def loo_loss_and_grad(theta, X, y, s=None, direct_r2=False):
    """F and dF / d(ls..., variance, noise, c) in the constrained theta."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.shape[0]
    Ky, r2, K = k_y(theta, X, zeros_if_none(s, n), direct_r2)
    Kinv = spd_inverse(Ky)
    alpha = sla.cho_solve(sla.cho_factor(Ky, lower=True), y - theta.mean_c)
    kap = np.diag(Kinv)
    q = alpha * alpha / kap
    loss = float(-np.sum(0.5 * np.log(kap) - 0.5 * q - 0.5 * LOG_2PI))
    c = 0.5 * (1.0 + q) / kap
    h = Kinv @ (alpha / kap)
    W = Kinv @ (c[:, None] * Kinv) - 0.5 * (np.outer(h, alpha) + np.outer(alpha, h))
    n_ls = theta.lengthscales.shape[0]
    g = np.empty(n_ls + 3)
    if n_ls == 1:
        g[0] = np.sum(W * gpr.dk_dlengthscale_iso(theta.kernel, r2, K, theta.variance, float(theta.lengthscales[0])))
    else:
        Wd = W * gpr._dk_dr2(theta.kernel, r2, K, theta.variance)
        for k in range(n_ls):
            diff = X[:, k][:, None] - X[:, k][None, :]
            g[k] = np.sum(Wd * (-2.0 * diff * diff / theta.lengthscales[k] ** 3))
    g[n_ls] = np.sum(W * K) / theta.variance
    g[n_ls + 1] = np.trace(W)
    g[n_ls + 2] = -np.sum(h)
    return loss, g


def loo_loss_and_grad_u(kernel, u, X, y, s=None, train_mean=True, mean_c_fixed=0.0):
    """F(u), dF/du in the optimiser's variables (``gpr.Theta.unpack``'s transforms and their chain rule); u without the
    mean's slot when ``train_mean`` is False.  Returns (loss, grad_u, theta)."""
    u = np.asarray(u, dtype=np.float64)
    full = u if train_mean else np.concatenate([u, [mean_c_fixed]])
    theta = gpr.Theta.unpack(kernel, full)
    f, g = loo_loss_and_grad(theta, X, y, s)
    n_ls = theta.lengthscales.shape[0]
    gu = g[: n_ls + 2] * gpr.sigmoid(u[: n_ls + 2])
    if train_mean:
        gu = np.concatenate([gu, [g[n_ls + 2]]])
    return f, gu, theta


def search_problem(n=30, seed=5):
    """The hyper-parameter search of the GPU tests: ``n`` seeded points of the unit square scored by the toy objective of
    ``tests/helpers.py`` over its bounds x in [-3, 5], y in [-3, 3].  Returns (coords [n, 2], scores [n])."""
    from tests.helpers import rotated_peaks

    coords = np.random.default_rng(seed).random((n, 2))
    scores = np.array([rotated_peaks((-3.0 + 8.0 * c[0], -3.0 + 6.0 * c[1])) for c in coords])
    return coords, scores
