"""
Float64 numpy / scipy restatement of GPflow 2's ``SGPR`` (Titsias 2009) with a Gaussian likelihood and fixed inducing
points -- the checker of the device SGPR path (pygpso_amd/csrc/sgpr.hip, ``pygpso_amd.sgpr.HipSGPR``).  Test
infrastructure only: the product never imports it.

Parameters (as ``HipGPR``): u = [softplus^-1 lengthscales..., softplus^-1 variance, softplus^-1 (sigma^2 - 1e-6)
[, c when the mean is trained]].  Z [M x D] is given.  Kuu = k(Z, Z) + 1e-6 I (GPflow's default jitter), Lu = chol Kuu,
A = Lu^-1 Kuf / sigma, B = I + A A^T, LB = chol B, cv = LB^-1 A (y - c) / sigma.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg

from oracle import gpr

JITTER = 1.0e-6
NOISE_FLOOR = 1.0e-6


def unpack(u, n_ls, train_mean, c_fixed=0.0):
    u = np.asarray(u, dtype=np.float64)
    ls = gpr.softplus(u[:n_ls])
    var = float(gpr.softplus(u[n_ls]))
    s2 = NOISE_FLOOR + float(gpr.softplus(u[n_ls + 1]))
    c = float(u[n_ls + 2]) if train_mean else float(c_fixed)
    return ls, var, s2, c


def initial_u(lengthscales, variance, s2, c=None):
    parts = [np.atleast_1d(gpr.softplus_inv(np.asarray(lengthscales, dtype=np.float64))),
             [float(gpr.softplus_inv(variance))], [float(gpr.softplus_inv(s2 - NOISE_FLOOR))]]
    if c is not None:
        parts.append([float(c)])
    return np.concatenate(parts)


def _ls_full(ls, d):
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    return np.full(d, ls[0]) if ls.shape[0] == 1 else ls


def kmat(kernel, X, ls, var, X2=None):
    ls = _ls_full(ls, X.shape[1])
    return gpr.gram(kernel, X, X if X2 is None else X2, ls, var)


def _tri(L, b, trans=False):
    return scipy.linalg.solve_triangular(L, b, lower=True, trans=1 if trans else 0)


class Factors:
    """Everything the bound, its gradient and the predictive share at one theta."""

    def __init__(self, kernel, ls, var, s2, c, X, y, Z):
        self.kernel, self.var, self.s2, self.c = kernel, float(var), float(s2), float(c)
        self.X = np.asarray(X, dtype=np.float64)
        self.Z = np.asarray(Z, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.ls = _ls_full(ls, self.X.shape[1])
        n, m = self.X.shape[0], self.Z.shape[0]
        sig = math.sqrt(self.s2)
        self.e = self.y - self.c
        self.Kuu = kmat(kernel, self.Z, self.ls, self.var) + JITTER * np.eye(m)
        self.Kuf = kmat(kernel, self.Z, self.ls, self.var, self.X)  # [M, N]
        self.Lu = np.linalg.cholesky(self.Kuu)
        self.A = _tri(self.Lu, self.Kuf) / sig
        self.AAT = self.A @ self.A.T
        self.B = np.eye(m) + self.AAT
        self.LB = np.linalg.cholesky(self.B)
        self.cv = _tri(self.LB, self.A @ self.e) / sig
        self.bound = (-0.5 * n * math.log(2.0 * math.pi) - np.sum(np.log(np.diag(self.LB))) - 0.5 * n * math.log(self.s2)
                      - 0.5 * (self.e @ self.e) / self.s2 + 0.5 * (self.cv @ self.cv)
                      - 0.5 * n * self.var / self.s2 + 0.5 * np.trace(self.AAT))


def factors(kernel, u, n_ls, train_mean, c_fixed, X, y, Z):
    ls, var, s2, c = unpack(u, n_ls, train_mean, c_fixed)
    return Factors(kernel, ls, var, s2, c, X, y, Z)


def bound(kernel, u, n_ls, train_mean, c_fixed, X, y, Z):
    return float(factors(kernel, u, n_ls, train_mean, c_fixed, X, y, Z).bound)


def _contract(kernel, W, P, Q, lsf, n_ls, var, square):
    """sum_ij W_ij dk(P_i, Q_j)/d(lengthscales..., variance)."""
    r2 = gpr.scaled_sqdist(P, None if square else Q, lsf)
    K = gpr.kernel_from_r2(kernel, r2, var)
    g = np.empty(n_ls + 1)
    if n_ls == 1:
        g[0] = np.sum(W * gpr.dk_dlengthscale_iso(kernel, r2, K, var, float(lsf[0])))
    else:
        dkdr2 = gpr._dk_dr2(kernel, r2, K, var)
        for k in range(P.shape[1]):
            diff = P[:, k][:, None] - Q[:, k][None, :]
            g[k] = np.sum(W * dkdr2 * (-2.0 * diff * diff / lsf[k] ** 3))
    g[n_ls] = np.sum(W * K) / var
    return g


def neg_bound_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, Z):
    """-bound and its gradient in u (closed form; the triangular factors stand where the formulas write an inverse).
    Returns (loss, grad_u, theta) with theta = (lengthscales..., variance, sigma^2, c)."""
    u = np.asarray(u, dtype=np.float64)
    f = factors(kernel, u, n_ls, train_mean, c_fixed, X, y, Z)
    n, m = f.X.shape[0], f.Z.shape[0]
    b = 1.0 / f.s2
    Lui = _tri(f.Lu, np.eye(m))
    T1 = _tri(f.LB, Lui)                     # LB^-1 Lu^-1
    Qinv = T1.T @ T1
    Kuuinv = Lui.T @ Lui
    a = f.s2 * (T1.T @ f.cv)                 # Q^-1 Kuf e
    w = f.Kuf.T @ a
    dKuf = b * (Kuuinv - Qinv) @ f.Kuf + np.outer(a, b * b * f.e - b ** 3 * w)
    dKuu = 0.5 * (Kuuinv - Qinv - b * b * np.outer(a, a) - Lui.T @ f.AAT @ Lui)
    ls = np.atleast_1d(gpr.softplus(u[:n_ls]))
    g = _contract(kernel, dKuf, f.Z, f.X, f.ls, n_ls, f.var, False) + _contract(kernel, dKuu, f.Z, f.Z, f.ls, n_ls, f.var, True)
    g[n_ls] += -0.5 * b * n
    tr_binv = np.sum(_tri(f.LB, np.eye(m)) ** 2)
    dF_db = (0.5 * n / b - 0.5 * f.s2 * (m - tr_binv) - 0.5 * (f.e @ f.e) + b * (f.e @ w) - 0.5 * b * b * (w @ w)
             - 0.5 * n * f.var + 0.5 * f.s2 * np.trace(f.AAT))
    dF_ds2 = -b * b * dF_db
    dF_dc = b * np.sum(f.e) - b * b * np.sum(w)
    sig = gpr.sigmoid(u)
    gu = np.empty(n_ls + 2 + (1 if train_mean else 0))
    gu[:n_ls] = -g[:n_ls] * sig[:n_ls]
    gu[n_ls] = -g[n_ls] * sig[n_ls]
    gu[n_ls + 1] = -dF_ds2 * sig[n_ls + 1]
    if train_mean:
        gu[n_ls + 2] = -dF_dc
    theta = np.concatenate([ls, [f.var, f.s2, f.c]])
    return float(-f.bound), gu, theta


def shifted_root(B, delta=None):
    """R (lower) with I - B^-1 / (1 + delta) = R^T R, for the smallest delta of 0, 1e-8, 2e-8, ... that factors (or the
    delta given).  Returns (R, delta)."""
    m = B.shape[0]
    Binv = np.linalg.inv(B)
    Binv = 0.5 * (Binv + Binv.T)
    J = np.eye(m)[::-1]
    d = 0.0 if delta is None else float(delta)
    while True:
        try:
            G = np.linalg.cholesky(J @ (np.eye(m) - Binv / (1.0 + d)) @ J)
            return J @ G.T @ J, d
        except np.linalg.LinAlgError:
            if delta is not None or d > 1.0:
                raise
            d = 1.0e-8 if d == 0.0 else 2.0 * d


class Posterior:
    """The predictive at theta.  predict_f is GPflow's two-term form; ``installed`` builds what the device installs over
    the rows Z: C = sqrt(1 + delta) R Lu^-1, beta = Lu^-T LB^-T cv, noise slot sigma^2 + delta variance."""

    def __init__(self, kernel, u, n_ls, train_mean, c_fixed, X, y, Z):
        self.f = factors(kernel, u, n_ls, train_mean, c_fixed, X, y, Z)
        self.kernel = kernel

    def _ks(self, Xs):
        f = self.f
        return kmat(self.kernel, f.Z, f.ls, f.var, np.asarray(Xs, dtype=np.float64))  # [M, m*]

    def predict_f(self, Xs):
        f = self.f
        t1 = _tri(f.Lu, self._ks(Xs))
        t2 = _tri(f.LB, t1)
        return t2.T @ f.cv + f.c, f.var - np.sum(t1 * t1, axis=0) + np.sum(t2 * t2, axis=0)

    def predict_y(self, Xs):
        mean, var = self.predict_f(Xs)
        return mean, var + self.f.s2

    def installed(self, delta=None):
        f = self.f
        m = f.Z.shape[0]
        R, d = shifted_root(f.B, delta)
        C = math.sqrt(1.0 + d) * R @ _tri(f.Lu, np.eye(m))
        beta = _tri(f.Lu, _tri(f.LB, f.cv, trans=True), trans=True)
        return C, beta, f.s2 + d * f.var, d

    def predict_y_installed(self, Xs, delta=None):
        C, beta, noise, _ = self.installed(delta)
        ks = self._ks(Xs)
        return ks.T @ beta + self.f.c, self.f.var - np.sum((C @ ks) ** 2, axis=0) + noise

    def best_ucb(self, Xs, varsigma=gpr.VARSIGMA_DEFAULT):
        mean, var = self.predict_y(Xs)
        ucb = mean + varsigma * var
        i = int(np.argmax(ucb))
        return i, float(mean[i]), float(var[i]), float(ucb[i])


def greedy_select(kernel, X, ls, var, m, return_margin=False):
    """Greedy conditional-variance selection = pivoted partial Cholesky of k(X, X): returns the M picked row indices (and
    the smallest relative margin between the pick and the runner-up over the steps after the first).  A largest remaining
    conditional variance at or below 1e-12 variance ends it with LinAlgError (k(X, X) numerically of rank < M)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    lsf = _ls_full(ls, X.shape[1])
    dvec = np.full(n, float(var))
    L = np.zeros((n, m))
    picked = np.zeros(n, dtype=bool)
    idx = np.empty(m, dtype=np.int64)
    margin = np.inf
    for j in range(m):
        cand = np.where(picked, -np.inf, dvec)
        p = int(np.argmax(cand))  # (numpy: the first of equal maxima = the lowest index)
        if j > 0 and n > j + 1:
            second = np.partition(cand, -2)[-2]
            margin = min(margin, (cand[p] - second) / cand[p])
        if not cand[p] > 1.0e-12 * float(var):
            raise np.linalg.LinAlgError(f"greedy selection: k(X, X) is numerically of rank {j} < m={m}")
        idx[j] = p
        picked[p] = True
        col = gpr.gram(kernel, X, X[p:p + 1], lsf, var)[:, 0]
        col = (col - L[:, :j] @ L[p, :j]) / math.sqrt(dvec[p])
        L[:, j] = col
        dvec = dvec - col * col
    return (idx, float(margin)) if return_margin else idx


def choose_inducing(kernel, X, ls, var, m):
    """Z as SGPRSurrogate chooses it: X itself while N <= M, the greedy picks beyond."""
    X = np.asarray(X, dtype=np.float64)
    return X.copy() if X.shape[0] <= m else X[greedy_select(kernel, X, ls, var, m)]
