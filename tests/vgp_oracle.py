"""
Float64 numpy / scipy restatement of GPflow 2's whitened ``VGP`` with a Gaussian likelihood -- the checker of the
device VGP path (pygpso_amd/csrc/vgp.hip, ``pygpso_amd.model.HipVGP``).  Test infrastructure only: the product never
imports it.

Parameters (as ``HipGPR``): u = [softplus^-1 lengthscales..., softplus^-1 variance, softplus^-1 (sigma^2 - 1e-6)
[, c when the mean is trained]].  Variational state: q(v) = N(mu, S S^T), S lower triangular.  K = k(X, X) + 1e-6 I
(GPflow's default jitter), L = chol(K), f = L v + c.
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


def _ls_full(ls, d):
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    return np.full(d, ls[0]) if ls.shape[0] == 1 else ls


def kmat(kernel, X, ls, var, X2=None):
    ls = _ls_full(ls, X.shape[1])
    return gpr.gram(kernel, X, X if X2 is None else X2, ls, var)


def chol_k(kernel, X, ls, var):
    K = kmat(kernel, X, ls, var) + JITTER * np.eye(X.shape[0])
    return np.linalg.cholesky(K)


def neg_elbo(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S):
    ls, var, s2, c = unpack(u, n_ls, train_mean, c_fixed)
    L = chol_k(kernel, X, ls, var)
    return _neg_elbo_L(L, s2, c, y, mu, S)


def _neg_elbo_L(L, s2, c, y, mu, S):
    n = y.shape[0]
    fmean = L @ mu + c
    LS = L @ S
    fvar = np.sum(LS * LS, axis=1)
    r = y - fmean
    data = np.sum(0.5 * np.log(2.0 * np.pi * s2) + (r * r + fvar) / (2.0 * s2))
    kl = 0.5 * (np.sum(S * S) + mu @ mu - n - np.sum(np.log(np.diag(S) ** 2)))
    return float(data + kl)


def neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S):
    """-ELBO and its gradient in u at fixed q (closed form through the Cholesky factor).  Returns (loss, grad_u, theta)
    with theta = (lengthscales..., variance, sigma^2, c)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    u = np.asarray(u, dtype=np.float64)
    n, d = X.shape
    ls, var, s2, c = unpack(u, n_ls, train_mean, c_fixed)
    lsf = _ls_full(ls, d)
    r2 = gpr.scaled_sqdist(X, None, lsf)
    Kf = gpr.kernel_from_r2(kernel, r2, var)
    L = np.linalg.cholesky(Kf + JITTER * np.eye(n))
    loss = _neg_elbo_L(L, s2, c, y, mu, S)
    Sig = S @ S.T
    fmean = L @ mu + c
    LS = L @ S
    fvar = np.sum(LS * LS, axis=1)
    r = y - fmean
    Lbar = np.tril((L @ Sig - np.outer(r, mu)) / s2)
    P = L.T @ Lbar
    P = np.tril(P) - 0.5 * np.diag(np.diag(P))
    Linv = scipy.linalg.solve_triangular(L, np.eye(n), lower=True)
    Kbar = 0.5 * Linv.T @ (P + P.T) @ Linv
    g_ls = np.empty(n_ls)
    if n_ls == 1:
        g_ls[0] = np.sum(Kbar * gpr.dk_dlengthscale_iso(kernel, r2, Kf, var, float(ls[0])))
    else:
        dkdr2 = gpr._dk_dr2(kernel, r2, Kf, var)
        for k in range(d):
            diff = X[:, k][:, None] - X[:, k][None, :]
            g_ls[k] = np.sum(Kbar * dkdr2 * (-2.0 * diff * diff / lsf[k] ** 3))
    g_var = np.sum(Kbar * Kf) / var
    g_s2 = n / (2.0 * s2) - np.sum(r * r + fvar) / (2.0 * s2 * s2)
    g_c = -np.sum(r) / s2
    sig = gpr.sigmoid(u)
    gu = np.empty(n_ls + 2 + (1 if train_mean else 0))
    gu[:n_ls] = g_ls * sig[:n_ls]
    gu[n_ls] = g_var * sig[n_ls]
    gu[n_ls + 1] = g_s2 * sig[n_ls + 1]
    if train_mean:
        gu[n_ls + 2] = g_c
    theta = np.concatenate([np.atleast_1d(ls), [var, s2, c]])
    return loss, gu, theta


def natgrad(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, gamma=1.0):
    """One natural-gradient step on q at fixed theta (GPflow's NaturalGradient, conjugate likelihood)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.shape[0]
    ls, var, s2, c = unpack(u, n_ls, train_mean, c_fixed)
    L = chol_k(kernel, X, ls, var)
    lam = np.eye(n) + L.T @ L / s2
    h = L.T @ (y - c) / s2
    if gamma != 1.0:
        Sinv = scipy.linalg.solve_triangular(S, np.eye(n), lower=True)
        lam_cur = Sinv.T @ Sinv
        lam = (1.0 - gamma) * lam_cur + gamma * lam
        h = (1.0 - gamma) * (lam_cur @ mu) + gamma * h
    V = scipy.linalg.solve_triangular(np.linalg.cholesky(lam), np.eye(n), lower=True)
    Sig = V.T @ V
    mu_new = Sig @ h
    return mu_new, np.linalg.cholesky(Sig)


class Posterior:
    """The predictive of the model at theta: mean = k*^T L^-T mu + c, var_f = k** - |L^-1 k*|^2 + |S^T L^-1 k*|^2."""

    def __init__(self, kernel, u, n_ls, train_mean, c_fixed, X, mu, S):
        self.kernel = kernel
        self.ls, self.var, self.s2, self.c = unpack(u, n_ls, train_mean, c_fixed)
        self.X = np.asarray(X, dtype=np.float64)
        self.L = chol_k(kernel, self.X, self.ls, self.var)
        self.mu, self.S = mu, S

    def predict_f(self, Xs, triangular=False):
        Xs = np.asarray(Xs, dtype=np.float64)
        ks = kmat(self.kernel, self.X, self.ls, self.var, Xs)  # [N, M]
        A = scipy.linalg.solve_triangular(self.L, ks, lower=True)
        mean = A.T @ self.mu + self.c
        if triangular:
            n = self.mu.shape[0]
            J = np.eye(n)[::-1]
            G = np.linalg.cholesky(J @ (np.eye(n) - self.S @ self.S.T) @ J)
            R = J @ G.T @ J
            var = self.var - np.sum((R @ A) ** 2, axis=0)
        else:
            var = self.var - np.sum(A * A, axis=0) + np.sum((self.S.T @ A) ** 2, axis=0)
        return mean, var

    def predict_y(self, Xs, triangular=False):
        m, v = self.predict_f(Xs, triangular)
        return m, v + self.s2


class Adam:
    """Keras's Adam (beta1 0.9, beta2 0.999, epsilon 1e-7) on a flat vector; state persists across calls."""

    def __init__(self, lr=0.01, beta1=0.9, beta2=0.999, eps=1.0e-7):
        self.lr, self.b1, self.b2, self.eps = lr, beta1, beta2, eps
        self.m = self.v = None
        self.t = 0

    def step(self, u, g):
        if self.m is None or self.m.shape != g.shape:
            self.m = np.zeros_like(g)
            self.v = np.zeros_like(g)
        self.t += 1
        self.m = self.b1 * self.m + (1.0 - self.b1) * g
        self.v = self.b2 * self.v + (1.0 - self.b2) * g * g
        a = self.lr * math.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        return u - a * self.m / (np.sqrt(self.v) + self.eps)


def train(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, iterations, gamma=1.0, adam=None):
    """The reference's VGPSurrogate._gp_train loop: per iteration one natgrad step on q, one Adam step on theta."""
    adam = adam if adam is not None else Adam()
    u = np.asarray(u, dtype=np.float64).copy()
    for _ in range(iterations):
        mu, S = natgrad(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, gamma)
        _, g, _ = neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S)
        u = adam.step(u, g)
    return u, mu, S, adam


def initial_u(lengthscales, variance, s2, c=None):
    parts = [np.atleast_1d(gpr.softplus_inv(np.asarray(lengthscales, dtype=np.float64))),
             [float(gpr.softplus_inv(variance))], [float(gpr.softplus_inv(s2 - NOISE_FLOOR))]]
    if c is not None:
        parts.append([float(c)])
    return np.concatenate(parts)
