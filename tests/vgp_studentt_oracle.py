"""
Float64 numpy restatement of GPflow 2's whitened ``VGP`` with a general scalar likelihood -- ``StudentT(scale, df)``, or the
Gaussian through the same quadrature -- the checker of the device's quadrature path (pygpso_amd/csrc/vgp.hip:
vgp_quad_kernel and friends; engine_variational.hip EngineCore::vgp_*).  Test infrastructure only: the product never imports it.

What GPflow does: ``ScalarLikelihood.variational_expectations`` by Gauss-Hermite quadrature with 20 points (nodes x sqrt(2),
weights / sqrt(pi)), the -ELBO as -sum VE + KL, its gradient by autodiff (the derivatives of the quadrature sum, below), and
``NaturalGradient`` (XiNat) at the current q: Lambda* = I + L^T diag(a) L, h* = L^T (g_m + a (m - c)), a = -2 dVE/dv.

A likelihood is ``(kind, df)``: ``("StudentT", df)`` with u[n_ls + 1] = softplus^-1(scale), or ``("GaussianGH", None)``
with u[n_ls + 1] = softplus^-1(sigma^2 - 1e-6) as in tests/vgp_oracle.py.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg
from scipy.special import gammaln

from oracle import gpr
from tests import vgp_oracle as V

N_GH = 20


def gh_rule(n_gh=N_GH):
    x, w = np.polynomial.hermite.hermgauss(n_gh)
    return x * np.sqrt(2.0), w / np.sqrt(np.pi)


def unpack(u, n_ls, train_mean, c_fixed, lik):
    """(lengthscales, variance, p, c): p the Student-t scale or the Gaussian variance."""
    ls, var, s2, c = V.unpack(u, n_ls, train_mean, c_fixed)
    if lik[0] == "StudentT":
        return ls, var, float(gpr.softplus(np.asarray(u, dtype=np.float64)[n_ls + 1])), c
    return ls, var, s2, c


def log_const(lik, p):
    if lik[0] == "StudentT":
        nu = lik[1]
        return gammaln(0.5 * (nu + 1.0)) - gammaln(0.5 * nu) - 0.5 * (math.log(p * p) + math.log(nu) + math.log(math.pi))
    return -0.5 * (math.log(2.0 * math.pi) + math.log(p))


def logdensity(lik, y, f, p):
    """psi(f) = log p(y | f), psi'(f) and d psi / dp (element-wise)."""
    e = np.asarray(y, dtype=np.float64) - f
    cst = log_const(lik, p)
    if lik[0] == "StudentT":
        nu = lik[1]
        den = nu * p * p + e * e
        psi = cst - 0.5 * (nu + 1.0) * np.log1p(e * e / (nu * p * p))
        return psi, (nu + 1.0) * e / den, -1.0 / p + (nu + 1.0) * e * e / (p * den)
    return cst - e * e / (2.0 * p), e / p, -0.5 / p + e * e / (2.0 * p * p)


def quadrature(lik, y, m, v, p, n_gh=N_GH):
    """Per point: VE, g_m = dVE/dm, g_v = dVE/dv, dVE/dp (the derivatives of the quadrature sum)."""
    x, w = gh_rule(n_gh)
    sv = np.sqrt(v)
    f = m[:, None] + sv[:, None] * x[None, :]
    psi, dpsi, dp = logdensity(lik, np.asarray(y, dtype=np.float64)[:, None], f, p)
    ve = psi @ w
    gm = dpsi @ w
    gv = (dpsi * x[None, :]) @ w / (2.0 * sv)
    return ve, gm, gv, dp @ w


def _moments(L, c, mu, S):
    m = L @ mu + c
    LS = L @ S
    return m, LS, np.sum(LS * LS, axis=1)


def _kl(mu, S):
    n = mu.shape[0]
    return 0.5 * (np.sum(S * S) + mu @ mu - n - np.sum(np.log(np.diag(S) ** 2)))


def neg_elbo(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, lik):
    ls, var, p, c = unpack(u, n_ls, train_mean, c_fixed, lik)
    L = V.chol_k(kernel, X, ls, var)
    m, _, v = _moments(L, c, mu, S)
    ve, _, _, _ = quadrature(lik, y, m, v, p)
    return float(-np.sum(ve) + _kl(mu, S))


def neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, lik):
    """-ELBO and its gradient in u at fixed q.  Returns (loss, grad_u, theta = (lengthscales..., variance, p, c))."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    u = np.asarray(u, dtype=np.float64)
    n, d = X.shape
    ls, var, p, c = unpack(u, n_ls, train_mean, c_fixed, lik)
    lsf = V._ls_full(ls, d)
    r2 = gpr.scaled_sqdist(X, None, lsf)
    Kf = gpr.kernel_from_r2(kernel, r2, var)
    L = np.linalg.cholesky(Kf + V.JITTER * np.eye(n))
    m, LS, v = _moments(L, c, mu, S)
    ve, gm, gv, dve = quadrature(lik, y, m, v, p)
    loss = float(-np.sum(ve) + _kl(mu, S))
    a = -2.0 * gv
    Lbar = np.tril(a[:, None] * (L @ (S @ S.T)) - np.outer(gm, mu))
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
    sig = gpr.sigmoid(u)
    gu = np.empty(n_ls + 2 + (1 if train_mean else 0))
    gu[:n_ls] = g_ls * sig[:n_ls]
    gu[n_ls] = g_var * sig[n_ls]
    gu[n_ls + 1] = -np.sum(dve) * sig[n_ls + 1]  # (d scale / du and d sigma^2 / du: both sigmoid(u))
    if train_mean:
        gu[n_ls + 2] = -np.sum(gm)
    theta = np.concatenate([np.atleast_1d(ls), [var, p, c]])
    return loss, gu, theta


def natural_params(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, lik, gamma=1.0):
    """The mixed natural parameters (Lambda, h) of one step at the current q."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.shape[0]
    ls, var, p, c = unpack(u, n_ls, train_mean, c_fixed, lik)
    L = V.chol_k(kernel, X, ls, var)
    m, _, v = _moments(L, c, mu, S)
    _, gm, gv, _ = quadrature(lik, y, m, v, p)
    a = -2.0 * gv
    lam = np.eye(n) + L.T @ (a[:, None] * L)
    h = L.T @ (gm + a * (m - c))
    if gamma != 1.0:
        Sinv = scipy.linalg.solve_triangular(S, np.eye(n), lower=True)
        lam_cur = Sinv.T @ Sinv
        lam = (1.0 - gamma) * lam_cur + gamma * lam
        h = (1.0 - gamma) * (lam_cur @ mu) + gamma * h
    return lam, h


def natgrad(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, lik, gamma=1.0):
    """One natural-gradient step on q at fixed theta; numpy.linalg.LinAlgError when Lambda is not positive definite."""
    lam, h = natural_params(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, lik, gamma)
    n = h.shape[0]
    Vm = scipy.linalg.solve_triangular(np.linalg.cholesky(lam), np.eye(n), lower=True)
    Sig = Vm.T @ Vm
    return Sig @ h, np.linalg.cholesky(Sig)


def predictive_noise(lik, p):
    return p * p * lik[1] / (lik[1] - 2.0) if lik[0] == "StudentT" else p


def install_shift(S):
    """The device install's delta: the first of 0, 1e-8, 2e-8, ... for which J (I - S S^T / (1 + delta)) J factorises."""
    n = S.shape[0]
    J = np.eye(n)[::-1]
    Sig = S @ S.T
    delta = 0.0
    while delta <= 1.0:
        try:
            np.linalg.cholesky(J @ (np.eye(n) - Sig / (1.0 + delta)) @ J)
            return delta
        except np.linalg.LinAlgError:
            delta = 1.0e-8 if delta == 0.0 else 2.0 * delta
    raise np.linalg.LinAlgError("no shift")


class Posterior(V.Posterior):
    """The predictive at theta: latent as tests/vgp_oracle.py, plus the likelihood's variance (Student-t: s^2 df / (df - 2)).
    ``installed=True``: the variance the device installs -- var_f + delta (k** - |L^-1 k*|^2) with delta = install_shift(S)
    (0 whenever S S^T < I)."""

    def __init__(self, kernel, u, n_ls, train_mean, c_fixed, X, mu, S, lik, installed=False):
        super().__init__(kernel, u, n_ls, train_mean, c_fixed, X, mu, S)
        self.s2 = predictive_noise(lik, unpack(u, n_ls, train_mean, c_fixed, lik)[2])
        self.delta = install_shift(S) if installed else 0.0

    def predict_f(self, Xs, triangular=False):
        mean, var = super().predict_f(Xs, triangular)
        if self.delta:
            ks = V.kmat(self.kernel, self.X, self.ls, self.var, np.asarray(Xs, dtype=np.float64))
            A = scipy.linalg.solve_triangular(self.L, ks, lower=True)
            var = var + self.delta * (self.var - np.sum(A * A, axis=0))
        return mean, var


def initial_u(lengthscales, variance, scale, c=None):
    """u for the Student-t: softplus^-1 of the lengthscales, the variance and the scale (no shift)[, c]."""
    u = V.initial_u(lengthscales, variance, 1.0, c)
    u[np.atleast_1d(lengthscales).shape[0] + 1] = float(gpr.softplus_inv(scale))
    return u


def train(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, iterations, gamma, adam, lik):
    """VGPSurrogate._gp_train: per iteration one natgrad step on q, one Adam step on theta."""
    u = np.asarray(u, dtype=np.float64).copy()
    for _ in range(iterations):
        mu, S = natgrad(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, lik, gamma)
        _, g, _ = neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, lik)
        u = adam.step(u, g)
    return u, mu, S, adam
