"""
Float64 numpy / scipy restatement of GPflow 2's ``SVGP`` (whitened, full q_sqrt, full batch, inducing points Z fixed) with
the Gaussian or the Student-t likelihood -- the checker of the device SVGP path (pygpso_amd/csrc/svgp.hip,
engine_variational.hip EngineCore::svgp_*, ``pygpso_amd.svgp.HipSVGP``).  Test infrastructure only: the product never imports it.

A likelihood is ``(kind, df)`` as in tests/vgp_studentt_oracle.py: ``("Gaussian", None)`` (closed form), ``("GaussianGH",
None)`` (the same Gaussian through 20-point Gauss-Hermite quadrature) or ``("StudentT", df)``; u as the VGP's.

Kuu = k(Z, Z) + 1e-6 I, Lu = chol Kuu, A = Lu^-1 Kuf, q(v) = N(mu, S S^T):  m_i = A_i^T mu + c,  v_i = variance - |A_i|^2 +
|S^T A_i|^2,  -ELBO = -sum VE_i(m_i, v_i) + KL(q || N(0, I)).  Natural gradient at the current q: Lambda* = I + A diag(a)
A^T, h* = A (g_m + a (m - c)), a = -2 dVE/dv, mixed with q's natural parameters by gamma.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg

from oracle import gpr
from tests import sgpr_oracle as S_
from tests import vgp_studentt_oracle as T

JITTER = S_.JITTER


def unpack(u, n_ls, train_mean, c_fixed, lik):
    """(lengthscales, variance, p, c): p the Student-t scale or the Gaussian variance."""
    return T.unpack(u, n_ls, train_mean, c_fixed, lik)


def _tri(L, b, trans=False):
    return scipy.linalg.solve_triangular(L, b, lower=True, trans=1 if trans else 0)


class Factors:
    def __init__(self, kernel, u, n_ls, train_mean, c_fixed, X, Z, lik):
        self.kernel = kernel
        self.X = np.asarray(X, dtype=np.float64)
        self.Z = np.asarray(Z, dtype=np.float64)
        ls, self.var, self.p, self.c = unpack(u, n_ls, train_mean, c_fixed, lik)
        self.ls = S_._ls_full(ls, self.X.shape[1])
        m = self.Z.shape[0]
        self.Kuu = S_.kmat(kernel, self.Z, self.ls, self.var) + JITTER * np.eye(m)
        self.Kuf = S_.kmat(kernel, self.Z, self.ls, self.var, self.X)
        self.Lu = np.linalg.cholesky(self.Kuu)
        self.A = _tri(self.Lu, self.Kuf)


def moments(A, mu, S, var, c):
    B = S.T @ A
    return A.T @ mu + c, var - np.sum(A * A, axis=0) + np.sum(B * B, axis=0)


def pointwise(lik, y, m, v, p):
    """Per point: VE, g_m = dVE/dm, g_v = dVE/dv, dVE/dp (closed form for "Gaussian", else the quadrature)."""
    if lik[0] == "Gaussian":
        e = np.asarray(y, dtype=np.float64) - m
        q = e * e + v
        return (-0.5 * math.log(2.0 * math.pi * p) - 0.5 * q / p, e / p, np.full_like(m, -0.5 / p),
                -0.5 / p + 0.5 * q / (p * p))
    return T.quadrature(lik, y, m, v, p)


def kl(mu, S):
    return T._kl(mu, S)


def neg_elbo(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, S, lik):
    f = Factors(kernel, u, n_ls, train_mean, c_fixed, X, Z, lik)
    m, v = moments(f.A, mu, S, f.var, f.c)
    ve = pointwise(lik, np.asarray(y, dtype=np.float64).reshape(-1), m, v, f.p)[0]
    return float(-np.sum(ve) + kl(mu, S))


def neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, S, lik):
    """-ELBO and its gradient in u at fixed q and Z.  Returns (loss, grad_u, theta = (lengthscales..., variance, p, c)).
    Abar = dELBO/dA = mu g_m^T + 2 (Sigma - I) A diag(g_v); dELBO/dKuf = Lu^-T Abar; d(-ELBO)/dLu = tril(Lu^-T Abar A^T),
    taken to Kuu by the Cholesky backward pass; d v_i / d variance = 1."""
    u = np.asarray(u, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    f = Factors(kernel, u, n_ls, train_mean, c_fixed, X, Z, lik)
    M = f.Z.shape[0]
    m, v = moments(f.A, mu, S, f.var, f.c)
    ve, gm, gv, dve = pointwise(lik, y, m, v, f.p)
    loss = float(-np.sum(ve) + kl(mu, S))
    Sig = S @ S.T
    Abar = np.outer(mu, gm) + 2.0 * (Sig - np.eye(M)) @ (f.A * gv[None, :])
    dKuf = _tri(f.Lu, Abar, trans=True)
    Lbar = np.tril(dKuf @ f.A.T)  # (of -ELBO)
    P = f.Lu.T @ Lbar
    P = np.tril(P) - 0.5 * np.diag(np.diag(P))
    Lui = _tri(f.Lu, np.eye(M))
    Kbar = 0.5 * Lui.T @ (P + P.T) @ Lui
    g = (S_._contract(kernel, Kbar, f.Z, f.Z, f.ls, n_ls, f.var, True)
         - S_._contract(kernel, dKuf, f.Z, f.X, f.ls, n_ls, f.var, False))
    g[n_ls] -= np.sum(gv)
    sig = gpr.sigmoid(u)
    gu = np.empty(n_ls + 2 + (1 if train_mean else 0))
    gu[:n_ls + 1] = g * sig[:n_ls + 1]
    gu[n_ls + 1] = -np.sum(dve) * sig[n_ls + 1]
    if train_mean:
        gu[n_ls + 2] = -np.sum(gm)
    theta = np.concatenate([np.atleast_1d(gpr.softplus(u[:n_ls])), [f.var, f.p, f.c]])
    return loss, gu, theta


def natural_params(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, S, lik, gamma=1.0, conj_s2=None):
    """(Lambda, h) of one step at the current q; conj_s2: the Gaussian step at that noise variance (the conjugate start)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    f = Factors(kernel, u, n_ls, train_mean, c_fixed, X, Z, lik)
    M = f.Z.shape[0]
    m, v = moments(f.A, mu, S, f.var, f.c)
    if conj_s2 is not None:
        _, gm, gv, _ = pointwise(("Gaussian", None), y, m, v, conj_s2)
    else:
        _, gm, gv, _ = pointwise(lik, y, m, v, f.p)
    a = -2.0 * gv
    lam = np.eye(M) + (f.A * a[None, :]) @ f.A.T
    h = f.A @ (gm + a * (m - f.c))
    if gamma != 1.0:
        Sinv = _tri(S, np.eye(M))
        lam_cur = Sinv.T @ Sinv
        lam = (1.0 - gamma) * lam_cur + gamma * lam
        h = (1.0 - gamma) * (lam_cur @ mu) + gamma * h
    return lam, h


def natgrad(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, S, lik, gamma=1.0, conj_s2=None):
    """One natural-gradient step on q; numpy.linalg.LinAlgError when a factorisation fails."""
    lam, h = natural_params(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, S, lik, gamma, conj_s2)
    M = h.shape[0]
    Vm = _tri(np.linalg.cholesky(lam), np.eye(M))
    Sig = Vm.T @ Vm
    return Sig @ h, np.linalg.cholesky(Sig)


def conjugate_start(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, lik, s2):
    M = np.asarray(Z).shape[0]
    return natgrad(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, np.zeros(M), np.eye(M), lik, 1.0, conj_s2=s2)


def predictive_noise(lik, p):
    return T.predictive_noise(lik, p)


class Posterior:
    """The predictive at theta: mean = k*u^T Lu^-T mu + c, var_f = k** - |Lu^-1 k*u|^2 + |S^T Lu^-1 k*u|^2; ``installed``:
    what the device installs over the rows Z (C = sqrt(1 + delta) R Lu^-1, I - S S^T / (1 + delta) = R^T R, beta =
    Lu^-T mu, noise slot the likelihood's variance + delta variance)."""

    def __init__(self, kernel, u, n_ls, train_mean, c_fixed, X, Z, mu, S, lik):
        self.f = Factors(kernel, u, n_ls, train_mean, c_fixed, X, Z, lik)
        self.kernel, self.mu, self.S = kernel, np.asarray(mu, dtype=np.float64), np.asarray(S, dtype=np.float64)
        self.noise = predictive_noise(lik, self.f.p)

    def _ks(self, Xs):
        f = self.f
        return S_.kmat(self.kernel, f.Z, f.ls, f.var, np.asarray(Xs, dtype=np.float64))

    def predict_f(self, Xs):
        B = _tri(self.f.Lu, self._ks(Xs))
        mean, var = moments(B, self.mu, self.S, self.f.var, self.f.c)
        return mean, var

    def predict_y(self, Xs):
        mean, var = self.predict_f(Xs)
        return mean, var + self.noise

    def installed(self):
        f = self.f
        M = f.Z.shape[0]
        d = T.install_shift(self.S)
        J = np.eye(M)[::-1]
        G = np.linalg.cholesky(J @ (np.eye(M) - self.S @ self.S.T / (1.0 + d)) @ J)
        R = J @ G.T @ J
        C = math.sqrt(1.0 + d) * R @ _tri(f.Lu, np.eye(M))
        beta = _tri(f.Lu, self.mu, trans=True)
        return C, beta, self.noise + d * f.var, d

    def predict_y_installed(self, Xs):
        C, beta, noise, _ = self.installed()
        ks = self._ks(Xs)
        return ks.T @ beta + self.f.c, self.f.var - np.sum((C @ ks) ** 2, axis=0) + noise


def train(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, S, iterations, gamma, adam, lik):
    """SVGPSurrogate._gp_train after q's start: per iteration one natgrad step on q, one Adam step on theta."""
    u = np.asarray(u, dtype=np.float64).copy()
    for _ in range(iterations):
        mu, S = natgrad(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, S, lik, gamma)
        _, g, _ = neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, S, lik)
        u = adam.step(u, g)
    return u, mu, S, adam


def initial_u(lengthscales, variance, p, lik, c=None):
    """u for the likelihood: p the Student-t scale (softplus^-1, no shift) or the Gaussian variance (1e-6 shift)."""
    if lik[0] == "StudentT":
        return T.initial_u(lengthscales, variance, p, c)
    return S_.initial_u(lengthscales, variance, p, c)
