"""
Float64 numpy restatement of the whitened ``VGP`` under the Bernoulli likelihood with the EXACT probit link -- the checker of
the device's GPSO_LIK_BERNOULLI path (pygpso_amd/csrc/vgp.hip: vgp_lik_eval's branch; engine_variational.hip
EngineCore::vgp_*) and of the probit predictive (csrc/success.hpp).  Test infrastructure only: the product never imports it.

After the pattern of tests/vgp_studentt_oracle.py: Gauss-Hermite quadrature with 20 points (nodes x sqrt(2), weights /
sqrt(pi)), the -ELBO as -sum VE + KL, its gradient through the derivatives of the quadrature sum, the natural-gradient step
at the current q (Lambda* = I + L^T diag(a) L, h* = L^T (g_m + a (m - c)), a = -2 dVE/dv), the install and the latent
predictive (tests/vgp_oracle.py's ``Posterior``), and P(success) = Phi(mean / sqrt(1 + var)).

The labels: a point is a success (s = +1) iff y > 0.5, else s = -1; psi(f) = log Phi(s f) -- not GPflow's ``inv_probit``,
which mixes a 1e-3 jitter in.  The likelihood has no parameter: u keeps the layout of tests/vgp_oracle.py, slot n_ls + 1 is
decoded as there and read by nothing, and its gradient entry is exactly 0.0.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg
from scipy.special import log_ndtr

from oracle import gpr
from tests import vgp_oracle as V

N_GH = 20
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def gh_rule(n_gh=N_GH):
    x, w = np.polynomial.hermite.hermgauss(n_gh)
    return x * np.sqrt(2.0), w / np.sqrt(np.pi)


def signs(y):
    return np.where(np.asarray(y, dtype=np.float64) > 0.5, 1.0, -1.0)


def logdensity(s, f):
    """psi(f) = log Phi(s f) and psi'(f) = s phi(f) / Phi(s f) = s exp(-f^2 / 2 - log sqrt(2 pi) - psi) (element-wise)."""
    psi = log_ndtr(s * f)
    return psi, s * np.exp(-0.5 * f * f - HALF_LOG_2PI - psi)


def quadrature(y, m, v, n_gh=N_GH):
    """Per point: VE, g_m = dVE/dm, g_v = dVE/dv (the derivatives of the quadrature sum)."""
    x, w = gh_rule(n_gh)
    sv = np.sqrt(v)
    f = m[:, None] + sv[:, None] * x[None, :]
    psi, dpsi = logdensity(signs(y)[:, None], f)
    return psi @ w, dpsi @ w, (dpsi * x[None, :]) @ w / (2.0 * sv)


def _moments(L, c, mu, S):
    LS = L @ S
    return L @ mu + c, LS, np.sum(LS * LS, axis=1)


def _kl(mu, S):
    n = mu.shape[0]
    return 0.5 * (np.sum(S * S) + mu @ mu - n - np.sum(np.log(np.diag(S) ** 2)))


def neg_elbo(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S):
    ls, var, _, c = V.unpack(u, n_ls, train_mean, c_fixed)
    L = V.chol_k(kernel, np.asarray(X, dtype=np.float64), ls, var)
    m, _, v = _moments(L, c, mu, S)
    return float(-np.sum(quadrature(y, m, v)[0]) + _kl(mu, S))


def neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S):
    """-ELBO and its gradient in u at fixed q.  Returns (loss, grad_u, theta = (lengthscales..., variance, slot, c)); the
    entry of the likelihood slot is exactly 0.0."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    u = np.asarray(u, dtype=np.float64)
    n, d = X.shape
    ls, var, slot, c = V.unpack(u, n_ls, train_mean, c_fixed)
    lsf = V._ls_full(ls, d)
    r2 = gpr.scaled_sqdist(X, None, lsf)
    Kf = gpr.kernel_from_r2(kernel, r2, var)
    L = np.linalg.cholesky(Kf + V.JITTER * np.eye(n))
    m, LS, v = _moments(L, c, mu, S)
    ve, gm, gv = quadrature(y, m, v)
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
    gu[n_ls + 1] = 0.0
    if train_mean:
        gu[n_ls + 2] = -np.sum(gm)
    return loss, gu, np.concatenate([np.atleast_1d(ls), [var, slot, c]])


def natural_params(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, gamma=1.0):
    """The mixed natural parameters (Lambda, h) of one step at the current q."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.shape[0]
    ls, var, _, c = V.unpack(u, n_ls, train_mean, c_fixed)
    L = V.chol_k(kernel, np.asarray(X, dtype=np.float64), ls, var)
    m, _, v = _moments(L, c, mu, S)
    _, gm, gv = quadrature(y, m, v)
    a = -2.0 * gv
    lam = np.eye(n) + L.T @ (a[:, None] * L)
    h = L.T @ (gm + a * (m - c))
    if gamma != 1.0:
        Sinv = scipy.linalg.solve_triangular(S, np.eye(n), lower=True)
        lam_cur = Sinv.T @ Sinv
        lam = (1.0 - gamma) * lam_cur + gamma * lam
        h = (1.0 - gamma) * (lam_cur @ mu) + gamma * h
    return lam, h


def natgrad(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, gamma=1.0):
    """One natural-gradient step on q at fixed theta."""
    lam, h = natural_params(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, gamma)
    n = h.shape[0]
    Vm = scipy.linalg.solve_triangular(np.linalg.cholesky(lam), np.eye(n), lower=True)
    Sig = Vm.T @ Vm
    return Sig @ h, np.linalg.cholesky(Sig)


def success_log_prob(mean, var):
    """log P(success) = log Phi(mean / sqrt(1 + max(var, 0)))."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    return log_ndtr(mean / np.sqrt(1.0 + np.maximum(var, 0.0)))


class Posterior(V.Posterior):
    """The install: the LATENT predictive of tests/vgp_oracle.py (noise slot 0, shift 0) and the probit predictive over it."""

    def predict_y(self, Xs, triangular=False):
        raise NotImplementedError("a Bernoulli VGP has no Gaussian predict_y")

    def predict_prob(self, Xs):
        """(prob, logprob) at the rows of Xs."""
        lp = success_log_prob(*self.predict_f(Xs))
        return np.exp(lp), lp


def initial_u(lengthscales, variance, c=None):
    """u in tests/vgp_oracle.py's layout; the likelihood slot holds 0.0 (softplus(0) + 1e-6: a valid decode, read by nothing)."""
    u = V.initial_u(lengthscales, variance, 1.0, c)
    u[np.atleast_1d(lengthscales).shape[0] + 1] = 0.0
    return u


def train(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, iterations, gamma, adam):
    """Per iteration one natgrad step on q, one Adam step on theta WITHOUT the likelihood slot (it is no variable)."""
    u = np.asarray(u, dtype=np.float64).copy()
    keep = np.arange(u.shape[0]) != n_ls + 1
    for _ in range(iterations):
        mu, S = natgrad(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S, gamma)
        _, g, _ = neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, mu, S)
        u[keep] = adam.step(u[keep], g[keep])
    return u, mu, S, adam


# ---- the device tests' cases (tests/test_gpu_vgp_bernoulli.py), checked on the CPU too (tests/test_vgp_bernoulli_cpu.py) ------
CASES = [(7, 1, "Matern12", False), (60, 2, "Matern52", True), (128, 3, "SquaredExponential", True), (129, 12, "Matern32", False)]


def case_problem(n, d, kernel, ard):
    """(X, labels, u, n_ls) of a case: labels are the sign of a smooth function of X about its median, seed fixed per case."""
    rng = np.random.default_rng(1000 + n + d)
    X = rng.random((n, d))
    w = rng.normal(size=d)
    g = np.sin(2.0 * X @ w / np.sqrt(d)) + 0.5 * X[:, 0]
    y = (g > np.median(g)).astype(np.float64)
    n_ls = d if ard else 1
    ls = 0.3 * np.sqrt(d) * (1.0 + 0.5 * np.arange(d) / d) if ard else 0.3 * np.sqrt(d)
    return X, y, initial_u(ls, 1.2, 0.1), n_ls


STEPS = ((1.0, 0.0), (0.5, 0.2))  # (gamma, shift of u) of the two natural-gradient steps
