"""
Float64 numpy restatement of the gradient of the sparse models' losses in the inducing points Z -- the checker of the
moving-Z evaluations (pygpso_amd/csrc/inducing.hip, gpso_sgpr_bound_uz / gpso_svgp_elbo_uz).  It stands on
tests/sgpr_oracle.py and tests/svgp_oracle.py (whose losses the CPU tests difference).  Test infrastructure only: the
product never imports it.

Every kernel is stationary in r^2 = sum_d (z_d - x_d)^2 / l_d^2.  With k' = dk/dr^2 and an objective F whose weights are
Wc = dF/dKuf [M x N] and the symmetric Wu = dF/dKuu [M x M] (dF = sum_ij Wu_ij dKuu_ij):

    Vc = Wc * k'(Z, X),   Vu = 2 Wu * k'(Z, Z) with its diagonal := 0   (z_m sits in row m and in column m of Kuu)
    dF/dZ[m, d] = (2 / l_d^2) (sum_n Vc[m, n] (z[m, d] - x[n, d]) + sum_j Vu[m, j] (z[m, d] - z[j, d]))

A pair with r^2 <= 1e-36 contributes zero (GPflow's sqrt(max(r^2, 1e-36)) and a zero difference): exact for the
Matern-3/2, -5/2 and the squared exponential, the convention at the Matern-1/2's kink.
"""
from __future__ import annotations

import contextlib

import numpy as np
import scipy.linalg

from oracle import gpr
from tests import sgpr_oracle as S
from tests import svgp_oracle as V

R2_FLOOR = 1.0e-36


def r2_direct(P, Q, ls):
    """r^2 from direct differences, dimension by dimension (>= 0, free of cancellation, exactly 0 for equal rows)."""
    r2 = np.zeros((P.shape[0], Q.shape[0]))
    for k in range(P.shape[1]):
        df = (P[:, k][:, None] - Q[:, k][None, :]) / ls[k]
        r2 += df * df
    return r2


@contextlib.contextmanager
def direct_r2_everywhere():
    """The second float64 restatement: inside this block the oracles build EVERY kernel matrix (Kuu, Kuf, and with them the
    factors and the weights) from direct-difference r^2 instead of the GEMM form.  The distance between a gradient computed
    inside and outside is the size of float64 rounding in it at that point -- large where Kuu or B is ill-conditioned."""
    gemm = gpr.scaled_sqdist

    def direct(X, X2, ls):
        X = np.asarray(X, dtype=np.float64)
        ls = S._ls_full(ls, X.shape[1])
        return r2_direct(X, X if X2 is None else np.asarray(X2, dtype=np.float64), ls)

    gpr.scaled_sqdist = direct
    try:
        yield
    finally:
        gpr.scaled_sqdist = gemm


def _v(kernel, W, r2, var):
    K = gpr.kernel_from_r2(kernel, r2, var)
    return np.where(r2 > R2_FLOOR, W * gpr._dk_dr2(kernel, r2, K, var), 0.0)


def contract_z(kernel, Wc, Wu, Z, X, ls, var):
    """dF/dZ [M, D] for the weights Wc = dF/dKuf and Wu = dF/dKuu, by direct differences."""
    Z, X = np.asarray(Z, dtype=np.float64), np.asarray(X, dtype=np.float64)
    ls = S._ls_full(ls, Z.shape[1])
    Vc = _v(kernel, Wc, r2_direct(Z, X, ls), var)
    Vu = _v(kernel, 2.0 * 0.5 * (Wu + Wu.T), r2_direct(Z, Z, ls), var)
    np.fill_diagonal(Vu, 0.0)
    g = np.empty(Z.shape)
    for k in range(Z.shape[1]):
        g[:, k] = (2.0 / ls[k] ** 2) * (np.sum(Vc * (Z[:, k][:, None] - X[:, k][None, :]), axis=1)
                                        + np.sum(Vu * (Z[:, k][:, None] - Z[:, k][None, :]), axis=1))
    return g


def contract_z_gemm(kernel, Wc, Wu, Z, X, ls, var):
    """The same gradient restated as the device orders it: r^2 in GEMM form (the oracle's gpr.scaled_sqdist) and the
    contraction as zs rowsum(V) - V xs.  The spread between this and ``contract_z`` is the size of float64 rounding in the
    quantity."""
    Z, X = np.asarray(Z, dtype=np.float64), np.asarray(X, dtype=np.float64)
    ls = S._ls_full(ls, Z.shape[1])
    zs, xs = Z / ls, X / ls
    r2c = gpr.scaled_sqdist(Z, X, ls)
    r2u = gpr.scaled_sqdist(Z, None, ls)
    Vc = _v(kernel, Wc, np.where(r2_direct(Z, X, ls) > R2_FLOOR, r2c, 0.0), var)
    Vu = _v(kernel, 2.0 * 0.5 * (Wu + Wu.T), np.where(r2_direct(Z, Z, ls) > R2_FLOOR, r2u, 0.0), var)
    np.fill_diagonal(Vu, 0.0)
    return (2.0 / ls)[None, :] * (zs * (Vc.sum(axis=1) + Vu.sum(axis=1))[:, None] - Vc @ xs - Vu @ zs)


# ---- SGPR -----------------------------------------------------------------------------------------------------------
def sgpr_weights(kernel, u, n_ls, train_mean, c_fixed, X, y, Z):
    """(factors, dF/dKuf, dF/dKuu) of the bound F: the dKuf and dKuu of sgpr_oracle.neg_bound_and_grad_u."""
    f = S.factors(kernel, u, n_ls, train_mean, c_fixed, X, y, Z)
    m = f.Z.shape[0]
    b = 1.0 / f.s2
    Lui = S._tri(f.Lu, np.eye(m))
    T1 = S._tri(f.LB, Lui)
    Qinv = T1.T @ T1
    Kuuinv = Lui.T @ Lui
    a = f.s2 * (T1.T @ f.cv)
    w = f.Kuf.T @ a
    dKuf = b * (Kuuinv - Qinv) @ f.Kuf + np.outer(a, b * b * f.e - b ** 3 * w)
    dKuu = 0.5 * (Kuuinv - Qinv - b * b * np.outer(a, a) - Lui.T @ f.AAT @ Lui)
    return f, dKuf, dKuu


def sgpr_grad_z(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, contract=contract_z):
    """d(-bound)/dZ [M, D]."""
    f, dKuf, dKuu = sgpr_weights(kernel, u, n_ls, train_mean, c_fixed, X, y, Z)
    return -contract(kernel, dKuf, dKuu, f.Z, f.X, f.ls, f.var)


def sgpr_loss_and_grads(kernel, u, n_ls, train_mean, c_fixed, X, y, Z):
    """(-bound, grad_u, grad_z)."""
    loss, gu, _ = S.neg_bound_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, Z)
    return loss, gu, sgpr_grad_z(kernel, u, n_ls, train_mean, c_fixed, X, y, Z)


# ---- SVGP -----------------------------------------------------------------------------------------------------------
def svgp_weights(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, Sq, lik):
    """(factors, dELBO/dKuf, d(-ELBO)/dKuu) at fixed q: the dKuf and Kbar of svgp_oracle.neg_elbo_and_grad_u."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    f = V.Factors(kernel, u, n_ls, train_mean, c_fixed, X, Z, lik)
    M = f.Z.shape[0]
    m, v = V.moments(f.A, mu, Sq, f.var, f.c)
    _, gm, gv, _ = V.pointwise(lik, y, m, v, f.p)
    Sig = Sq @ Sq.T
    Abar = np.outer(mu, gm) + 2.0 * (Sig - np.eye(M)) @ (f.A * gv[None, :])
    dKuf = scipy.linalg.solve_triangular(f.Lu, Abar, lower=True, trans=1)
    Lbar = np.tril(dKuf @ f.A.T)
    P = f.Lu.T @ Lbar
    P = np.tril(P) - 0.5 * np.diag(np.diag(P))
    Lui = scipy.linalg.solve_triangular(f.Lu, np.eye(M), lower=True)
    Kbar = 0.5 * Lui.T @ (P + P.T) @ Lui
    return f, dKuf, Kbar


def svgp_grad_z(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, Sq, lik, contract=contract_z):
    """d(-ELBO)/dZ [M, D] at fixed q (the k_diag term does not depend on Z; q is whitened)."""
    f, dKuf, Kbar = svgp_weights(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, Sq, lik)
    return contract(kernel, -dKuf, Kbar, f.Z, f.X, f.ls, f.var)


def svgp_loss_and_grads(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, Sq, lik):
    """(-ELBO, grad_u, grad_z)."""
    loss, gu, _ = V.neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, Sq, lik)
    return loss, gu, svgp_grad_z(kernel, u, n_ls, train_mean, c_fixed, X, y, Z, mu, Sq, lik)
