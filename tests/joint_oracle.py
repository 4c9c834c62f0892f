"""float64 numpy/scipy restatement of the joint predictive, in the manner of
``tests/predict_grad_oracle.py``.  For a predictive (C, alpha, rows, theta) with mean = alpha^T k* + c and
var = variance - |C k*|^2, xs = x / l and M test points t_1 .. t_M:

    V = C K*  (K*[i, m] = k(x_i, t_m)),   mu = K*^T alpha + c,   Sigma = K** - V^T V + diag_add I,

K** and K* from direct differences (no cancellation at coincident points).  Sigma is symmetric to the bit: K** by
construction, the product by averaging it with its transpose.

Test infrastructure: the kernel map is ``oracle/gpr.py``'s.  Nothing here is imported by ``pygpso_amd``.
"""
import numpy as np
import scipy.linalg as sla

from oracle import gpr
from tests.predict_grad_oracle import linv_of


def _ls(theta, d):
    ls = np.asarray(theta.lengthscales, dtype=np.float64)
    return np.broadcast_to(ls, (d,)) if ls.shape[0] == 1 else ls


def _kernel_direct(theta, A, B):
    """k(a_i, b_j) with r^2 from direct differences of the scaled rows."""
    ls = _ls(theta, A.shape[1])
    diff = (A / ls)[:, None, :] - (B / ls)[None, :, :]
    return gpr.kernel_from_r2(theta.kernel, np.sum(diff * diff, axis=-1), theta.variance)


def predictive_joint(C, alpha, rows, theta, Xs, diag_add=0.0):
    """(mean [M], cov [M, M]) of a generic predictive: C [n, n] (v = C k*), alpha [n], rows [n, D]."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    Ks = _kernel_direct(theta, Xs, rows)  # [M, n]
    V = Ks @ np.asarray(C).T              # row m: v = C k*
    P = V @ V.T
    cov = _kernel_direct(theta, Xs, Xs) - 0.5 * (P + P.T)
    cov[np.diag_indices(Xs.shape[0])] += diag_add
    return Ks @ np.asarray(alpha) + theta.mean_c, cov


def gpr_predict_joint(post, Xs, diag_add=0.0):
    """The exact GP's: ``post`` from ``oracle.gpr.posterior`` (or ``tests.hetero_oracle.posterior``: same members)."""
    return predictive_joint(linv_of(post.L), post.alpha, post.X, post.theta, Xs, diag_add)


def textbook_joint(theta, X, y, Xs, diag_add=0.0):
    """K** - K*^T (K + noise I)^-1 K* and K*^T (K + noise I)^-1 (y - c) + c by a dense symmetric solve: C is never formed."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    Ky = _kernel_direct(theta, X, X)
    Ky[np.diag_indices(X.shape[0])] += theta.noise
    Ks = _kernel_direct(theta, X, Xs)  # [n, M]
    sol = sla.solve(Ky, np.column_stack([Ks, np.asarray(y, dtype=np.float64) - theta.mean_c]), assume_a="pos")
    cov = _kernel_direct(theta, Xs, Xs) - Ks.T @ sol[:, :-1]
    cov[np.diag_indices(Xs.shape[0])] += diag_add
    return Ks.T @ sol[:, -1] + theta.mean_c, cov


def draws(mean, cov, z):
    """mean + chol(cov) z per row of z [S, M] (cov with its diag_add already on it)."""
    return mean[None, :] + np.asarray(z) @ np.linalg.cholesky(cov).T


def chol_perturbation_bound(cov, delta):
    """First-order bound on |chol(cov + E) - chol(cov)|_F for a symmetric E with entries up to delta:
    sqrt(lambda_max) M delta / (sqrt 2 lambda_min) (|E|_F <= M delta)."""
    lam = np.linalg.eigvalsh(cov)
    return float(np.sqrt(lam[-1]) * cov.shape[0] * delta / (np.sqrt(2.0) * lam[0]))
