"""float64 numpy restatement of the pathwise draws of the variational posteriors, beside
``tests/paths_oracle.py`` (whose feature map, kernel map, evaluation and arg-max helpers it uses).  A whitened posterior over
the resident rows Zr (n of them) is (Lu = chol(k(Zr, Zr) + 1e-6 I), mu, Q) with q(v) = N(mu, Q Q^T):

    P[i, s]  = sum_j phi_j(Zr_i) w[s, j]
    v[:, s]  = beta + Lu^-T (Q eps[s, :] - Lu^-1 P[:, s]),   beta = Lu^-T mu
    value[s](t) = c + sum_j phi_j(t) w[s, j] + sum_i k(Zr_i, t) v[i, s]

built per family from ``tests/vgp_oracle.py`` (+ ``vgp_studentt_oracle``), ``tests/sgpr_oracle.py`` and
``tests/svgp_oracle.py``: Q is the lower root S of q for the VGP and the SVGP and LB^-T for the SGPR (mu = LB^-T cv).  The
install's shift delta never enters.  ``dtype=np.longdouble`` repeats the features, the kernel map, the triangular solves and
the products in extended precision from the same float64 (Lu, mu, Q): the conditioning check of the GPU cases.

Test infrastructure only: nothing here is imported by ``pygpso_amd``.
"""
import numpy as np
import scipy.linalg as sla

from oracle import gpr
from tests import paths_oracle as po
from tests import sgpr_oracle as SG
from tests import svgp_oracle as SV
from tests import vgp_oracle as V
from tests import vgp_studentt_oracle as T
from tests.joint_oracle import _kernel_direct

JITTER = V.JITTER
GAUSSIAN = ("Gaussian", None)


class QPosterior:
    """(theta, X = the resident rows, L = Lu, mu, Q): the attribute names ``paths_oracle.features / evaluate`` read."""

    def __init__(self, kernel, ls, var, c, rows, Lu, mu, Q):
        self.theta = gpr.Theta(kernel, np.atleast_1d(ls), var, 0.0, c)
        self.X = np.ascontiguousarray(rows, dtype=np.float64)
        self.L = np.asarray(Lu, dtype=np.float64)
        self.mu = np.asarray(mu, dtype=np.float64).reshape(-1)
        self.Q = np.asarray(Q, dtype=np.float64)


def vgp_posterior(kernel, u, n_ls, train_mean, c_fixed, X, mu, S, lik=GAUSSIAN):
    ls, var, _, c = T.unpack(u, n_ls, train_mean, c_fixed, lik)
    X = np.asarray(X, dtype=np.float64)
    return QPosterior(kernel, ls, var, c, X, V.chol_k(kernel, X, ls, var), mu, S)


def sgpr_posterior(kernel, u, n_ls, train_mean, c_fixed, X, y, Z):
    f = SG.factors(kernel, u, n_ls, train_mean, c_fixed, X, y, Z)
    Q = sla.solve_triangular(f.LB, np.eye(f.LB.shape[0]), lower=True).T  # LB^-T: B^-1 = Q Q^T
    return QPosterior(kernel, f.ls, f.var, f.c, f.Z, f.Lu, Q @ f.cv, Q)


def svgp_posterior(kernel, u, n_ls, train_mean, c_fixed, X, Z, mu, S, lik=GAUSSIAN):
    f = SV.Factors(kernel, u, n_ls, train_mean, c_fixed, X, Z, lik)
    return QPosterior(kernel, f.ls, f.var, f.c, f.Z, f.Lu, mu, S)


def _solve(L, B, transposed, dtype):
    if dtype == np.float64:
        return sla.solve_triangular(L, B, lower=True, trans=1 if transposed else 0)
    return po._substitute(np.asarray(L, dtype=dtype), np.asarray(B, dtype=dtype), transposed)


def solve_v(post, omega, phase, w, eps, dtype=np.float64):
    """v [n, S]."""
    P = po.features(post.theta, omega, phase, post.X, dtype) @ np.asarray(w, dtype=dtype).T
    if eps is None:
        E = np.zeros_like(P)
    else:
        E = np.asarray(post.Q, dtype=dtype) @ np.asarray(eps, dtype=dtype).T
    beta = _solve(post.L, np.asarray(post.mu, dtype=dtype)[:, None], True, dtype)
    return beta + _solve(post.L, E - _solve(post.L, P, False, dtype), True, dtype)


def path_values(post, omega, phase, w, eps, Xs, dtype=np.float64):
    """Draw and evaluate in one: values [S, M]."""
    return po.evaluate(post, omega, phase, w, solve_v(post, omega, phase, w, eps, dtype), Xs, dtype)


def predictive_mean(post, Xs):
    """The family's predictive mean c + k*^T Lu^-T mu (k from direct differences, as the paths evaluate it)."""
    ks = _kernel_direct(post.theta, post.X, np.asarray(Xs, dtype=np.float64))  # [n, M]
    return ks.T @ sla.solve_triangular(post.L, post.mu, lower=True, trans=1) + post.theta.mean_c


def expected_moments(post, Xs):
    """What the draws' moments approach when the features' Gram is exactly k (its expectation): (mean [M], cov [M, M],
    var_f [M], gap [M]).  The feature prior carries no jitter but Lu does: with K~ = Lu Lu^T = K + 1e-6 I,

        cov = k** - k*^T (2 K~^-1 - K~^-1 K K~^-1) k* + k*^T Lu^-T Sigma Lu^-1 k*,

    which is the model's var_f = k** - |Lu^-1 k*|^2 + |Q^T Lu^-1 k*|^2 on the diagonal up to gap = cov_aa - var_f_a =
    -1e-6 |K~^-1 k*_a|^2, of magnitude at most k*^T K~^-1 k*."""
    th = post.theta
    Xs = np.asarray(Xs, dtype=np.float64)
    ks = _kernel_direct(th, post.X, Xs)
    A = sla.solve_triangular(post.L, ks, lower=True)        # Lu^-1 k*
    W = sla.solve_triangular(post.L, A, lower=True, trans=1)  # K~^-1 k*
    K = post.L @ post.L.T - JITTER * np.eye(post.L.shape[0])
    QA = post.Q.T @ A
    cov = _kernel_direct(th, Xs, Xs) - 2.0 * A.T @ A + W.T @ K @ W + QA.T @ QA
    var_f = th.variance - np.sum(A * A, axis=0) + np.sum(QA * QA, axis=0)
    return A.T @ post.mu + th.mean_c, cov, var_f, np.diag(cov) - var_f
