"""float64 numpy restatement of pathwise posterior draws, in the manner of ``tests/joint_oracle.py``.
For a fitted exact GP (theta, X, y, L = chol(K + diag(noise + s))) and random inputs omega [F, D] (scaled coordinates),
phase [F], w [S, F], eps [S, N] (None: zeros):

    phi_j(x) = sqrt(2 variance / F) cos(omega_j . x / l + phase_j)
    R[i, q] = (y_i - c) - sum_j phi_j(x_i) w[q, j] - sqrt(noise + s_i) eps[q, i]
    v = L^-T (L^-1 R)
    value[q, a] = c + sum_j phi_j(t_a) w[q, j] + sum_i k(x_i, t_a) v[i, q]

k from direct differences (``joint_oracle._kernel_direct``).  ``dtype=np.longdouble`` repeats the features, the kernel map,
the triangular solves and the contractions in extended precision from the same float64 L (the conditioning check of the
GPU cases).  ``textbook_values`` is the twin that gets v from a dense solve against K_y and never forms L^-1.

Test infrastructure: the kernel map is ``oracle/gpr.py``'s.  Nothing here is imported by ``pygpso_amd``.
"""
import numpy as np
import scipy.linalg as sla

from oracle import gpr
from tests.joint_oracle import _kernel_direct, _ls
from tests.predict_grad_oracle import linv_of


def features(theta, omega, phase, X, dtype=np.float64):
    """Phi [M, F] at the rows of X (unscaled)."""
    omega = np.asarray(omega, dtype=dtype)
    Xs = np.asarray(X, dtype=dtype) / np.asarray(_ls(theta, np.shape(X)[1]), dtype=dtype)
    scale = np.sqrt(dtype(2.0) * dtype(theta.variance) / dtype(omega.shape[0]))
    return scale * np.cos(Xs @ omega.T + np.asarray(phase, dtype=dtype)[None, :])


def residual(post, s, omega, phase, w, eps, dtype=np.float64):
    """R [N, S]."""
    th = post.theta
    w = np.asarray(w, dtype=dtype)
    R = (np.asarray(post.y, dtype=dtype) - dtype(th.mean_c))[:, None] - features(th, omega, phase, post.X, dtype) @ w.T
    if eps is not None:
        d = dtype(th.noise) + (np.zeros(post.X.shape[0], dtype=dtype) if s is None else np.asarray(s, dtype=dtype))
        R = R - np.sqrt(d)[:, None] * np.asarray(eps, dtype=dtype).T
    return R


def _substitute(L, B, transposed):
    """L^-1 B (or L^-T B) by substitution in B's dtype: numpy's solvers stop at float64."""
    n = L.shape[0]
    out = np.zeros_like(B)
    order = range(n - 1, -1, -1) if transposed else range(n)
    for i in order:
        row = L[i + 1:, i] if transposed else L[i, :i]
        done = out[i + 1:] if transposed else out[:i]
        out[i] = (B[i] - row @ done) / L[i, i]
    return out


def solve_v(post, R):
    """v [N, S] = L^-T (L^-1 R): through ``linv_of`` in float64, by substitution in extended precision."""
    if R.dtype == np.float64:
        Li = linv_of(post.L)
        return Li.T @ (Li @ R)
    L = np.asarray(post.L, dtype=R.dtype)
    return _substitute(L, _substitute(L, R, False), True)


def _kernel_any(theta, A, B, dtype):
    if dtype == np.float64:
        return _kernel_direct(theta, A, B)
    ls = np.asarray(_ls(theta, A.shape[1]), dtype=dtype)
    diff = (np.asarray(A, dtype=dtype) / ls)[:, None, :] - (np.asarray(B, dtype=dtype) / ls)[None, :, :]
    return gpr.kernel_from_r2(theta.kernel, np.sum(diff * diff, axis=-1), dtype(theta.variance))


def evaluate(post, omega, phase, w, v, Xs, dtype=np.float64):
    """values [S, M] of the paths (w, v) at the rows of Xs."""
    th = post.theta
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    prior = np.asarray(w, dtype=dtype) @ features(th, omega, phase, Xs, dtype).T
    update = np.asarray(v, dtype=dtype).T @ _kernel_any(th, post.X, Xs, dtype)
    return dtype(th.mean_c) + prior + update


def path_values(post, s, omega, phase, w, eps, Xs, dtype=np.float64):
    """Draw and evaluate in one: values [S, M]."""
    v = solve_v(post, residual(post, s, omega, phase, w, eps, dtype))
    return evaluate(post, omega, phase, w, v, Xs, dtype)


def textbook_values(theta, X, y, s, omega, phase, w, eps, Xs):
    """The same values with v = K_y^-1 R by a dense symmetric solve (K_y from direct differences)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    d = theta.noise + (np.zeros(n) if s is None else np.asarray(s, dtype=np.float64))
    Ky = _kernel_direct(theta, X, X)
    Ky[np.diag_indices(n)] += d
    R = (np.asarray(y, dtype=np.float64) - theta.mean_c)[:, None] - features(theta, omega, phase, X) @ np.asarray(w).T
    if eps is not None:
        R = R - np.sqrt(d)[:, None] * np.asarray(eps).T
    v = sla.solve(Ky, R, assume_a="pos")
    return theta.mean_c + np.asarray(w) @ features(theta, omega, phase, Xs).T + v.T @ _kernel_direct(theta, X, np.asarray(Xs, dtype=np.float64))


def seg_argmax(values, seg_off=None):
    """Per draw and segment the FIRST arg-max relative to the segment start and the maximum: (idx [S, nseg], val [S, nseg]);
    an empty segment gives -1 and NaN (``gpso_best_ucb``'s record for one)."""
    values = np.asarray(values)
    s, m = values.shape
    so = np.array([0, m]) if seg_off is None else np.asarray(seg_off, dtype=np.int64)
    nseg = so.shape[0] - 1
    idx = np.full((s, nseg), -1, dtype=np.int64)
    val = np.full((s, nseg), np.nan)
    for g in range(nseg):
        if so[g + 1] > so[g]:
            block = values[:, so[g]:so[g + 1]]
            idx[:, g] = np.argmax(block, axis=1)
            val[:, g] = block[np.arange(s), idx[:, g]]
    return idx, val


def top_two_gap(values, seg_off=None):
    """Per draw and segment the difference between the two highest values (inf for a segment of fewer than two rows)."""
    values = np.asarray(values)
    s, m = values.shape
    so = np.array([0, m]) if seg_off is None else np.asarray(seg_off, dtype=np.int64)
    gap = np.full((s, so.shape[0] - 1), np.inf)
    for g in range(so.shape[0] - 1):
        if so[g + 1] - so[g] >= 2:
            top = np.sort(values[:, so[g]:so[g + 1]], axis=1)
            gap[:, g] = top[:, -1] - top[:, -2]
    return gap


def exact_posterior(post, Xs):
    """(mean [M], cov [M, M]) of the latent f at Xs: what the draws' moments approach."""
    th = post.theta
    Ks = _kernel_direct(th, post.X, np.asarray(Xs, dtype=np.float64))  # [N, M]
    V = linv_of(post.L) @ Ks
    return Ks.T @ post.alpha + th.mean_c, _kernel_direct(th, Xs, Xs) - V.T @ V
