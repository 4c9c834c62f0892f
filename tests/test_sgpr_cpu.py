"""
CPU checks of the SGPR path: the numpy oracle (tests/sgpr_oracle.py) against itself and against the frozen exact-GPR oracle
(central differences, the installed one-term predictive, the GPR limit Z = X, monotonicity of the Titsias bound, the greedy
selection against a brute-force restatement) and the surrogate's constructor limits.
"""
import math

import numpy as np
import pytest

from oracle import gpr
from tests import sgpr_oracle as S
from tests.helpers import synthetic_problem

J = S.JITTER


def _problem(n, d, m, seed):
    rng = np.random.default_rng(1000 + seed)  # (another stream than synthetic_problem's: its first draws ARE X)
    X, y = synthetic_problem(n, d, seed=seed)
    return X, y, rng.random((m, d))  # (Z away from X: no coincident pairs in Kuf, where Matern-1/2 has its kink)


@pytest.mark.parametrize("kernel", gpr.KERNELS)
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("train_mean", [False, True])
def test_oracle_gradient_matches_central_differences(kernel, ard, train_mean, monkeypatch):
    # (Matern-1/2 turns the ~1e-16 GEMM-form r^2 of Kuu's diagonal into ~1e-8 of k, noise that a difference quotient
    # amplifies; the analytic gradient takes dk there as 0.  The quotient here sees an exact diagonal, as tests/test_vgp_cpu.py's.)
    sqd = gpr.scaled_sqdist

    def exact_diagonal(X, X2, ls):
        r2 = sqd(X, X2, ls)
        if X2 is None or X2 is X:
            np.fill_diagonal(r2, 0.0)
        return r2

    monkeypatch.setattr(gpr, "scaled_sqdist", exact_diagonal)
    n, d, m = 40, 3, 9
    X, y, Z = _problem(n, d, m, seed=3)
    ls = np.array([0.6, 0.9, 1.3]) if ard else 0.8
    u = S.initial_u(ls, 1.3, 0.05, 0.2 if train_mean else None)
    n_ls = d if ard else 1
    f, g, theta = S.neg_bound_and_grad_u(kernel, u, n_ls, train_mean, 0.1, X, y, Z)
    assert np.isclose(f, -S.bound(kernel, u, n_ls, train_mean, 0.1, X, y, Z), rtol=1e-13)
    assert theta.shape == (n_ls + 3,) and theta[-1] == (0.2 if train_mean else 0.1)
    h, tol = 1e-6, 1e-6
    for k in range(u.shape[0]):
        up, um = u.copy(), u.copy()
        up[k] += h
        um[k] -= h
        fd = (S.bound(kernel, um, n_ls, train_mean, 0.1, X, y, Z) - S.bound(kernel, up, n_ls, train_mean, 0.1, X, y, Z)) / (2 * h)
        assert abs(fd - g[k]) <= tol * max(1.0, abs(fd)), (k, fd, g[k])


@pytest.mark.parametrize("kernel", ["Matern52", "SquaredExponential"])
def test_installed_one_term_predictive_equals_two_term_form(kernel):
    X, y, Z = _problem(300, 4, 64, seed=5)
    u = S.initial_u(0.5, 1.2, 0.01, 0.1)
    post = S.Posterior(kernel, u, 1, True, 0.0, X, y, Z)
    Xs = np.random.default_rng(6).random((500, 4))
    m2, v2 = post.predict_y(Xs)
    m1, v1 = post.predict_y_installed(Xs)
    assert post.installed()[3] == 0.0
    # both forms subtract O(variance) terms: 1e-10 of the prior variance is ~1e5 roundings of them
    assert np.max(np.abs(m1 - m2)) <= 1e-10 * max(1.0, np.max(np.abs(m2)))
    assert np.max(np.abs(v1 - v2)) <= 1e-10 * post.f.var
    # a forced shift: served variance in [exact, exact + delta k**], the mean untouched
    delta = 1e-3
    md, vd = post.predict_y_installed(Xs, delta=delta)
    assert np.max(np.abs(md - m2)) <= 1e-10 * max(1.0, np.max(np.abs(m2)))
    assert np.all(vd >= v2 - 1e-10 * post.f.var) and np.all(vd <= v2 + delta * post.f.var + 1e-10 * post.f.var)
    ks = post._ks(Xs)
    t1 = np.linalg.solve(post.f.Lu, ks)
    want = v2 + delta * (post.f.var - np.sum(t1 * t1, axis=0))
    assert np.max(np.abs(vd - want)) <= 1e-10 * post.f.var


def test_gpr_limit_z_equals_x():
    n, d, s2 = 300, 4, 1e-2
    X, y = synthetic_problem(n, d, seed=0)
    u = S.initial_u(0.5, 1.0, s2, 0.05)
    ls, var, s2u, c = S.unpack(u, 1, True)
    theta = gpr.Theta("Matern52", float(ls[0]), var, s2u, c)
    nlml, _ = gpr.nlml_and_grad(theta, X, y)
    bound = S.bound("Matern52", u, 1, True, 0.0, X, y, X)
    gap = -nlml - bound
    print(f"GPR limit: gap {gap:.4g}, N J / sigma^2 = {n * J / s2u:.4g}")
    assert gap >= -1e-9 * abs(nlml)          # a lower bound (up to rounding of two O(|nlml|) numbers)
    assert gap <= 2.0 * n * J / s2u          # the jitter's trace term, first order N J / sigma^2
    # predictions: the SGPR with Z = X is the GPR of the kernel k Kuu^-1 k, Kuu = K + J I.  Qff - K = -J K (K + J)^-1 has
    # norm <= J, and a perturbation E of the Gram moves mean and variance by at most |E| |K_y^-1| times O(|k*|) factors:
    # |dmean| <= J |alpha|_1-type terms, bounded here by (J / sigma^2) * (|y - c|_2 sqrt(N) + ...).  The test uses
    # tol = 4 (J / sigma^2) * scale with scale = the quantity's own size (max |mean - c| + |y - c|_inf; variance), which the
    # first-order expansion (K_y + E)^-1 = K_y^-1 - K_y^-1 E K_y^-1 bounds since |K_y^-1| <= 1 / sigma^2 and |k*| <= variance.
    post_g = gpr.posterior(theta, X, y)
    post_s = S.Posterior("Matern52", u, 1, True, 0.0, X, y, X)
    Xs = np.random.default_rng(1).random((400, d))
    mg, vg = gpr.predict_y(post_g, Xs)
    ms, vs = post_s.predict_y(Xs)
    eps = J / s2u
    tol_m = 4.0 * eps * (np.max(np.abs(mg - c)) + np.max(np.abs(y - c)))
    tol_v = 4.0 * eps * var
    print(f"GPR limit: |dmean| {np.max(np.abs(ms - mg)):.3g} (tol {tol_m:.3g}), |dvar| {np.max(np.abs(vs - vg)):.3g} (tol {tol_v:.3g})")
    assert np.max(np.abs(ms - mg)) <= tol_m
    assert np.max(np.abs(vs - vg)) <= tol_v


def test_bound_is_monotone_in_greedy_picks():
    X, y = synthetic_problem(200, 3, seed=2)
    u = S.initial_u(0.4, 1.0, 0.02, 0.0)
    ls, var, _, _ = S.unpack(u, 1, True)
    idx = S.greedy_select("Matern52", X, ls, var, 48)
    prev = -np.inf
    for m in (4, 8, 16, 24, 32, 48):
        b = S.bound("Matern52", u, 1, True, 0.0, X, y, X[idx[:m]])
        assert b >= prev - 1e-9 * abs(b), (m, b, prev)
        prev = b
    nlml, _ = gpr.nlml_and_grad(gpr.Theta("Matern52", float(ls[0]), var, S.unpack(u, 1, True)[2], 0.0), X, y)
    assert prev <= -nlml + 1e-9 * abs(nlml)


def _greedy_brute_force(kernel, X, ls, var, m):
    """Greedy conditional-variance selection restated without the partial Cholesky: the conditional variance of every row
    given the picked ones from a dense solve."""
    n = X.shape[0]
    K = S.kmat(kernel, X, ls, var)
    picked = []
    for _ in range(m):
        if picked:
            Kpp = K[np.ix_(picked, picked)]
            Kxp = K[:, picked]
            cond = np.full(n, var) - np.sum(Kxp * np.linalg.solve(Kpp, Kxp.T).T, axis=1)
        else:
            cond = np.full(n, float(var))
        cond[picked] = -np.inf
        picked.append(int(np.argmax(cond)))
    return np.array(picked)


def test_greedy_selection_against_brute_force():
    X, _ = synthetic_problem(120, 3, seed=4)
    idx, margin = S.greedy_select("Matern52", X, 0.5, 1.0, 30, return_margin=True)
    assert idx[0] == 0 and len(set(idx.tolist())) == 30  # (the first pick is an exact tie: the lowest index)
    assert margin > 1e-9
    np.testing.assert_array_equal(idx, _greedy_brute_force("Matern52", X, 0.5, 1.0, 30))
    np.testing.assert_array_equal(S.choose_inducing("Matern52", X, 0.5, 1.0, 200), X)
    np.testing.assert_array_equal(S.choose_inducing("Matern52", X, 0.5, 1.0, 30), X[idx])


def test_greedy_selection_stops_at_a_rank_deficient_gram():
    X, _ = synthetic_problem(30, 3, seed=7)
    Xd = np.vstack([X, X[:10]])
    np.testing.assert_array_equal(S.greedy_select("Matern52", Xd, 0.5, 1.0, 30), S.greedy_select("Matern52", X, 0.5, 1.0, 30))
    with pytest.raises(np.linalg.LinAlgError):
        S.greedy_select("Matern52", Xd, 0.5, 1.0, 31)


def test_issue_selection_cases_keep_their_margin():
    """The small input the device selection is checked on keeps its runner-up margin above 1e-9 relative (the large one is
    asserted by the GPU test itself)."""
    X, _ = synthetic_problem(300, 4, seed=0)
    _, margin = S.greedy_select("Matern52", X, 0.5, 1.0, 64, return_margin=True)
    assert margin > 1e-9, margin


def test_constructor_and_argument_limits():
    from pygpso_amd import SGPRSurrogate
    from pygpso_amd import kernels as K

    with pytest.raises(ValueError):
        SGPRSurrogate(gp_kernel=K.Matern52(), dtype="float32")
    with pytest.raises(ValueError):
        SGPRSurrogate(gp_kernel=K.Matern52(), num_inducing=0)
    with pytest.raises(ValueError):
        SGPRSurrogate(gp_kernel=K.Matern52(), inducing="random")
    with pytest.raises(ValueError):
        SGPRSurrogate(gp_kernel=K.Matern52(), inducing=np.zeros((0, 2)))
    with pytest.raises(ValueError):
        SGPRSurrogate(gp_kernel=K.Matern52(), inducing=np.array([[0.1, math.nan]]))
    for dtype in ("float64", "mixed"):
        s = SGPRSurrogate(gp_kernel=K.Matern52(), gp_meanf=K.Constant(), dtype=dtype, num_inducing=32)
        assert s.dtype == dtype and isinstance(s.optimiser, K.Scipy) and s.num_inducing == 32 and s.inducing == "greedy"
    s = SGPRSurrogate(gp_kernel=K.Matern52(), inducing=np.full((5, 2), 0.5), num_inducing=99)
    assert s.num_inducing == 5
    d = SGPRSurrogate.default(num_inducing=64)
    assert d.num_inducing == 64 and d.gp_lik_sigma == 1e-3


def test_product_modules_do_not_import_the_oracle():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "pygpso_amd", "sgpr.py")) as fh:
        assert "oracle" not in fh.read()
