"""
Sparse GP regression on inducing points on the MI355X: the device calls (gpso_sgpr_*) against the float64 oracle
(tests/sgpr_oracle.py) through the C-ABI wrappers and through ``HipSGPR`` / ``SGPRSurrogate``.

What is compared: Kuf, Lu, LB, cv (gpso_sgpr_get_factor), the bound, its gradient, the installed C and beta (the
getters), Z, the greedy picks and every predict path in float64 and mixed contexts.
"""
import ctypes as C
import os
from shutil import rmtree

import numpy as np
import pytest
import scipy.optimize

from oracle import gpr
from tests import sgpr_oracle as S
from tests.helpers import rotated_peaks, synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TMP = os.path.join(HERE, "_tmp_gpu_sgpr")
# Device against oracle, relative to the largest reference entry.  2e-9 is what tests/test_gpu_vgp.py uses for the same
# kinds of quantity; Matern-1/2 has its stated exception there (1e-5 on values, 1e-4 on the gradient: the sqrt at r = 0
# amplifies the rounding of r^2, which oracle (GEMM form) and device (direct differences) form differently).  The errors
# observed on the MI355X for every case below are recorded in profiles/sgpr_parity.json.
TOL, TOL_M12, TOL_G_M12 = 2e-9, 1e-5, 1e-4


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _ls(d, ard):
    return 0.3 * np.sqrt(d) * (1.0 + 0.5 * np.arange(d) / d) if ard else 0.3 * np.sqrt(d)


CASES = [(300, 64, 4, "Matern52", False), (300, 64, 12, "SquaredExponential", True), (500, 100, 2, "Matern32", False),
         (400, 80, 12, "Matern12", True), (130, 100, 48, "SquaredExponential", True), (600, 128, 48, "Matern52", True),
         (2048, 256, 12, "Matern52", True), (2048, 256, 2, "Matern32", False), (8192, 512, 20, "Matern32", False),
         (16384, 1024, 40, "Matern52", True)]


@pytest.mark.parametrize("n,m,d,kernel,ard", CASES)
def test_device_bound_gradient_install_against_oracle(n, m, d, kernel, ard):
    from pygpso_amd import HipGPEngine, _lib

    X, y = synthetic_problem(n, d, seed=n + d)
    n_ls = d if ard else 1
    u = S.initial_u(_ls(d, ard), 1.2, 0.01, 0.1)
    ls, var, _, _ = S.unpack(u, n_ls, True)
    Z = X[S.greedy_select(kernel, X, ls, var, m)]
    tol = TOL_M12 if kernel == "Matern12" else TOL
    tol_g = TOL_G_M12 if kernel == "Matern12" else TOL
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    eng.sgpr_set_inducing(Z)
    Zd, n_data = eng.sgpr_get_inducing()
    np.testing.assert_array_equal(Zd, Z)
    assert n_data == n and eng.n == m and eng.padded_n % 128 == 0 and eng.padded_n >= m
    f, g, th = eng.sgpr_bound_u(kernel, u, n_ls, True, 0.0)
    f_ref, g_ref, th_ref = S.neg_bound_and_grad_u(kernel, u, n_ls, True, 0.0, X, y, Z)
    e_f, e_g = abs(f - f_ref) / abs(f_ref), _rel(g, g_ref)
    fac = S.factors(kernel, u, n_ls, True, 0.0, X, y, Z)
    e_kuf, e_lu = _rel(eng.sgpr_get_factor("Kuf"), fac.Kuf), _rel(eng.sgpr_get_factor("Lu"), fac.Lu)
    LBd = eng.sgpr_get_factor("LB")
    e_lb, e_cv = _rel(LBd, fac.LB), _rel(eng.sgpr_get_factor("cv"), fac.cv)
    f2, _, _ = eng.sgpr_bound_u(kernel, u, n_ls, True, 0.0, want_grad=False)
    delta = eng.sgpr_posterior(kernel, u, n_ls, True, 0.0)
    post = S.Posterior(kernel, u, n_ls, True, 0.0, X, y, Z)
    C_ref, beta_ref, noise_ref, d_ref = post.installed()
    Cd, bd = eng.get_matrix(_lib.MAT_LINV), eng.get_vector(_lib.VEC_ALPHA)
    e_c, e_b = _rel(Cd, C_ref), _rel(bd, beta_ref)
    leaves = synthetic_leaves(2048, d, seed=3)
    m_ref, v_ref = post.predict_y(leaves)
    md, vd = eng.predict(leaves)
    e_m, e_v = _rel(md, m_ref), _rel(vd, v_ref)
    print(f"SGPR_PARITY n={n} m={m} d={d} kernel={kernel} ard={ard} Kuf={e_kuf:.3e} Lu={e_lu:.3e} LB={e_lb:.3e} cv={e_cv:.3e} bound={e_f:.3e} grad={e_g:.3e} C={e_c:.3e} beta={e_b:.3e} "
          f"mean={e_m:.3e} var={e_v:.3e} delta={delta:g}")
    eng.close()
    np.testing.assert_allclose(th, th_ref, rtol=1e-15)
    assert f2 == f  # the same evaluation without the gradient: the same bits
    assert np.all(np.triu(LBd, 1) == 0.0)
    assert e_kuf <= tol and e_lu <= tol and e_lb <= tol and e_cv <= tol, (e_kuf, e_lu, e_lb, e_cv)
    assert e_f <= tol, (f, f_ref)
    assert e_g <= tol_g, (g, g_ref)
    assert delta == d_ref == 0.0
    assert e_c <= tol and e_b <= tol, (e_c, e_b)
    assert e_m <= tol and e_v <= tol, (e_m, e_v)


def _sgpr_engine(n, d, m, dtype="float64", kernel="Matern52", seed=0, predict_math=None):
    from pygpso_amd import HipGPEngine

    X, y = synthetic_problem(n, d, seed=seed)
    u = S.initial_u(0.3 * np.sqrt(d), 1.1, 0.01, 0.05)
    ls, var, _, _ = S.unpack(u, 1, True)
    Z = S.choose_inducing(kernel, X, ls, var, m)
    eng = HipGPEngine(dtype, device=0, predict_math=predict_math)
    eng.set_data(X, y)
    eng.sgpr_set_inducing(Z)
    eng.sgpr_posterior(kernel, u, 1, True, 0.0)
    return eng, S.Posterior(kernel, u, 1, True, 0.0, X, y, Z)


def _float_bounds_hold(post, leaves, mean, var, winner):
    """Float predict arithmetic against the float64 oracle: the bounds of __graft_entry__.smoke()'s mixed leg, and the float
    winner rule (the oracle's arg-max, or a leaf whose oracle UCB lies within 2e-5 max(1, |ucb|) of it)."""
    m_ref, v_ref = post.predict_y(leaves)
    assert np.max(np.abs(var - v_ref)) <= 2e-5 * post.f.var, float(np.max(np.abs(var - v_ref)))
    assert np.max(np.abs(mean - m_ref)) <= 1e-4 * max(1.0, float(np.max(np.abs(post.f.y))))
    ucb_all = m_ref + gpr.VARSIGMA_DEFAULT * v_ref
    assert winner == int(np.argmax(ucb_all)) or ucb_all.max() - ucb_all[winner] <= 2e-5 * max(1.0, abs(ucb_all.max()))


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
@pytest.mark.parametrize("n,d,m", [(300, 6, 64), (1500, 12, 200)])
def test_predict_and_best_ucb_against_oracle(n, d, m, dtype):
    eng, post = _sgpr_engine(n, d, m, dtype=dtype)
    leaves = synthetic_leaves(4096, d, seed=11)
    m_ref, v_ref = post.predict_y(leaves)
    mean, var = eng.predict(leaves)
    idx, mu, va, ucb = eng.best_ucb(leaves, gpr.VARSIGMA_DEFAULT)
    if dtype == "float64":
        assert _rel(mean, m_ref) <= 1e-9 and _rel(var, v_ref) <= 1e-9, (_rel(mean, m_ref), _rel(var, v_ref))
        i_ref, _, _, u_ref = post.best_ucb(leaves)
        assert int(idx[0]) == i_ref
        assert abs(ucb[0] - u_ref) <= 1e-9 * abs(u_ref)
    else:
        _float_bounds_hold(post, leaves, mean, var, int(idx[0]))
    # begin / end: the same winner as the synchronous call, bit for bit
    got = eng.best_ucb_end(eng.best_ucb_begin(leaves, gpr.VARSIGMA_DEFAULT))
    for a, b in zip(got, (idx, mu, va, ucb)):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    eng.close()


def test_mixed_context_serves_the_installed_posterior():
    n, d, m = 1024, 6, 256
    eng, post = _sgpr_engine(n, d, m, dtype="mixed")
    leaves = synthetic_leaves(4096, d, seed=12)
    m_ref, v_ref = post.predict_y(leaves)
    mean, var = eng.predict(leaves)
    # float predict arithmetic: the bounds of __graft_entry__.smoke()'s mixed leg
    assert np.max(np.abs(var - v_ref)) <= 2e-5 * post.f.var, float(np.max(np.abs(var - v_ref)))
    assert np.max(np.abs(mean - m_ref)) <= 1e-4 * max(1.0, float(np.max(np.abs(post.f.y))))
    i = int(eng.best_ucb(leaves, gpr.VARSIGMA_DEFAULT)[0][0])
    ucb_all = m_ref + gpr.VARSIGMA_DEFAULT * v_ref
    assert i == int(np.argmax(ucb_all)) or ucb_all.max() - ucb_all[i] <= 2e-5 * max(1.0, abs(ucb_all.max()))
    eng.close()


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_best_ucb_grow_equals_best_ucb_on_grown_rows(dtype):
    d = 4
    eng, post = _sgpr_engine(400, d, 64, dtype=dtype)
    rng = np.random.default_rng(5)
    lo = rng.random((3, d)) * 0.5
    bounds = np.stack([lo, lo + 0.3 + 0.2 * rng.random((3, d))], axis=-1)
    depth = 3
    grown = eng.grow(bounds, depth)
    per = grown.shape[1]
    rows = grown.reshape(-1, d)
    got = eng.best_ucb_grow(bounds, depth, gpr.VARSIGMA_DEFAULT)
    seg = np.arange(4, dtype=np.int64) * per
    want = eng.best_ucb(rows, gpr.VARSIGMA_DEFAULT, seg_off=seg)
    if dtype == "float64":
        for a, b in zip(got, want):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    else:
        # float contexts generate the grown centres on the device in their own arithmetic: each segment's winner is held to
        # the float winner rule and the smoke bounds against the oracle on that segment's rows, not to bit equality
        for s_ in range(3):
            seg_rows = rows[s_ * per:(s_ + 1) * per]
            mean, var = eng.predict(seg_rows)
            _float_bounds_hold(post, seg_rows, mean, var, int(got[0][s_]))
            m_ref, v_ref = post.predict_y(seg_rows)
            i = int(got[0][s_])
            assert abs(got[1][s_] - m_ref[i]) <= 1e-4 * max(1.0, float(np.max(np.abs(post.f.y))))
            assert abs(got[2][s_] - v_ref[i]) <= 2e-5 * post.f.var
    eng.close()


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_sharded_replay_equals_single_context(dtype):
    from pygpso_amd import _lib

    d, world, m = 6, 3, 5000
    eng, _ = _sgpr_engine(600, d, 96, dtype=dtype)
    leaves = synthetic_leaves(m, d, seed=21)
    want = eng.best_ucb(leaves, gpr.VARSIGMA_DEFAULT)
    payloads = []
    for r in range(world):
        lo_c, hi_c = C.c_int64(), C.c_int64()
        _lib.load().gpso_shard_range(m, r, world, C.byref(lo_c), C.byref(hi_c))
        payloads.append(eng.shard_winners(r, world, leaves[lo_c.value:hi_c.value], m, gpr.VARSIGMA_DEFAULT))
    got = eng.fold_winners(np.stack(payloads), 1, m)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    eng.close()


SELECT_CASES = [(300, 4, 64, 0.5), (2048, 12, 256, 0.25 * np.sqrt(12))]


@pytest.mark.parametrize("n,d,m,ls", SELECT_CASES)
def test_device_selection_equals_the_oracles_picks(n, d, m, ls):
    from pygpso_amd import HipGPEngine

    X, y = synthetic_problem(n, d, seed=0)
    idx_ref, margin = S.greedy_select("Matern52", X, ls, 1.0, m, return_margin=True)
    print(f"SGPR_SELECT n={n} d={d} m={m} smallest runner-up margin {margin:.3e}")
    assert margin > 1e-9, margin
    u = S.initial_u(ls, 1.0, 0.01, 0.0)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    idx = eng.sgpr_select_inducing("Matern52", u, 1, m)
    np.testing.assert_array_equal(idx, idx_ref)
    Z, n_data = eng.sgpr_get_inducing()
    np.testing.assert_array_equal(Z, X[idx_ref])
    assert n_data == n
    # the selection leaves a context ready to train: the bound on the picked Z
    f, _, _ = eng.sgpr_bound_u("Matern52", u, 1, True, 0.0, want_grad=False)
    assert abs(f + S.bound("Matern52", u, 1, True, 0.0, X, y, X[idx_ref])) <= TOL * abs(f)
    eng.close()


def test_selection_reports_a_rank_deficient_gram():
    """Duplicated rows in X and m close to N: the conditional variances run out before m picks.  The device says so
    (GPSO_E_NOTPD with the rank reached) where the oracle raises, sets no Z, and the context still takes a feasible m."""
    from pygpso_amd import HipGPEngine, _lib

    X, y = synthetic_problem(40, 3, seed=5)
    X = np.vstack([X, X[:20]])
    y = np.concatenate([y, y[:20]])
    u = S.initial_u(0.5, 1.0, 0.01, 0.0)
    with pytest.raises(np.linalg.LinAlgError):
        S.greedy_select("Matern52", X, 0.5, 1.0, 55)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    with pytest.raises(np.linalg.LinAlgError) as err:
        eng.sgpr_select_inducing("Matern52", u, 1, 55)
    assert "rank" in str(err.value) and "m=55" in str(err.value)
    with pytest.raises(_lib.GpsoHipError):
        eng.sgpr_get_inducing()
    eng.n = 60
    idx = eng.sgpr_select_inducing("Matern52", u, 1, 30)
    np.testing.assert_array_equal(idx, S.greedy_select("Matern52", X, 0.5, 1.0, 30))
    eng.close()


def test_failure_paths_and_call_order():
    from pygpso_amd import HipGPEngine, _lib

    d = 3
    X, y = synthetic_problem(60, d, seed=2)
    u = S.initial_u(0.5, 1.0, 0.01, 0.0)
    eng = HipGPEngine("float64", device=0)
    # out of order: nothing set
    for call in (lambda: eng.sgpr_bound_u("Matern52", u, 1, True, 0.0), lambda: eng.sgpr_posterior("Matern52", u, 1, True, 0.0),
                 lambda: eng.sgpr_get_inducing()):
        with pytest.raises(_lib.GpsoHipError) as err:
            call()
        assert err.value.code == _lib.E_STATE
    eng.d = d
    with pytest.raises(_lib.GpsoHipError):
        eng.sgpr_set_inducing(X[:5])  # before gpso_set_data
    eng.set_data(X, y)
    with pytest.raises(_lib.GpsoHipError):
        eng.sgpr_bound_u("Matern52", u, 1, True, 0.0)  # data, but no Z
    with pytest.raises(ValueError):
        eng.sgpr_select_inducing("Matern52", u, 1, 61)  # m > N
    with pytest.raises(_lib.GpsoHipError):
        eng.sgpr_get_factor("cv")  # no evaluation yet
    eng.sgpr_set_inducing(X[:20])
    f0, _, _ = eng.sgpr_bound_u("Matern52", u, 1, True, 0.0, want_grad=False)
    assert eng.sgpr_get_factor("cv").shape == (20,)
    eng.sgpr_posterior("Matern52", u, 1, True, 0.0)
    with pytest.raises(_lib.GpsoHipError):
        eng.sgpr_get_factor("LB")  # the install has used its buffer
    leaves = synthetic_leaves(256, d, seed=4)
    before = eng.predict(leaves)
    # rejected calls leave Z and the installed posterior as they were
    bad = X[:7].copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        eng.sgpr_set_inducing(bad)
    with pytest.raises(ValueError):
        eng.sgpr_bound_u("Matern52", u, 2, True, 0.0)  # n_ls neither 1 nor D
    with pytest.raises(ValueError):
        eng.sgpr_select_inducing("Matern52", u, 2, 10)  # refused before it touches the hyper-parameters of the posterior
    with pytest.raises(ValueError):
        eng.sgpr_set_inducing(np.zeros((70000, d)))  # above the row limit: the data and Z stay
    after = eng.predict(leaves)
    np.testing.assert_array_equal(before[0], after[0])
    np.testing.assert_array_equal(before[1], after[1])
    np.testing.assert_array_equal(eng.sgpr_get_inducing()[0], X[:20])
    # no append on an SGPR predictive
    with pytest.raises(_lib.GpsoHipError) as err:
        eng.append(np.full((1, d), 0.5), np.array([0.1]))
    assert err.value.code == _lib.E_STATE and "SGPR" in str(err.value)
    with pytest.raises(_lib.GpsoHipError):
        eng.get_matrix(_lib.MAT_CHOL)
    # new data drops Z
    eng.set_data(X, y)
    with pytest.raises(_lib.GpsoHipError):
        eng.sgpr_bound_u("Matern52", u, 1, True, 0.0)
    eng.close()
    # float32 contexts: GPSO_E_ARG
    e32 = HipGPEngine("float32", device=0)
    e32.set_data(X, y)
    with pytest.raises(ValueError):
        e32.sgpr_set_inducing(X[:5])
    e32.close()


def test_duplicated_rows_and_more_inducing_points_than_data():
    """I - B^-1 is singular when N < M or Z repeats a row: the install shifts by delta (or Kuu, singular up to the jitter,
    fails its factorisation with GPSO_E_NOTPD naming Kuu); the served variance is never below the exact one and at most
    delta k** above it."""
    from pygpso_amd import HipGPEngine

    d = 3
    X, y = synthetic_problem(40, d, seed=6)
    u = S.initial_u(0.5, 1.0, 0.01, 0.0)
    leaves = synthetic_leaves(512, d, seed=7)
    rng = np.random.default_rng(8)
    for Z in (np.vstack([X[:30], X[:3]]), rng.random((70, d))):  # duplicated rows; N = 40 < M = 70
        eng = HipGPEngine("float64", device=0)
        eng.set_data(X, y)
        eng.sgpr_set_inducing(Z)
        try:
            delta = eng.sgpr_posterior("Matern52", u, 1, True, 0.0)
        except np.linalg.LinAlgError as err:
            assert "Kuu" in str(err) and "pivot" in str(err)
            eng.close()
            continue
        post = S.Posterior("Matern52", u, 1, True, 0.0, X, y, Z)
        m_ref, v_ref = post.predict_y(leaves)
        mean, var = eng.predict(leaves)
        print(f"SGPR_DELTA m={Z.shape[0]} delta={delta:g} max(var - exact)={np.max(var - v_ref):.3e} min={np.min(var - v_ref):.3e}")
        assert 0.0 <= delta <= 1.0
        # (the exact variance itself carries the rounding of a Kuu with condition ~1e6: 1e-9 of k** on both sides)
        assert np.all(var >= v_ref - 1e-9 * post.f.var) and np.all(var <= v_ref + (delta + 1e-9) * post.f.var)
        assert _rel(mean, m_ref) <= 1e-7
        eng.close()


# ---- the classes ------------------------------------------------------------------------------------------------------
def _surrogates(m, d=3, n=60, seed=1):
    from pygpso_amd import GPPoint, GPRSurrogate, PointLabels, SGPRSurrogate
    from pygpso_amd import kernels as K

    X, y = synthetic_problem(n, d, seed=seed)
    pts = [GPPoint(X[i], float(y[i]), 0.0, float(y[i]), PointLabels.evaluated) for i in range(n)]
    mk = lambda: dict(gp_kernel=K.Matern52(lengthscales=0.4, variance=1.0), gp_meanf=K.Constant(0.0), points=list(pts))
    return SGPRSurrogate(num_inducing=m, **mk()), GPRSurrogate(**mk()), X, y


def test_sgpr_surrogate_reproduces_gpr_while_n_le_m():
    """The model an SGPRSurrogate builds while N <= M (Z = X, through its own _gp_train) against the GPRSurrogate's model at
    the SAME theta: the GPR's trained lengthscale, variance and mean with the noise set to 1e-2 in both (the trained
    noise sits near its 1e-6 floor, where J / sigma^2 is of order one and the jitter tolerance says nothing)."""
    s, g, X, y = _surrogates(m=128)
    g._gp_train(X, y[:, None])
    s._gp_train(X, y[:, None])
    gm, model = g.gpflow_model, s.gpflow_model
    assert s.gpflow_model.inducing_index is None
    gm.likelihood.variance = 1.0e-2
    gm._resident = False
    model.kernel.lengthscales, model.kernel.variance = gm.kernel.lengthscales, gm.kernel.variance
    model.mean_function.c, model.likelihood.variance = gm.mean_function.c, 1.0e-2
    model._resident = False
    np.testing.assert_array_equal(model.inducing_points, X)
    leaves = synthetic_leaves(1000, X.shape[1], seed=2)
    mg, vg = gm.predict_y(leaves)
    ms, vs = model.predict_y(leaves)
    eps = S.JITTER / gm.likelihood.variance
    c = float(gm.mean_function.c)
    tol_m = 4.0 * eps * (np.max(np.abs(np.asarray(mg) - c)) + np.max(np.abs(y - c)))  # (tests/test_sgpr_cpu.py derives it)
    tol_v = 4.0 * eps * gm.kernel.variance
    print(f"SGPR_LIMIT |dmean| {np.max(np.abs(ms - mg)):.3e} (tol {tol_m:.3e}) |dvar| {np.max(np.abs(vs - vg)):.3e} (tol {tol_v:.3e})")
    assert np.max(np.abs(np.asarray(ms) - np.asarray(mg))) <= tol_m
    assert np.max(np.abs(np.asarray(vs) - np.asarray(vg))) <= tol_v
    gap = model.training_loss() - gm.training_loss()
    assert -1e-9 * abs(gm.training_loss()) <= gap <= 2.0 * X.shape[0] * eps
    assert "SGPR.inducing_variable.Z" in model.summary() and ".inducing_variable.Z" in model.parameter_dict()


def _optimiser(d, budget, surrogate):
    from pygpso_amd import GPSOptimiser, ParameterSpace

    space = ParameterSpace(parameter_names=[f"x{k}" for k in range(d)], parameter_bounds=[[-3.0, 5.0], [-3.0, 3.0]] if d == 2 else [[-3.0, 5.0]] * d)
    return GPSOptimiser(parameter_space=space, gp_surrogate=surrogate, exploration_method="tree", exploration_depth=1 if d > 4 else 5,
                        budget=budget, stopping_condition="evaluations", update_cycle=1, n_workers=1)


def _objective(d):
    if d == 2:
        return rotated_peaks
    return lambda p: float(-np.sum((np.asarray(p)[:d] - 1.0) ** 2) / d + np.cos(np.asarray(p)[0]))


@pytest.mark.parametrize("d,budget,m", [(2, 40, 16), (12, 60, 32)])
def test_optimiser_run_replayed_step_by_step_on_the_oracle(d, budget, m):
    """Every UPDATE of a run (N crosses M on the way) replayed on the oracle from the state the device started it in: the
    same Z (compared where the oracle's runner-up margin on the run's own data exceeds 1e-9; the device's Z is taken as it
    is otherwise), and an optimum as good as the oracle's own L-BFGS-B search reaches from the same start; then the final
    posterior's scores of the stored GP-based points.  NOT replayed: the optimiser loop's per-step arg-max choices
    (explore / select) -- those run on the predict paths, which the tests above hold to the oracle."""
    from pygpso_amd import SGPRSurrogate
    from pygpso_amd import kernels as K

    surr = SGPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), num_inducing=m)
    opt = _optimiser(d, budget, surr)
    calls = []
    orig = surr._gp_train

    def recording(x, y):
        model = surr.gpflow_model
        u0 = S.initial_u(0.25, 1.0, 1e-3, 0.0) if model is None else model._pack()
        orig(x, y)
        model = surr.gpflow_model
        calls.append((x.copy(), y.copy(), u0, model.inducing_points, model._pack(), model._last_nlml))

    surr._gp_train = recording
    best = opt.run(_objective(d))
    assert best is not None and np.isfinite(best.score_mu)
    ns = [c[0].shape[0] for c in calls]
    assert min(ns) <= m < max(ns), f"N never crossed M = {m}: {ns}"
    for x, y, u0, z_dev, u_dev, f_dev in calls:
        ls, var, _, _ = S.unpack(u0, 1, True)
        if x.shape[0] <= m:
            np.testing.assert_array_equal(z_dev, x)
        else:
            idx, margin = S.greedy_select("Matern52", x, ls, var, m, return_margin=True)
            if margin > 1e-9:  # (a run's own data may hold near-ties; then the device's Z is taken as it is)
                np.testing.assert_array_equal(z_dev, x[idx])
        f_at_dev = -S.bound("Matern52", u_dev, 1, True, 0.0, x, y[:, 0], z_dev)
        res = scipy.optimize.minimize(lambda u: S.neg_bound_and_grad_u("Matern52", u, 1, True, 0.0, x, y[:, 0], z_dev)[:2], u0,
                                      jac=True, method="L-BFGS-B")
        # L-BFGS-B stops on a relative decrease of 2.2e-9 (factr 1e7); two searches whose evaluations differ in the last
        # digits may stop an iteration apart: 1e-6 of the loss bounds that, 1e-3 nats absolutely near a loss of zero
        assert f_at_dev <= res.fun + max(1e-3, 1e-6 * abs(res.fun)), (x.shape[0], f_at_dev, res.fun)
    # the final posterior scores the stored GP-based points as the oracle does at the device's hyper-parameters
    from pygpso_amd import PointLabels

    x, y, _, z_dev, u_dev, _ = calls[-1]
    post = S.Posterior("Matern52", u_dev, 1, True, 0.0, x, y[:, 0], z_dev)
    gp = [p for p in surr.points if p.label == PointLabels.gp_based]
    assert gp
    m_ref, v_ref = post.predict_y(np.array([p.normed_coord for p in gp]))
    np.testing.assert_allclose([p.score_mu for p in gp], m_ref, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose([p.score_sigma for p in gp], v_ref, rtol=1e-6, atol=1e-8)


def test_save_from_saved_identical_predictions_and_resume():
    from pygpso_amd import GPSOptimiser, SGPRSurrogate
    from pygpso_amd import kernels as K

    surr = SGPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), num_inducing=12)
    opt = _optimiser(2, 30, surr)
    opt.run(rotated_peaks)
    leaves = synthetic_leaves(500, 2, seed=3)
    want = surr.gpflow_model.predict_y(leaves)
    assert surr.gpflow_model.data[0].shape[0] > 12  # (the saved Z is a greedy choice, not the data)
    opt.save_state(TMP)
    try:
        loaded = SGPRSurrogate.from_saved(TMP)
        assert loaded.num_inducing == 12 and loaded.inducing == "greedy"
        np.testing.assert_array_equal(loaded.gpflow_model.inducing_points, surr.gpflow_model.inducing_points)
        got = loaded.gpflow_model.predict_y(leaves)
        np.testing.assert_array_equal(np.asarray(got[0]), np.asarray(want[0]))
        np.testing.assert_array_equal(np.asarray(got[1]), np.asarray(want[1]))
        best, _ = GPSOptimiser.resume_from_saved(TMP, additional_budget=10, objective_function=rotated_peaks,
                                                 gp_surrogate=SGPRSurrogate)
        assert best is not None and np.isfinite(best.score_mu)
    finally:
        rmtree(TMP, ignore_errors=True)
