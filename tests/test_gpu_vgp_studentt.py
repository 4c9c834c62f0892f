"""
The variational GP's Student-t likelihood on the MI355X: the device's quadrature sequence (gpso_vgp_set_likelihood) against
the float64 oracle (tests/vgp_studentt_oracle.py), the Gaussian through that sequence against the closed-form Gaussian
path, the indefinite step, the predictive through every predict path, robustness to gross outliers, an optimiser run
replayed on the oracle, and save / resume of VGPSurrogate(likelihood=StudentT(...)).
"""
import ctypes as C
import json
import os
from shutil import rmtree

import numpy as np
import pytest

from oracle import gpr
from tests import vgp_oracle as V
from tests import vgp_studentt_oracle as T
from tests.helpers import rotated_peaks, synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TMP = os.path.join(HERE, "_tmp_gpu_vgp_studentt")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _engine(X, y, lik=("StudentT", 3.0)):
    from pygpso_amd import HipGPEngine

    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    eng.vgp_set_likelihood(lik[0], lik[1] if lik[1] is not None else 0.0, T.N_GH)
    eng.vgp_set_q()
    return eng


# ---- device against oracle --------------------------------------------------------------------------------------------
CASES = [(10, 2, "Matern52", False), (10, 12, "SquaredExponential", True), (100, 2, "Matern32", False),
         (100, 12, "Matern12", True), (300, 12, "Matern52", True), (300, 2, "SquaredExponential", False),
         (2048, 12, "Matern32", False), (2048, 2, "Matern52", True),
         (200, 48, "Matern52", True), (130, 48, "SquaredExponential", True)]  # (tests/test_gpu_vgp.py's cases)
# scale 1, df 5: the standardised targets stay within a few scales of the mean, and the oracle's Lambda of both steps keeps
# its smallest eigenvalue near 1 on every case (asserted > 0.3 below)
CASE_LIK = ("StudentT", 5.0)
CASE_SCALE = 1.0


@pytest.mark.parametrize("n,d,kernel,ard", CASES)
def test_device_natgrad_elbo_against_oracle(n, d, kernel, ard):
    X, y = synthetic_problem(n, d, seed=n + d)
    n_ls = d if ard else 1
    ls = 0.3 * np.sqrt(d) * (1.0 + 0.5 * np.arange(d) / d) if ard else 0.3 * np.sqrt(d)
    u = T.initial_u(ls, 1.2, CASE_SCALE, 0.1)
    # (the tolerances of tests/test_gpu_vgp.py: Matern-1/2's r = sqrt(r^2) on the diagonal, 1e-5 / 1e-4; else 2e-9)
    tol = 1e-5 if kernel == "Matern12" else 2e-9
    tol_g = 1e-4 if kernel == "Matern12" else 2e-9
    eng = _engine(X, y, CASE_LIK)
    mu, S = np.zeros(n), np.eye(n)
    for gamma, shift in ((1.0, 0.0), (0.5, 0.2)):
        uu = u + shift
        lam, _ = T.natural_params(kernel, uu, n_ls, True, 0.0, X, y, mu, S, CASE_LIK, gamma)
        assert np.linalg.eigvalsh(lam).min() > 0.3  # (the problem keeps the step positive definite with margin)
        eng.vgp_natgrad(kernel, uu, n_ls, True, 0.0, gamma)
        mu, S = T.natgrad(kernel, uu, n_ls, True, 0.0, X, y, mu, S, CASE_LIK, gamma)
        dmu, dS = eng.vgp_get_q()
        assert _rel(dmu, mu) <= tol, (gamma, _rel(dmu, mu))
        assert _rel(dS @ dS.T, S @ S.T) <= tol, (gamma, _rel(dS @ dS.T, S @ S.T))
        eng.vgp_set_q(mu, S)
        f, g, th = eng.vgp_elbo_u(kernel, uu, n_ls, True, 0.0)
        f_ref, g_ref, th_ref = T.neg_elbo_and_grad_u(kernel, uu, n_ls, True, 0.0, X, y, mu, S, CASE_LIK)
        assert abs(f - f_ref) <= tol * abs(f_ref), (f, f_ref)
        assert _rel(g, g_ref) <= tol_g, (g, g_ref)
        np.testing.assert_allclose(th, th_ref, rtol=1e-15)  # (slot n_ls + 1: the scale, softplus without a shift)
    eng.close()


@pytest.mark.parametrize("n,d,kernel", [(256, 4, "Matern52"), (300, 2, "SquaredExponential")])
def test_gaussian_through_the_quadrature_equals_the_gaussian_path(n, d, kernel):
    """GPSO_LIK_GAUSSIAN_GH (the general sequence with the Gaussian's log density) against the closed-form Gaussian path on
    the device: q, loss and gradient to 1e-12."""
    X, y = synthetic_problem(n, d, seed=7)
    u = V.initial_u(0.4 * np.sqrt(d), 1.1, 0.1, 0.05)
    eg = _engine(X, y, ("Gaussian", None))
    eh = _engine(X, y, ("GaussianGH", None))
    for gamma, shift in ((1.0, 0.0), (0.5, 0.1)):
        uu = u + shift
        eg.vgp_natgrad(kernel, uu, 1, True, 0.0, gamma)
        eh.vgp_natgrad(kernel, uu, 1, True, 0.0, gamma)
        (mg, Sg), (mh, Sh) = eg.vgp_get_q(), eh.vgp_get_q()
        assert _rel(mh, mg) <= 1e-12, (gamma, _rel(mh, mg))
        assert _rel(Sh, Sg) <= 1e-12, (gamma, _rel(Sh, Sg))
        eh.vgp_set_q(mg, Sg)  # the same q for the loss
        fg, gg, tg = eg.vgp_elbo_u(kernel, uu, 1, True, 0.0)
        fh, gh, th = eh.vgp_elbo_u(kernel, uu, 1, True, 0.0)
        assert abs(fh - fg) <= 1e-12 * abs(fg), (fh, fg)
        assert _rel(gh, gg) <= 1e-12, (gh, gg)
        np.testing.assert_array_equal(th, tg)
    eg.close()
    eh.close()


def test_indefinite_step_raises_and_keeps_q():
    """An outlier whose step the oracle proves indefinite: the device answers NOTPD and q is bit for bit the one before."""
    lik = ("StudentT", 3.0)
    X, y = synthetic_problem(40, 2, seed=8)
    y = y.copy()
    y[7] += 30.0
    u = T.initial_u(0.3, 1.0, 0.05, 0.0)
    rng = np.random.default_rng(9)
    mu0 = 0.2 * rng.normal(size=40)
    S0 = np.tril(0.05 * rng.normal(size=(40, 40)), -1) + np.diag(0.6 + 0.3 * rng.random(40))
    lam, _ = T.natural_params("Matern52", u, 1, True, 0.0, X, y, mu0, S0, lik, 1.0)
    assert np.linalg.eigvalsh(lam).min() < -0.1
    eng = _engine(X, y, lik)
    eng.vgp_set_q(mu0, S0)
    before = eng.vgp_get_q()
    with pytest.raises(np.linalg.LinAlgError):
        eng.vgp_natgrad("Matern52", u, 1, True, 0.0, 1.0)
    after = eng.vgp_get_q()
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    # ... and the context goes on: the loss at that q is the oracle's
    f, _, _ = eng.vgp_elbo_u("Matern52", u, 1, True, 0.0)
    f_ref = T.neg_elbo("Matern52", u, 1, True, 0.0, X, y, before[0], before[1], lik)
    assert abs(f - f_ref) <= 1e-9 * abs(f_ref)
    eng.close()


def test_set_likelihood_arguments():
    from pygpso_amd import _lib

    X, y = synthetic_problem(20, 2, seed=1)
    eng = _engine(X, y, ("Gaussian", None))
    x, w = np.polynomial.hermite.hermgauss(20)
    lib, h = _lib.load(), eng._h
    for kind, df, n_gh in ((_lib.LIK_STUDENT_T, 2.0, 20), (_lib.LIK_STUDENT_T, 1.0, 20), (_lib.LIK_STUDENT_T, 3.0, 0),
                           (_lib.LIK_STUDENT_T, 3.0, 65), (3, 3.0, 20), (-1, 3.0, 20)):
        assert lib.gpso_vgp_set_likelihood(h, kind, df, n_gh, _lib.dptr(x), _lib.dptr(w)) == _lib.E_ARG, (kind, df, n_gh)
    assert lib.gpso_vgp_set_likelihood(h, _lib.LIK_STUDENT_T, 3.0, 20, None, None) == _lib.E_ARG
    assert lib.gpso_vgp_set_likelihood(h, _lib.LIK_GAUSSIAN, 0.0, 0, None, None) == _lib.OK
    eng.close()


# ---- the predictive ---------------------------------------------------------------------------------------------------
LIK_P = ("StudentT", 4.0)


def _st_engine(n, d, seed=0, scale=1.0, outlier=None):
    """A Student-t predictive on the device.  scale 1 and no outlier: S S^T stays below I (asserted), the installed form
    is exact; an outlier leaves S S^T above I in a direction (a < 0 in the tails), the install shifts by delta > 0."""
    X, y = synthetic_problem(n, d, seed=seed)
    if outlier is not None:
        y = y.copy()
        y[outlier] += 20.0
    u = T.initial_u(0.3 * np.sqrt(d), 1.1, scale, 0.05)
    mu, S = np.zeros(n), np.eye(n)
    for _ in range(2):
        mu, S = T.natgrad("Matern52", u, 1, True, 0.0, X, y, mu, S, LIK_P, 0.5)
    if outlier is None:
        assert np.linalg.eigvalsh(S @ S.T).max() < 1.0 - 1e-4
    eng = _engine(X, y, LIK_P)
    eng.vgp_set_q(mu, S)
    eng.vgp_posterior("Matern52", u, 1, True, 0.0)
    return eng, T.Posterior("Matern52", u, 1, True, 0.0, X, mu, S, LIK_P), u


@pytest.mark.parametrize("n,d", [(100, 6), (700, 12)])
def test_predict_and_best_ucb_against_oracle(n, d):
    """S S^T < I: the install is exact -- the oracle's two-term GPflow predictive, to 1e-9"""
    eng, post, u = _st_engine(n, d)
    leaves = synthetic_leaves(4096, d, seed=11)
    m_ref, v_ref = post.predict_y(leaves)
    m, v = eng.predict(leaves)
    assert _rel(m, m_ref) <= 1e-9 and _rel(v, v_ref) <= 1e-9, (_rel(m, m_ref), _rel(v, v_ref))
    # the variance carries the Student-t's scale^2 df / (df - 2)
    scale = T.unpack(u, 1, True, 0.0, LIK_P)[2]
    _, vf = post.predict_f(leaves)
    np.testing.assert_allclose(v - vf, scale ** 2 * 4.0 / 2.0, rtol=0, atol=1e-8)
    idx, mu, var, ucb = eng.best_ucb(leaves, gpr.VARSIGMA_DEFAULT)
    u_ref = m_ref + gpr.VARSIGMA_DEFAULT * v_ref
    assert int(idx[0]) == int(np.argmax(u_ref))
    assert abs(ucb[0] - u_ref.max()) <= 1e-9 * abs(u_ref.max())
    eng.close()


def test_predictive_above_the_prior_is_shifted_within_its_bound():
    """An outlier leaves S S^T above I: the device installs var_f + delta (k** - |L^-1 k*|^2) with the oracle's delta, which
    lies within delta k** of GPflow's variance (and never below it); the mean is exact."""
    n, d = 200, 4
    eng, post, u = _st_engine(n, d, outlier=17)
    X, y = synthetic_problem(n, d, seed=0)
    Sq = eng.vgp_get_q()[1]
    delta = T.install_shift(Sq)
    assert 0.0 < delta < 1e-2
    inst = T.Posterior("Matern52", u, 1, True, 0.0, X, post.mu, post.S, LIK_P, installed=True)
    assert inst.delta == delta
    leaves = synthetic_leaves(4096, d, seed=13)
    m, v = eng.predict(leaves)
    m_ref, v_ref = post.predict_y(leaves)
    mi, vi = inst.predict_y(leaves)
    assert _rel(m, m_ref) <= 1e-9 and _rel(v, vi) <= 1e-9, (_rel(m, m_ref), _rel(v, vi))
    assert np.all(v >= v_ref - 1e-9) and np.all(v - v_ref <= delta * post.var + 1e-9)
    eng.close()


def test_best_ucb_grow_equals_best_ucb_on_grown_rows():
    d = 4
    eng, _, _ = _st_engine(200, d)
    rng = np.random.default_rng(5)
    lo = rng.random((3, d)) * 0.5
    bounds = np.stack([lo, lo + 0.3 + 0.2 * rng.random((3, d))], axis=-1)
    depth = 3
    grown = eng.grow(bounds, depth)
    per = grown.shape[1]
    rows = grown.reshape(-1, d)
    got = eng.best_ucb_grow(bounds, depth, gpr.VARSIGMA_DEFAULT)
    want = eng.best_ucb(rows, gpr.VARSIGMA_DEFAULT, seg_off=np.arange(4, dtype=np.int64) * per)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    eng.close()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_sharded_replay_equals_single_context(world):
    from pygpso_amd import _lib

    d, m = 6, 5000
    eng, post, _ = _st_engine(300, d)
    leaves = synthetic_leaves(m, d, seed=21)
    want = eng.best_ucb(leaves, gpr.VARSIGMA_DEFAULT)
    m_ref, v_ref = post.predict_y(leaves)
    assert int(want[0][0]) == int(np.argmax(m_ref + gpr.VARSIGMA_DEFAULT * v_ref))
    payloads = []
    for r in range(world):
        lo_c, hi_c = C.c_int64(), C.c_int64()
        _lib.load().gpso_shard_range(m, r, world, C.byref(lo_c), C.byref(hi_c))
        payloads.append(eng.shard_winners(r, world, leaves[lo_c.value:hi_c.value], m, gpr.VARSIGMA_DEFAULT))
    got = eng.fold_winners(np.stack(payloads), 1, m)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    eng.close()


# ---- robustness: the point of the feature -----------------------------------------------------------------------------
def _clean(X):
    return np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + 0.5 * X[:, 1]


def test_student_t_resists_gross_outliers():
    """120 points of a smooth 2-D function with 5 % gross outliers (+20), theta fixed: the Student-t VGP (scale 0.2, df 3,
    natgrad gamma = 0.1 until q stops moving) against the Gaussian VGP whose noise variance is the Student-t's predictive
    one (0.12; gamma = 1: its exact posterior).  The oracle measures RMSE 0.046 against 2.53 (ratio 0.018) on a grid of
    400 points; the test requires the device's ratio to stay <= 0.1."""
    from pygpso_amd import HipGPEngine

    lik = ("StudentT", 3.0)
    rng = np.random.default_rng(0)
    n = 120
    X = rng.random((n, 2))
    y = _clean(X) + 0.05 * rng.normal(size=n)
    y[rng.choice(n, n // 20, replace=False)] += 20.0
    grid = rng.random((400, 2))
    u = T.initial_u(0.3, 1.0, 0.2, 0.0)
    eng = _engine(X, y, lik)
    mu, S = eng.vgp_get_q()
    for it in range(600):
        eng.vgp_natgrad("Matern52", u, 1, True, 0.0, 0.1)
        m2, S2 = eng.vgp_get_q()
        step = max(np.max(np.abs(m2 - mu)), np.max(np.abs(S2 - S)))
        mu, S = m2, S2
        if step < 1e-10:
            break
    assert step < 1e-10, (it, step)
    eng.vgp_posterior("Matern52", u, 1, True, 0.0)
    m_t, _ = eng.predict(grid)
    eng.close()
    eg = HipGPEngine("float64", device=0)
    eg.set_data(X, y)
    eg.vgp_set_q()
    ug = V.initial_u(0.3, 1.0, 0.2 ** 2 * 3.0, 0.0)
    eg.vgp_natgrad("Matern52", ug, 1, True, 0.0, 1.0)
    eg.vgp_posterior("Matern52", ug, 1, True, 0.0)
    m_g, _ = eg.predict(grid)
    eg.close()
    rmse_t = float(np.sqrt(np.mean((m_t - _clean(grid)) ** 2)))
    rmse_g = float(np.sqrt(np.mean((m_g - _clean(grid)) ** 2)))
    assert rmse_t <= 0.1 * rmse_g, (rmse_t, rmse_g)
    # the device's converged q is the oracle's
    mu_r, S_r = np.zeros(n), np.eye(n)
    for _ in range(it + 1):
        mu_r, S_r = T.natgrad("Matern52", u, 1, True, 0.0, X, y, mu_r, S_r, lik, 0.1)
    assert _rel(mu, mu_r) <= 1e-8 and _rel(S, S_r) <= 1e-8


# ---- the optimiser loop -----------------------------------------------------------------------------------------------
def _outlier_objective():
    """rotated_peaks with a gross outlier (+20) on every 12th evaluation: a diverged simulation now and then"""
    count = [0]

    def f(point):
        count[0] += 1
        return rotated_peaks(point) + (20.0 if count[0] % 12 == 0 else 0.0)

    return f


def _st_optimiser(budget, df=3.0):
    from pygpso_amd import GPSOptimiser, ParameterSpace, VGPSurrogate
    from pygpso_amd import kernels as K

    with open(os.path.join(HERE, "golden", "reference_goldens.json")) as fh:
        g4 = json.load(fh)["G4"]
    space = ParameterSpace(parameter_names=["x", "y"], parameter_bounds=g4["bounds"])
    surr = VGPSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0),
                        likelihood=K.StudentT(scale=1.0, df=df), natgrad_learning_rate=0.1)
    return GPSOptimiser(parameter_space=space, gp_surrogate=surr, exploration_method="tree",
                        exploration_depth=g4["depth"], budget=budget, stopping_condition="evaluations",
                        update_cycle=1, n_workers=1)


def test_optimiser_run_matches_an_oracle_replay():
    from pygpso_amd import PointLabels

    lik = ("StudentT", 3.0)
    opt = _st_optimiser(50)
    surr = opt.gp_surr
    calls = []
    orig = surr._gp_train

    def recording(x, y):
        model = surr.gpflow_model
        before = None if model is None else model.data
        orig(x, y)
        calls.append((before, surr.gpflow_model.data, surr.gpflow_model.q_carried, surr.gpflow_model._pack()))

    surr._gp_train = recording
    best = opt.run(_outlier_objective())
    assert best is not None and np.isfinite(best.score_mu)
    assert len(calls) >= 2
    ev = [p for p in surr.points if p.label == PointLabels.evaluated]
    assert sum(p.score_mu > 15.0 for p in ev) >= 3  # (the outliers are in the data)
    adam = V.Adam(0.01)
    u = mu = S = None
    for i, (before, (x, y), carried, u_dev) in enumerate(calls):
        n = x.shape[0]
        if before is None:
            u = T.initial_u(0.25, 1.0, 1.0, 0.0)
            mu, S = np.zeros(n), np.eye(n)
        else:
            n0 = before[0].shape[0]
            assert carried, f"update {i}: q restarted at the prior"
            np.testing.assert_array_equal(x[:n0], before[0])
            mu2, S2 = np.zeros(n), np.eye(n)
            mu2[:n0], S2[:n0, :n0] = mu, S
            mu, S = mu2, S2
        u, mu, S, adam = T.train("Matern52", u, 1, True, 0.0, x, y[:, 0], mu, S, surr.train_iters, 0.1, adam, lik)
        np.testing.assert_allclose(u_dev, u, rtol=1e-8, atol=1e-10)
    x, y = calls[-1][1]
    post = T.Posterior("Matern52", u, 1, True, 0.0, x, mu, S, lik, installed=True)
    gp = [p for p in surr.points if p.label == PointLabels.gp_based]
    assert gp
    m_ref, v_ref = post.predict_y(np.array([p.normed_coord for p in gp]))
    np.testing.assert_allclose([p.score_mu for p in gp], m_ref, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose([p.score_sigma for p in gp], v_ref, rtol=1e-6, atol=1e-9)
    ucb_ref = m_ref + surr.gp_varsigma * v_ref
    np.testing.assert_array_equal(surr.highest_ucb.normed_coord, gp[int(np.argmax(ucb_ref))].normed_coord)
    # the model reports its trained scale
    pd = surr.gpflow_model.parameter_dict()
    assert ".likelihood.scale" in pd and ".likelihood.variance" not in pd
    assert pd[".likelihood.scale"] == pytest.approx(T.unpack(u_dev, 1, True, 0.0, lik)[2], rel=1e-14)
    assert "VGP.likelihood.scale" in surr.gpflow_model.summary()


# ---- save and resume --------------------------------------------------------------------------------------------------
def _assert_same_surrogate(s, t):
    a, b = s.gpflow_model.parameter_dict(), t.gpflow_model.parameter_dict()
    assert sorted(a) == sorted(b) and ".likelihood.scale" in a
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]))
    assert t.likelihood.name == "StudentT" and t.gpflow_model.likelihood.df == s.gpflow_model.likelihood.df
    Xs = synthetic_leaves(257, 2, seed=3)
    for u, v in zip(s.gpflow_model.predict_y(Xs), t.gpflow_model.predict_y(Xs)):
        np.testing.assert_array_equal(np.asarray(u), np.asarray(v))


def test_save_and_from_saved_keep_scale_and_df():
    opt = _st_optimiser(20, df=4.5)  # (df 4.5: the reference's from_saved would come back with 3)
    opt.run(_outlier_objective())
    s = opt.gp_surr
    s.save(TMP)
    try:
        from pygpso_amd import VGPSurrogate

        with open(os.path.join(TMP, s.GPR_INFO)) as fh:
            info = json.load(fh)
        assert info["vgp_likelihood"] == "StudentT" and info["vgp_likelihood_df"] == 4.5
        t = VGPSurrogate.from_saved(TMP)
        assert t.gpflow_model.likelihood.df == 4.5 and t.natgrad_gamma == 0.1
        _assert_same_surrogate(s, t)
    finally:
        rmtree(TMP)


def test_optimiser_save_state_and_resume():
    from pygpso_amd import GPSOptimiser, VGPSurrogate

    opt = _st_optimiser(25, df=4.5)
    opt.run(_outlier_objective())
    opt.save_state(TMP)
    try:
        _assert_same_surrogate(opt.gp_surr, VGPSurrogate.from_saved(TMP))
        best, _ = GPSOptimiser.resume_from_saved(TMP, additional_budget=10, objective_function=rotated_peaks,
                                                 gp_surrogate=VGPSurrogate)
        assert best is not None and np.isfinite(best.score_mu)
    finally:
        rmtree(TMP)
