"""
The variational GP on the MI355X: the reference's five VGPSurrogate tests (tests/test_gp_surrogate.py:350-490 of the
reference) through the drop-in class in float64, and the device calls against the float64 oracle (tests/vgp_oracle.py).
"""
import json
import os
from shutil import rmtree

import numpy as np
import pytest

from oracle import gpr
from tests import vgp_oracle as V
from tests.helpers import kat_fixture, rotated_peaks, synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "reference_goldens_vgp.json")) as fh:
    GV = json.load(fh)["VG1"]
TMP = os.path.join(HERE, "_tmp_gpu_vgp")


def _kat_surrogate(with_points=True):
    from pygpso_amd import GPPoint, PointLabels, VGPSurrogate
    from pygpso_amd import kernels as K

    pts = [GPPoint(*p[:4], PointLabels(p[4])) for p in kat_fixture()] if with_points else None
    return VGPSurrogate(gp_kernel=K.Matern52(), gp_meanf=K.Constant(), likelihood=K.Gaussian(variance=1.0e-3),
                        optimiser=K.Adam(0.01), points=pts, natgrad_learning_rate=1.0, train_iterations=5)


def _trained_kat():
    s = _kat_surrogate()
    x, y = s.current_training_data
    s._gp_train(x=x, y=y[:, np.newaxis])
    return s


# ---- the reference's five tests ---------------------------------------------------------------------------------------
def test_vgp_init():
    from pygpso_amd import GPListOfPoints, VGPSurrogate

    s = _kat_surrogate(with_points=False)
    assert isinstance(s, VGPSurrogate) and isinstance(s.points, GPListOfPoints) and len(s.points) == 0
    s = _kat_surrogate()
    assert isinstance(s, VGPSurrogate) and isinstance(s.points, GPListOfPoints) and len(s.points) == 10


def test_vgp_gp_train_kat():
    s = _trained_kat()
    mean, var = s.gpflow_model.predict_y(np.array(GV["predict_at"]))
    assert float(np.around(mean[0, 0], decimals=8)) == GV["mean"]
    assert float(np.around(var[0, 0], decimals=8)) == GV["var"]


def test_vgp_gp_predict():
    from pygpso_amd import PointLabels

    s = _trained_kat()
    s.gp_predict(np.array(GV["predict_at"]))
    p = s.points[-1]
    assert len(s.points) == 11 and p.label == PointLabels.gp_based
    assert float(np.around(p.score_mu, 8)) == GV["mean"] and float(np.around(p.score_sigma, 8)) == GV["var"]


def test_vgp_gp_eval_best_ucb():
    s = _trained_kat()
    mean, var, ucb = s.gp_eval_best_ucb(np.array(GV["predict_at"]))
    assert float(np.around(mean, 8)) == GV["mean"] and float(np.around(var, 8)) == GV["var"]
    assert float(np.around(ucb, 8)) == float(np.around(mean + s.gp_varsigma * var, 8))
    assert len(s.points) == 10


def test_vgp_save_and_from_saved():
    from pygpso_amd import VGPSurrogate

    s = _trained_kat()
    s.save(TMP)
    try:
        t = VGPSurrogate.from_saved(TMP)
        a, b = s.gpflow_model.parameter_dict(), t.gpflow_model.parameter_dict()
        assert sorted(a) == sorted(b) and ".q_mu" in a and ".q_sqrt" in a
        for k in a:
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]))
        Xs = synthetic_leaves(257, 2, seed=3)
        for u, v in zip(s.gpflow_model.predict_y(Xs), t.gpflow_model.predict_y(Xs)):
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
        assert isinstance(t.optimiser, type(s.optimiser)) and t.optimiser.iterations == 0
    finally:
        rmtree(TMP)


# ---- device calls against the oracle ----------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


CASES = [(10, 2, "Matern52", False), (10, 12, "SquaredExponential", True), (100, 2, "Matern32", False),
         (100, 12, "Matern12", True), (300, 12, "Matern52", True), (300, 2, "SquaredExponential", False),
         (2048, 12, "Matern32", False), (2048, 2, "Matern52", True),
         (200, 48, "Matern52", True), (130, 48, "SquaredExponential", True)]  # (D = 48: the largest, ARD gradient of 51)


@pytest.mark.parametrize("n,d,kernel,ard", CASES)
def test_device_natgrad_elbo_against_oracle(n, d, kernel, ard):
    from pygpso_amd import HipGPEngine

    X, y = synthetic_problem(n, d, seed=n + d)
    n_ls = d if ard else 1
    ls = 0.3 * np.sqrt(d) * (1.0 + 0.5 * np.arange(d) / d) if ard else 0.3 * np.sqrt(d)
    u = V.initial_u(ls, 1.2, 0.01, 0.1)
    # Matern-1/2: its sqrt at r = 0 amplifies the rounding noise of the GEMM-form r^2 on the diagonal, which the oracle and
    # the device's Gram round differently (the GPR parity tests allow 1e-5 for it), and its dk/dr^2 ~ 1/r takes the
    # gradient kernel's direct-difference r where the oracle has the GEMM form: 1e-5 on q and the loss, 1e-4 on the
    # gradient.  The other kernels: 2e-9 (the half step's S^-T S^-1 of a dense D = 2 squared-exponential problem at N = 300
    # measures 1.1e-9).
    tol = 1e-5 if kernel == "Matern12" else 2e-9
    tol_g = 1e-4 if kernel == "Matern12" else 2e-9
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    eng.vgp_set_q()
    mu, S = np.zeros(n), np.eye(n)
    for gamma, shift in ((1.0, 0.0), (0.5, 0.2)):
        uu = u + shift  # the half step at other hyper-parameters
        eng.vgp_natgrad(kernel, uu, n_ls, True, 0.0, gamma)
        mu, S = V.natgrad(kernel, uu, n_ls, True, 0.0, X, y, mu, S, gamma)
        dmu, dS = eng.vgp_get_q()
        assert _rel(dmu, mu) <= tol, (gamma, _rel(dmu, mu))
        assert _rel(dS @ dS.T, S @ S.T) <= tol, (gamma, _rel(dS @ dS.T, S @ S.T))
        eng.vgp_set_q(mu, S)  # continue from the oracle's q: the two paths see the same state
        f, g, th = eng.vgp_elbo_u(kernel, uu, n_ls, True, 0.0)
        f_ref, g_ref, th_ref = V.neg_elbo_and_grad_u(kernel, uu, n_ls, True, 0.0, X, y, mu, S)
        assert abs(f - f_ref) <= tol * abs(f_ref), (f, f_ref)
        assert _rel(g, g_ref) <= tol_g, (g, g_ref)
        np.testing.assert_allclose(th, th_ref, rtol=1e-15)
    eng.close()


def _vgp_engine(n, d, dtype="float64", kernel="Matern52", seed=0, predict_math=None):
    from pygpso_amd import HipGPEngine

    X, y = synthetic_problem(n, d, seed=seed)
    u = V.initial_u(0.3 * np.sqrt(d), 1.1, 0.01, 0.05)
    mu, S = np.zeros(n), np.eye(n)
    for _ in range(2):
        mu, S = V.natgrad(kernel, u, 1, True, 0.0, X, y, mu, S, 1.0)
        u = u - 0.05
    eng = HipGPEngine(dtype, device=0, predict_math=predict_math)
    eng.set_data(X, y)
    eng.vgp_set_q(mu, S)
    eng.vgp_posterior(kernel, u, 1, True, 0.0)
    return eng, V.Posterior(kernel, u, 1, True, 0.0, X, mu, S)


@pytest.mark.parametrize("n,d", [(100, 6), (700, 12)])
def test_predict_and_best_ucb_against_oracle(n, d):
    eng, post = _vgp_engine(n, d)
    leaves = synthetic_leaves(4096, d, seed=11)
    m_ref, v_ref = post.predict_y(leaves)
    m, v = eng.predict(leaves)
    assert _rel(m, m_ref) <= 1e-9 and _rel(v, v_ref) <= 1e-9, (_rel(m, m_ref), _rel(v, v_ref))
    idx, mu, var, ucb = eng.best_ucb(leaves, gpr.VARSIGMA_DEFAULT)
    u_ref = m_ref + gpr.VARSIGMA_DEFAULT * v_ref
    assert int(idx[0]) == int(np.argmax(u_ref))
    assert abs(ucb[0] - u_ref.max()) <= 1e-9 * abs(u_ref.max())
    eng.close()


@pytest.mark.parametrize("math", ["native", "bf16x6", "bf16x3", "f16x3"])
def test_mixed_predict_maths(math):
    n, d = 512, 6
    eng, post = _vgp_engine(n, d, dtype="mixed", predict_math=math)
    leaves = synthetic_leaves(4096, d, seed=12)
    m_ref, v_ref = post.predict_y(leaves)
    m, v = eng.predict(leaves)
    _, y = synthetic_problem(n, d, seed=0)
    # the smoke / GPR bounds of the float maths: 2e-5 sigma^2 on the variance (bf16x3: 2e-4, tests/test_gpu_parity.py),
    # 1e-4 max|y| on the mean
    bound = 2e-4 if math == "bf16x3" else 2e-5
    assert np.max(np.abs(v - v_ref)) <= bound * post.var, (math, np.max(np.abs(v - v_ref)))
    assert np.max(np.abs(m - m_ref)) <= 1e-4 * max(1.0, float(np.max(np.abs(y)))), math
    eng.close()


def test_best_ucb_grow_equals_best_ucb_on_grown_rows():
    d = 4
    eng, _ = _vgp_engine(200, d)
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
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    eng.close()


def test_sharded_replay_equals_single_context():
    d, world, m = 6, 3, 5000
    eng, _ = _vgp_engine(300, d)
    leaves = synthetic_leaves(m, d, seed=21)
    want = eng.best_ucb(leaves, gpr.VARSIGMA_DEFAULT)
    from pygpso_amd import _lib

    payloads = []
    import ctypes as C

    for r in range(world):
        lo_c, hi_c = C.c_int64(), C.c_int64()
        _lib.load().gpso_shard_range(m, r, world, C.byref(lo_c), C.byref(hi_c))
        lo, hi = lo_c.value, hi_c.value
        payloads.append(eng.shard_winners(r, world, leaves[lo:hi], m, gpr.VARSIGMA_DEFAULT))
    got = eng.fold_winners(np.stack(payloads), 1, m)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    eng.close()


def test_vgp_predictive_refuses_append():
    eng, _ = _vgp_engine(50, 3)
    with pytest.raises(Exception):
        eng.append(np.full((1, 3), 0.5), np.array([0.1]))
    eng.close()


# ---- the optimiser loop -----------------------------------------------------------------------------------------------
def _vgp_optimiser(budget, surrogate=None):
    from pygpso_amd import GPSOptimiser, ParameterSpace, VGPSurrogate
    from pygpso_amd import kernels as K

    with open(os.path.join(HERE, "golden", "reference_goldens.json")) as fh:
        g4 = json.load(fh)["G4"]
    space = ParameterSpace(parameter_names=["x", "y"], parameter_bounds=g4["bounds"])
    surr = surrogate or VGPSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0))
    return GPSOptimiser(parameter_space=space, gp_surrogate=surr, exploration_method="tree",
                        exploration_depth=g4["depth"], budget=budget, stopping_condition="evaluations",
                        update_cycle=1, n_workers=1)


def test_optimiser_run_matches_an_oracle_replay():
    from pygpso_amd import PointLabels

    opt = _vgp_optimiser(50)
    surr = opt.gp_surr
    calls = []
    orig = surr._gp_train

    def recording(x, y):
        model = surr.gpflow_model
        before = None if model is None else model.data
        orig(x, y)
        calls.append((before, surr.gpflow_model.data, surr.gpflow_model.q_carried, surr.gpflow_model._pack()))

    surr._gp_train = recording
    best = opt.run(rotated_peaks)
    assert best is not None and np.isfinite(best.score_mu)
    assert len(calls) >= 2
    # replay every update in the model's row order, Adam state and q carried, on the oracle
    adam = V.Adam(0.01)
    u = mu = S = None
    for i, (before, (x, y), carried, u_dev) in enumerate(calls):
        n = x.shape[0]
        if before is None:
            u = V.initial_u(0.25, 1.0, 1e-3, 0.0)
            mu, S = np.zeros(n), np.eye(n)
        else:
            # the evaluated points only grow: every update keeps q for the rows already held, in their order
            n0 = before[0].shape[0]
            assert carried, f"update {i}: q restarted at the prior"
            np.testing.assert_array_equal(x[:n0], before[0])
            np.testing.assert_array_equal(y[:n0], before[1])
            mu2, S2 = np.zeros(n), np.eye(n)
            mu2[:n0], S2[:n0, :n0] = mu, S
            mu, S = mu2, S2
        u, mu, S, adam = V.train("Matern52", u, 1, True, 0.0, x, y[:, 0], mu, S, surr.train_iters, 1.0, adam)
        theta_dev = V.unpack(u_dev, 1, True)
        theta_ref = V.unpack(u, 1, True)
        np.testing.assert_allclose(np.concatenate([theta_dev[0], theta_dev[1:]]),
                                   np.concatenate([theta_ref[0], theta_ref[1:]]), rtol=1e-8)
    # the same best point: the replay's data has its maximum where the run's best point is ...
    x, y = calls[-1][1]
    ev = [p for p in surr.points if p.label == PointLabels.evaluated]
    ys = np.array([p.score_mu for p in ev])
    assert best.score_mu == ys.max() == y.max()
    np.testing.assert_array_equal(best.normed_coord, ev[int(np.argmax(ys))].normed_coord)
    # ... and the replay's final posterior scores the stored GP-based points as the run did, with the same best UCB
    post = V.Posterior("Matern52", u, 1, True, 0.0, x, mu, S)
    gp = [p for p in surr.points if p.label == PointLabels.gp_based]
    assert gp
    m_ref, v_ref = post.predict_y(np.array([p.normed_coord for p in gp]))
    np.testing.assert_allclose([p.score_mu for p in gp], m_ref, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose([p.score_sigma for p in gp], v_ref, rtol=1e-6, atol=1e-9)
    ucb_ref = m_ref + surr.gp_varsigma * v_ref
    np.testing.assert_array_equal(surr.highest_ucb.normed_coord, gp[int(np.argmax(ucb_ref))].normed_coord)


def test_data_growth_keeps_q_on_the_device():
    """gpso_vgp_extend_q inside one padded size (N 100 -> 120) and across one (120 -> 140): q of the held rows, the prior
    for the new ones"""
    from pygpso_amd import HipGPEngine

    d = 3
    X, y = synthetic_problem(140, d, seed=9)
    u = V.initial_u(0.5, 1.0, 0.01, 0.0)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X[:100], y[:100])
    eng.vgp_set_q()
    eng.vgp_natgrad("Matern52", u, 1, True, 0.0, 1.0)
    mu, S = eng.vgp_get_q()
    for n in (120, 140):
        eng.set_data(X[:n], y[:n])
        eng.vgp_extend_q()
        m2, S2 = eng.vgp_get_q()
        want_mu, want_S = np.zeros(n), np.eye(n)
        want_mu[: mu.shape[0]], want_S[: mu.shape[0], : mu.shape[0]] = mu, S
        np.testing.assert_array_equal(m2, want_mu)
        np.testing.assert_array_equal(S2, want_S)
        mu, S = m2, S2
    eng.close()


def test_getters_on_a_vgp_predictive():
    from pygpso_amd import _lib

    eng, post = _vgp_engine(60, 3)
    with pytest.raises(_lib.GpsoHipError):
        eng.get_matrix(_lib.MAT_CHOL)
    with pytest.raises(_lib.GpsoHipError):
        eng.get_vector(_lib.VEC_WHITE)
    import scipy.linalg

    Linv = scipy.linalg.solve_triangular(post.L, np.eye(60), lower=True)
    np.testing.assert_allclose(eng.get_vector(_lib.VEC_ALPHA), Linv.T @ post.mu, rtol=0, atol=1e-9)
    eng.close()


def test_optimiser_save_and_resume():
    from pygpso_amd import GPSOptimiser, VGPSurrogate

    opt = _vgp_optimiser(25)
    opt.run(rotated_peaks)
    opt.save_state(TMP)
    try:
        best, _ = GPSOptimiser.resume_from_saved(TMP, additional_budget=10, objective_function=rotated_peaks,
                                                 gp_surrogate=VGPSurrogate)
        assert best is not None and np.isfinite(best.score_mu)
    finally:
        rmtree(TMP)


def test_scipy_optimiser_drives_the_vgp():
    from pygpso_amd import kernels as K

    s = _kat_surrogate()
    s.optimiser = K.Scipy()
    s.train_iters = 1
    x, y = s.current_training_data
    s._gp_train(x=x, y=y[:, np.newaxis])
    u_dev = s.gpflow_model._pack()
    n = x.shape[0]
    mu, S = V.natgrad("Matern52", V.initial_u(1.0, 1.0, 1e-3, 0.0), 1, True, 0.0, x, y, np.zeros(n), np.eye(n), 1.0)
    import scipy.optimize

    res = scipy.optimize.minimize(lambda u: V.neg_elbo_and_grad_u("Matern52", u, 1, True, 0.0, x, y, mu, S)[:2],
                                  V.initial_u(1.0, 1.0, 1e-3, 0.0), jac=True, method="L-BFGS-B")
    np.testing.assert_allclose(np.concatenate([V.unpack(u_dev, 1, True)[0], V.unpack(u_dev, 1, True)[1:]]),
                               np.concatenate([V.unpack(res.x, 1, True)[0], V.unpack(res.x, 1, True)[1:]]), rtol=1e-6)
