"""
The sparse variational GP on inducing points on the MI355X: the device calls (gpso_svgp_*) against the float64 oracle
(tests/svgp_oracle.py) and against the device's own SGPR (the Titsias identity), through the C-ABI wrappers and through
``HipSVGP`` / ``SVGPSurrogate``: q after natural-gradient steps, -ELBO, its gradient, the installed C and beta, every
predict path, determinism, the indefinite step, robustness to gross outliers, the failure paths, and an optimiser run
replayed on the oracle with save / resume.
"""
import ctypes as C
import json
import os
from shutil import rmtree

import numpy as np
import pytest

from oracle import gpr
from tests import sgpr_oracle as S_
from tests import svgp_oracle as O
from tests import vgp_oracle as V
from tests import vgp_studentt_oracle as T
from tests.helpers import rotated_peaks, synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TMP = os.path.join(HERE, "_tmp_gpu_svgp")
# the project's parity tolerances (tests/test_gpu_sgpr.py): 2e-9; Matern-1/2 1e-5 on values, 1e-4 on gradients
TOL, TOL_M12, TOL_G_M12 = 2e-9, 1e-5, 1e-4
GAUSS, STUDENT = ("Gaussian", None), ("StudentT", 5.0)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _ls(d, ard):
    return 0.3 * np.sqrt(d) * (1.0 + 0.5 * np.arange(d) / d) if ard else 0.3 * np.sqrt(d)


def _engine(X, y, Z, lik, dtype="float64"):
    from pygpso_amd import HipGPEngine

    eng = HipGPEngine(dtype, device=0)
    eng.set_data(X, y)
    eng.vgp_set_likelihood(lik[0], lik[1] if lik[1] is not None else 0.0, T.N_GH)
    eng.sgpr_set_inducing(Z)
    return eng


def _conj_s2(lik, p):
    return O.predictive_noise(lik, p)


# ---- 1. device against oracle -----------------------------------------------------------------------------------------
CASES = [(300, 64, 4, "Matern52", False), (500, 100, 2, "Matern32", False), (400, 80, 12, "Matern12", True),
         (2048, 256, 12, "SquaredExponential", True), (8192, 512, 20, "Matern32", False),
         (16384, 1024, 48, "Matern52", True)]


@pytest.mark.parametrize("lik", [GAUSS, STUDENT], ids=["gauss", "studentt"])
@pytest.mark.parametrize("n,m,d,kernel,ard", CASES)
def test_device_against_oracle(n, m, d, kernel, ard, lik):
    from pygpso_amd import _lib

    X, y = synthetic_problem(n, d, seed=n + d)
    n_ls = d if ard else 1
    u = O.initial_u(_ls(d, ard), 1.2, 1.0 if lik == STUDENT else 0.01, lik, c=0.1)
    ls, var, p, _ = O.unpack(u, n_ls, True, 0.0, lik)
    Z = X[S_.greedy_select(kernel, X, ls, var, m)]
    tol = TOL_M12 if kernel == "Matern12" else TOL
    tol_g = TOL_G_M12 if kernel == "Matern12" else TOL
    eng = _engine(X, y, Z, lik)
    errs = {}
    # the start: the prior for the Gaussian (then a gamma = 1 step), the conjugate start for the Student-t
    if lik == GAUSS:
        mu, S = O.natgrad(kernel, u, n_ls, True, 0.0, X, y, Z, np.zeros(m), np.eye(m), lik, 1.0)
        eng.svgp_natgrad(kernel, u, n_ls, True, 0.0, 1.0)
    else:
        s2 = _conj_s2(lik, p)
        mu, S = O.conjugate_start(kernel, u, n_ls, True, 0.0, X, y, Z, lik, s2)
        eng.svgp_init_q(kernel, u, n_ls, True, 0.0, s2)
    mud, Sd = eng.svgp_get_q()
    errs["q0"] = max(_rel(mud, mu), _rel(Sd, S))
    # steps of gamma 1 and 0.1 where the oracle's step is definite; where it is not, the device must say so
    for gamma in (1.0, 0.1):
        try:
            mu, S = O.natgrad(kernel, u, n_ls, True, 0.0, X, y, Z, mu, S, lik, gamma)
        except np.linalg.LinAlgError:
            with pytest.raises(np.linalg.LinAlgError):
                eng.svgp_natgrad(kernel, u, n_ls, True, 0.0, gamma)
            mu, S = eng.svgp_get_q()  # (unchanged: checked in test_indefinite_step_keeps_q)
            continue
        eng.svgp_natgrad(kernel, u, n_ls, True, 0.0, gamma)
        mud, Sd = eng.svgp_get_q()
        errs[f"q{gamma:g}"] = max(_rel(mud, mu), _rel(Sd, S))
        mu, S = mud, Sd  # (each step is compared from the same q)
    f, g, th = eng.svgp_elbo_u(kernel, u, n_ls, True, 0.0)
    f_ref, g_ref, th_ref = O.neg_elbo_and_grad_u(kernel, u, n_ls, True, 0.0, X, y, Z, mu, S, lik)
    errs["elbo"], errs["grad"] = abs(f - f_ref) / abs(f_ref), _rel(g, g_ref)
    delta = eng.svgp_posterior(kernel, u, n_ls, True, 0.0)
    post = O.Posterior(kernel, u, n_ls, True, 0.0, X, Z, mu, S, lik)
    C_ref, beta_ref, _, d_ref = post.installed()
    errs["C"], errs["beta"] = _rel(eng.get_matrix(_lib.MAT_LINV), C_ref), _rel(eng.get_vector(_lib.VEC_ALPHA), beta_ref)
    leaves = synthetic_leaves(2048, d, seed=3)
    md, vd = eng.predict(leaves)
    m_ref, v_ref = post.predict_y_installed(leaves)
    errs["mean"], errs["var"] = _rel(md, m_ref), _rel(vd, v_ref)
    print(f"SVGP_PARITY n={n} m={m} d={d} kernel={kernel} ard={ard} lik={lik[0]} "
          + " ".join(f"{k}={v:.3e}" for k, v in errs.items()) + f" delta={delta:g}")
    eng.close()
    np.testing.assert_allclose(th, th_ref, rtol=1e-15)
    for k in ("q0", "q1", "q0.1", "elbo", "C", "beta", "mean", "var"):
        if k in errs:
            assert errs[k] <= tol, (k, errs[k])
    assert errs["grad"] <= tol_g, errs["grad"]
    assert delta == d_ref


# ---- 2. two independent device paths agree (the Titsias identity) ----------------------------------------------------
@pytest.mark.parametrize("n,m,d,kernel", [(300, 40, 3, "Matern52"), (4096, 512, 12, "Matern32")])
def test_gaussian_step_equals_the_sgpr(n, m, d, kernel):
    from pygpso_amd import HipGPEngine

    X, y = synthetic_problem(n, d, seed=n)
    u = S_.initial_u(0.3 * np.sqrt(d), 1.1, 0.02, 0.15)
    ls, var, _, _ = S_.unpack(u, 1, True)
    Z = S_.choose_inducing(kernel, X, ls, var, m)
    eng = _engine(X, y, Z, GAUSS)
    eng.svgp_natgrad(kernel, u, 1, True, 0.0, 1.0)
    f_svgp, _, _ = eng.svgp_elbo_u(kernel, u, 1, True, 0.0, want_grad=False)
    f_sgpr, _, _ = eng.sgpr_bound_u(kernel, u, 1, True, 0.0, want_grad=False)
    leaves = synthetic_leaves(2048, d, seed=4)
    eng.svgp_posterior(kernel, u, 1, True, 0.0)
    m1, v1 = eng.predict(leaves)
    eng.sgpr_posterior(kernel, u, 1, True, 0.0)
    m2, v2 = eng.predict(leaves)
    print(f"SVGP_TITSIAS n={n} m={m} loss={abs(f_svgp - f_sgpr) / abs(f_sgpr):.3e} mean={_rel(m1, m2):.3e} var={_rel(v1, v2):.3e}")
    eng.close()
    assert abs(f_svgp - f_sgpr) <= 2e-9 * abs(f_sgpr), (f_svgp, f_sgpr)
    assert _rel(m1, m2) <= 2e-9 and _rel(v1, v2) <= 2e-9


# ---- 3. every predict path serves the SVGP posterior ----------------------------------------------------------------
def _svgp_engine(n, d, m, dtype="float64", lik=STUDENT, seed=0):
    X, y = synthetic_problem(n, d, seed=seed)
    u = O.initial_u(0.3 * np.sqrt(d), 1.1, 1.0 if lik == STUDENT else 0.01, lik, c=0.05)
    ls, var, p, _ = O.unpack(u, 1, True, 0.0, lik)
    Z = S_.choose_inducing("Matern52", X, ls, var, m)
    eng = _engine(X, y, Z, lik, dtype=dtype)
    eng.svgp_init_q("Matern52", u, 1, True, 0.0, _conj_s2(lik, p))
    eng.svgp_natgrad("Matern52", u, 1, True, 0.0, 0.5)
    mu, S = eng.svgp_get_q()
    eng.svgp_posterior("Matern52", u, 1, True, 0.0)
    return eng, O.Posterior("Matern52", u, 1, True, 0.0, X, Z, mu, S, lik), y


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_predict_paths(dtype):
    d = 6
    eng, post, y = _svgp_engine(1500, d, 200, dtype=dtype)
    leaves = synthetic_leaves(4096, d, seed=11)
    m_ref, v_ref = post.predict_y_installed(leaves)
    mean, var = eng.predict(leaves)
    idx, mu, va, ucb = eng.best_ucb(leaves, gpr.VARSIGMA_DEFAULT)
    ucb_all = m_ref + gpr.VARSIGMA_DEFAULT * v_ref
    if dtype == "float64":
        assert _rel(mean, m_ref) <= 1e-9 and _rel(var, v_ref) <= 1e-9, (_rel(mean, m_ref), _rel(var, v_ref))
        assert int(idx[0]) == int(np.argmax(ucb_all))
    else:  # (the bounds of __graft_entry__.smoke()'s mixed leg and the float winner rule)
        assert np.max(np.abs(var - v_ref)) <= 2e-5 * post.f.var
        assert np.max(np.abs(mean - m_ref)) <= 1e-4 * max(1.0, float(np.max(np.abs(y))))
        i = int(idx[0])
        assert i == int(np.argmax(ucb_all)) or ucb_all.max() - ucb_all[i] <= 2e-5 * max(1.0, abs(ucb_all.max()))
    got = eng.best_ucb_end(eng.best_ucb_begin(leaves, gpr.VARSIGMA_DEFAULT))
    for a, b in zip(got, (idx, mu, va, ucb)):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    # grow: the winners of best_ucb on the grown rows
    rng = np.random.default_rng(5)
    lo = rng.random((3, d)) * 0.5
    bounds = np.stack([lo, lo + 0.3 + 0.2 * rng.random((3, d))], axis=-1)
    grown = eng.grow(bounds, 3)
    per = grown.shape[1]
    g = eng.best_ucb_grow(bounds, 3, gpr.VARSIGMA_DEFAULT)
    if dtype == "float64":
        w = eng.best_ucb(grown.reshape(-1, d), gpr.VARSIGMA_DEFAULT, seg_off=np.arange(4, dtype=np.int64) * per)
        for a, b in zip(g, w):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    # sharded replay: a single context's answer
    from pygpso_amd import _lib

    world, m = 3, leaves.shape[0]
    payloads = []
    for r in range(world):
        lo_c, hi_c = C.c_int64(), C.c_int64()
        _lib.load().gpso_shard_range(m, r, world, C.byref(lo_c), C.byref(hi_c))
        payloads.append(eng.shard_winners(r, world, leaves[lo_c.value:hi_c.value], m, gpr.VARSIGMA_DEFAULT))
    got = eng.fold_winners(np.stack(payloads), 1, m)
    for a, b in zip(got, (idx, mu, va, ucb)):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    eng.close()


# ---- 4. determinism ---------------------------------------------------------------------------------------------------
def test_repeated_calls_give_identical_bits():
    X, y = synthetic_problem(3000, 8, seed=9)
    u = O.initial_u(0.9, 1.0, 1.0, STUDENT, c=0.0)
    Z = S_.choose_inducing("Matern32", X, 0.9, 1.0, 300)
    eng = _engine(X, y, Z, STUDENT)
    eng.svgp_init_q("Matern32", u, 1, True, 0.0, 5.0 / 3.0)
    q0 = eng.svgp_get_q()
    eng.svgp_natgrad("Matern32", u, 1, True, 0.0, 0.3)
    q1 = eng.svgp_get_q()
    eng.svgp_set_q(*q0)
    eng.svgp_natgrad("Matern32", u, 1, True, 0.0, 0.3)
    q2 = eng.svgp_get_q()
    a = eng.svgp_elbo_u("Matern32", u, 1, True, 0.0)
    b = eng.svgp_elbo_u("Matern32", u, 1, True, 0.0)
    eng.close()
    for x1, x2 in zip(q1, q2):
        np.testing.assert_array_equal(x1, x2)
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[1], b[1])


# ---- 5. / 6. gross outliers ------------------------------------------------------------------------------------------
def _outlier_problem(n=2000):
    rng = np.random.default_rng(0)
    X = rng.random((n, 2))
    y = np.sin(6.0 * X[:, 0]) + np.cos(4.0 * X[:, 1]) + 0.05 * rng.standard_normal(n)
    y[rng.choice(n, n // 20, replace=False)] += 20.0
    g = (np.arange(20) + 0.5) / 20.0
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    return X, y, grid, np.sin(6.0 * grid[:, 0]) + np.cos(4.0 * grid[:, 1])


OUT_LIK = ("StudentT", 3.0)


def _outlier_engine():
    X, y, grid, truth = _outlier_problem()
    from pygpso_amd import HipGPEngine

    u = O.initial_u(0.3, 1.0, 0.2, OUT_LIK, c=0.0)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    eng.vgp_set_likelihood("StudentT", 3.0, T.N_GH)
    eng.sgpr_select_inducing("Matern52", u, 1, 64)
    Z = eng.sgpr_get_inducing()[0]
    return eng, u, X, y, Z, grid, truth


def test_indefinite_step_keeps_q():
    eng, u, X, y, Z, _, _ = _outlier_engine()
    m = Z.shape[0]
    mu, S = np.zeros(m), np.eye(m)
    k_fail = None
    for k in range(2):
        try:
            mu, S = O.natgrad("Matern52", u, 1, False, 0.0, X, y, Z, mu, S, OUT_LIK, 0.1)
        except np.linalg.LinAlgError:
            k_fail = k
            break
    assert k_fail is not None, "the oracle's step from the prior is definite: the case does not test the failure"
    failed = False
    for k in range(2):
        before = eng.svgp_get_q()
        try:
            eng.svgp_natgrad("Matern52", u, 1, False, 0.0, 0.1)
        except np.linalg.LinAlgError:
            after = eng.svgp_get_q()
            for a, b in zip(before, after):
                np.testing.assert_array_equal(a, b)
            failed = True
            break
    eng.close()
    assert failed, "no GPSO_E_NOTPD by step 1"


def test_student_t_resists_gross_outliers():
    """Conjugate start, gamma 0.1 until max |dq| < 1e-10: the Student-t SVGP's RMSE on the grid against the SGPR's at
    noise variance 0.12 on the same Z; the ratio must stay <= 0.1 (the oracle: 0.0082), and the converged q is the oracle's."""
    eng, u, X, y, Z, grid, truth = _outlier_engine()
    m = Z.shape[0]
    s2 = 0.2 ** 2 * 3.0
    eng.svgp_init_q("Matern52", u, 1, False, 0.0, s2)
    mu, S = O.conjugate_start("Matern52", u, 1, False, 0.0, X, y, Z, OUT_LIK, s2)
    steps = 0
    q = eng.svgp_get_q()
    while steps < 2000:
        eng.svgp_natgrad("Matern52", u, 1, False, 0.0, 0.1)
        mu, S = O.natgrad("Matern52", u, 1, False, 0.0, X, y, Z, mu, S, OUT_LIK, 0.1)
        q2 = eng.svgp_get_q()
        steps += 1
        dq = max(np.max(np.abs(q2[0] - q[0])), np.max(np.abs(q2[1] - q[1])))
        q = q2
        if dq < 1e-10:
            break
    eng.svgp_posterior("Matern52", u, 1, False, 0.0)
    mean_t, _ = eng.predict(grid)
    u_g = S_.initial_u(0.3, 1.0, 0.12)
    eng.sgpr_posterior("Matern52", u_g, 1, False, 0.0)
    mean_g, _ = eng.predict(grid)
    eng.close()
    rmse_t = float(np.sqrt(np.mean((mean_t - truth) ** 2)))
    rmse_g = float(np.sqrt(np.mean((mean_g - truth) ** 2)))
    e_q = max(_rel(q[0], mu), _rel(q[1], S))
    print(f"SVGP_OUTLIERS steps={steps} rmse_t={rmse_t:.4f} rmse_sgpr={rmse_g:.4f} ratio={rmse_t / rmse_g:.4f} q_vs_oracle={e_q:.3e}")
    assert steps < 2000
    assert rmse_t / rmse_g <= 0.1, (rmse_t, rmse_g)
    assert e_q <= 1e-8, e_q


# ---- 7. failure paths and call order ----------------------------------------------------------------------------------
def test_failure_paths_and_call_order():
    from pygpso_amd import HipGPEngine

    X, y = synthetic_problem(200, 3, seed=2)
    u = O.initial_u(0.5, 1.0, 0.01, GAUSS, c=0.0)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    for call in (lambda: eng.svgp_natgrad("Matern52", u, 1, True, 0.0, 1.0),
                 lambda: eng.svgp_elbo_u("Matern52", u, 1, True, 0.0),
                 lambda: eng.svgp_posterior("Matern52", u, 1, True, 0.0), lambda: eng.svgp_get_q(),
                 lambda: eng.svgp_init_q()):
        with pytest.raises(RuntimeError, match="inducing points"):
            call()
    # the VGP on the data before Z: as before
    eng.vgp_set_q()
    eng.vgp_natgrad("Matern52", u, 1, True, 0.0, 1.0)
    vq = eng.vgp_get_q()
    assert vq[0].shape == (200,)
    Z = X[:30]
    eng.sgpr_set_inducing(Z)
    mu, S = eng.svgp_get_q()  # (setting Z: the prior)
    np.testing.assert_array_equal(mu, np.zeros(30))
    np.testing.assert_array_equal(S, np.eye(30))
    with pytest.raises(ValueError):
        eng.svgp_natgrad("Matern52", u, 1, True, 0.0, 1.5)
    eng.svgp_natgrad("Matern52", u, 1, True, 0.0, 1.0)
    f_sgpr, g_sgpr, _ = eng.sgpr_bound_u("Matern52", u, 1, True, 0.0)
    f_ref, g_ref, _ = S_.neg_bound_and_grad_u("Matern52", u, 1, True, 0.0, X, y, Z)
    assert abs(f_sgpr - f_ref) <= 2e-9 * abs(f_ref) and _rel(g_sgpr, g_ref) <= 2e-9  # (the SGPR beside the SVGP: unaffected)
    eng.svgp_posterior("Matern52", u, 1, True, 0.0)
    with pytest.raises(RuntimeError, match="SVGP"):
        eng.append(X[:1] + 0.01, y[:1])
    # a new Z: q back at the prior; the next set_data: Z and q dropped
    eng.svgp_natgrad("Matern52", u, 1, True, 0.0, 1.0)
    eng.sgpr_set_inducing(X[:30])
    np.testing.assert_array_equal(eng.svgp_get_q()[0], np.zeros(30))
    eng.set_data(X, y)
    with pytest.raises(RuntimeError, match="inducing points"):
        eng.svgp_get_q()
    eng.close()
    eng32 = HipGPEngine("float32", device=0)
    eng32.set_data(X, y)
    with pytest.raises(ValueError):
        eng32.svgp_elbo_u("Matern52", u, 1, True, 0.0)
    eng32.close()


# ---- 8. SVGPSurrogate inside GPSOptimiser --------------------------------------------------------------------------------
def _outlier_objective():
    """rotated_peaks with a gross outlier (+20) on every 12th evaluation (as tests/test_gpu_vgp_studentt.py)"""
    count = [0]

    def f(point):
        count[0] += 1
        return rotated_peaks(point) + (20.0 if count[0] % 12 == 0 else 0.0)

    return f


def _svgp_optimiser(budget, df=3.0, num_inducing=16):
    from pygpso_amd import GPSOptimiser, ParameterSpace, SVGPSurrogate
    from pygpso_amd import kernels as K

    with open(os.path.join(HERE, "golden", "reference_goldens.json")) as fh:
        g4 = json.load(fh)["G4"]
    space = ParameterSpace(parameter_names=["x", "y"], parameter_bounds=g4["bounds"])
    surr = SVGPSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0),
                         likelihood=K.StudentT(scale=1.0, df=df), num_inducing=num_inducing, natgrad_learning_rate=0.1)
    return GPSOptimiser(parameter_space=space, gp_surrogate=surr, exploration_method="tree",
                        exploration_depth=g4["depth"], budget=budget, stopping_condition="evaluations",
                        update_cycle=1, n_workers=1)


def test_optimiser_run_matches_an_oracle_replay():
    from pygpso_amd import PointLabels

    lik = ("StudentT", 3.0)
    opt = _svgp_optimiser(40)
    surr = opt.gp_surr
    calls = []
    orig = surr._gp_train

    def recording(x, y):
        model = surr.gpflow_model
        u0 = T.initial_u(0.25, 1.0, 1.0, 0.0) if model is None else model._pack().copy()
        orig(x, y)
        mdl = surr.gpflow_model
        calls.append((x.copy(), y.copy(), mdl.inducing_points.copy(), u0, mdl._pack().copy()))

    surr._gp_train = recording
    best = opt.run(_outlier_objective())
    assert best is not None and np.isfinite(best.score_mu)
    assert len(calls) >= 2
    ev = [p for p in surr.points if p.label == PointLabels.evaluated]
    assert sum(p.score_mu > 15.0 for p in ev) >= 2
    adam = V.Adam(0.01)
    for i, (x, y, Z, u0, u_dev) in enumerate(calls):
        if x.shape[0] > 16:
            np.testing.assert_array_equal(Z, S_.choose_inducing("Matern52", x, *O.unpack(u0, 1, True, 0.0, lik)[:2], 16))
        s2 = O.predictive_noise(lik, O.unpack(u0, 1, True, 0.0, lik)[2])
        mu, S = O.conjugate_start("Matern52", u0, 1, True, 0.0, x, y[:, 0], Z, lik, s2)
        u, mu, S, adam = O.train("Matern52", u0, 1, True, 0.0, x, y[:, 0], Z, mu, S, surr.train_iters, 0.1, adam, lik)
        np.testing.assert_allclose(u_dev, u, rtol=1e-8, atol=1e-10)
    x, y, Z, _, _ = calls[-1]
    post = O.Posterior("Matern52", u, 1, True, 0.0, x, Z, mu, S, lik)
    gp = [p for p in surr.points if p.label == PointLabels.gp_based]
    assert gp
    m_ref, v_ref = post.predict_y_installed(np.array([p.normed_coord for p in gp]))
    np.testing.assert_allclose([p.score_mu for p in gp], m_ref, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose([p.score_sigma for p in gp], v_ref, rtol=1e-6, atol=1e-9)
    pd = surr.gpflow_model.parameter_dict()
    assert ".likelihood.scale" in pd and ".q_sqrt" in pd and ".inducing_variable.Z" in pd
    assert "SVGP.likelihood.scale" in surr.gpflow_model.summary()


def _assert_same_surrogate(s, t):
    a, b = s.gpflow_model.parameter_dict(), t.gpflow_model.parameter_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]))
    assert t.likelihood.name == "StudentT" and t.gpflow_model.likelihood.df == s.gpflow_model.likelihood.df
    Xs = synthetic_leaves(257, 2, seed=3)
    for u, v in zip(s.gpflow_model.predict_y(Xs), t.gpflow_model.predict_y(Xs)):
        np.testing.assert_array_equal(np.asarray(u), np.asarray(v))


def test_save_from_saved_and_resume():
    from pygpso_amd import GPSOptimiser, SVGPSurrogate

    opt = _svgp_optimiser(25, df=4.5)
    opt.run(_outlier_objective())
    s = opt.gp_surr
    s.save(TMP)
    try:
        with open(os.path.join(TMP, s.GPR_INFO)) as fh:
            info = json.load(fh)
        assert info["model"] == "SVGP" and info["svgp_likelihood_df"] == 4.5
        t = SVGPSurrogate.from_saved(TMP)
        assert t.natgrad_gamma == 0.1 and t.num_inducing == 16
        _assert_same_surrogate(s, t)
    finally:
        rmtree(TMP)
    opt.save_state(TMP)
    try:
        _assert_same_surrogate(opt.gp_surr, SVGPSurrogate.from_saved(TMP))
        best, _ = GPSOptimiser.resume_from_saved(TMP, additional_budget=10, objective_function=rotated_peaks,
                                                 gp_surrogate=SVGPSurrogate)
        assert best is not None and np.isfinite(best.score_mu)
    finally:
        rmtree(TMP)
