"""Leave-one-out predictive and LOO-CV objective, CPU side: the float64 oracle (tests/loo_oracle.py) against its own
definition (N refits) and against central differences, and the host layer (``HipGPR(objective=...)``, ``GPRSurrogate``,
persistence) over a recording stub engine whose arithmetic is that oracle."""
import json
import os
from shutil import rmtree

import numpy as np
import pytest

from oracle import gpr
from pygpso_amd import GPRSurrogate
from pygpso_amd import kernels as K
from pygpso_amd.model import HipGPR
from tests import hetero_oracle as ho
from tests import loo_oracle as lo
from tests.helpers import rotated_peaks, synthetic_problem
from tests.oracle_engine import OracleEngine

TMP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_tmp_loo")
SMOOTH = ("Matern52", "Matern32", "SquaredExponential")
# (N, D, ARD) of the closed form's check against N refits; half of the cases carry a per-point noise vector
SHAPES = [(3, 1, False), (17, 3, True), (64, 12, True), (129, 6, False)]


def _case(n, d, ard, kernel, noise, seed):
    X, y = synthetic_problem(n, d, seed=seed)
    rng = np.random.default_rng(seed + 100)
    # around the lengthscale of tests.helpers.default_theta_values (0.25 sqrt D)
    ls = (0.25 * np.sqrt(d) * rng.uniform(0.7, 1.4, size=d)) if ard else np.array([0.25 * np.sqrt(d)])
    s = ho.draw_s(n, 0.9, seed=seed + 1) if seed % 2 else None
    return X, y, s, gpr.Theta(kernel, ls, 0.9, noise, 0.15)


# ---- the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [1.0e-3, 1.0e-1])
@pytest.mark.parametrize("kernel", SMOOTH)
@pytest.mark.parametrize("n,d,ard", SHAPES)
def test_closed_form_is_n_refits(n, d, ard, kernel, noise):
    X, y, s, th = _case(n, d, ard, kernel, noise, seed=n + (noise > 1e-2))
    mean, var, lpd, loss = lo.loo_closed(th, X, y, s)
    mean_b, var_b, lpd_b, loss_b = lo.loo_brute(th, X, y, s)
    scale = max(1.0, float(np.max(np.abs(y))))
    errs = (np.max(np.abs(mean - mean_b)) / scale, np.max(np.abs(var - var_b) / var_b), np.max(np.abs(lpd - lpd_b)),
            abs(loss - loss_b) / max(1.0, abs(loss_b)))
    print(f"closed form vs {n} refits ({kernel}, D={d}, noise {noise:g}): mean {errs[0]:.2e} var {errs[1]:.2e} lpd {errs[2]:.2e} "
          f"loss {errs[3]:.2e}")
    # the two are the same rational function of K_y; what separates them is the conditioning of the solves
    # (cond K_y <= N variance / noise ~ 1e5: ~1e-11), measured 2.4e-12
    assert max(errs) <= 1.0e-10, errs


def test_closed_form_is_n_refits_at_300_points():
    X, y, s, th = _case(300, 4, True, "Matern52", 1.0e-3, seed=301)
    a, b = lo.loo_closed(th, X, y, s), lo.loo_brute(th, X, y, s)
    assert np.max(np.abs(a[0] - b[0])) <= 1.0e-10 * max(1.0, float(np.max(np.abs(y))))
    assert np.max(np.abs(a[1] - b[1]) / b[1]) <= 1.0e-10 and np.max(np.abs(a[2] - b[2])) <= 1.0e-10


@pytest.mark.parametrize("noise", [1.0e-3, 1.0e-1])
@pytest.mark.parametrize("n,d,ard", SHAPES[:3])
def test_closed_form_is_n_refits_matern12(n, d, ard, noise):
    """Matern-1/2: the GEMM-form r^2 of the oracle is ~1e-16 instead of 0 on the diagonal and the kernel's sqrt turns that
    into k(x_i, x_i) = variance (1 - 1e-8); the brute force's own predictive variance K_y,ii - ... sees the same matrix, so
    the two agree to the 1e-6 of that perturbation's effect; with r^2 from direct differences, to rounding."""
    X, y, s, th = _case(n, d, ard, "Matern12", noise, seed=n + (noise > 1e-2))
    for direct, tol in ((False, 1.0e-6), (True, 1.0e-10)):
        a = lo.loo_closed(th, X, y, s, direct_r2=direct)
        b = lo.loo_brute(th, X, y, s, direct_r2=direct)
        scale = max(1.0, float(np.max(np.abs(y))))
        err = max(np.max(np.abs(a[0] - b[0])) / scale, np.max(np.abs(a[1] - b[1]) / b[1]), np.max(np.abs(a[2] - b[2])))
        assert err <= tol, (direct, err)


def _fd_check(th, X, y, s, direct_r2, tol):
    n_ls = th.lengthscales.shape[0]
    f, g = lo.loo_loss_and_grad(th, X, y, s, direct_r2=direct_r2)
    assert abs(f - lo.loo_closed(th, X, y, s, direct_r2=direct_r2)[3]) <= 1e-12 * max(1.0, abs(f))
    flat = np.concatenate([th.lengthscales, [th.variance, th.noise, th.mean_c]])
    worst = 0.0
    for k in range(flat.shape[0]):
        h = 1.0e-6 * max(1.0, abs(flat[k]))
        vals = []
        for sign in (+1.0, -1.0):
            q = flat.copy()
            q[k] += sign * h
            vals.append(lo.loo_loss_and_grad(gpr.Theta(th.kernel, q[:n_ls], q[-3], q[-2], q[-1]), X, y, s, direct_r2=direct_r2)[0])
        fd = (vals[0] - vals[1]) / (2.0 * h)
        worst = max(worst, abs(fd - g[k]) / max(1.0, abs(g[k])))
    print(f"gradient vs central differences ({th.kernel}, N={X.shape[0]}, noise {th.noise:g}): {worst:.2e}")
    # central differences at h ~ 1e-6: truncation h^2 F''' and rounding eps |F| cond / h -- the 1e-5 is THEIR limit
    assert worst <= tol, worst


@pytest.mark.parametrize("noise", [1.0e-3, 1.0e-1])
@pytest.mark.parametrize("kernel", SMOOTH)
@pytest.mark.parametrize("n,d,ard", SHAPES[:3])
def test_gradient_against_central_differences(n, d, ard, kernel, noise):
    X, y, s, th = _case(n, d, ard, kernel, noise, seed=n + (noise > 1e-2))
    _fd_check(th, X, y, s, False, 1.0e-5)


@pytest.mark.parametrize("noise", [1.0e-3, 1.0e-1])
@pytest.mark.parametrize("n,d,ard", SHAPES[:3])
def test_gradient_against_central_differences_matern12(n, d, ard, noise):
    """With the GEMM-form r^2 the finite differences of the Matern-1/2 are themselves noise (sqrt of a 1e-16 residue on the
    diagonal moves with theta): the formula is checked with r^2 by direct differences."""
    X, y, s, th = _case(n, d, ard, "Matern12", noise, seed=n + (noise > 1e-2))
    _fd_check(th, X, y, s, True, 1.0e-5)


def test_unconstrained_chain_rule():
    X, y, s, th = _case(17, 3, True, "Matern52", 1.0e-2, seed=9)
    u = th.pack()
    f, gu, th2 = lo.loo_loss_and_grad_u("Matern52", u, X, y, s)
    f_c, g_c = lo.loo_loss_and_grad(th2, X, y, s)
    assert f == f_c and np.array_equal(gu[:5], g_c[:5] * gpr.sigmoid(u[:5])) and gu[5] == g_c[5]
    f_nm, gu_nm, th3 = lo.loo_loss_and_grad_u("Matern52", u[:-1], X, y, s, train_mean=False, mean_c_fixed=u[-1])
    assert f_nm == f and np.array_equal(gu_nm, gu[:-1]) and th3.mean_c == th2.mean_c


# ---- host plumbing over a recording stub --------------------------------------------------------------------------------
class RecordingEngine(OracleEngine):
    """``OracleEngine`` with the calls ``HipGPR`` chooses between, each recorded by name."""

    dtype_name = "float64"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def close(self):
        pass

    def fit_eval(self, *a, **kw):
        self.calls.append("fit_eval")
        return super().fit_eval(*a, **kw)

    def _theta_u(self, kernel, u, n_ls, train_mean, mean_c_fixed):
        full = np.asarray(u, dtype=np.float64) if train_mean else np.concatenate([u, [mean_c_fixed]])
        return gpr.Theta.unpack(kernel, full)

    def fit_eval_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        self.calls.append("fit_eval_u")
        th = self._theta_u(kernel, u, n_ls, train_mean, mean_c_fixed)
        f, g = super().fit_eval(kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
        gu = g[: n_ls + 2] * gpr.sigmoid(np.asarray(u[: n_ls + 2]))
        if train_mean:
            gu = np.concatenate([gu, [g[n_ls + 2]]])
        return f, gu, np.concatenate([th.lengthscales, [th.variance, th.noise, th.mean_c]])

    def fit_batch_max(self):
        return 256

    def fit_eval_u_batch(self, kernel, U, n_ls, train_mean, mean_c_fixed=0.0):
        self.calls.append("fit_eval_u_batch")
        out = [self.fit_eval_u(kernel, u, n_ls, train_mean, mean_c_fixed) for u in U]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.ones(len(out), dtype=bool)

    def fit_eval_loo_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        self.calls.append("fit_eval_loo_u")
        f, gu, th = lo.loo_loss_and_grad_u(kernel, u, self.X, self.y, None, train_mean, mean_c_fixed)
        self.post = gpr.posterior(th, self.X, self.y)
        return f, gu, np.concatenate([th.lengthscales, [th.variance, th.noise, th.mean_c]]), self.post.nlml

    def loo(self):
        self.calls.append("loo")
        return lo.loo_closed(self.post.theta, self.X, self.y)


class Float32Engine(RecordingEngine):
    dtype_name = "float32"


@pytest.fixture(autouse=True)
def stub_engine(monkeypatch):
    monkeypatch.setattr(GPRSurrogate, "engine_factory", RecordingEngine)
    yield
    if os.path.isdir(TMP):
        rmtree(TMP)


def _model(objective=None, engine=None, n=12):
    X, y = synthetic_problem(n, 2, seed=2)
    kw = {} if objective is None else {"objective": objective}
    return HipGPR(data=(X, y[:, None]), kernel=K.Matern52(lengthscales=0.4, variance=1.0), mean_function=K.Constant(0.0),
                  noise_variance=1.0e-2, engine=engine or RecordingEngine(), **kw)


def test_loo_objective_routes_to_the_loo_call_and_never_to_the_nlml_batch():
    m = _model("loo")
    u = m._pack()
    f, gu = m._loss_and_grad(u)
    f_ref, gu_ref, th = lo.loo_loss_and_grad_u("Matern52", u, *[m.data[0], m.data[1][:, 0]])
    assert f == f_ref and np.array_equal(gu, gu_ref)
    assert m._last_nlml == gpr.posterior(th, m.data[0], m.data[1][:, 0]).nlml  # (the NLML rides along)
    U = np.stack([u, u + 0.1, u - 0.2])
    loss, grad, ok = m._loss_and_grad_batch(U)
    assert ok.all() and loss[0] == f_ref and np.array_equal(grad[0], gu_ref)
    assert loss[1] == lo.loo_loss_and_grad_u("Matern52", U[1], m.data[0], m.data[1][:, 0])[0]
    assert m.engine.calls == ["fit_eval_loo_u"] * 4
    assert m.num_loss_evals == 4
    # training_loss is the chosen objective at the current theta, log_marginal_likelihood stays the marginal likelihood
    th0 = gpr.Theta("Matern52", 0.4, 1.0, 1.0e-2, 0.0)
    assert m.training_loss() == lo.loo_closed(th0, m.data[0], m.data[1][:, 0])[3]
    assert m.log_marginal_likelihood() == -gpr.posterior(th0, m.data[0], m.data[1][:, 0]).nlml
    mean, var, lpd, loss0, z = m.loo()
    assert np.array_equal(z, (m.data[1][:, 0] - mean) / np.sqrt(var)) and loss0 == m.training_loss()


def test_default_objective_routes_exactly_as_before():
    m = _model()
    assert m.objective == "nlml"
    u = m._pack()
    f, gu = m._loss_and_grad(u)
    assert (f, list(gu)) == (lambda r: (r[0], list(r[1])))(gpr.loss_and_grad_unconstrained("Matern52", u, m.data[0], m.data[1][:, 0]))
    m._loss_and_grad_batch(np.stack([u, u + 0.1]))
    assert m.engine.calls[:2] == ["fit_eval_u", "fit_eval_u_batch"] and "fit_eval_loo_u" not in m.engine.calls
    assert m.training_loss() == gpr.posterior(gpr.Theta("Matern52", 0.4, 1.0, 1.0e-2, 0.0), m.data[0], m.data[1][:, 0]).nlml
    assert "loo" not in m.engine.calls


def test_refusals_at_construction():
    with pytest.raises(NotImplementedError):
        _model("loo", engine=Float32Engine())
    with pytest.raises(NotImplementedError):
        _model("loo", engine=OracleEngine())  # (an engine without the LOO calls: what a multi-GPU group is)
    with pytest.raises(ValueError):
        _model("cv")
    _model("nlml", engine=Float32Engine())
    with pytest.raises(NotImplementedError):
        _model("nlml", engine=OracleEngine()).loo()


def _surrogate(**kw):
    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy(),
                        **kw)
    rng = np.random.default_rng(0)
    coords = rng.random((14, 2))
    scores = np.array([rotated_peaks((-3 + 8 * c[0], -3 + 6 * c[1])) for c in coords])
    surr.append(coords, scores)
    return surr


def test_surrogate_trains_on_the_loo_loss_and_reports_diagnostics():
    surr = _surrogate(objective="loo")
    surr.gp_update()
    m = surr.gpflow_model
    assert m.objective == "loo" and set(m.engine.calls) <= {"fit_eval_loo_u", "fit_eval", "loo"} and "fit_eval_loo_u" in m.engine.calls
    x, y = surr.current_training_data
    th0 = gpr.Theta("Matern52", 0.25, 1.0, 1.0e-3, 0.0)
    assert m.training_loss() < lo.loo_closed(th0, x, y)[3]
    diag = surr.loo_diagnostics()
    assert sorted(diag) == ["coords", "lpd", "mean", "score", "var", "z"]
    mean, var, lpd, _ = lo.loo_closed(gpr.Theta(*m._theta()), x, y)
    assert np.array_equal(diag["coords"], x) and np.array_equal(diag["score"], y)
    assert np.array_equal(diag["mean"], mean) and np.array_equal(diag["var"], var) and np.array_equal(diag["lpd"], lpd)
    assert np.array_equal(diag["z"], (y - mean) / np.sqrt(var))


def test_multistart_runs_row_by_row_under_the_loo_objective():
    surr = _surrogate(objective="loo")
    surr.optimiser = K.Scipy(restarts=3, seed=1)
    surr.gp_update()
    calls = surr.gpflow_model.engine.calls
    assert "fit_eval_u_batch" not in calls and "fit_eval_u" not in calls and calls.count("fit_eval_loo_u") > 3
    assert len(surr.optimiser.last_result["restarts"]) == 3


def test_save_and_from_saved_keep_the_objective_and_a_default_save_has_no_such_key():
    surr = _surrogate(objective="loo")
    surr.gp_update()
    surr.save(TMP)
    with open(os.path.join(TMP, GPRSurrogate.GPR_INFO)) as fh:
        assert json.load(fh)["objective"] == "loo"
    back = GPRSurrogate.from_saved(TMP)
    assert back.objective == "loo" and back.gpflow_model.objective == "loo"
    assert back.gpflow_model.training_loss() == surr.gpflow_model.training_loss()
    rmtree(TMP)
    plain = _surrogate()
    plain.gp_update()
    plain.save(TMP)
    with open(os.path.join(TMP, GPRSurrogate.GPR_INFO)) as fh:
        info = json.load(fh)
    assert "objective" not in info
    assert sorted(info) == ["dtype", "gp_likelihood", "gp_varsigma", "gpr_kernel", "gpr_kernel_shape", "gpr_meanf",
                            "gpr_meanf_shape", "optimiser", "refit_every", "refit_guard"]
    back = GPRSurrogate.from_saved(TMP)
    assert back.objective == "nlml" and back.gpflow_model.objective == "nlml"


def test_the_sparse_and_variational_surrogates_do_not_take_the_keyword():
    from pygpso_amd.gp_surrogate import SGPRSurrogate, SVGPSurrogate, VGPSurrogate

    for cls in (VGPSurrogate, SGPRSurrogate, SVGPSurrogate):
        with pytest.raises(TypeError):
            cls(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), objective="loo")
