"""Per-point observation noise, CPU side: the float64 oracle (tests/hetero_oracle.py) against central differences and
against ``oracle.gpr`` at a constant s, and the host layer (point store, surrogates, optimiser, persistence) over a stub
engine whose arithmetic is that oracle."""
import json
import os
from shutil import rmtree

import numpy as np
import pytest

from oracle import gpr
from pygpso_amd import GPPoint, GPRSurrogate, GPSOptimiser, ParameterSpace, PointLabels
from pygpso_amd import kernels as K
from pygpso_amd.gp_surrogate import SGPRSurrogate, SVGPSurrogate, VGPSurrogate
from tests import hetero_oracle as ho
from tests.helpers import rotated_peaks, synthetic_problem
from tests.hetero_oracle import NoisyPeaks, recomputed_variances
from tests.oracle_engine import OracleEngine

TMP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_tmp_hetero")


class HeteroOracleEngine(OracleEngine):
    """``OracleEngine`` with the per-point term of ``HipGPEngine``: ``set_noise_diag`` and ``append(..., s)``."""

    def set_data(self, X, y):
        super().set_data(X, y)
        self.s = None  # (every set_data clears the vector)

    def set_noise_diag(self, s):
        if s is not None:
            s = np.asarray(s, dtype=np.float64).reshape(-1)
            assert s.shape[0] == self.n and np.all(s >= 0.0)
        self.s = s
        self.post = None

    def _s(self):
        return np.zeros(self.n) if self.s is None else self.s

    def close(self):
        pass

    def fit_eval(self, kernel, lengthscales, variance, noise, mean_c, want_grad=True):
        th = gpr.Theta(kernel, lengthscales, variance, noise, mean_c)
        f, g = ho.nlml_and_grad(th, self.X, self.y, self._s())
        self.post = ho.posterior(th, self.X, self.y, self._s())
        return f, (g if want_grad else None)

    def append(self, Xnew, ynew, s=None):
        th, s_all = self.post.theta, None
        k = np.atleast_2d(Xnew).shape[0]
        if self.s is not None or s is not None:
            s_all = np.concatenate([self._s(), np.zeros(k) if s is None else np.asarray(s, dtype=np.float64).reshape(-1)])
        self.set_data(np.vstack([self.X, np.atleast_2d(Xnew)]), np.concatenate([self.y, np.asarray(ynew).reshape(-1)]))
        self.s = s_all
        self.post = ho.posterior(th, self.X, self.y, self._s())
        return self.post.nlml, True


@pytest.fixture(autouse=True)
def stub_engine(monkeypatch):
    monkeypatch.setattr(GPRSurrogate, "engine_factory", HeteroOracleEngine)
    yield
    if os.path.isdir(TMP):
        rmtree(TMP)


# ---- the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,ard", [("Matern52", False), ("SquaredExponential", False), ("Matern52", True)])
def test_oracle_gradient_against_central_differences(kernel, ard):
    n, d = 23, 3
    X, y = synthetic_problem(n, d, seed=3)
    s = ho.draw_s(n, 0.8, seed=4)
    ls = np.array([0.4, 0.7, 0.55]) if ard else np.array([0.5])
    th = gpr.Theta(kernel, ls, 0.8, 2.0e-2, 0.1)
    f, g = ho.nlml_and_grad(th, X, y, s)
    assert f == ho.nlml(th, X, y, s)
    flat = np.concatenate([th.lengthscales, [th.variance, th.noise, th.mean_c]])
    for k in range(flat.shape[0]):
        h = 1.0e-6 * max(1.0, abs(flat[k]))
        vals = []
        for sign in (+1.0, -1.0):
            q = flat.copy()
            q[k] += sign * h
            vals.append(ho.nlml(gpr.Theta(kernel, q[:ls.shape[0]], q[-3], q[-2], q[-1]), X, y, s))
        fd = (vals[0] - vals[1]) / (2.0 * h)
        # central differences of a smooth function at h = 1e-6: truncation ~ h^2 f''' and rounding ~ eps |f| / h ~ 1e-9
        assert abs(fd - g[k]) <= 1.0e-6 * max(1.0, abs(g[k])), (k, fd, g[k])


def test_constant_s_is_the_homoscedastic_oracle_at_shifted_noise():
    n, d, t = 31, 2, 3.0e-2
    X, y = synthetic_problem(n, d, seed=5)
    th = gpr.Theta("Matern52", 0.3, 1.2, 1.0e-2, -0.2)
    shifted = gpr.Theta("Matern52", 0.3, 1.2, 1.0e-2 + t, -0.2)
    f, g = ho.nlml_and_grad(th, X, y, np.full(n, t))
    f0, g0 = gpr.nlml_and_grad(shifted, X, y)
    assert f == f0 and np.array_equal(g, g0)  # (noise + t is the same double either way)
    post, post0 = ho.posterior(th, X, y, np.full(n, t)), gpr.posterior(shifted, X, y)
    assert np.array_equal(post.L, post0.L) and np.array_equal(post.alpha, post0.alpha)
    xs = np.random.default_rng(0).random((9, d))
    m, v = ho.predict_y(post, xs)
    m0, v0 = gpr.predict_y(post0, xs)
    # predict_y adds the SHARED noise only: the constant-s model's variance is t below the shifted-noise model's
    assert np.array_equal(m, m0) and np.allclose(v, v0 - t, rtol=0, atol=1e-15)


def test_appended_posterior_is_the_posterior_of_all_points():
    X, y = synthetic_problem(20, 2, seed=6)
    s = ho.draw_s(20, 1.0, seed=7)
    th = gpr.Theta("SquaredExponential", 0.4, 1.0, 1.0e-2, 0.0)
    a = ho.appended_posterior(th, X[:16], y[:16], s[:16], X[16:], y[16:], s[16:])
    b = ho.posterior(th, X, y, s)
    assert np.array_equal(a.L, b.L) and a.nlml == b.nlml
    z = ho.appended_posterior(th, X[:16], y[:16], s[:16], X[16:], y[16:])
    assert np.array_equal(z.L, ho.posterior(th, X, y, np.concatenate([s[:16], np.zeros(4)])).L)


# ---- the parallel store -------------------------------------------------------------------------------------------------
def _surrogate(cls=GPRSurrogate, **kw):
    return cls(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), **kw)


def test_gppoint_stays_the_five_field_tuple():
    assert GPPoint._fields == ("normed_coord", "score_mu", "score_sigma", "score_ucb", "label")


def test_parallel_store_survives_append_find_and_save_load():
    surr = _surrogate()
    assert surr.current_training_noise is None
    coords = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    surr.append(coords, np.array([1.0, 2.0, 3.0]), score_vars=np.array([0.01, 0.0, 0.03]))
    surr.append(np.array([[0.7, 0.8]]), np.array([4.0]))  # none given for this one: zero
    surr.points.append(GPPoint(np.array([0.9, 0.9]), 0.5, 0.1, 0.7, PointLabels.gp_based))
    np.testing.assert_array_equal(surr.current_training_noise, [0.01, 0.0, 0.03, 0.0])
    pts = surr.points
    assert pts.noise_by_coords(np.array([0.5, 0.6 + 5e-13])) == 0.03  # the duplicate tolerance of find_by_coords
    assert pts.noise_by_coords(np.array([0.9, 0.9])) == 0.0 and pts.noise_by_coords(np.array([0.0, 0.0])) == 0.0
    assert pts.find_by_coords(np.array([0.1, 0.2])).score_mu == 1.0
    # an evaluated duplicate keeps its score and so its variance; a gp_based point replaced by an evaluation gets one
    surr.append(np.array([[0.1, 0.2]]), np.array([9.0]), score_vars=np.array([0.5]))
    surr.append(np.array([[0.9, 0.9]]), np.array([7.0]), score_vars=np.array([0.07]))
    x, y = surr.current_training_data
    np.testing.assert_array_equal(y, [1.0, 2.0, 3.0, 4.0, 7.0])
    np.testing.assert_array_equal(surr.current_training_noise, [0.01, 0.0, 0.03, 0.0, 0.07])
    with pytest.raises(ValueError):
        surr.append(np.array([[0.2, 0.2]]), np.array([1.0]), score_vars=np.array([-1.0]))
    with pytest.raises(ValueError):
        surr.append(np.array([[0.2, 0.2]]), np.array([1.0]), score_vars=np.array([np.nan]))
    # save -> load
    surr._gp_train(x, y[:, np.newaxis], s=surr.current_training_noise)
    np.testing.assert_array_equal(surr.gpflow_model.noise_diag, [0.01, 0.0, 0.03, 0.0, 0.07])
    surr.save(TMP)
    assert os.path.exists(os.path.join(TMP, "points_noise.json"))
    loaded = GPRSurrogate.from_saved(TMP)
    assert list(loaded.points) == list(surr.points)
    np.testing.assert_array_equal(loaded.current_training_noise, surr.current_training_noise)
    np.testing.assert_array_equal(loaded.gpflow_model.noise_diag, surr.gpflow_model.noise_diag)
    xs = np.random.default_rng(1).random((7, 2))
    for a, b in zip(surr.gpflow_model.predict_y(xs), loaded.gpflow_model.predict_y(xs)):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def test_model_carries_the_vector_through_fit_append_and_a_reopened_engine(monkeypatch):
    from pygpso_amd.model import HipGPR

    X, y = synthetic_problem(14, 2, seed=8)
    s = ho.draw_s(14, 1.0, seed=9)
    monkeypatch.setattr(HipGPR, "_open_engine", lambda self, dtype: HeteroOracleEngine(dtype))
    model = HipGPR((X[:10], y[:10, None]), K.Matern52(lengthscales=0.3, variance=1.0), K.Constant(0.0),
                   noise_variance=1.0e-2, dtype="float32", noise_diag=s[:10])
    th = gpr.Theta("Matern52", 0.3, 1.0, 1.0e-2, 0.0)
    assert model.training_loss() == ho.nlml(th, X[:10], y[:10], s[:10])
    model.append_data(X[10:12], y[10:12], s_new=s[10:12])
    model.append_data(X[12:], y[12:])  # zeros
    s_all = np.concatenate([s[:12], np.zeros(2)])
    np.testing.assert_array_equal(model.noise_diag, s_all)
    assert model._last_nlml == ho.nlml(th, X, y, s_all)
    f_batch, _, ok = model._loss_and_grad_batch(model.trainable_variables[None, :])
    assert ok[0] and abs(f_batch[0] - ho.nlml(th, X, y, s_all)) <= 1e-12 * abs(f_batch[0])  # (theta through pack / unpack)
    # an engine the model reopens (float32 -> mixed) gets the vector behind the data
    model.engine.dtype_name = "float32"
    assert model._escalate(RuntimeError("precision"))
    np.testing.assert_array_equal(model.engine.s, s_all)
    assert abs(model.training_loss() - ho.nlml(th, X, y, s_all)) <= 1e-12 * abs(model._last_nlml)
    with pytest.raises(ValueError):
        model.noise_diag = s[:3]
    model.data = (X, y[:, None])  # new data clears it, as gpso_set_data does
    assert model.noise_diag is None and model.engine.s is None


def test_gp_update_passes_the_variances_down_and_the_append_path_too():
    X, y = synthetic_problem(12, 2, seed=10)
    s = ho.draw_s(12, 1.0, seed=11)
    surr = _surrogate(refit_every=3, refit_guard=None)
    surr.append(X[:8], y[:8], score_vars=s[:8])
    surr.gp_update()
    np.testing.assert_array_equal(surr.gpflow_model.engine.s, s[:8])
    surr.append(X[8:10], y[8:10], score_vars=s[8:10])
    surr.gp_update()  # an update between re-optimisations: append_data(..., s_new)
    assert surr.gpflow_model.data[0].shape[0] == 10
    np.testing.assert_array_equal(surr.gpflow_model.engine.s, s[:10])
    model = surr.gpflow_model
    th = gpr.Theta("Matern52", np.atleast_1d(model.kernel.lengthscales), model.kernel.variance, model.likelihood.variance,
                   model.mean_function.c)
    assert model._last_nlml == ho.nlml(th, X[:10], y[:10], s[:10])


# ---- the optimiser --------------------------------------------------------------------------------------------------------
def _space():
    return ParameterSpace(parameter_names=["x", "y"], parameter_bounds=[[-3, 5], [-3, 3]])


def _optimiser(budget=18, depth=3):
    return GPSOptimiser(parameter_space=_space(), exploration_method="tree", exploration_depth=depth, budget=budget,
                        stopping_condition="evaluations", update_cycle=1, n_workers=1)


def test_optimiser_stores_the_variance_of_each_mean_score():
    obj = NoisyPeaks(seed=1)
    opt = _optimiser()
    opt.run(obj, eval_repeats=4, eval_repeats_noise=True)
    s = opt.gp_surr.current_training_noise
    assert s.shape[0] == opt.gp_surr.num_evaluated == opt.n_eval_counter and np.all(s > 0.0)
    np.testing.assert_allclose(s, recomputed_variances(opt, obj.calls, 4), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(opt.gp_surr.gpflow_model.engine.s, s)
    # the keyword survives save_state / resume_from_saved, and so do the variances
    opt.save_state(TMP)
    with open(os.path.join(TMP, GPSOptimiser.OPT_ATTRS_FILE)) as fh:
        assert json.load(fh)["eval_repeats_noise"] is True
    _, opt2 = GPSOptimiser.resume_from_saved(TMP, additional_budget=4, objective_function=obj)
    assert opt2.eval_repeats_noise is True
    s2 = opt2.gp_surr.current_training_noise
    # (an evaluation overwrites its gp_based point in place: the evaluated points do not only grow at the end of the list)
    assert s2.shape[0] > s.shape[0] and np.all(s2 > 0.0) and set(s.tolist()) <= set(s2.tolist())
    np.testing.assert_allclose(s2, recomputed_variances(opt2, obj.calls, 4), rtol=1e-12, atol=0)


def test_the_two_value_errors():
    with pytest.raises(ValueError, match="eval_repeats"):
        _optimiser().run(rotated_peaks, eval_repeats=1, eval_repeats_noise=True)
    with pytest.raises(ValueError, match="np.mean"):
        _optimiser().run(rotated_peaks, eval_repeats=4, eval_repeats_function=np.median, eval_repeats_noise=True)


@pytest.mark.parametrize("cls", [VGPSurrogate, SGPRSurrogate, SVGPSurrogate])
def test_the_other_surrogates_refuse_stored_variances(cls):
    surr = _surrogate(cls)
    X, y = synthetic_problem(6, 2, seed=12)
    surr.append(X, y, score_vars=np.zeros(6))  # all zero: nothing to refuse yet (it fails later, on the missing device)
    surr.append(np.array([[0.5, 0.5]]), np.array([0.3]), score_vars=np.array([0.01]))
    with pytest.raises(NotImplementedError, match="per-point observation noise"):
        surr.gp_update()


def _parent_folder_bytes(opt):
    """What the code before per-point noise wrote for this optimiser's surrogate and attributes, restated from its pinned
    schema: points.json, GPRmodel.json, GPRinfo.json, opt_attributes.json."""
    surr, model = opt.gp_surr, opt.gp_surr.gpflow_model
    rows = [{"normed_coord": np.asarray(p.normed_coord).tolist(), "score_mu": float(p.score_mu),
             "score_sigma": float(p.score_sigma), "score_ucb": float(p.score_ucb), "label": p.label.name}
            for p in surr.points]
    params = {k: np.asarray(v).tolist() for k, v in model.parameter_dict().items()}
    info = {"gpr_kernel": model.kernel.name, "gpr_kernel_shape": list(np.shape(model.kernel.lengthscales)),
            "gpr_meanf": type(model.mean_function).__name__, "gpr_meanf_shape": [], "gp_varsigma": surr.gp_varsigma,
            "gp_likelihood": surr.gp_lik_sigma, "optimiser": ["Scipy"], "dtype": surr.dtype,
            "refit_every": surr.refit_every, "refit_guard": surr.refit_guard}
    attrs = {a: getattr(opt, a) for a in ["iterations", "budget", "eval_repeats", "last_explored_levels", "last_update_idx",
                                          "method", "max_depth", "stop_cond", "update_cycle", "n_eval_counter", "n_workers",
                                          "expl_seed"]}
    return {"points.json": json.dumps(rows), "GPRmodel.json": json.dumps(params), "GPRinfo.json": json.dumps(info),
            "opt_attributes.json": json.dumps(attrs)}


def test_a_folder_saved_without_noise_is_what_it_always_was_and_an_old_state_resumes():
    opt = _optimiser(budget=12)
    opt.run(NoisyPeaks(seed=2), eval_repeats=2)
    assert opt.gp_surr.current_training_noise is None and opt.gp_surr.gpflow_model.noise_diag is None
    assert opt.gp_surr.gpflow_model.engine.s is None  # set_noise_diag was never called
    opt.save_state(TMP)
    expected = _parent_folder_bytes(opt)
    assert sorted(os.listdir(TMP)) == sorted(list(expected) + [GPSOptimiser.PARAM_SPACE_FILE])
    for name, text in expected.items():
        with open(os.path.join(TMP, name)) as fh:
            assert fh.read() == text, name
    # ... which is also an OLD state file: no eval_repeats_noise key, no points_noise.json -- it resumes, keyword False
    _, opt2 = GPSOptimiser.resume_from_saved(TMP, additional_budget=3, objective_function=NoisyPeaks(seed=3))
    assert opt2.eval_repeats_noise is False and opt2.gp_surr.current_training_noise is None
    assert opt2.n_eval_counter > opt.n_eval_counter
    # a later save of a surrogate whose variances are all zero removes nothing it does not own and writes no noise file
    opt2.save_state(TMP)
    assert not os.path.exists(os.path.join(TMP, "points_noise.json"))


def test_an_engine_group_forwards_the_vector_to_every_fitting_rank():
    """``HipGPEngineGroup`` with two fake devices: ``set_noise_diag`` and ``append(..., s)`` reach the fitting rank(s) -- rank
    0 of a broadcasting group, every rank of a replicating one -- and the two-argument ``append`` stays a two-argument call."""
    from pygpso_amd import distributed as D

    calls = []

    class Eng:
        dtype_name, dtype = "float64", 0

        def __init__(self, dtype="float64", device=0, **_):
            self.device, self.n, self.d, self.rank, self.world = device, 0, 0, 0, 1

        def close(self):
            pass

        def comm_init(self, rank, world, uid):
            self.rank, self.world = rank, world

        def set_data(self, X, y):
            self.n, self.d = X.shape

        def set_noise_diag(self, s):
            calls.append(("set_noise_diag", self.rank, None if s is None else tuple(s)))

        def append(self, *args):
            calls.append(("append", self.rank, len(args)))
            self.n += len(args[1])
            return 0.5, True

    for posterior, ranks in (("broadcast", [0]), ("replicate", [0, 1])):
        del calls[:]
        grp = D.HipGPEngineGroup("float64", devices=[0, 1], engine_cls=Eng, make_id=lambda: b"n" * 128, posterior=posterior)
        grp.set_data(np.zeros((3, 2)), np.zeros(3))
        grp.set_noise_diag(np.array([0.1, 0.0, 0.2]))
        grp.append(np.zeros((1, 2)), np.zeros(1), np.array([0.3]))
        grp.append(np.zeros((1, 2)), np.zeros(1))
        assert grp.n == 5
        assert sorted(calls) == sorted([("set_noise_diag", r, (0.1, 0.0, 0.2)) for r in ranks]
                                       + [("append", r, 3) for r in ranks] + [("append", r, 2) for r in ranks])
