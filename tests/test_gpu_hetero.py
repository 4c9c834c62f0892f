"""
GPU tests of per-point observation noise (``gpso_set_noise_diag`` / ``gpso_append_noise``): K_y = k(X, X) + diag(noise + s)
on every fit path, through the C-ABI, against the float64 oracle of tests/hetero_oracle.py.

Stated tolerances
  float64 ..... L, L^-1, alpha, NLML, gradient, mean, var <= 1e-9 relative (tests/test_gpu_parity.py::test_fit_stages_fp64);
                constant s against the homoscedastic fit at noise + t: 1e-12 relative
  float ....... FLOAT_BOUNDS of tests/test_gpu_parity.py (its tightest row), and no GPSO_E_PRECISION on the first predict
  bits ........ s = zeros equals an untouched context; a batch entry equals the single call; gpso_append on a context with s
                equals gpso_append_noise with zeros
Shapes are the smallest at which each path can go wrong (one block / two blocks / the largest size of the one-launch fit,
a tile edge of the general single-level path, the two-level path, the 192-row tile edge of the append).
"""
import json
import os
from shutil import rmtree

import numpy as np
import pytest

from oracle import gpr
from tests import hetero_oracle as ho
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

VS = gpr.VARSIGMA_DEFAULT
FLOAT_BOUNDS_C3 = (1.8e-4, 1.3e-5)  # tests/test_gpu_parity.py: FLOAT_BOUNDS["C3"], the tightest row (|d mean| / max|y|, |d var| / sigma^2)
TMP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_tmp_gpu_hetero")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hetero_keyword_off_run.json")


def _engine(dtype="float64", **kw):
    from pygpso_amd import HipGPEngine

    return HipGPEngine(dtype, **kw)


def _theta(d, y, kernel="Matern52", noise=1e-3, ard=False, variance=1.3):
    ls = 0.25 * np.sqrt(d) * (np.linspace(0.8, 1.3, d) if ard else np.ones(1))
    return gpr.Theta(kernel, ls, variance, noise, float(y.mean()))


def _fit(eng, X, y, th, s="unset", grad=True):
    eng.set_data(X, y)
    if not isinstance(s, str):
        eng.set_noise_diag(s)
    return eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=grad)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


def _bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays]


_ref_cache = {}


def _reference(n, d, kernel, ard):
    """Problem, s and what the oracle says about them, computed once per case and shared (never modified)."""
    key = (n, d, kernel, ard)
    if key not in _ref_cache:
        X, y = synthetic_problem(n, d, seed=11)
        th = _theta(d, y, kernel=kernel, ard=ard)
        s = ho.draw_s(n, th.variance, seed=n + d)
        post = ho.posterior(th, X, y, s)
        f, g = ho.nlml_and_grad(th, X, y, s)
        Xs = synthetic_leaves(64, d, seed=2)
        mean, var = ho.predict_y(post, Xs)
        _ref_cache[key] = dict(X=X, y=y, th=th, s=s, post=post, f=f, g=g, Linv=ho.linv(post), Xs=Xs, mean=mean, var=var)
    return _ref_cache[key]


# ---- 1. unset == zeros ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,dtype", [(52, 2, "float64"), (200, 3, "float32")])
def test_zeros_give_the_bits_of_an_untouched_context(n, d, dtype):
    X, y = synthetic_problem(n, d, seed=1)
    th = _theta(d, y)
    Xs = synthetic_leaves(64, d, seed=2)
    out = []
    for s in ("unset", np.zeros(n)):
        eng = _engine(dtype)
        f, g = _fit(eng, X, y, th, s)
        mean, var = eng.predict(Xs)
        out.append(_bits([f], g, mean, var))
    assert out[0] == out[1]


# ---- 2. constant s ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(52, 2), (130, 4)])
def test_constant_s_is_the_homoscedastic_fit_at_noise_plus_t(n, d):
    from pygpso_amd import _lib as L

    t = 7.0e-3
    X, y = synthetic_problem(n, d, seed=4)
    th = _theta(d, y)
    shifted = gpr.Theta(th.kernel, th.lengthscales, th.variance, th.noise + t, th.mean_c)
    a, b = _engine(), _engine()
    fa, ga = _fit(a, X, y, th, np.full(n, t))
    fb, gb = _fit(b, X, y, shifted)
    assert abs(fa - fb) <= 1e-12 * abs(fb)
    assert np.max(np.abs(ga - gb) / np.maximum(1.0, np.abs(gb))) <= 1e-12  # (its noise entry included: trace W either way)
    assert _rel(a.get_vector(L.VEC_ALPHA), b.get_vector(L.VEC_ALPHA)) <= 1e-12


# ---- 3 + 4. stages, predict and best-UCB against the hetero oracle (float64) ------------------------------------------------
STAGE_CASES = [
    # n, d, kernel, ard, fused_small, single_level_max
    (10, 2, "Matern52", False, 1, None),             # one block of the one-launch fit
    (70, 3, "SquaredExponential", False, 1, None),   # its two-block algebra (the off-diagonal block receives no s)
    (128, 12, "Matern52", True, 1, None),            # the largest one-launch size, ARD
    (70, 3, "Matern52", False, 0, None),             # the general single-level path
    (130, 4, "SquaredExponential", False, 1, None),  # ... across a tile edge
    (200, 3, "Matern52", False, 1, 0),               # the two-level path
]


@pytest.mark.parametrize("n,d,kernel,ard,fused,slmax", STAGE_CASES)
def test_stages_predict_and_best_ucb_fp64(n, d, kernel, ard, fused, slmax):
    from pygpso_amd import _lib as L

    r = _reference(n, d, kernel, ard)
    th, post = r["th"], r["post"]
    eng = _engine()
    eng._check(eng._lib.gpso_set_option(eng._h, L.OPT_FIT_FUSED_SMALL, fused))
    if slmax is not None:
        eng.set_fit_single_level_max(slmax)
    f, g = _fit(eng, r["X"], r["y"], th, r["s"])
    assert eng.fit_math() == ("small" if (fused and n <= 128) else "f64")
    np.testing.assert_array_equal(eng.get_vector(L.VEC_NOISE_DIAG), r["s"])
    errs = dict(L=_rel(eng.get_matrix(L.MAT_CHOL), post.L), Linv=_rel(eng.get_matrix(L.MAT_LINV), r["Linv"]),
                alpha=_rel(eng.get_vector(L.VEC_ALPHA), post.alpha), nlml=abs(f - r["f"]) / abs(r["f"]),
                grad=float(np.max(np.abs(g - r["g"]) / np.maximum(1.0, np.abs(r["g"])))))
    mean, var = eng.predict(r["Xs"])
    errs["mean"] = float(np.max(np.abs(mean - r["mean"])) / max(1.0, float(np.max(np.abs(r["y"])))))
    errs["var"] = float(np.max(np.abs(var - r["var"])) / th.variance)
    print(f"hetero stages N={n} D={d} {kernel}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= 1e-9 for v in errs.values()), errs
    idx, mu, vv, ucb = eng.best_ucb(r["Xs"], VS)
    i_ref = int(np.argmax(r["mean"] + VS * r["var"]))
    assert int(idx[0]) == i_ref
    assert ucb[0] == mu[0] + VS * vv[0] and (mu[0], vv[0]) == (mean[i_ref], var[i_ref])


# ---- 5. float contexts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,slmax,s_kind", [("float32", None, "drawn"), ("float32", 0, "large"), ("mixed", None, "span1000")])
def test_float_contexts_pass_their_self_test_and_stay_inside_the_float_bounds(dtype, slmax, s_kind):
    n, d = 200, 3
    X, y = synthetic_problem(n, d, seed=11)
    th = _theta(d, y)
    s = ho.draw_s(n, th.variance, seed=21)
    if s_kind == "large":  # max s = 10 x the kernel variance: the plane scales of the two-level float fit
        s[np.argmax(s)] = 10.0 * th.variance
    elif s_kind == "span1000":  # s spanning a factor 1000 (and exact zeros)
        pos = np.flatnonzero(s > 0.0)
        s[pos[np.argmin(s[pos])]] = 1.0e-4 * th.variance
        assert s.max() / s[s > 0.0].min() >= 999.0
    post = ho.posterior(th, X, y, s)
    Xs = synthetic_leaves(64, d, seed=2)
    mean_ref, var_ref = ho.predict_y(post, Xs)
    eng = _engine(dtype)
    if slmax is not None:
        eng.set_fit_single_level_max(slmax)
    f, _ = _fit(eng, X, y, th, s, grad=False)
    if slmax == 0:
        assert eng.fit_math() in ("f16x3", "bf16x6")
    mean, var = eng.predict(Xs)  # the first predict runs the self-test: GPSO_E_PRECISION would raise here
    info = eng.precision_info()
    assert info["passed"]
    em = float(np.max(np.abs(mean - mean_ref)) / np.max(np.abs(y)))
    ev = float(np.max(np.abs(var - var_ref)) / th.variance)
    print(f"hetero float {dtype} slmax={slmax} {s_kind}: |d mean| {em:.2e} ({em / FLOAT_BOUNDS_C3[0]:.2f} of the bound), "
          f"|d var| {ev:.2e} ({ev / FLOAT_BOUNDS_C3[1]:.2f}), self-test |d mean| {info['max_abs_err_mean']:.2e} "
          f"|d var| {info['max_abs_err_var']:.2e}, math {info['predict_math']}, fit {eng.fit_math()}")
    assert abs(f - post.nlml) <= (1e-9 if dtype == "mixed" else 2e-5) * abs(post.nlml)
    assert em <= FLOAT_BOUNDS_C3[0] and ev <= FLOAT_BOUNDS_C3[1]


# ---- 6. batch ----------------------------------------------------------------------------------------------------------------
def test_batch_entries_are_the_single_calls_and_leave_the_context_alone():
    n, d = 52, 2
    X, y = synthetic_problem(n, d, seed=6)
    th = _theta(d, y)
    s = ho.draw_s(n, th.variance, seed=7)
    eng = _engine()
    _fit(eng, X, y, th, s)
    Xs = synthetic_leaves(64, d, seed=2)
    before = (eng.posterior_hash(), _bits(*eng.predict(Xs)))
    u0 = th.pack()
    U = np.stack([u0, u0 + 0.3, u0 - 0.2])
    loss, grad, ok = eng.fit_eval_u_batch(th.kernel, U, 1, True)
    assert ok.all()
    assert (eng.posterior_hash(), _bits(*eng.predict(Xs))) == before
    single = _engine()
    single.set_data(X, y)
    single.set_noise_diag(s)
    for b in range(3):
        f, g, theta = single.fit_eval_u(th.kernel, U[b], 1, True)
        assert _bits([f], g) == _bits([loss[b]], grad[b]), b
        fo, _ = ho.nlml_and_grad(gpr.Theta(th.kernel, theta[:1], theta[1], theta[2], theta[3]), X, y, s)
        assert abs(f - fo) <= 1e-9 * abs(fo)  # (... and it is the hetero model's loss, not the shared-noise one)


# ---- 7. append -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,in_place", [(60, 4, False), (130, 7, True), (190, 5, True)])
def test_append_noise_against_the_from_scratch_oracle(n, k, in_place):
    from pygpso_amd import _lib as L

    d = 3
    X, y = synthetic_problem(n + k, d, seed=8)
    th = _theta(d, y)
    s = ho.draw_s(n + k, th.variance, seed=9)
    s[n] = 0.05 * th.variance  # (a new point with a non-zero term whatever the draw)
    post = ho.appended_posterior(th, X[:n], y[:n], s[:n], X[n:], y[n:], s[n:])
    eng = _engine()
    _fit(eng, X[:n], y[:n], th, s[:n], grad=False)
    f, got_in_place = eng.append(X[n:], y[n:], s[n:])
    assert got_in_place == in_place, eng.last_message()
    np.testing.assert_array_equal(eng.get_vector(L.VEC_NOISE_DIAG), s)
    Xs = synthetic_leaves(64, d, seed=2)
    mean, var = eng.predict(Xs)
    mean_ref, var_ref = ho.predict_y(post, Xs)
    errs = dict(nlml=abs(f - post.nlml) / abs(post.nlml), L=_rel(eng.get_matrix(L.MAT_CHOL), post.L),
                Linv=_rel(eng.get_matrix(L.MAT_LINV), ho.linv(post)), alpha=_rel(eng.get_vector(L.VEC_ALPHA), post.alpha),
                mean=float(np.max(np.abs(mean - mean_ref)) / max(1.0, float(np.max(np.abs(y))))),
                var=float(np.max(np.abs(var - var_ref)) / th.variance))
    print(f"hetero append {n} + {k}: " + ", ".join(f"{q} {v:.2e}" for q, v in errs.items()))
    assert all(v <= 1e-9 for v in errs.values()), errs
    # a fit from scratch on the same context afterwards sees the N + k points AND their s
    f2, _ = eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    assert abs(f2 - post.nlml) <= 1e-9 * abs(post.nlml)


@pytest.mark.parametrize("n,k", [(60, 4), (130, 7)])
def test_plain_append_on_a_context_with_s_appends_zeros_bit_for_bit(n, k):
    from pygpso_amd import _lib as L

    d = 3
    X, y = synthetic_problem(n + k, d, seed=8)
    th = _theta(d, y)
    s = ho.draw_s(n, th.variance, seed=9)
    Xs = synthetic_leaves(64, d, seed=2)
    out = []
    for snew in (None, np.zeros(k)):
        eng = _engine()
        _fit(eng, X[:n], y[:n], th, s, grad=False)
        f, _ = eng.append(X[n:], y[n:], snew)
        out.append((_bits([f], eng.get_vector(L.VEC_NOISE_DIAG), *eng.predict(Xs)), eng.posterior_hash()))
    assert out[0] == out[1]
    np.testing.assert_array_equal(eng.get_vector(L.VEC_NOISE_DIAG), np.concatenate([s, np.zeros(k)]))


def test_append_noise_on_a_context_without_a_vector_creates_one():
    from pygpso_amd import _lib as L

    n, k, d = 130, 3, 2
    X, y = synthetic_problem(n + k, d, seed=10)
    th = _theta(d, y)
    snew = np.array([0.0, 0.02, 0.004]) * th.variance
    eng = _engine()
    _fit(eng, X[:n], y[:n], th, grad=False)
    f, in_place = eng.append(X[n:], y[n:], snew)
    s_all = np.concatenate([np.zeros(n), snew])
    post = ho.posterior(th, X, y, s_all)
    assert in_place and abs(f - post.nlml) <= 1e-9 * abs(post.nlml)
    np.testing.assert_array_equal(eng.get_vector(L.VEC_NOISE_DIAG), s_all)


# ---- 8. statuses -----------------------------------------------------------------------------------------------------------
def test_statuses():
    from pygpso_amd import _lib as L

    n, d = 20, 2
    X, y = synthetic_problem(n, d, seed=12)
    th = _theta(d, y)
    eng = _engine()
    rc = eng._lib.gpso_set_noise_diag(eng._h, L.dptr(np.zeros(n)), n)
    assert rc == L.E_STATE and "gpso_set_data" in eng.last_message()  # no data
    eng.set_data(X, y)
    for bad in (np.zeros(n - 1), np.r_[np.zeros(n - 1), -1e-9], np.r_[np.zeros(n - 1), np.nan], np.r_[np.zeros(n - 1), np.inf]):
        bad = np.ascontiguousarray(bad)
        assert eng._lib.gpso_set_noise_diag(eng._h, L.dptr(bad), bad.shape[0]) == L.E_ARG, bad[-1]
    np.testing.assert_array_equal(eng.get_vector(L.VEC_NOISE_DIAG), np.zeros(n))  # unset: zeros
    s = ho.draw_s(n, th.variance, seed=13)
    eng.set_noise_diag(s)
    np.testing.assert_array_equal(eng.get_vector(L.VEC_NOISE_DIAG), s)
    f, _ = eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    assert abs(f - ho.nlml(th, X, y, s)) <= 1e-9 * abs(f)
    # the posterior is invalidated like a data change
    eng.set_noise_diag(None)
    with pytest.raises(L.GpsoHipError) as err:
        eng.predict(X[:3])
    assert err.value.code == L.E_STATE
    f0, _ = eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    assert abs(f0 - gpr.posterior(th, X, y).nlml) <= 1e-9 * abs(f0)
    # a negative snew
    with pytest.raises(ValueError):
        eng.append(X[:1] + 0.01, y[:1], np.array([-1.0]))
    # every gpso_set_data clears the vector
    eng.set_noise_diag(s)
    eng.set_data(X, y)
    np.testing.assert_array_equal(eng.get_vector(L.VEC_NOISE_DIAG), np.zeros(n))
    # the variational and sparse entry points refuse a context with a vector set -- and say why
    eng.set_noise_diag(s)
    u = th.pack()
    for call in (lambda: eng.vgp_elbo_u(th.kernel, u, 1, True), lambda: eng.vgp_set_q(),
                 lambda: eng.sgpr_set_inducing(X[:5]), lambda: eng.sgpr_bound_u(th.kernel, u, 1, True),
                 lambda: eng.svgp_elbo_u(th.kernel, u, 1, True), lambda: eng.sgpr_bound_uz(th.kernel, u, 1, True)):
        with pytest.raises(ValueError, match="per-point noise"):
            call()
    eng.set_noise_diag(None)
    eng.vgp_set_q()  # cleared: accepted again


# ---- 9. end to end ---------------------------------------------------------------------------------------------------------
def _space():
    from pygpso_amd import ParameterSpace

    return ParameterSpace(parameter_names=["x", "y"], parameter_bounds=[[-3, 5], [-3, 3]])


def _run(noise_keyword, seed=5, budget=30):
    from pygpso_amd import GPSOptimiser

    obj = ho.NoisyPeaks(seed=seed)
    opt = GPSOptimiser(parameter_space=_space(), exploration_method="tree", exploration_depth=4, budget=budget,
                       stopping_condition="evaluations", update_cycle=1, n_workers=1)
    if noise_keyword is None:
        opt.run(obj, eval_repeats=4)
    else:
        opt.run(obj, eval_repeats=4, eval_repeats_noise=noise_keyword)
    return opt, obj


def run_record(opt):
    """theta and the point list of a finished run, exact (JSON round-trips a double through its repr)."""
    model = opt.gp_surr.gpflow_model
    return {"theta": {k: np.asarray(v).tolist() for k, v in model.parameter_dict().items()},
            "points": [[np.asarray(p.normed_coord).tolist(), float(p.score_mu), float(p.score_sigma), float(p.score_ucb),
                        p.label.name] for p in opt.gp_surr.points]}


def test_end_to_end_noisy_objective_with_the_variance_of_the_mean():
    from pygpso_amd import GPSOptimiser
    from pygpso_amd import _lib as L

    opt, obj = _run(True)
    model = opt.gp_surr.gpflow_model
    s = ho.recomputed_variances(opt, obj.calls, 4)
    assert s.shape[0] == opt.gp_surr.num_evaluated >= 30 and np.all(s > 0.0)
    x, _ = opt.gp_surr.current_training_data
    model._ensure_resident()
    # (the model holds the evaluated points in the list's order after a re-optimisation: gp_update hands them over so)
    np.testing.assert_array_equal(model.data[0], x)
    np.testing.assert_allclose(model.engine.get_vector(L.VEC_NOISE_DIAG), s, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(model.engine.get_vector(L.VEC_NOISE_DIAG), opt.gp_surr.current_training_noise)
    Xs = synthetic_leaves(64, 2, seed=2)
    before = _bits(*model.predict_y(Xs))
    opt.save_state(TMP)
    try:
        surr = type(opt.gp_surr).from_saved(TMP)
        assert _bits(*surr.gpflow_model.predict_y(Xs)) == before
        _, opt2 = GPSOptimiser.resume_from_saved(TMP, additional_budget=2, objective_function=obj)
        assert opt2.eval_repeats_noise is True and opt2.gp_surr.num_evaluated > opt.gp_surr.num_evaluated
        np.testing.assert_allclose(opt2.gp_surr.current_training_noise, ho.recomputed_variances(opt2, obj.calls, 4),
                                   rtol=1e-12, atol=0)
    finally:
        rmtree(TMP)


def test_the_run_with_the_keyword_off_is_the_run_of_the_commit_before_the_keyword(monkeypatch):
    """theta and the point list of the run with ``eval_repeats_noise`` off (given as False, or left at its default) against
    tests/golden/hetero_keyword_off_run.json: the record ``run_record`` made of ``_run(None)`` on the package and library
    of the commit before per-point noise existed -- exact (JSON round-trips a double).  On top of that, neither
    ``gpso_set_noise_diag`` nor ``gpso_append_noise`` is ever reached and nothing is stored beside the points."""
    from pygpso_amd import HipGPEngine

    def refuse(self, *args, **kwargs):
        raise AssertionError("a per-point entry point was reached with eval_repeats_noise off")

    monkeypatch.setattr(HipGPEngine, "set_noise_diag", refuse)
    real_append = HipGPEngine.append
    monkeypatch.setattr(HipGPEngine, "append", lambda self, X, y, s=None: refuse(self) if s is not None else real_append(self, X, y))
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    for keyword in (False, None):
        opt, _ = _run(keyword)
        assert opt.gp_surr.current_training_noise is None and opt.gp_surr.gpflow_model.noise_diag is None
        record = run_record(opt)
        assert record["theta"] == golden["theta"], keyword
        assert record["points"] == golden["points"], keyword
