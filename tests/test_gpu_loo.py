"""
GPU tests of the leave-one-out predictive (``gpso_loo``) and the LOO-CV objective (``gpso_fit_eval_loo`` / ``_u``), through
the C-ABI, against the float64 oracle of tests/loo_oracle.py.

Stated tolerances (the project's own for float64 stages, tests/test_gpu_parity.py::test_fit_stages_fp64)
  float64 / mixed . loss and the returned NLML 1e-9 relative; gradient 1e-8 by max(1, |g|); mean 1e-8 max|y|, var 1e-8 relative,
                    lpd 1e-8 by max(1, |lpd|); Matern-1/2 at that test's 1e-5 (1e-4 where it takes ten times the tolerance)
  float32 ......... FLOAT32_LOO_BOUNDS below: 5 x the maxima measured on these shapes (profiles/loo_float_errors.txt)
  bits ............ what gpso_fit_eval_loo leaves resident equals a fresh context's gpso_fit_eval; gpso_loo reads only
Shapes: 2 the smallest legal N; 128 | 129 the edge of the one-launch path and of the padding; 300 pads to 384 (several 64-tiles,
a ragged last one); (40, 26) a padded D too wide for the one-workgroup kernel's LDS.  Half of the cases carry a per-point noise vector.
"""
import json
import os

import numpy as np
import pytest

from oracle import gpr
from tests import hetero_oracle as ho
from tests import loo_oracle as lo
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

KERNELS = ("Matern52", "Matern32", "Matern12", "SquaredExponential")
SHAPES = [(2, 1, False), (3, 1, False), (17, 3, True), (64, 12, True), (128, 6, False), (129, 3, True), (300, 5, True),
          (40, 26, True)]  # (the last: a padded D above 24, where the one-workgroup kernel reads the scaled inputs from global memory)
NOISES = (1.0e-3, 1.0e-1)
CASES = [(n, d, ard, k) for (n, d, ard) in SHAPES for k in KERNELS if n <= 129 or k in ("Matern52", "SquaredExponential")]
FLOAT_SHAPES = [(64, 12, True), (129, 3, True), (300, 5, True)]
# float32 engines, gpso_loo against the oracle on FLOAT_SHAPES: (max |d mean| / max|y|, max |d var| / var), 5 x the measured
# maxima of profiles/loo_float_errors.txt (the SMALL_FLOAT_BOUNDS convention of tests/test_gpu_parity.py)
FLOAT32_LOO_BOUNDS = (3.3e-5, 1.2e-3)  # measured 6.6e-6, 2.3e-4 (N = 300)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_default_objective_theta.json")


def _engine(dtype="float64", **kw):
    from pygpso_amd import HipGPEngine

    return HipGPEngine(dtype, **kw)


def _fused(eng, on):
    from pygpso_amd import _lib as L

    eng._check(eng._lib.gpso_set_option(eng._h, L.OPT_FIT_FUSED_SMALL, int(on)))


_ref_cache = {}


def reference(n, d, ard, kernel, noise):
    """Problem, theta, s (every other case) and what the oracle says, computed once per case and shared (never modified)."""
    key = (n, d, ard, kernel, noise)
    if key not in _ref_cache:
        X, y = synthetic_problem(n, d, seed=17 + n)
        ls = 0.25 * np.sqrt(d) * (np.linspace(0.8, 1.3, d) if ard else np.ones(1))
        th = gpr.Theta(kernel, ls, 1.3, noise, float(y.mean()))
        with_s = bool((SHAPES.index((n, d, ard)) + KERNELS.index(kernel) + NOISES.index(noise)) % 2)
        s = ho.draw_s(n, th.variance, seed=n + d) if with_s else None
        mean, var, lpd, loss = lo.loo_closed(th, X, y, s)
        f, g = lo.loo_loss_and_grad(th, X, y, s)
        nlml = ho.posterior(th, X, y, np.zeros(n) if s is None else s).nlml
        u = th.pack()
        fu, gu, _ = lo.loo_loss_and_grad_u(kernel, u, X, y, s)
        _ref_cache[key] = dict(X=X, y=y, th=th, s=s, mean=mean, var=var, lpd=lpd, loss=loss, f=f, g=g, nlml=nlml, u=u, fu=fu, gu=gu)
    return _ref_cache[key]


def _load(eng, r):
    eng.set_data(r["X"], r["y"])
    if r["s"] is not None:
        eng.set_noise_diag(r["s"])


def objective_errors(r, f, g, nlml):
    return dict(loss=abs(f - r["f"]) / abs(r["f"]), nlml=abs(nlml - r["nlml"]) / abs(r["nlml"]),
                grad=float(np.max(np.abs(g - r["g"]) / np.maximum(1.0, np.abs(r["g"])))))


def predictive_errors(r, mean, var, lpd):
    return dict(mean=float(np.max(np.abs(mean - r["mean"])) / np.max(np.abs(r["y"]))),
                var=float(np.max(np.abs(var - r["var"]) / r["var"])),
                lpd=float(np.max(np.abs(lpd - r["lpd"]) / np.maximum(1.0, np.abs(r["lpd"])))))


def _tols(kernel):
    t = 1.0e-5 if kernel == "Matern12" else 1.0e-9
    return dict(loss=t, nlml=t, grad=10 * t, mean=10 * t, var=10 * t, lpd=10 * t)


def _hold(errs, tols, what):
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= tols[k], (what, k, v, tols[k])


# ---- 1. the objective, the _u variant and the predictive against the oracle, on both paths ------------------------------
@pytest.mark.parametrize("n,d,ard,kernel", CASES)
def test_objective_and_predictive_against_the_oracle(n, d, ard, kernel):
    tols = _tols(kernel)
    for noise in NOISES:
        r = reference(n, d, ard, kernel, noise)
        th = r["th"]
        for fused in ((1, 0) if n <= 128 else (1,)):
            eng = _engine()
            _fused(eng, fused)
            _load(eng, r)
            f, g, nlml = eng.fit_eval_loo(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
            assert eng.fit_math() == ("small" if (fused and n <= 128) else "f64")
            what = f"N={n} D={d} {kernel} noise {noise:g} s={'yes' if r['s'] is not None else 'no'} fused={fused}"
            _hold(objective_errors(r, f, g, nlml), tols, "loo objective " + what)
            mean, var, lpd, loss = eng.loo()
            assert abs(loss - r["loss"]) <= tols["loss"] * abs(r["loss"])
            _hold(predictive_errors(r, mean, var, lpd), tols, "loo predictive " + what)
            # the optimiser's variables: the same evaluation behind the host-side transforms
            fu, gu, theta, nlml_u = eng.fit_eval_loo_u(th.kernel, r["u"], th.lengthscales.shape[0], True)
            assert abs(fu - r["fu"]) <= tols["loss"] * abs(r["fu"]) and abs(nlml_u - r["nlml"]) <= tols["nlml"] * abs(r["nlml"])
            assert float(np.max(np.abs(gu - r["gu"]) / np.maximum(1.0, np.abs(r["gu"])))) <= tols["grad"]
            np.testing.assert_allclose(theta, np.concatenate([th.lengthscales, [th.variance, th.noise, th.mean_c]]), rtol=1e-12)
            # without a trained mean: one entry fewer, the same others
            fm, gm, _, _ = eng.fit_eval_loo_u(th.kernel, r["u"][:-1], th.lengthscales.shape[0], False, th.mean_c)
            assert fm == fu and np.array_equal(gm, gu[:-1])
            # no gradient asked for: the same loss
            f2, g2, _ = eng.fit_eval_loo(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
            assert g2 is None and f2 == f


def test_a_smaller_evaluation_after_a_larger_one_reads_no_stale_padding():
    """300 then 260 points on one context, both padded to 384: the second evaluation finds the first one's rows in the
    padding of K^-1, L^-1 and the weight buffers; nothing may read them."""
    big = reference(300, 5, True, "Matern52", 1.0e-3)
    eng = _engine()
    X, y = big["X"][:260], big["y"][:260]
    th = big["th"]
    eng.set_data(big["X"], big["y"])
    eng.fit_eval_loo(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    eng.set_data(X, y)
    got = eng.fit_eval_loo(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    assert eng.padded_n == 384
    fresh = _engine()
    fresh.set_data(X, y)
    want = fresh.fit_eval_loo(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2]
    f_ref, g_ref = lo.loo_loss_and_grad(th, X, y)
    assert abs(got[0] - f_ref) <= 1e-9 * abs(f_ref) and np.max(np.abs(got[1] - g_ref) / np.maximum(1.0, np.abs(g_ref))) <= 1e-8


# ---- 2. residency -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,ard,dtype", [(64, 12, True, "float64"), (129, 3, True, "float64"), (300, 5, True, "float64"),
                                           (64, 12, True, "mixed"), (300, 5, True, "mixed")])
def test_the_evaluation_leaves_the_bits_of_a_plain_fit_and_loo_reads_only(n, d, ard, dtype):
    from pygpso_amd import _lib as L

    r = reference(n, d, ard, "Matern52", 1.0e-3)
    th = r["th"]
    Xs = synthetic_leaves(64, d, seed=2)
    a, b = _engine(dtype), _engine(dtype)
    _load(a, r)
    _load(b, r)
    a.fit_eval_loo(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    f_b, _ = b.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    state = lambda e: [np.asarray(v).tobytes() for v in (e.get_matrix(L.MAT_LINV), e.get_matrix(L.MAT_CHOL), e.get_vector(L.VEC_ALPHA),
                                                         e.get_matrix(L.MAT_KINV))]  # noqa: E731
    sa = state(a)
    assert sa == state(b)  # (GPSO_MAT_KINV too: the header says it is still K_y^-1)
    pa = [np.asarray(v).tobytes() for v in a.predict(Xs)]
    assert pa == [np.asarray(v).tobytes() for v in b.predict(Xs)]
    first = a.loo()
    second = a.loo()
    assert all(np.array_equal(x, y) for x, y in zip(first[:3], second[:3])) and first[3] == second[3]
    assert state(a) == sa and [np.asarray(v).tobytes() for v in a.predict(Xs)] == pa
    # the same call gives the same bits
    again = _engine(dtype)
    _load(again, r)
    one = a.fit_eval_loo(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    two = again.fit_eval_loo(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    assert one[0] == two[0] and np.array_equal(one[1], two[1]) and one[2] == two[2] == f_b


def test_last_ms_covers_the_call():
    r = reference(300, 5, True, "Matern52", 1.0e-3)
    th = r["th"]
    eng = _engine()
    _load(eng, r)
    args = (th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    eng.fit_eval_loo(*args)  # (warm: buffers, code objects)

    def fastest(call):
        times = []
        for _ in range(3):
            call(*args)
            times.append(eng.last_ms(2))
        return min(times)

    plain, loo = fastest(eng.fit_eval), fastest(eng.fit_eval_loo)
    print(f"last_ms(2), N=300: fit + gradient {plain * 1e3:.0f} us, LOO evaluation {loo * 1e3:.0f} us")
    assert loo > plain > 0.0  # (the fit's launches and the LOO's behind them, between one pair of events)


# ---- 3. float contexts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,ard", FLOAT_SHAPES)
def test_loo_on_a_mixed_engine_holds_the_float64_tolerances(n, d, ard):
    r = reference(n, d, ard, "Matern52", 1.0e-3)
    th = r["th"]
    eng = _engine("mixed")
    _load(eng, r)
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    mean, var, lpd, loss = eng.loo()
    _hold(predictive_errors(r, mean, var, lpd), _tols("Matern52"), f"loo predictive mixed N={n}")
    assert abs(loss - r["loss"]) <= 1e-9 * abs(r["loss"])


@pytest.mark.parametrize("n,d,ard", FLOAT_SHAPES)
def test_loo_on_a_float32_engine_holds_its_measured_bounds(n, d, ard):
    r = reference(n, d, ard, "Matern52", 1.0e-3)
    th = r["th"]
    eng = _engine("float32")
    _load(eng, r)
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    mean, var, lpd, loss = eng.loo()
    e = predictive_errors(r, mean, var, lpd)
    print(f"loo predictive float32 N={n}: mean {e['mean']:.2e} var {e['var']:.2e} lpd {e['lpd']:.2e}")
    assert e["mean"] <= FLOAT32_LOO_BOUNDS[0] and e["var"] <= FLOAT32_LOO_BOUNDS[1]
    assert np.all(np.isfinite(lpd)) and np.isfinite(loss)


# ---- 4. append ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_s", [False, True])
def test_loo_after_an_append_covers_the_new_points(with_s):
    n, k, d = 200, 5, 3
    X, y = synthetic_problem(n + k, d, seed=23)
    th = gpr.Theta("Matern52", 0.25 * np.sqrt(d), 1.3, 1.0e-3, float(y[:n].mean()))
    s = ho.draw_s(n + k, th.variance, seed=24) if with_s else None
    eng = _engine()
    eng.set_data(X[:n], y[:n])
    if with_s:
        eng.set_noise_diag(s[:n])
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    _, in_place = eng.append(X[n:], y[n:], s[n:]) if with_s else eng.append(X[n:], y[n:])
    assert in_place
    mean, var, lpd, loss = eng.loo()
    assert mean.shape == (n + k,)
    m_ref, v_ref, l_ref, f_ref = lo.loo_closed(th, X, y, s)
    r = dict(y=y, mean=m_ref, var=v_ref, lpd=l_ref)
    _hold(predictive_errors(r, mean, var, lpd), _tols("Matern52"), f"loo after append (s={with_s})")
    assert abs(loss - f_ref) <= 1e-9 * abs(f_ref)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    from pygpso_amd import _lib as L
    from tests import sgpr_oracle as S

    r = reference(17, 3, True, "Matern52", 1.0e-3)
    th = r["th"]
    args = (th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    eng = _engine()
    with pytest.raises(L.GpsoHipError) as err:  # nothing at all
        eng.loo()
    assert err.value.code == L.E_STATE
    eng.set_data(r["X"], r["y"])
    with pytest.raises(L.GpsoHipError) as err:  # data, no fit
        eng.loo()
    assert err.value.code == L.E_STATE
    # an installed posterior carries no targets
    post = gpr.posterior(th, r["X"], r["y"])
    eng.set_posterior(r["X"], post.L, post.alpha, *args)
    with pytest.raises(L.GpsoHipError) as err:
        eng.loo()
    assert err.value.code == L.E_STATE
    # ... nor does an SGPR predictive
    sg = _engine()
    sg.set_data(r["X"], r["y"])
    u = S.initial_u(0.3 * np.sqrt(3), 1.1, 0.01, 0.05)
    sg.sgpr_set_inducing(r["X"][:8])
    sg.sgpr_posterior("Matern52", u, 1, True, 0.0)
    with pytest.raises(L.GpsoHipError) as err:
        sg.loo()
    assert err.value.code == L.E_STATE
    # an open asynchronous ticket
    eng.set_data(r["X"], r["y"])
    eng.fit_eval(*args, want_grad=False)
    ticket = eng.best_ucb_begin(synthetic_leaves(32, 3), gpr.VARSIGMA_DEFAULT)
    with pytest.raises(L.GpsoHipError) as err:
        eng.loo()
    assert err.value.code == L.E_STATE
    eng.best_ucb_end(ticket)
    eng.loo()
    # N = 1
    one = _engine()
    one.set_data(r["X"][:1], r["y"][:1])
    one.fit_eval(*args, want_grad=False)
    with pytest.raises(ValueError):
        one.loo()
    with pytest.raises(ValueError):
        one.fit_eval_loo(*args)
    # the objective in float32
    f32 = _engine("float32")
    f32.set_data(r["X"], r["y"])
    with pytest.raises(ValueError, match="GPSO_F64 or GPSO_MIXED"):
        f32.fit_eval_loo(*args)
    # not positive definite, then a valid evaluation.  (Duplicated rows at noise +1e-6 still factorise in float64 -- the
    # duplicate's pivot is 2e-6 --; at noise -1e-6 that pivot is -2e-6: not positive definite for certain.)
    for fused in (1, 0):
        bad = _engine()
        _fused(bad, fused)
        Xd = np.vstack([r["X"], r["X"][:6]])
        yd = np.concatenate([r["y"], r["y"][:6]])
        bad.set_data(Xd, yd)
        with pytest.raises(np.linalg.LinAlgError):
            bad.fit_eval_loo(th.kernel, th.lengthscales, th.variance, -1.0e-6, th.mean_c)
        f, g, _ = bad.fit_eval_loo(th.kernel, th.lengthscales, th.variance, 1.0e-2, th.mean_c)
        th2 = gpr.Theta(th.kernel, th.lengthscales, th.variance, 1.0e-2, th.mean_c)
        f_ref, g_ref = lo.loo_loss_and_grad(th2, Xd, yd)
        assert abs(f - f_ref) <= 1e-9 * abs(f_ref) and np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref))) <= 1e-8


# ---- 6. the search ----------------------------------------------------------------------------------------------------------
def _surrogate(**kw):
    from pygpso_amd import GPRSurrogate
    from pygpso_amd import kernels as K

    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy(), **kw)
    coords, scores = lo.search_problem()
    surr.append(coords, scores)
    return surr, coords, scores


def _theta_of(model):
    name, ls, var, noise, c = model._theta()
    return gpr.Theta(name, ls, var, noise, c)


def test_a_surrogate_trained_on_the_loo_loss():
    surr, coords, scores = _surrogate(objective="loo")
    start = lo.loo_closed(gpr.Theta("Matern52", 0.25, 1.0, 1.0e-3, 0.0), coords, scores)[3]
    surr.gp_update()
    model = surr.gpflow_model
    res = surr.optimiser.last_result
    th = _theta_of(model)
    f_ref = lo.loo_closed(th, coords, scores)[3]
    print(f"LOO search: {start:.6f} -> {res.fun:.6f} in {res.nfev} evaluations (oracle at the result: {f_ref:.6f})")
    assert res.fun < start
    assert abs(res.fun - f_ref) <= 1e-9 * abs(f_ref)
    assert abs(model.training_loss() - res.fun) <= 1e-12 * abs(res.fun)
    assert abs(model.log_marginal_likelihood() + gpr.posterior(th, coords, scores).nlml) <= 1e-9 * abs(model.log_marginal_likelihood())
    diag = surr.loo_diagnostics()
    mean, var, lpd, _ = model.engine.loo()
    assert np.array_equal(diag["mean"], mean) and np.array_equal(diag["var"], var) and np.array_equal(diag["lpd"], lpd)
    assert np.array_equal(diag["coords"], coords) and np.array_equal(diag["score"], scores)
    assert np.array_equal(diag["z"], (scores - mean) / np.sqrt(var))


def test_multistart_under_the_loo_objective():
    from pygpso_amd import kernels as K

    surr, coords, scores = _surrogate(objective="loo")
    surr.optimiser = K.Scipy(restarts=3, seed=2)
    surr.gp_update()
    res = surr.optimiser.last_result
    assert len(res.restarts) == 3
    f_ref = lo.loo_closed(_theta_of(surr.gpflow_model), coords, scores)[3]
    assert abs(res.fun - f_ref) <= 1e-9 * abs(f_ref)


def test_the_default_objective_gives_the_recorded_theta_bit_for_bit():
    """The bits in tests/golden were recorded by running this surrogate on the commit before the objective keyword existed."""
    surr, _, _ = _surrogate()
    surr.gp_update()
    th = _theta_of(surr.gpflow_model)
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = [float(v).hex() for v in np.concatenate([th.lengthscales, [th.variance, th.noise, th.mean_c]])]
    assert got == want["theta_hex"], (got, want)
    assert surr.gpflow_model.num_loss_evals == want["loss_evaluations"]
