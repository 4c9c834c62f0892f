"""
CPU tests of the predictive's input gradients: the float64 oracle of tests/predict_grad_oracle.py
against central differences of ``oracle.gpr.predict_y``, the bounded lockstep search behind ``GPSurrogate.polish`` with the
oracle in place of the engine, and the defaults of ``kernels._LbfgsbSearch``.  (That ``gpso_predict_grad`` is declared,
exported and bound is tests/test_cabi_cpu.py's: it reads the header.)
"""
import numpy as np
import pytest

from oracle import gpr
from tests import predict_grad_oracle as po
from tests.helpers import rotated_peaks, synthetic_problem

KERNELS = ("Matern52", "Matern32", "Matern12", "SquaredExponential")
SHAPES = [(2, 1), (17, 3), (64, 12), (128, 6), (129, 3), (300, 5), (40, 26)]
NOISES = (1.0e-3, 1.0e-1)


def _case(n, d, kernel, ard, noise, m=12):
    X, y = synthetic_problem(n, d, seed=17 + n)
    ls = 0.25 * np.sqrt(d) * (np.linspace(0.8, 1.3, d) if ard else np.ones(1))
    th = gpr.Theta(kernel, ls, 1.3, noise, float(y.mean()))
    return gpr.posterior(th, X, y), np.random.default_rng(5).uniform(-0.2, 1.2, size=(m, d))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_oracle_against_central_differences_of_predict_y(n, d, kernel):
    """h = 1e-6 and the differences' own 1e-6 by max(1, max|g|) (as tests/test_loo_cpu.py); mean and var to 1e-12."""
    for ard in (False, True):
        for noise in NOISES:
            post, Xs = _case(n, d, kernel, ard, noise)
            mean, var, dmean, dvar = po.gpr_predict_grad(post, Xs)
            m0, v0 = gpr.predict_y(post, Xs)
            assert np.max(np.abs(mean - m0)) <= 1e-12 * max(1.0, np.max(np.abs(m0)))
            assert np.max(np.abs(var - v0)) <= 1e-12 * max(1.0, np.max(np.abs(v0)))
            fm, fv = po.central_differences(lambda Z: gpr.predict_y(post, Z), Xs, h=1.0e-6)
            em = np.max(np.abs(dmean - fm)) / max(1.0, np.max(np.abs(dmean)))
            ev = np.max(np.abs(dvar - fv)) / max(1.0, np.max(np.abs(dvar)))
            print(f"N={n} D={d} {kernel} ard={ard} noise={noise:g}: dmean {em:.2e}, dvar {ev:.2e}")
            assert em <= 1e-6 and ev <= 1e-6


@pytest.mark.parametrize("kernel", KERNELS)
def test_coincident_rows_are_finite_and_contribute_zero(kernel):
    """A test point ON training row i: every output finite, and the gradients are those of the predictive with the pair's
    own derivative term left out."""
    post, _ = _case(17, 3, kernel, True, 1.0e-3)
    Xs = post.X[[4, 9]].copy()
    mean, var, dmean, dvar = po.gpr_predict_grad(post, Xs)
    assert all(np.all(np.isfinite(a)) for a in (mean, var, dmean, dvar))
    th = post.theta
    C = po.linv_of(post.L)
    for row, i in enumerate((4, 9)):
        diff = (Xs[row] - post.X) / th.lengthscales
        r2 = np.sum(diff * diff, axis=1)
        assert r2[i] == 0.0
        K = gpr.kernel_from_r2(th.kernel, r2, th.variance)
        dK = gpr._dk_dr2(th.kernel, r2, K, th.variance)
        keep = np.arange(post.X.shape[0]) != i
        w = C.T @ (C @ K)
        want_m = (2.0 * dK * post.alpha)[keep] @ diff[keep] / th.lengthscales
        want_v = (-4.0 * dK * w)[keep] @ diff[keep] / th.lengthscales
        np.testing.assert_allclose(dmean[row], want_m, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(dvar[row], want_v, rtol=1e-12, atol=1e-13)


def test_generic_predictive_is_the_exact_gps():
    post, Xs = _case(64, 12, "Matern52", True, 1.0e-3)
    a = po.gpr_predict_grad(post, Xs)
    b = po.predictive_grad(po.linv_of(post.L), post.alpha, post.X, post.theta, Xs)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- the lockstep polish with the oracle in place of the engine ------------------------------------------------------------
def _polish_setup():
    coords, scores, starts, box = po.polish_problem()
    post = gpr.posterior(gpr.Theta("Matern52", 0.25, 1.0, 1.0e-3, float(scores.mean())), coords, scores)
    weight = gpr.VARSIGMA_DEFAULT

    def value_and_grad(x):  # row by row: a row's bits must not depend on the BLAS blocking of the batch it came in
        out = [po.gpr_predict_grad(post, r[None, :]) for r in x]
        return (np.array([o[0][0] + weight * o[1][0] for o in out]), np.stack([o[2][0] + weight * o[3][0] for o in out]))

    return value_and_grad, starts, box


def test_polish_lockstep_takes_each_searchs_own_iterates_stays_in_the_box_and_converges():
    from pygpso_amd.gp_surrogate import polish_lockstep

    fun, starts, box = _polish_setup()
    opts = {"ftol": 10 * np.finfo(float).eps}
    three = polish_lockstep(fun, starts[:3], box[:3, :, 0], box[:3, :, 1], opts)
    for i, s in enumerate(three):
        alone = polish_lockstep(fun, starts[i:i + 1], box[i:i + 1, :, 0], box[i:i + 1, :, 1], opts)[0]
        assert np.array_equal(alone.x, s.x) and alone.fun == s.fun and alone.nfev == s.nfev and alone.nit == s.nit
        lo, up = box[i, :, 0], box[i, :, 1]
        assert np.all(s.x >= lo) and np.all(s.x <= up)
        value, grad = fun(s.x[None, :])
        assert value[0] >= fun(starts[i:i + 1])[0][0]
        pg = po.projected_gradient(s.x, grad[0], lo, up)
        print(f"search {i}: x = {s.x}, value {value[0]:.9f}, projected gradient {pg:.2e}, {s.nfev} evaluations")
        assert pg <= 1.0e-5  # (the search's pgtol)
        assert s.success


def test_polish_falls_back_to_scipy_minimize_without_the_private_routine(monkeypatch):
    """A SciPy whose ``setulb`` has another signature: the starts go one after another through
    ``scipy.optimize.minimize(method="L-BFGS-B", bounds=...)`` -- the same routine with the same inputs, so the end points
    of the lockstep searches, inside the boxes.  Unknown options are refused on this path too."""
    from pygpso_amd import gp_surrogate
    from pygpso_amd.gp_surrogate import polish_lockstep

    fun, starts, box = _polish_setup()
    opts = {"ftol": 10 * np.finfo(float).eps}
    direct = polish_lockstep(fun, starts, box[:, :, 0], box[:, :, 1], opts)
    calls = []

    def counting(x):
        calls.append(x.shape[0])
        return fun(x)

    monkeypatch.setattr(gp_surrogate._LbfgsbSearch, "routine", classmethod(lambda cls: None))
    fallback = polish_lockstep(counting, starts, box[:, :, 0], box[:, :, 1], opts)
    assert calls and set(calls) == {1}  # (one point per evaluation: no lockstep on this path)
    assert len(fallback) == len(direct)
    for a, b, bx in zip(fallback, direct, box):
        np.testing.assert_allclose(a.x, b.x, rtol=0, atol=1e-12)
        assert abs(a.fun - b.fun) <= 1e-12 * max(1.0, abs(b.fun)) and a.nfev == b.nfev and a.success
        assert np.all(a.x >= bx[:, 0]) and np.all(a.x <= bx[:, 1])
    with pytest.raises(ValueError):
        polish_lockstep(fun, starts[:1], box[:1, :, 0], box[:1, :, 1], {"maxcor": 5})


def test_polish_lockstep_refuses_an_unknown_option():
    from pygpso_amd.gp_surrogate import polish_lockstep

    fun, starts, box = _polish_setup()
    with pytest.raises(ValueError):
        polish_lockstep(fun, starts[:1], box[:1, :, 0], box[:1, :, 1], {"maxcor": 5})


# ---- _LbfgsbSearch ---------------------------------------------------------------------------------------------------------
def test_lbfgsb_search_without_bounds_hands_setulb_the_unbounded_arrays():
    """What the hyper-parameter searches construct: no bounds -> nbd = 0 and zero bound arrays, x0 as given."""
    from pygpso_amd.kernels import _LbfgsbSearch

    x0 = np.array([0.3, -1.2, 4.0])
    for s in (_LbfgsbSearch(None, x0), _LbfgsbSearch(None, x0, lower=None, upper=None)):
        n, m = 3, 10
        assert s.nbd.dtype == np.int32 and np.array_equal(s.nbd, np.zeros(n, np.int32))
        assert s.low_bnd.dtype == np.float64 and np.array_equal(s.low_bnd, np.zeros(n))
        assert s.upper_bnd.dtype == np.float64 and np.array_equal(s.upper_bnd, np.zeros(n))
        assert np.array_equal(s.x, x0) and s.x is not x0
        assert (s.m, s.maxls, s.maxfun, s.maxiter, s.pgtol) == (10, 20, 15000, 15000, 1e-5)
        assert s.factr == 2.2204460492503131e-09 / np.finfo(float).eps
        assert s.wa.shape == (2 * m * n + 5 * n + 11 * m * m + 8 * m,) and s.iwa.shape == (3 * n,)


def test_lbfgsb_search_bounds_codes_and_clipping():
    from pygpso_amd.kernels import _LbfgsbSearch

    s = _LbfgsbSearch(None, [0.5, -2.0, 9.0, 1.0], lower=[0.0, -1.0, -np.inf, -np.inf], upper=[1.0, np.inf, 3.0, np.inf])
    assert list(s.nbd) == [2, 1, 3, 0]
    assert list(s.low_bnd) == [0.0, -1.0, 0.0, 0.0] and list(s.upper_bnd) == [1.0, 0.0, 3.0, 0.0]
    assert list(s.x) == [0.5, -1.0, 3.0, 1.0]
    with pytest.raises(ValueError):
        _LbfgsbSearch(None, [0.0], lower=[1.0], upper=[0.0])


def test_bounded_search_agrees_with_scipy_minimize():
    """The bounded search run alone against scipy.optimize.minimize(method="L-BFGS-B", bounds=...): the same routine with
    the same inputs, so the same end point."""
    import scipy.optimize

    from pygpso_amd.kernels import _LbfgsbSearch

    setulb = _LbfgsbSearch.routine()
    assert setulb is not None, "SciPy's private L-BFGS-B routine has another signature: the lockstep searches cannot run"

    def fun(x):
        p = (-3.0 + 8.0 * x[0], -3.0 + 6.0 * x[1])
        h = 1e-6
        g = np.array([(rotated_peaks((p[0] + h, p[1])) - rotated_peaks((p[0] - h, p[1]))) / (2 * h) * 8.0,
                      (rotated_peaks((p[0], p[1] + h)) - rotated_peaks((p[0], p[1] - h))) / (2 * h) * 6.0])
        return -rotated_peaks(p), -g

    x0, lo, up = np.array([0.4, 0.6]), np.array([0.2, 0.3]), np.array([0.7, 0.9])
    s = _LbfgsbSearch(setulb, x0, lower=lo, upper=up)
    while True:
        x = s.advance()
        if x is None:
            break
        s.feed(*fun(x))
    ref = scipy.optimize.minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, up)))
    np.testing.assert_allclose(s.x, ref.x, rtol=0, atol=1e-12)
    assert s.nfev == ref.nfev
