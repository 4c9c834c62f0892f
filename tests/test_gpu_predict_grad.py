"""
GPU tests of ``gpso_predict_grad`` (mean, variance and their gradients in the test points) through the
C-ABI and of ``GPSurrogate.polish`` on top of it, against the float64 oracle of tests/predict_grad_oracle.py.

Stated tolerances (the project's own for float64 stages, as tests/test_gpu_loo.py states them; they hold on float64 AND mixed
engines, because the call reads the dense double factor on both)
  smooth kernels .. mean 1e-8 max|y|, var 1e-8 of the kernel variance, gradients 1e-8 by max(1, max|g|) per case
  Matern-1/2 ...... that file's 1e-5 where it takes ten times: 1e-4 on all three (the sqrt at r = 0 amplifies the rounding
                    of r^2, which the oracle's Gram (GEMM form) and the device's form differently)
  installed forms . mean and var against gpso_predict on the same float64 context 1e-9 (by max(1, |.|)); gradients against
                    central differences of gpso_predict itself, h = 1e-6: "the differences' own 1e-6" by max(1, max|g|)
Shapes, the smallest that reach every path: N = 2 one row; 17 a partial 16-tile; 64, 128 one row block; 129 two row blocks
of pg_apply and three column blocks of pg_grad, with padding; 300 several of each; D = 1, 3, 12, 26 (D_pad = 28 > 24);
M = 1, 16, 17, 300 (a partial 64-point tile, several tiles) and 1027 = the chunk + 3 at N = 129.
The achieved maxima are recorded in profiles/predict_grad_parity.json by tools/predict_grad_errors.py.
"""
import filecmp
import os
import shutil

import numpy as np
import pytest

from oracle import gpr
from tests import hetero_oracle as ho
from tests import predict_grad_oracle as po
from tests.helpers import synthetic_problem

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TMP = os.path.join(HERE, "_tmp_gpu_predict_grad")
KERNELS = ("Matern52", "Matern32", "Matern12", "SquaredExponential")
SHAPES = [(2, 1), (17, 3), (64, 12), (128, 6), (129, 3), (300, 5), (40, 26)]
NOISES = (1.0e-3, 1.0e-1)
MS = (1, 16, 17, 300)
CHUNK = 1024  # kPredictGradChunk


def _engine(dtype="float64", **kw):
    from pygpso_amd import HipGPEngine

    return HipGPEngine(dtype, **kw)


def points_at(m, d, seed=5):
    return np.random.default_rng(seed).uniform(-0.2, 1.2, size=(m, d))


_ref_cache = {}


def reference(n, d, ard, kernel, noise):
    """Problem, theta, s (every other case), the oracle's posterior and its answer at max(MS) test points; computed once per
    case and shared (never modified)."""
    key = (n, d, ard, kernel, noise)
    if key not in _ref_cache:
        X, y = synthetic_problem(n, d, seed=17 + n)
        ls = 0.25 * np.sqrt(d) * (np.linspace(0.8, 1.3, d) if ard else np.ones(1))
        th = gpr.Theta(kernel, ls, 1.3, noise, float(y.mean()))
        with_s = bool((SHAPES.index((n, d)) + KERNELS.index(kernel) + NOISES.index(noise) + int(ard)) % 2)
        s = ho.draw_s(n, th.variance, seed=n + d) if with_s else None
        post = ho.posterior(th, X, y, np.zeros(n) if s is None else s)
        Xs = points_at(max(MS), d)
        _ref_cache[key] = dict(X=X, y=y, th=th, s=s, post=post, Xs=Xs, out=po.gpr_predict_grad(post, Xs))
    return _ref_cache[key]


def fitted(r, dtype="float64"):
    eng = _engine(dtype)
    eng.set_data(r["X"], r["y"])
    if r["s"] is not None:
        eng.set_noise_diag(r["s"])
    th = r["th"]
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    return eng


def errors(got, want, y, variance):
    mean, var, dmean, dvar = got
    return dict(mean=float(np.max(np.abs(mean - want[0])) / np.max(np.abs(y))),
                var=float(np.max(np.abs(var - want[1])) / variance),
                dmean=float(np.max(np.abs(dmean - want[2])) / max(1.0, np.max(np.abs(want[2])))),
                dvar=float(np.max(np.abs(dvar - want[3])) / max(1.0, np.max(np.abs(want[3])))))


def tolerances(kernel):
    t = 1.0e-5 if kernel == "Matern12" else 1.0e-9
    return dict(mean=10 * t, var=10 * t, dmean=10 * t, dvar=10 * t)


def _hold(errs, tols, what):
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= tols[k], (what, k, v, tols[k])


# ---- 1. parity with the oracle on float64 and mixed engines ----------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_parity_with_the_oracle(n, d, kernel):
    tols = tolerances(kernel)
    for ard in (False, True):
        for noise in NOISES:
            r = reference(n, d, ard, kernel, noise)
            for dtype in ("float64", "mixed"):
                eng = fitted(r, dtype)
                for m in MS:
                    got = eng.predict_grad(r["Xs"][:m])
                    assert got[0].shape == (m,) and got[1].shape == (m,) and got[2].shape == (m, d) and got[3].shape == (m, d)
                    want = tuple(a[:m] for a in r["out"])
                    what = f"N={n} D={d} {kernel} ard={ard} noise {noise:g} s={'yes' if r['s'] is not None else 'no'} {dtype} M={m}"
                    _hold(errors(got, want, r["y"], r["th"].variance), tols, "predict_grad " + what)
                eng.close()


def test_more_test_points_than_one_chunk():
    """M = chunk + 3 at N = 129: a second pass over the workspace whose last 64-point tile holds three live points."""
    r = reference(129, 3, True, "Matern52", 1.0e-3)
    Xs = points_at(CHUNK + 3, 3, seed=8)
    want = po.gpr_predict_grad(r["post"], Xs)
    eng = fitted(r)
    got = eng.predict_grad(Xs)
    _hold(errors(got, want, r["y"], r["th"].variance), tolerances("Matern52"), f"predict_grad N=129 M={CHUNK + 3}")
    tail = eng.predict_grad(Xs[CHUNK:])
    for a, b in zip(got, tail):
        assert np.array_equal(a[CHUNK:], b)


def test_coincident_test_points_are_finite():
    """Test points ON training rows: every output finite for the four kernels (the pair itself contributes zero to the
    gradients), and the oracle's answer within the tolerances."""
    for kernel in KERNELS:
        r = reference(64, 12, True, kernel, 1.0e-3)
        Xs = np.vstack([r["X"][:20], r["Xs"][:5]])
        want = po.gpr_predict_grad(r["post"], Xs)
        got = fitted(r).predict_grad(Xs)
        assert all(np.all(np.isfinite(a)) for a in got)
        _hold(errors(got, want, r["y"], r["th"].variance), tolerances(kernel), f"predict_grad on training rows {kernel}")


# ---- 2. every kind of posterior --------------------------------------------------------------------------------------------
def _agrees_with_predict(eng, Xs, what):
    """mean and var against gpso_predict on the same (float64) context, gradients against its central differences."""
    mean, var, dmean, dvar = eng.predict_grad(Xs)
    m0, v0 = eng.predict(Xs)
    fm, fv = po.central_differences(lambda Z: eng.predict(Z), Xs, h=1.0e-6)
    e = dict(mean=float(np.max(np.abs(mean - m0) / np.maximum(1.0, np.abs(m0)))),
             var=float(np.max(np.abs(var - v0) / np.maximum(1.0, np.abs(v0)))),
             dmean=float(np.max(np.abs(dmean - fm)) / max(1.0, np.max(np.abs(dmean)))),
             dvar=float(np.max(np.abs(dvar - fv)) / max(1.0, np.max(np.abs(dvar)))))
    _hold(e, dict(mean=1e-9, var=1e-9, dmean=1e-6, dvar=1e-6), what)


def test_after_an_append():
    """k = 3 points appended in place to N = 130: against the oracle's from-scratch posterior of the 133."""
    X, y = synthetic_problem(133, 4, seed=2)
    th = gpr.Theta("Matern52", 0.5 * np.linspace(0.8, 1.3, 4), 1.3, 1.0e-3, float(y.mean()))
    eng = _engine()
    eng.set_data(X[:130], y[:130])
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    _, in_place = eng.append(X[130:], y[130:])
    assert in_place
    Xs = points_at(40, 4)
    want = po.gpr_predict_grad(gpr.posterior(th, X, y), Xs)
    _hold(errors(eng.predict_grad(Xs), want, y, th.variance), tolerances("Matern52"), "predict_grad after gpso_append")
    _agrees_with_predict(eng, Xs, "appended posterior against gpso_predict")


def test_after_set_posterior():
    r = reference(129, 3, True, "Matern32", 1.0e-1)
    th, post = r["th"], r["post"]
    eng = _engine()
    eng.set_posterior(r["X"], post.L, post.alpha, th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    Xs = r["Xs"][:40]
    _hold(errors(eng.predict_grad(Xs), tuple(a[:40] for a in r["out"]), r["y"], th.variance), tolerances("Matern32"),
          "predict_grad after gpso_set_posterior")
    _agrees_with_predict(eng, Xs, "installed posterior against gpso_predict")


def test_after_a_vgp_posterior():
    from tests import vgp_oracle as V

    X, y = synthetic_problem(60, 3, seed=4)
    u = V.initial_u(0.3 * np.sqrt(3), 1.1, 0.01, 0.05)
    eng = _engine()
    eng.set_data(X, y)
    eng.vgp_set_q()
    eng.vgp_natgrad("Matern52", u, 1, True, 0.0, 0.5)  # (half a step: q is neither the prior nor the exact posterior)
    eng.vgp_posterior("Matern52", u, 1, True, 0.0)
    _agrees_with_predict(eng, points_at(40, 3), "VGP posterior against gpso_predict")


def _sparse_engine(lik):
    from tests import sgpr_oracle as S

    X, y = synthetic_problem(60, 3, seed=6)
    Z = S.choose_inducing("Matern52", X, 0.3 * np.sqrt(3), 1.1, 20)
    eng = _engine()
    eng.set_data(X, y)
    if lik is not None:
        eng.vgp_set_likelihood(*lik)
    eng.sgpr_set_inducing(Z)
    return eng


def test_after_an_sgpr_posterior():
    from tests import sgpr_oracle as S

    eng = _sparse_engine(None)
    u = S.initial_u(0.3 * np.sqrt(3), 1.1, 0.02, 0.15)
    eng.sgpr_bound_u("Matern52", u, 1, True, 0.0, want_grad=False)
    eng.sgpr_posterior("Matern52", u, 1, True, 0.0)
    assert eng.n == 20
    _agrees_with_predict(eng, points_at(40, 3), "SGPR posterior (M = 20, N = 60) against gpso_predict")


def test_after_an_svgp_posterior():
    from tests import svgp_oracle as O
    from tests import vgp_studentt_oracle as T

    lik = ("StudentT", 4.0)
    eng = _sparse_engine((lik[0], lik[1], T.N_GH))
    u = O.initial_u(0.3 * np.sqrt(3), 1.1, 0.3, lik, c=0.05)
    eng.svgp_init_q("Matern52", u, 1, True, 0.0, 0.3 ** 2 * 2.0)
    eng.svgp_natgrad("Matern52", u, 1, True, 0.0, 0.5)
    eng.svgp_posterior("Matern52", u, 1, True, 0.0)
    _agrees_with_predict(eng, points_at(40, 3), "SVGP posterior (Student-t) against gpso_predict")


# ---- 3. invariance and purity ----------------------------------------------------------------------------------------------
def test_same_bits_again_and_alone_and_nothing_else_moves():
    r = reference(300, 5, True, "Matern52", 1.0e-3)
    eng = fitted(r)
    Xs = r["Xs"]
    h0, p0 = eng.posterior_hash(), eng.predict(Xs)
    a = eng.predict_grad(Xs)
    b = eng.predict_grad(Xs)
    few = eng.predict_grad(Xs[:17])
    for x, y_, z in zip(a, b, few):
        assert np.array_equal(x, y_)
        assert np.array_equal(x[:17], z)
    assert eng.posterior_hash() == h0
    p1 = eng.predict(Xs)
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])


def test_a_smaller_problem_after_a_larger_one_gives_a_fresh_contexts_bits():
    """120 points, then 40 on the same context (both padded to 128): the larger problem's rows sit in the padding of the
    factor, alpha and the scaled inputs; nothing may read them."""
    X, y = synthetic_problem(120, 5, seed=3)
    th = ("Matern52", [0.6], 1.3, 1.0e-3, float(y.mean()))
    Xs = points_at(70, 5)
    used = _engine()
    for n in (120, 40):
        used.set_data(X[:n], y[:n])
        used.fit_eval(*th, want_grad=False)
        got = used.predict_grad(Xs)
    fresh = _engine()
    fresh.set_data(X[:40], y[:40])
    fresh.fit_eval(*th, want_grad=False)
    for a, b in zip(got, fresh.predict_grad(Xs)):
        assert np.array_equal(a, b)


def test_device_float32_points_and_device_outputs_equal_the_host_path():
    import torch

    r = reference(129, 3, True, "SquaredExponential", 1.0e-3)
    eng = fitted(r)
    xs32 = r["Xs"][:100].astype(np.float32)
    host = eng.predict_grad(xs32)
    dev = torch.device("cuda", eng.device)
    xt = torch.from_numpy(xs32).to(dev)
    out = (torch.empty(100, dtype=torch.float64, device=dev), torch.empty(100, dtype=torch.float64, device=dev),
           torch.empty(100, 3, dtype=torch.float64, device=dev), torch.empty(100, 3, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    eng.predict_grad(xt, out=out)
    for a, b in zip(host, out):
        assert np.array_equal(a, b.cpu().numpy())
    # an output that is not wanted may be None (the C-ABI's nullable outputs): the others are the same bits
    dvar_only = torch.empty(100, 3, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.predict_grad(xt, out=(None, None, None, dvar_only))
    assert np.array_equal(host[3], dvar_only.cpu().numpy())
    assert np.array_equal(host[0], eng.predict_grad(xs32.astype(np.float64))[0])  # (the same values as float64)


def test_timing_covers_the_call():
    eng = fitted(reference(129, 3, True, "Matern52", 1.0e-3))
    eng.set_timing(True)
    eng.predict(points_at(7, 3))
    eng.predict_grad(points_at(300, 3))
    assert eng.last_ms(1) > 0.0
    assert eng.last_count(0) == 300 and eng.last_count(1) == 300  # (the counts describe the same call as the time)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------
def _code(eng, Xs):
    """The status gpso_predict_grad itself returns for host points and host outputs (the wrapper turns it into exceptions)."""
    import ctypes as C

    from pygpso_amd import _lib as L

    xs = np.ascontiguousarray(Xs, dtype=np.float64)
    m, d = xs.shape
    out = [np.empty(m), np.empty(m), np.empty((m, d)), np.empty((m, d))]
    return eng._lib.gpso_predict_grad(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, m,
                                      *[C.c_void_p(a.ctypes.data) for a in out], L.MEM_HOST)


def test_refusals_and_the_context_works_afterwards():
    import ctypes as C

    from pygpso_amd import _lib as L
    from tests.test_gpu_distributed import _handoff

    r = reference(129, 3, True, "Matern52", 1.0e-3)
    Xs = r["Xs"][:20]
    # a float32 context
    e32 = fitted(r, "float32")
    assert _code(e32, Xs) == L.E_ARG
    e32.predict(Xs)
    # no posterior
    eng = _engine()
    eng.set_data(r["X"], r["y"])
    assert _code(eng, Xs) == L.E_STATE
    th = r["th"]
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    want = eng.predict_grad(Xs)
    # an open best-UCB ticket
    ticket = eng.best_ucb_begin(r["Xs"], gpr.VARSIGMA_DEFAULT)
    assert _code(eng, Xs) == L.E_STATE
    eng.best_ucb_end(ticket)
    # m = 0, and all four outputs NULL
    assert _code(eng, np.empty((0, 3))) == L.E_ARG
    xs = np.ascontiguousarray(Xs)
    rc = eng._lib.gpso_predict_grad(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, 20, None, None, None, None, L.MEM_HOST)
    assert rc == L.E_ARG
    # ... any one output is enough
    only = np.empty((20, 3))
    rc = eng._lib.gpso_predict_grad(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, 20, None, None, None,
                                    C.c_void_p(only.ctypes.data), L.MEM_HOST)
    assert rc == L.OK and np.array_equal(only, want[3])
    for a, b in zip(want, eng.predict_grad(Xs)):
        assert np.array_equal(a, b)
    # an adopted posterior (the hand-off replayed with plain copies)
    dst = _engine()
    _handoff(eng, dst)
    assert _code(dst, Xs) == L.E_STATE
    m0, v0 = eng.predict(Xs)
    m1, v1 = dst.predict(Xs)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


def test_predict_f_grad_takes_the_familys_predictive_noise_off_the_variance():
    """``predict_f_grad`` = ``predict_y_grad`` with ``predictive_noise()`` off var and the same gradients: the exact GP
    (the likelihood variance) and a Student-t VGP (scale^2 df / (df - 2)); its var agrees with ``predict_f``'s."""
    from pygpso_amd import kernels as K
    from pygpso_amd.model import HipGPR
    from pygpso_amd.vgp import HipVGP

    X, y = synthetic_problem(40, 3, seed=4)
    Xs = points_at(25, 3)
    kern = lambda: K.Matern52(lengthscales=0.5, variance=1.1)
    gpr_model = HipGPR((X, y[:, None]), kern(), K.Constant(0.05), noise_variance=0.02)
    vgp_model = HipVGP((X, y[:, None]), kern(), K.Constant(0.05), likelihood=K.StudentT(0.3, 4.0))
    for model, noise in ((gpr_model, 0.02), (vgp_model, 0.3 ** 2 * 4.0 / 2.0)):
        assert abs(model.predictive_noise() - noise) <= 1e-15
        my, vy, dmy, dvy = model.predict_y_grad(Xs)
        mf, vf, dmf, dvf = model.predict_f_grad(Xs)
        assert my.shape == (25,) and vy.shape == (25,) and dmy.shape == (25, 3) and dvy.shape == (25, 3)
        assert np.array_equal(mf, my) and np.array_equal(dmf, dmy) and np.array_equal(dvf, dvy)
        assert np.array_equal(vf, vy - model.predictive_noise())
        mean_f, var_f = model.predict_f(Xs)
        assert np.max(np.abs(np.asarray(var_f)[:, 0] - vf)) <= 1e-9 and np.max(np.abs(np.asarray(mean_f)[:, 0] - mf)) <= 1e-9


# ---- 5. polish ---------------------------------------------------------------------------------------------------------------
def _check_polish(surr, oracle_grad, starts, box):
    weight = surr.gp_varsigma
    m0, v0, _, _ = surr.gp_predict_grad(starts)
    stored = list(surr.points)
    os.makedirs(TMP, exist_ok=True)
    before, after = os.path.join(TMP, "before"), os.path.join(TMP, "after")
    surr.save(before)
    coords, mean, var, value, results = surr.polish(starts, objective="ucb", box=box)
    surr.save(after)
    assert coords.shape == starts.shape and len(results) == starts.shape[0]
    assert np.all(value >= m0 + weight * v0)
    assert np.all(coords >= box[:, :, 0]) and np.all(coords <= box[:, :, 1])
    _, _, dmean, dvar = oracle_grad(coords)
    for x, g, b in zip(coords, dmean + weight * dvar, box):
        pg = po.projected_gradient(x, g, b[:, 0], b[:, 1])
        print(f"polish: x = {x}, projected gradient (oracle) {pg:.2e}")
        assert pg <= 1.0e-5
    assert list(surr.points) == stored
    cmp = filecmp.dircmp(before, after)
    assert not cmp.left_only and not cmp.right_only and not cmp.diff_files and cmp.common_files
    shutil.rmtree(TMP, ignore_errors=True)
    return value


def test_polish_through_the_gpr_surrogate():
    from pygpso_amd import GPRSurrogate
    from pygpso_amd import kernels as K

    coords, scores, starts, box = po.polish_problem()
    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy())
    surr.append(coords, scores)
    surr.gp_update()
    name, ls, var, noise, c = surr.gpflow_model._theta()
    post = gpr.posterior(gpr.Theta(name, ls, var, noise, c), coords, scores)
    _check_polish(surr, lambda x: po.gpr_predict_grad(post, x), starts, box)
    # the mean as the objective, in the unit cube: the values do not fall either
    m0 = surr.gp_predict_grad(starts)[0]
    xm, mean, _, value, _ = surr.polish(starts, objective="mean")
    assert np.array_equal(mean, value) and np.all(value >= m0) and np.all(xm >= 0.0) and np.all(xm <= 1.0)


def test_polish_through_the_sgpr_surrogate():
    from pygpso_amd import SGPRSurrogate, _lib
    from pygpso_amd import kernels as K

    coords, scores, starts, box = po.polish_problem()
    surr = SGPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), num_inducing=12)
    surr.append(coords, scores)
    surr.gp_update()
    model = surr.gpflow_model
    surr.gp_predict_grad(starts)  # (installs the predictive over Z: the getters below return its form)
    name, ls, var, noise, c = model._theta()
    C_, beta, Z = model.engine.get_matrix(_lib.MAT_LINV), model.engine.get_vector(_lib.VEC_ALPHA), model.inducing_points
    th = gpr.Theta(name, ls, var, noise, c)
    _check_polish(surr, lambda x: po.predictive_grad(C_, beta, Z, th, x), starts, box)
