"""
GPU parity tests: the HIP path, called through the C-ABI, against the CPU oracle on identical
seeded inputs.  Run on the GPU box with ``pytest -m gpu``.

Stated tolerances
  float64 ..... |d mean|, |d var| <= 1e-9 * scale; L, L^-1, alpha, NLML, gradient <= 1e-9 relative
                (Matern12: 1e-5 -- its sqrt at r = 0 amplifies the rounding noise of the GEMM-form r^2
                on the diagonal, |r^2| ~ 1e-16 -> r ~ 1e-8, differently in any two implementations)
  float32 ..... noise/variance ratio >= 1e-3: small shapes |d mean| <= 2e-3 * max|y|,
                |d var| <= 2e-4 * sigma^2; at the BASELINE sizes the per-family bounds of FLOAT_BOUNDS (<= 5x measured) and,
                for the f32-class split modes, within 4x of the native f32 kernel's error; NLML 2e-5 relative; winners
                compared by oracle-UCB value
"""
import numpy as np
import pytest

from oracle import gpr, tree
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

VS = gpr.VARSIGMA_DEFAULT


def _engine(dtype="float64"):
    from pygpso_amd import HipGPEngine

    return HipGPEngine(dtype)


def _problem(n, d, kernel="Matern52", noise=1e-3, ard=False, seed=0, variance=1.3):
    X, y = synthetic_problem(n, d, seed=seed)
    ls = 0.25 * np.sqrt(d) * (np.linspace(0.8, 1.3, d) if ard else np.ones(1))
    th = gpr.Theta(kernel, ls, variance, noise, float(y.mean()) if n > 1 else 0.1)
    return X, y, th


def _fit(eng, X, y, th, grad=True):
    eng.set_data(X, y)
    return eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=grad)


# float32 fit + float predict at the small shapes (N <= 2048, noise / variance = 1e-3): (|d mean| / max|y|, |d var| / sigma^2)
SMALL_FLOAT_BOUNDS = (6e-4, 2.1e-5)  # <= 5x the measured maxima (1.38e-4: SE, N = 512; 4.2e-6: N = 256) -- profiles/r04_float_errors.txt

# float32 engines: the winner is the oracle's arg-max, or a leaf whose ORACLE ucb lies within the rounding of a float
# prediction of it -- 2e-5 max(1, |ucb_max|): the mean carries ~1e-5-class float error (|d mean| measured 1e-5 ..
# 3e-4 max|y| across the float32 cases; a tie within that band cannot be told apart in float), the variance 3e-6 sigma^2
# x varsigma.  The same rule tests/test_gpu_precision.py:_check applies.
WINNER_GAP = 2e-5


def _winner_is_the_oracles(best, mean_ref, var_ref, gap=WINNER_GAP):
    from tests.helpers import winner_is_the_oracles

    winner_is_the_oracles(best[0][0], mean_ref + VS * var_ref, gap, "test_gpu_parity")


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["Matern52", "Matern32", "Matern12", "SquaredExponential"])
@pytest.mark.parametrize("n,d,ard", [(50, 2, False), (256, 6, False), (300, 5, True), (129, 3, True)])
def test_fit_stages_fp64(kernel, n, d, ard):
    from pygpso_amd import _lib as L

    tol = 1e-5 if kernel == "Matern12" else 1e-9
    X, y, th = _problem(n, d, kernel, ard=ard)
    post = gpr.posterior(th, X, y)
    f_ref, g_ref = gpr.nlml_and_grad(th, X, y)
    eng = _engine()
    f, g = _fit(eng, X, y, th)
    Linv_ref = np.linalg.inv(post.L)
    assert _rel(eng.get_matrix(L.MAT_CHOL), post.L) < tol
    assert _rel(eng.get_matrix(L.MAT_LINV), Linv_ref) < tol * 10
    assert _rel(eng.get_matrix(L.MAT_KINV), Linv_ref.T @ Linv_ref) < tol * 10
    assert _rel(eng.get_vector(L.VEC_ALPHA), post.alpha) < tol * 10
    assert abs(f - f_ref) <= tol * abs(f_ref)
    assert g.shape == g_ref.shape
    assert np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref))) < tol * 10


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_smaller_fit_after_a_larger_one_at_the_same_padded_size(dtype):
    """The single-level fit writes only the 64-row blocks that hold training rows: after a fit at N = 1000 a fit at
    N = 900 on the same context (both pad to 1024; its 64-row blocks end at 960) finds the old factor's rows in the padding
    block of L^-1.  Nothing
    may read them: NLML, gradient, L, L^-1 and K^-1 are the oracle's (round-4 advice)."""
    from pygpso_amd import _lib as L

    d = 4
    X, y, th = _problem(1000, d, variance=1.0)
    eng = _engine(dtype)
    _fit(eng, X, y, th)
    n = 900
    Xs_, ys_ = X[:n], y[:n]
    f, g = _fit(eng, Xs_, ys_, th)
    assert eng.padded_n == 1024
    post = gpr.posterior(th, Xs_, ys_)
    f_ref, g_ref = gpr.nlml_and_grad(th, Xs_, ys_)
    tol = 1e-9 if dtype == "float64" else 2e-5
    assert abs(f - f_ref) <= tol * abs(f_ref)
    assert np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref))) < (1e-8 if dtype == "float64" else 5e-3)
    if dtype == "float64":
        Linv_ref = np.linalg.inv(post.L)
        assert _rel(eng.get_matrix(L.MAT_CHOL), post.L) < 1e-9
        assert _rel(eng.get_matrix(L.MAT_LINV), Linv_ref) < 1e-8
        assert _rel(eng.get_matrix(L.MAT_KINV), Linv_ref.T @ Linv_ref) < 1e-8
    fresh = _engine(dtype)
    f2, g2 = _fit(fresh, Xs_, ys_, th)
    assert f == f2 and np.array_equal(g, g2)  # the bits of a context that never held the larger problem
    Xl = synthetic_leaves(700, d)
    assert all(np.array_equal(a, b) for a, b in zip(eng.predict(Xl), fresh.predict(Xl)))


def test_a_nan_leaf_stays_nan_in_every_predict_math():
    """A NaN coordinate gives NaN mean / var / ucb whatever runs the prediction, and -- np.argmax's rule, which the
    reference applies to GPflow's output -- wins the arg-max.  (Round 4: the fp16 contraction's clamp turned it into a
    far-away point with the prior's mean and variance; every OTHER path, on inspection in round 5, turned its r^2 into 0
    against every training point through max(r^2, 1e-36): finite garbage with a negative variance.  The leaves' norms
    carry the NaN to the finalize stage now.)"""
    n, d = 600, 5
    X, y, th = _problem(n, d, variance=1.0)
    Xl = synthetic_leaves(512, d)
    Xl[17, 2] = np.nan
    for dtype, math, contraction in [("float64", None, None), ("mixed", "native", None), ("mixed", "bf16x6", None),
                                     ("mixed", "f16x3", "f16"), ("mixed", "f16x3", "f32")]:
        eng = _engine(dtype) if math is None else __import__("pygpso_amd").HipGPEngine(dtype, predict_math=math)
        if contraction:
            eng.set_contraction(contraction)
        _fit(eng, X, y, th, grad=False)
        mean, var = eng.predict(Xl)
        assert np.isnan(mean[17]) and np.isnan(var[17]), (dtype, math, contraction, mean[17], var[17])
        assert np.all(np.isfinite(np.delete(mean, 17))) and np.all(np.isfinite(np.delete(var, 17)))
        idx, mu, vv, ucb = eng.best_ucb(Xl, VS)
        assert int(idx[0]) == 17 and np.isnan(ucb[0]), (dtype, math, contraction, idx, ucb)
        post = gpr.posterior(th, X, y)
        assert gpr.best_ucb(post, Xl)[0] == 17  # the oracle (numpy semantics) agrees


@pytest.mark.parametrize("n,d,m", [(1, 2, 7), (5, 2, 121), (64, 1, 1), (128, 4, 256), (129, 3, 257),
                                   (256, 6, 4096), (300, 12, 1000), (200, 40, 300), (77, 48, 33)])
def test_predict_fp64(n, d, m):
    X, y, th = _problem(n, d)
    post = gpr.posterior(th, X, y)
    Xs = synthetic_leaves(m, d)
    eng = _engine()
    _fit(eng, X, y, th, grad=False)
    mean, var = eng.predict(Xs)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    scale = max(1.0, float(np.max(np.abs(y))))
    assert np.max(np.abs(mean - mean_ref)) <= 1e-9 * scale
    assert np.max(np.abs(var - var_ref)) <= 1e-9 * th.variance
    idx, mu, vv, ucb = eng.best_ucb(Xs, VS)
    i_ref, mu_ref, var_r, ucb_ref = gpr.best_ucb(post, Xs)
    assert int(idx[0]) == i_ref
    assert abs(mu[0] - mu_ref) <= 1e-9 * scale and abs(vv[0] - var_r) <= 1e-9 and abs(ucb[0] - ucb_ref) <= 1e-9 * scale
    # the winner's ucb is exactly mean + varsigma * var of the returned values (two roundings)
    assert ucb[0] == mu[0] + VS * vv[0]


@pytest.mark.parametrize("n,d,m", [(256, 6, 4096), (300, 12, 1000), (2048, 12, 2048)])
def test_fit_and_predict_fp32(n, d, m):
    X, y, th = _problem(n, d, noise=1e-3, variance=1.0)
    post = gpr.posterior(th, X, y)
    f_ref, g_ref = gpr.nlml_and_grad(th, X, y)
    Xs = synthetic_leaves(m, d)
    eng = _engine("float32")
    f, g = _fit(eng, X, y, th)
    assert abs(f - f_ref) <= 2e-5 * abs(f_ref)
    assert np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref))) < 5e-3
    mean, var = eng.predict(Xs)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    em, ev = np.max(np.abs(mean - mean_ref)) / np.max(np.abs(y)), np.max(np.abs(var - var_ref)) / th.variance
    print(f"fp32 fit+predict N={n} D={d}: |d mean| {em:.2e} max|y|, |d var| {ev:.2e} sigma^2")
    assert em <= SMALL_FLOAT_BOUNDS[0] and ev <= SMALL_FLOAT_BOUNDS[1]
    _winner_is_the_oracles(eng.best_ucb(Xs, VS), mean_ref, var_ref)


# ---- split-bf16 predict math (float32 contexts): stated tolerances vs the float64 oracle ----------
#   bf16x6: the f32 tolerances (|d mean| <= 2e-3 max|y|, |d var| <= 2e-4 sigma^2); measured ~3e-6 sigma^2
#   f16x3:  (two fp16 pieces, three products, power-of-two scaling) the same: measured 1.3e-7 .. 2.8e-6 sigma^2, at or
#           below native f32 on every posterior of tools/split_math_accuracy.py (profiles/r03_split_math_accuracy.jsonl)
#   bf16x3: same bound on the mean (the mean never goes through the split), |d var| <= 2e-4 sigma^2;
#           measured ~2e-5 sigma^2
@pytest.mark.parametrize("mode", ["f16x3", "bf16x6", "bf16x3"])
@pytest.mark.parametrize("n,d,m,kernel", [(256, 6, 4096, "Matern52"), (512, 12, 3000, "SquaredExponential"),
                                          (2048, 12, 4096, "Matern52"), (1024, 40, 2048, "Matern32"),
                                          (300, 5, 1000, "Matern52")])  # last: N_pad % 256 != 0 -> native kernel
def test_split_bf16_predict_math(mode, n, d, m, kernel):
    from pygpso_amd import HipGPEngine

    X, y, th = _problem(n, d, kernel, noise=1e-3, variance=1.0)
    post = gpr.posterior(th, X, y)
    Xs = synthetic_leaves(m, d)
    eng = HipGPEngine("float32", predict_math=mode)
    _fit(eng, X, y, th, grad=False)
    mean, var = eng.predict(Xs)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    em, ev = np.max(np.abs(mean - mean_ref)) / np.max(np.abs(y)), np.max(np.abs(var - var_ref)) / th.variance
    print(f"split {mode} N={n} D={d} {kernel}: |d mean| {em:.2e} max|y|, |d var| {ev:.2e} sigma^2")
    assert em <= SMALL_FLOAT_BOUNDS[0] and ev <= (SMALL_FLOAT_BOUNDS[1] if mode != "bf16x3" else 2e-4)
    if mode in ("bf16x6", "f16x3"):  # f32-class: within 4x of what the native f32 kernel achieves on the same problem
        nat = HipGPEngine("float32")
        _fit(nat, X, y, th, grad=False)
        _, var_nat = nat.predict(Xs)
        assert np.max(np.abs(var - var_ref)) <= 4 * np.max(np.abs(var_nat - var_ref)) + 1e-6
    _winner_is_the_oracles(eng.best_ucb(Xs, VS), mean_ref, var_ref)
    # position independence and determinism hold in these modes too
    perm = np.random.default_rng(1).permutation(m)
    m2, v2 = eng.predict(Xs[perm])
    assert np.array_equal(mean[perm], m2) and np.array_equal(var[perm], v2)


@pytest.mark.parametrize("variance,yscale", [(1e-4, 1e-2), (3.7e3, 60.0), (2.0 ** 20, 1024.0)])
def test_fp16_split_scaling_over_kernel_variances(variance, yscale):
    """The fp16 split scales L^-1 and the generated tile by powers of two into fp16's range (max |L^-1| 2^sa and
    sigma^2 2^sb in [2^13, 2^14)): the accuracy relative to sigma^2 must not depend on the scale of the problem."""
    from pygpso_amd import HipGPEngine

    n, d, m = 512, 6, 2048
    X, y0 = synthetic_problem(n, d, seed=4)
    y = y0 * yscale
    th = gpr.Theta("Matern52", 0.25 * np.sqrt(d) * np.ones(1), variance, 1e-3 * variance, float(y.mean()))
    post = gpr.posterior(th, X, y)
    Xs = synthetic_leaves(m, d, seed=5)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    errs = {}
    for math in ("f16x3", "native"):
        eng = HipGPEngine("mixed", predict_math=math)
        _fit(eng, X, y, th, grad=False)
        mean, var = eng.predict(Xs)
        assert eng.precision_info()["predict_math"] == math
        errs[math] = (float(np.max(np.abs(var - var_ref)) / variance), float(np.max(np.abs(mean - mean_ref)) / np.max(np.abs(y))))
    assert errs["f16x3"][0] <= 1e-5 and errs["f16x3"][1] <= 1e-5, errs  # (measured: 3.9e-6 / 5.0e-6 at the smallest scale)
    assert errs["f16x3"][0] <= 4 * errs["native"][0] + 1e-6, errs


def test_auto_ladder_walks_down_and_starts_over():
    """GPSO_MATH_AUTO: fp16 split -> bf16x6 -> f32 MFMA kernel, one rung down per failed self-test of the posterior at
    hand, from the top again with the next posterior.  Tolerances nothing in float can meet walk the whole ladder (and
    end in the refusal); the next fit with ordinary tolerances is served by the first rung, with the bits a fresh
    engine produces."""
    from pygpso_amd import HipGPEngine
    from pygpso_amd._lib import GpsoPrecisionError

    X, y, th = _problem(512, 4)
    Xs = synthetic_leaves(700, 4)
    eng = HipGPEngine("mixed", tol_var=1e-13, tol_mean=1e-13)
    _fit(eng, X, y, th, grad=False)
    with pytest.raises(GpsoPrecisionError):
        eng.predict(Xs)
    eng.set_tolerances(1e-4, 1e-4)
    _fit(eng, X, y, th, grad=False)
    a = eng.predict(Xs)
    assert eng.precision_info()["predict_math"] == "f16x3"
    fresh = HipGPEngine("mixed")
    _fit(fresh, X, y, th, grad=False)
    b = fresh.predict(Xs)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    exp = HipGPEngine("mixed", predict_math="f16x3")
    _fit(exp, X, y, th, grad=False)
    c = exp.predict(Xs)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_predict_math_option_rules():
    from pygpso_amd import HipGPEngine, _lib as L

    with pytest.raises(ValueError):
        HipGPEngine("float64", predict_math="bf16x6")  # float32 contexts only
    X, y, th = _problem(512, 4)
    Xs = synthetic_leaves(700, 4)
    eng = HipGPEngine("float32")
    _fit(eng, X, y, th, grad=False)
    d = eng.predict(Xs)  # the default, GPSO_MATH_AUTO: its first rung here (padded N a multiple of 256, self-test passes)
    assert eng.precision_info()["predict_math"] == "f16x3"
    eng.set_predict_math("native")  # switching after the fit takes effect on the spot
    a = eng.predict(Xs)
    assert eng.precision_info()["predict_math"] == "native"
    eng.set_predict_math("f16x3")  # ... and repacks L^-1
    b = eng.predict(Xs)
    eng.set_predict_math("native")
    c = eng.predict(Xs)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert np.array_equal(d[0], b[0]) and np.array_equal(d[1], b[1])
    assert np.max(np.abs(a[1] - b[1])) < 1e-4 and not np.array_equal(a[1], b[1])
    eng.set_predict_math("auto")
    e = eng.predict(Xs)
    assert np.array_equal(d[1], e[1])
    # shapes the split kernel does not take (padded N not a multiple of 256) run the f32 MFMA kernel
    X2, y2, th2 = _problem(100, 4)
    eng2 = HipGPEngine("float32")
    _fit(eng2, X2, y2, th2, grad=False)
    eng2.predict(Xs)
    assert eng2.precision_info()["predict_math"] == "native"


def test_segments_ragged_empty_and_first_max_ties():
    X, y, th = _problem(100, 3)
    post = gpr.posterior(th, X, y)
    eng = _engine()
    _fit(eng, X, y, th, grad=False)
    base = synthetic_leaves(500, 3)
    # duplicate the overall winner later in the batch: np.argmax must keep the FIRST occurrence
    i_best = gpr.best_ucb(post, base)[0]
    Xs = np.vstack([base, base[i_best][None], base[:10]])
    seg = np.array([0, 0, 1, 257, 500, 501, 511, 511])  # empty, single, ragged ...
    idx, mu, vv, ucb = eng.best_ucb(Xs, VS, seg)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    ucb_ref = mean_ref + VS * var_ref
    for s in range(len(seg) - 1):
        a, b = seg[s], seg[s + 1]
        if a == b:
            assert idx[s] == -1 and np.isnan(ucb[s])
        else:
            assert idx[s] == int(np.argmax(ucb_ref[a:b])), s
            assert abs(ucb[s] - ucb_ref[a:b].max()) < 1e-9
    whole = eng.best_ucb(Xs, VS)
    assert int(whole[0][0]) == i_best  # not the duplicate at row 500
    assert ucb[5 - 1] == whole[3][0]  # duplicate row scores bit-identically to the original


def test_empty_batch_and_error_paths():
    from pygpso_amd import _lib as L

    eng = _engine()
    with pytest.raises(L.GpsoHipError) as e:
        eng.predict(np.zeros((3, 2)))
    assert e.value.code == L.E_STATE
    X, y, th = _problem(20, 2)
    _fit(eng, X, y, th, grad=False)
    mean, var = eng.predict(np.zeros((0, 2)))
    assert mean.shape == (0,) and var.shape == (0,)
    idx, mu, vv, ucb = eng.best_ucb(np.zeros((0, 2)), VS)
    assert idx[0] == -1 and np.isnan(mu[0])
    with pytest.raises(ValueError):
        eng.predict(np.zeros((3, 5)))  # wrong D
    with pytest.raises(ValueError):
        eng.best_ucb(np.zeros((4, 2)), VS, np.array([0, 3]))  # seg_off must end at M
    with pytest.raises(ValueError):
        eng.fit_eval("Matern52", [0.3, 0.3, 0.3], 1.0, 1e-3, 0.0)  # n_ls neither 1 nor D
    with pytest.raises(ValueError):
        eng.fit_eval("Matern52", [-0.3], 1.0, 1e-3, 0.0)
    with pytest.raises(KeyError):
        eng.fit_eval("NoSuchKernel", [0.3], 1.0, 1e-3, 0.0)


@pytest.mark.parametrize("dtype,n,d,noise", [("float64", 700, 5, 1e-3), ("float64", 1100, 3, 1e-3), ("float32", 900, 6, 1e-2),
                                             ("float32", 900, 6, 1e-3)])
def test_two_level_cholesky_path_matches_oracle(dtype, n, d, noise):
    """Sizes above 4096 factorise two-level (outer rank-256 SYRK + look-ahead column) and invert L by
    level doubling; GPSO_OPT_FIT_SINGLE_LEVEL_MAX = 0 forces that path at a size the oracle can check."""
    from pygpso_amd import _lib as L

    X, y, th = _problem(n, d, noise=noise)
    post = gpr.posterior(th, X, y)
    f_ref, g_ref = gpr.nlml_and_grad(th, X, y)
    eng = _engine(dtype)
    eng.set_fit_single_level_max(0)
    f, g = _fit(eng, X, y, th)
    Linv_ref = np.linalg.inv(post.L)
    # float: L to a few float ulps of its largest entry; L^-1 and K^-1 carry cond(L) = sqrt(cond(K_y)) x eps on top
    # (cond(K_y) ~ sigma^2 N / noise x clustering: 1e5 at noise 1e-2, 1e6 at 1e-3)
    tol = 1e-9 if dtype == "float64" else 2e-4
    tol_inv = tol * 10 * (1.0 if dtype == "float64" or noise >= 1e-2 else 4.0)
    assert _rel(eng.get_matrix(L.MAT_CHOL), post.L) < tol
    assert _rel(eng.get_matrix(L.MAT_LINV), Linv_ref) < tol_inv
    assert _rel(eng.get_matrix(L.MAT_KINV), Linv_ref.T @ Linv_ref) < tol_inv
    assert abs(f - f_ref) <= (tol if dtype == "float64" else 2e-5) * abs(f_ref)
    # gradient of a float fit: measured 7e-5 .. 4e-4 at N = 4096 .. 4600 (tools/grad_error_probe.py,
    # profiles/r03_grad_error.jsonl), LAPACK's float32 potrf / trtri / gemm on the host reach 7e-6 .. 5e-5 on the same
    # problems, eps x cond is 1e-2 .. 1e-1: rounding of a float factorisation, five times inside this bound
    assert np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref))) < (1e-8 if dtype == "float64" else 2e-3)
    # and the two paths agree with each other on predictions
    Xs = synthetic_leaves(300, d)
    m2, v2 = eng.predict(Xs)
    eng1 = _engine(dtype)
    _fit(eng1, X, y, th)
    m1, v1 = eng1.predict(Xs)
    ptol = 1e-9 if dtype == "float64" else 2e-3
    assert np.max(np.abs(m1 - m2)) < ptol * max(1.0, np.max(np.abs(y))) and np.max(np.abs(v1 - v2)) < ptol


@pytest.mark.parametrize("dtype,noise", [("float64", 1e-3), ("float32", 1e-2), ("float32", 1e-3)])
def test_fit_and_gradient_at_4600_points(dtype, noise):
    """N = 4600 is past the single-level limit and large enough for the 128x128-tile instantiations of
    the LDS-DMA GEMM (rank-256 SYRK, K^-1 = L^-T L^-1) in both element types: NLML, gradient and a few
    predictions against the float64 oracle."""
    n, d = 4600, 8
    X, y, th = _problem(n, d, noise=noise)
    f_ref, g_ref = gpr.nlml_and_grad(th, X, y)
    post = gpr.posterior(th, X, y)
    eng = _engine(dtype)
    f, g = _fit(eng, X, y, th)
    Xs = synthetic_leaves(500, d)
    mean, var = eng.predict(Xs)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    if dtype == "float64":
        assert abs(f - f_ref) <= 1e-9 * abs(f_ref)
        assert np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref))) < 1e-7
        assert np.max(np.abs(mean - mean_ref)) < 1e-8 and np.max(np.abs(var - var_ref)) < 1e-8
    else:
        assert abs(f - f_ref) <= 5e-5 * abs(f_ref)
        # measured 7e-5 (both noise levels; LAPACK in float32 on the host: 7e-6 .. 9e-6; eps x cond(K_y) = 1e-2 .. 4e-2):
        # profiles/r03_grad_error.jsonl
        assert np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref))) < 2e-3
        assert np.max(np.abs(mean - mean_ref)) < 3e-3 * np.max(np.abs(y))
        assert np.max(np.abs(var - var_ref)) < 3e-4 * th.variance


def test_not_positive_definite_raises_linalgerror():
    # the reference lets TF's Cholesky failure escape run(); here: LinAlgError naming the pivot
    X = np.array([[0.1, 0.2], [0.1, 0.2], [0.4, 0.4], [0.7, 0.1]])
    eng = _engine()
    eng.set_data(X, np.zeros(4))
    with pytest.raises(np.linalg.LinAlgError, match="pivot"):
        eng.fit_eval("SquaredExponential", [0.3], 1.0, -1.0e-3, 0.0)
    # and the context stays usable afterwards
    f, _ = eng.fit_eval("SquaredExponential", [0.3], 1.0, 1.0e-3, 0.0)
    assert np.isfinite(f)


def test_deterministic_bitwise():
    X, y, th = _problem(300, 6)
    Xs = synthetic_leaves(3000, 6)
    for dtype in ("float64", "float32"):
        eng = _engine(dtype)
        f1, g1 = _fit(eng, X, y, th)
        a = eng.predict(Xs)
        f2, g2 = _fit(eng, X, y, th)
        b = eng.predict(Xs)
        assert f1 == f2 and np.array_equal(g1, g2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        eng2 = _engine(dtype)  # a second context gives the same bits
        _fit(eng2, X, y, th)
        c = eng2.predict(Xs)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_leaf_order_does_not_change_a_leafs_result():
    X, y, th = _problem(200, 5)
    Xs = synthetic_leaves(1500, 5)
    perm = np.random.default_rng(5).permutation(1500)
    for dtype in ("float64", "float32"):
        eng = _engine(dtype)
        _fit(eng, X, y, th, grad=False)
        m1, v1 = eng.predict(Xs)
        m2, v2 = eng.predict(Xs[perm])
        assert np.array_equal(m1[perm], m2) and np.array_equal(v1[perm], v2)


def test_set_posterior_interop_matches_device_fit():
    X, y, th = _problem(150, 4)
    post = gpr.posterior(th, X, y)
    Xs = synthetic_leaves(700, 4)
    eng = _engine()
    eng.set_posterior(X, post.L, post.alpha, th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    mean, var = eng.predict(Xs)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    assert np.max(np.abs(mean - mean_ref)) < 1e-9 and np.max(np.abs(var - var_ref)) < 1e-9


def test_device_resident_leaves_and_outputs():
    import torch

    X, y, th = _problem(256, 6)
    Xs = synthetic_leaves(5000, 6)
    eng = _engine("float32")
    _fit(eng, X, y, th, grad=False)
    m_host, v_host = eng.predict(Xs.astype(np.float32))
    xs_dev = torch.from_numpy(Xs.astype(np.float32)).cuda()
    mean_t = torch.empty(5000, dtype=torch.float64, device="cuda")
    var_t = torch.empty(5000, dtype=torch.float64, device="cuda")
    eng.predict(xs_dev, out=(mean_t, var_t))
    assert np.array_equal(mean_t.cpu().numpy(), m_host) and np.array_equal(var_t.cpu().numpy(), v_host)
    a = eng.best_ucb(xs_dev, VS)
    b = eng.best_ucb(Xs.astype(np.float32), VS)
    assert all(np.array_equal(x, y_) for x, y_ in zip(a, b))
    # float64 leaves into a float32 context are converted on the device
    c = eng.best_ucb(torch.from_numpy(Xs).cuda(), VS)
    assert abs(c[3][0] - a[3][0]) < 1e-4
    # running on a caller-provided stream
    s = torch.cuda.Stream()
    eng.set_stream(s.cuda_stream)
    d = eng.best_ucb(xs_dev, VS)
    eng.set_stream(None)
    assert all(np.array_equal(x, y_) for x, y_ in zip(a, d))


# ---- ternary generator ---------------------------------------------------------------------------
@pytest.mark.parametrize("d,depth", [(1, 6), (2, 5), (3, 7), (6, 8), (12, 6), (40, 4)])
def test_grow_bit_identical(d, depth):
    rng = np.random.default_rng(d * 100 + depth)
    boxes = []
    for _ in range(3):
        b = [(0.0, 1.0)] * d
        for _ in range(int(rng.integers(0, 7))):
            b = tree.split_bounds(b)[int(rng.integers(3))]
        boxes.append(b)
    eng = _engine()
    got = eng.grow(np.array(boxes), depth)
    assert got.shape == (3, tree.grow_count(depth), d)
    for s, b in enumerate(boxes):
        assert np.array_equal(got[s], tree.grow(b, depth)), s


def test_best_ucb_grow_equals_scoring_host_grown_leaves():
    X, y, th = _problem(60, 2)
    post = gpr.posterior(th, X, y)
    eng = _engine()
    _fit(eng, X, y, th, grad=False)
    kids = tree.split_bounds([(0.0, 1.0), (0.0, 1.0)])
    boxes = np.array([kids[0], kids[2]])
    idx, mu, vv, ucb = eng.best_ucb_grow(boxes, 5, VS)
    for s, b in enumerate((kids[0], kids[2])):
        coords = tree.grow(b, 5)
        i_ref, mu_ref, var_ref, ucb_ref = gpr.best_ucb(post, coords)
        assert int(idx[s]) == i_ref  # first of the duplicated centre rows
        assert abs(ucb[s] - ucb_ref) < 1e-9
        one = eng.best_ucb(coords, VS)
        assert (int(one[0][0]), one[1][0], one[2][0], one[3][0]) == (int(idx[s]), mu[s], vv[s], ucb[s])


def test_best_ucb_grow_scores_each_distinct_centre_once():
    """A centre child's centre is its parent's (reference: gpso/param_space.py:186-200 emits both), so
    only 3^(depth-1) of the (3^depth - 1)/2 rows are distinct.  Boxes cut from the unit cube repeat bit
    for bit: exactly 1/3 of the rows is dropped, the reported index is still the reference's."""
    X, y, th = _problem(60, 2)
    eng = _engine()
    _fit(eng, X, y, th, grad=False)
    kids = tree.split_bounds([(0.0, 1.0), (0.0, 1.0)])
    boxes = np.array([kids[0], kids[2]])
    for depth, rows, uniq in ((1, 1, 1), (2, 4, 3), (5, 121, 81), (8, 3280, 2187)):
        idx, mu, vv, ucb = eng.best_ucb_grow(boxes, depth, VS)
        assert eng.last_count(1) == 2 * rows and eng.last_count(0) == 2 * uniq
        for s, b in enumerate((kids[0], kids[2])):
            one = eng.best_ucb(tree.grow(b, depth), VS)
            assert (int(one[0][0]), one[1][0], one[2][0], one[3][0]) == (int(idx[s]), mu[s], vv[s], ucb[s])


@pytest.mark.parametrize("d,depth,nbox", [(1, 6, 3), (2, 6, 5), (3, 7, 4), (5, 5, 7)])
def test_best_ucb_grow_on_arbitrary_boxes_keeps_near_duplicates(d, depth, nbox):
    """For arbitrary boxes a centre child's centre can differ from its parent's in the last bit: such a
    row is a different input and must still be scored (the appended tail of the compact list).  The
    result is bit-identical to scoring the host-grown list, box by box."""
    rng = np.random.default_rng(100 * d + depth)
    X, y, th = _problem(80, d)
    eng = _engine()
    _fit(eng, X, y, th, grad=False)
    lo = rng.uniform(0.0, 0.6, (nbox, d))
    boxes = np.stack([lo, lo + rng.uniform(0.05, 0.4, (nbox, d))], axis=2)
    idx, mu, vv, ucb = eng.best_ucb_grow(boxes, depth, VS)
    scored, asked = eng.last_count(0), eng.last_count(1)
    rows, uniq = tree.grow_count(depth), 3 ** (depth - 1)
    distinct = 0
    for s in range(nbox):
        coords = tree.grow([tuple(b) for b in boxes[s]], depth)
        distinct += len(np.unique(coords.view(np.dtype((np.void, 8 * d)))))
        one = eng.best_ucb(coords, VS)
        assert (int(one[0][0]), one[1][0], one[2][0], one[3][0]) == (int(idx[s]), mu[s], vv[s], ucb[s])
    assert asked == nbox * rows
    # every bit-distinct row is scored; rows equal to their PARENT are dropped (rows that merely coincide
    # with some other row are not looked for)
    assert distinct <= scored <= nbox * rows
    assert scored > nbox * uniq or distinct == nbox * uniq


def test_best_ucb_grow_edge_cases():
    """depth 0 (no rows: every box reports the empty-segment record), depth 1 (the box centre only) and many
    boxes in one call."""
    X, y, th = _problem(40, 3)
    eng = _engine()
    _fit(eng, X, y, th, grad=False)
    rng = np.random.default_rng(3)
    boxes = []
    for _ in range(37):
        b = [(0.0, 1.0)] * 3
        for _ in range(int(rng.integers(1, 6))):
            b = tree.split_bounds(b)[int(rng.integers(3))]
        boxes.append(b)
    boxes = np.array(boxes)
    idx, mu, vv, ucb = eng.best_ucb_grow(boxes, 0, VS)
    assert np.all(idx == -1) and np.all(np.isnan(ucb)) and eng.last_count(1) == 0
    idx, mu, vv, ucb = eng.best_ucb_grow(boxes, 1, VS)
    centres = np.array([[(lo + hi) / 2 for lo, hi in b] for b in boxes])
    m1, v1 = eng.predict(centres)
    assert np.all(idx == 0) and np.array_equal(mu, m1) and np.array_equal(vv, v1)
    idx, mu, vv, ucb = eng.best_ucb_grow(boxes, 4, VS)
    assert eng.last_count(0) == 37 * 27 and eng.last_count(1) == 37 * 40
    for s in (0, 11, 36):
        one = eng.best_ucb(tree.grow([tuple(r) for r in boxes[s]], 4), VS)
        assert (int(one[0][0]), one[1][0], one[2][0], one[3][0]) == (int(idx[s]), mu[s], vv[s], ucb[s])


def test_best_ucb_grow_in_several_chunks():
    """depth 13 x 2 boxes = 1.6 M reference rows (1.06 M distinct): more than one 1 Mi-leaf pass of the
    tile kernel, so the live count is split per chunk on the device."""
    X, y, th = _problem(64, 3)
    eng = _engine("float32")
    _fit(eng, X, y, th, grad=False)
    kids = tree.split_bounds([(0.0, 1.0)] * 3)
    boxes = np.array([kids[0], kids[2]])
    depth = 13
    idx, mu, vv, ucb = eng.best_ucb_grow(boxes, depth, VS)
    assert eng.last_count(1) == 2 * tree.grow_count(depth) and eng.last_count(0) == 2 * 3 ** (depth - 1)
    full = eng.grow(boxes, depth)
    for s in range(2):
        one = eng.best_ucb(full[s], VS)
        assert (int(one[0][0]), one[1][0], one[2][0], one[3][0]) == (int(idx[s]), mu[s], vv[s], ucb[s])


# ---- BASELINE.json sizes: oracle on a subsample + size-independent properties ----------------------
def _properties(eng, X, y, th, Xs, post, n_check, family="C3", native=None):
    """``family``: which row of FLOAT_BOUNDS the oracle comparison is held to; ``native``: an engine with the f32 MFMA
    kernel holding the same posterior -- a split-math engine must then also be within 4x of its error."""
    m = Xs.shape[0]
    mean, var = eng.predict(Xs)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    # 0 < predictive variance <= prior variance + noise
    assert var.min() > 0.0 and var.max() <= (th.variance + th.noise) * (1 + 1e-5)
    # oracle on a random subsample
    sub = np.random.default_rng(9).choice(m, n_check, replace=False)
    mean_ref, var_ref = gpr.predict_y(post, Xs[sub])
    bm, bv = FLOAT_BOUNDS[family]
    math = eng.precision_info()["predict_math"]
    em, ev = np.max(np.abs(mean[sub] - mean_ref)) / np.max(np.abs(y)), np.max(np.abs(var[sub] - var_ref)) / th.variance
    print(f"{family} {math}: |d mean| {em:.2e} ({em / bm:.2f} of the bound), |d var| {ev:.2e} ({ev / bv:.2f})")
    assert em <= bm
    assert ev <= (bv if math != "bf16x3" else 2e-4)
    if native is not None and math in ("f16x3", "bf16x6"):
        _, var_nat = native.predict(Xs[sub])
        assert _close_to_native(var[sub], var_nat, var_ref)
    # at the training inputs the posterior interpolates: |mean - y| small, latent variance ~ 0
    k = min(512, X.shape[0])
    mt, vt = eng.predict(X[:k])
    assert np.max(np.abs(mt - y[:k])) < 0.2 and np.all(vt < 4 * th.noise + 1e-3 * th.variance)
    # the global winner is the best of the per-segment winners
    seg = np.linspace(0, m, 9).astype(np.int64)
    idx, mu, vv, ucb = eng.best_ucb(Xs, VS, seg)
    whole = eng.best_ucb(Xs, VS)
    j = int(np.argmax(ucb))
    assert whole[3][0] == ucb[j] and int(whole[0][0]) == seg[j] + idx[j]
    full_ucb = mean + VS * var
    assert int(whole[0][0]) == int(np.argmax(full_ucb)) and whole[3][0] == full_ucb.max()


def test_more_than_one_chunk_of_leaves_and_many_segments():
    """> 2^20 leaves are processed in chunks inside one call; 500 ragged segments in one launch."""
    X, y, th = _problem(100, 2)
    post = gpr.posterior(th, X, y)
    eng = _engine()
    _fit(eng, X, y, th, grad=False)
    m = (1 << 20) + 12345
    Xs = synthetic_leaves(m, 2, seed=7)
    cuts = np.sort(np.random.default_rng(8).choice(np.arange(1, m), 499, replace=False))
    seg = np.concatenate([[0], cuts, [m]])
    idx, mu, vv, ucb = eng.best_ucb(Xs, VS, seg)
    mean, var = eng.predict(Xs)
    full = mean + VS * var
    for s in (0, 1, 250, 498, 499):  # spot-check segments, including the ones across the chunk seam
        a, b = seg[s], seg[s + 1]
        assert idx[s] == int(np.argmax(full[a:b])) and ucb[s] == full[a:b].max()
    k = int(np.searchsorted(seg, 1 << 20)) - 1  # the segment containing the chunk boundary
    assert idx[k] == int(np.argmax(full[seg[k]:seg[k + 1]]))
    sub = np.random.default_rng(9).choice(m, 4096, replace=False)
    mean_ref, var_ref = gpr.predict_y(post, Xs[sub])
    assert np.max(np.abs(mean[sub] - mean_ref)) < 1e-9 and np.max(np.abs(var[sub] - var_ref)) < 1e-9


def test_dimension_and_size_limits():
    eng = _engine()
    with pytest.raises(ValueError):
        eng.set_data(np.zeros((4, 49)), np.zeros(4))  # D > 48
    with pytest.raises(ValueError):
        eng.set_data(np.zeros((0, 3)), np.zeros(0))  # no training point
    X, y, th = _problem(33, 48)  # D = 48 is the maximum
    _fit(eng, X, y, th)
    assert eng.predict(synthetic_leaves(5, 48))[0].shape == (5,)


_c5_cache = {}


def _c5_reference(noise):
    """C5's training set and what the float64 oracle says about it -- ONE CPU factorisation at N = 16384 per noise
    level, shared by the tests that run C5 at size (the factor itself is not kept: 2 GB): NLML, and predict_y on a
    fixed 96-leaf sub-sample of the first 131 072 synthetic leaves (the leaves of a larger batch start with the same rows)."""
    if noise not in _c5_cache:
        n, d, m = 16384, 40, 131072
        X, y, th = _problem(n, d, variance=1.0, noise=noise)
        post = gpr.posterior(th, X, y)
        sub = np.sort(np.random.default_rng(5).choice(m, 96, replace=False))
        leaves = synthetic_leaves(m, d).astype(np.float32)
        mean_ref, var_ref = gpr.predict_y(post, leaves[sub].astype(np.float64))
        _c5_cache[noise] = dict(X=X, y=y, th=th, nlml=post.nlml, sub=sub, mean_ref=mean_ref, var_ref=var_ref)
    return _c5_cache[noise]


# float parity bounds at the BASELINE sizes: <= 5x what is measured (printed by the tests as measured / bound), per family
# (profiles/r04_float_errors.txt; worst over native / bf16x6 / f16x3, bf16x3's variance has its own 2e-4 = 5 x 4.2e-5):
#   C3 (N 2048, D 12):   |d mean| 3.6e-5 max|y|, |d var| 2.9e-6 sigma^2
#   C4 (N 8192, D 20):   7.3e-5, 4.9e-6 (share and full batch)
#   C5 (N 16384, D 40):  1.02e-4, 7.9e-6 (noise 1e-2 and 1e-3, share and full batch)
FLOAT_BOUNDS = {"C3": (1.8e-4, 1.3e-5), "C4": (3.3e-4, 2.4e-5), "C5": (4.5e-4, 3.9e-5)}


def _close_to_native(var, var_nat, var_ref):
    """The split modes' guard: f32-class means within 4x of what the f32 MFMA kernel achieves on the
    same posterior and leaves."""
    return np.max(np.abs(var - var_ref)) <= 4 * np.max(np.abs(var_nat - var_ref)) + 1e-6


@pytest.mark.parametrize("noise", [1e-2, 1e-3])  # 1e-3: SURVEY 8(d)'s and bench.py --workload c5's
def test_config_C5_one_gpu_share_at_size(noise):
    """Config C5 at its size: D = 40, N_train = 16384, ONE GPU's share of the 1 M leaves = 131 072, in
    float32 and in the split-bf16 modes (the variant the config's "bf16" names here: DESIGN.md 4.1b).
    Size-independent properties on all leaves + the float64 oracle (a CPU potrf at 16384) on a sub-sample."""
    from pygpso_amd import HipGPEngine

    n, d, m = 16384, 40, 131072
    ref = _c5_reference(noise)
    X, y, th, sub, mean_ref, var_ref = ref["X"], ref["y"], ref["th"], ref["sub"], ref["mean_ref"], ref["var_ref"]
    Xs = synthetic_leaves(m, d).astype(np.float32)
    ys = max(1.0, float(np.max(np.abs(y))))
    eng = HipGPEngine("float32")
    f, _ = _fit(eng, X, y, th, grad=False)
    assert abs(f - ref["nlml"]) <= 1e-4 * abs(ref["nlml"])
    results = {}
    bm, bv = FLOAT_BOUNDS["C5"]
    for math in ("native", "bf16x6", "f16x3", "bf16x3"):
        eng.set_predict_math(math)
        mean, var = eng.predict(Xs)
        assert np.all(np.isfinite(mean)) and var.min() > 0 and var.max() <= (th.variance + th.noise) * (1 + 1e-5)
        em, ev = np.max(np.abs(mean[sub] - mean_ref)) / ys, np.max(np.abs(var[sub] - var_ref)) / th.variance
        print(f"C5 noise {noise:g} {math}: |d mean| {em:.2e} ({em / bm:.2f} of the bound), |d var| {ev:.2e} ({ev / bv:.2f})")
        assert em <= bm, math
        assert ev <= (bv if math != "bf16x3" else 2e-4), math
        idx, mu, vv, ucb = eng.best_ucb(Xs, VS)
        full = mean + VS * var
        assert int(idx[0]) == int(np.argmax(full)) and ucb[0] == full.max()  # fused arg-max == numpy's
        results[math] = (mean, var)
    for math in ("bf16x6", "f16x3"):  # f32-class: within 4x of the native f32 kernel on the same leaves
        assert _close_to_native(results[math][1][sub], results["native"][1][sub], var_ref), math
    mt, vt = eng.predict(X[:512].astype(np.float32))
    assert np.max(np.abs(mt - y[:512])) < 0.5 and np.all(vt < 4 * th.noise + 1e-3)
    # the mean never goes through the split: identical in both split modes
    assert np.array_equal(results["bf16x6"][0], results["bf16x3"][0])
    # (the fp16 split scales the generated tile by a power of two -- exact -- and undoes it on the partial sums in double:
    # with the same contraction its mean is the bf16 modes'; by default it contracts x.x* on the fp16 pipe: float class)
    assert np.max(np.abs(results["f16x3"][0] - results["bf16x6"][0])) <= 2 * bm * ys
    eng.set_predict_math("f16x3")
    eng.set_contraction("f32")
    assert np.max(np.abs(eng.predict(Xs)[0] - results["bf16x6"][0])) <= 1e-12 * ys
    eng.set_contraction("auto")
    assert np.max(np.abs(results["bf16x6"][1] - results["native"][1])) <= 5e-5
    assert np.max(np.abs(results["f16x3"][1] - results["native"][1])) <= 5e-5
    assert np.max(np.abs(results["bf16x3"][1] - results["native"][1])) <= 2e-4


def test_config_C2_full_oracle():
    n, d, m = 256, 6, 4096
    X, y, th = _problem(n, d, variance=1.0)
    post = gpr.posterior(th, X, y)
    Xs = synthetic_leaves(m, d)
    eng = _engine("float64")
    _fit(eng, X, y, th)
    mean, var = eng.predict(Xs)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    assert np.max(np.abs(mean - mean_ref)) < 1e-9 and np.max(np.abs(var - var_ref)) < 1e-9
    assert int(eng.best_ucb(Xs, VS)[0][0]) == gpr.best_ucb(post, Xs)[0]


def test_config_C3_properties_fp32():
    n, d, m = 2048, 12, 65536
    X, y, th = _problem(n, d, variance=1.0)
    post = gpr.posterior(th, X, y)
    eng = _engine("float32")
    _fit(eng, X, y, th, grad=False)
    assert eng.precision_info()["predict_math"] == "f16x3"  # the default math of the bench line
    nat = HipGPEngine_native(X, y, th)
    _properties(eng, X, y, th, synthetic_leaves(m, d), post, 512, "C3", nat)
    _properties(nat, X, y, th, synthetic_leaves(m, d), post, 512, "C3")


def HipGPEngine_native(X, y, th):
    from pygpso_amd import HipGPEngine

    nat = HipGPEngine("float32", predict_math="native")
    _fit(nat, X, y, th, grad=False)
    return nat


@pytest.mark.parametrize("math", ["native", "f16x3", "bf16x6", "bf16x3"])
def test_config_C4_one_gpu_shard_properties_fp32(math):
    from pygpso_amd import HipGPEngine

    n, d, m = 8192, 20, 32768  # 256k leaves / 8 GPUs
    X, y, th = _problem(n, d, variance=1.0)
    post = _c4_posterior(th, X, y)
    eng = HipGPEngine("float32", predict_math=math)
    f, _ = _fit(eng, X, y, th, grad=False)
    assert abs(f - post.nlml) <= 1e-4 * abs(post.nlml)
    _properties(eng, X, y, th, synthetic_leaves(m, d), post, 128, "C4", None if math == "native" else HipGPEngine_native(X, y, th))


_c4_cache = {}


def _c4_posterior(th, X, y):
    if "post" not in _c4_cache:  # one CPU factorisation at N = 8192 for the three math modes
        _c4_cache["post"] = gpr.posterior(th, X, y)
    return _c4_cache["post"]


@pytest.mark.parametrize("noise", [1e-2, 1e-3])
def test_float_fit_on_the_bf16_matrix_cores_agrees_with_the_f32_path(noise):
    """Float fits above the single-level limit run their large products (rank-W trailing updates, level-doubling
    inverse, K^-1) on the 16-bit matrix cores (GPSO_OPT_FIT_BF16_SYRK): 2 (default, round 5) two fp16 pieces of the
    power-of-two scaled operands, three MFMAs per product; 1 three bf16 pieces, six MFMAs.  N = 4096 (N_pad / panel a
    power of two: both the update and the inverse take the split path), each against the same fit on the f32 MFMA and
    against the float64 oracle -- the SAME bounds for both splits (none loosened for the fp16 one)."""
    from pygpso_amd import HipGPEngine, _lib as L

    n, d = 4096, 6
    X, y, th = _problem(n, d, variance=1.0, noise=noise)
    post = gpr.posterior(th, X, y)
    res = {}
    for flag in (2, 1, 0):
        eng = HipGPEngine("float32")
        eng._check(eng._lib.gpso_set_option(eng._h, L.OPT_FIT_BF16_SYRK, flag))
        f, g = _fit(eng, X, y, th, grad=True)  # (with the gradient: K^-1 = L^-T L^-1 is a split product as well)
        res[flag] = (f, eng.get_matrix(L.MAT_LINV), eng.get_vector(L.VEC_ALPHA), eng.get_matrix(L.MAT_CHOL),
                     g, eng.get_matrix(L.MAT_KINV))
    _, g_ref = gpr.nlml_and_grad(th, X, y)
    for flag in (2, 1, 0):  # each path against the oracle, float tolerances
        f, linv, alpha, chol, g, kinv = res[flag]
        assert abs(f - post.nlml) <= 2e-5 * abs(post.nlml), flag
        # measured (profiles/r03_grad_error.jsonl): split-bf16 products 8e-5 / 1.7e-4, f32 MFMA products 3.6e-4 / 3.8e-4 at
        # noise 1e-2 / 1e-3; LAPACK float32 on the host 4e-5 / 5e-5; eps x cond(K_y) = 1.4e-2 / 1.1e-1
        assert np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref))) < 2e-3, flag
        assert np.max(np.abs(chol - post.L)) <= 2e-4 * np.max(np.abs(post.L)), flag
        # alpha = K_y^-1 (y - c): a forward error, it scales with cond(K_y) = 1.2e5 / 9.3e5 at the two noise levels
        # (measured 2.4e-3 at 1e-3 on both product paths; eps x cond = 0.11)
        assert np.max(np.abs(alpha - post.alpha)) <= (2e-3 if noise >= 1e-2 else 1e-2) * np.max(np.abs(post.alpha)), flag
    # and against each other: the split products are float-class.  Both are float factorisations of the same matrix:
    # they differ by rounding amplified by the conditioning -- L^-1 by cond(L) = sqrt(cond(K_y)) (340 / 960 at the two
    # noise levels), K^-1 by cond(K_y) (1.2e5 / 9.3e5); measured at noise 1e-3: 3.6e-4 on L^-1
    amp = 1.0 if noise >= 1e-2 else 4.0
    scale = np.max(np.abs(res[0][1]))
    for flag in (2, 1):
        ratios = {"linv": np.max(np.abs(res[flag][1] - res[0][1])) / (2e-4 * amp * scale),
                  "chol": np.max(np.abs(res[flag][3] - res[0][3])) / (5e-5 * np.max(np.abs(res[0][3]))),
                  "kinv": np.max(np.abs(res[flag][5] - res[0][5])) / (2e-4 * amp * amp * np.max(np.abs(res[0][5]))),
                  "grad": np.max(np.abs(res[flag][4] - res[0][4]) / np.maximum(1.0, np.abs(res[0][4]))) / 2e-3}
        errs = {"nlml": abs(res[flag][0] - post.nlml) / abs(post.nlml),
                "grad_vs_oracle": float(np.max(np.abs(res[flag][4] - g_ref) / np.maximum(1.0, np.abs(g_ref)))),
                "chol_vs_oracle": float(np.max(np.abs(res[flag][3] - post.L)) / np.max(np.abs(post.L)))}
        print(f"fit planes mode {flag} (noise {noise}): measured / tolerance vs the f32 path:", {k: round(float(v), 3) for k, v in ratios.items()},
              "| vs the oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
        assert all(v <= 1.0 for v in ratios.values()), (flag, ratios)


@pytest.mark.parametrize("dtype,math", [("float32", "f16x3"), ("float32", "bf16x6"), ("float32", "bf16x3"), ("float32", "native"),
                                        ("mixed", "f16x3"), ("mixed", "bf16x6"), ("mixed", "bf16x3"), ("mixed", "native"),
                                        ("float64", "native")])
@pytest.mark.parametrize("n,d", [(200, 3), (512, 1), (1024, 12)])
def test_run_to_run_determinism(dtype, math, n, d):
    """No kernel of the path sums with atomics: the same posterior and leaves give the same BITS every time.  A
    result that changes between runs is a race or a hazard -- the packed accumulation of the two column tiles'
    means in the split-bf16 kernel (profiles/r02h_packed_mean_bug.txt) showed as a wrong mean in 8 % of the runs
    of the (200, 3) case, and at N = 2048 in the (mixed, bf16x3) instantiation whose generation runs on the f64 MFMA
    (test_run_to_run_determinism_c3_g7 below).  A float32 engine that refuses the posterior is replaced by a mixed
    one -- what the product does -- instead of skipping.  tools/race_probe.py is the long version."""
    from pygpso_amd import HipGPEngine
    from pygpso_amd._lib import GpsoPrecisionError

    X, y = synthetic_problem(n, d, seed=7 * n + d)
    Xs = synthetic_leaves(257, d, seed=11 * n + d)
    ls = 0.25 * np.sqrt(d) * np.ones(1)
    ref = None
    ladder = [(dtype, math)] + {"float32": [("mixed", math), ("float64", "native")], "mixed": [("float64", "native")]}.get(dtype, [])
    for _ in range(25):
        while True:  # what HipGPR._escalate does: the next more precise engine, on the device
            dtype, math = ladder[0]
            eng = HipGPEngine(dtype, predict_math=math)
            eng.set_data(X, y)
            try:
                f, g = eng.fit_eval("Matern32", ls, 1.3, 1e-3, float(y.mean()), want_grad=True)
                mean, var = eng.predict(Xs)
                break
            except GpsoPrecisionError:
                assert ref is None and len(ladder) > 1  # a verdict, not a flake: the same on every run
                ladder.pop(0)
        cur = (np.float64(f).tobytes(), np.asarray(g).tobytes(), mean.tobytes(), var.tobytes())
        if ref is None:
            ref = cur
            post = gpr.posterior(gpr.Theta("Matern32", ls, 1.3, 1e-3, float(y.mean())), X, y)
            mean_ref, _ = gpr.predict_y(post, Xs)
            assert np.max(np.abs(mean - mean_ref)) <= (1e-9 if dtype == "float64" else 4e-4) * max(1.0, np.max(np.abs(y)))
        assert cur == ref


@pytest.mark.parametrize("math,tol_var", [("bf16x3", 1e-4), ("bf16x6", 5e-6), ("f16x3", 5e-6), ("native", 5e-6)])
def test_run_to_run_determinism_c3_g7(math, tol_var):
    """The posterior on which the packed-mean failure showed most often (18 % of the predict calls,
    profiles/r02h_packed_mean_bug.txt B): "C3-G7" of tests/test_gpu_precision.py -- C3's shape (N = 2048, D = 12) with
    the reference's hyper-parameters after the first G7 update and the noise at GPflow's 1e-6 floor -- in a mixed
    engine, whose generation then runs on the f64 MFMA.  The engine is re-created and the device idles between calls,
    as under the optimiser loop: the failure was a first-launch / clock-ramp effect."""
    import time

    from pygpso_amd import HipGPEngine
    from tests.test_gpu_precision import _problem as precision_problem

    X, y, th, leaves, post, mean_ref, var_ref = precision_problem("C3-G7")
    ref = None
    for rep in range(10):
        eng = HipGPEngine("mixed", predict_math=math, tol_var=2 * tol_var)
        eng.set_data(X, y)
        eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
        for call in range(3):
            mean, var = eng.predict(leaves)
            cur = (mean.tobytes(), var.tobytes())
            if ref is None:
                ref = cur
                assert np.max(np.abs(var - var_ref)) <= tol_var * th.variance
            assert cur == ref, (rep, call, float(np.max(np.abs(mean - mean_ref))))
            time.sleep(0.02)
        eng.close()


@pytest.mark.parametrize("dtype,math,gen,contraction",
                         [("float32", "f16x3", "float32", "auto"), ("float32", "f16x3", "float32", "f32"), ("float32", "f16x3", "float32", "f16"),
                          ("mixed", "f16x3", "float64", "auto"), ("float32", "bf16x3", "float32", "auto"), ("mixed", "bf16x3", "float64", "auto"),
                          ("float32", "bf16x6", "float32", "auto"), ("mixed", "bf16x6", "float64", "auto")])
@pytest.mark.parametrize("n,d,m,kernel", [(256, 6, 1000, "Matern52"), (2048, 12, 4096, "Matern52"), (768, 3, 700, "Matern32"),
                                          (512, 24, 513, "SquaredExponential"), (1024, 40, 300, "Matern12"), (512, 1, 257, "Matern52"),
                                          (600, 8, 513, "Matern52"), (300, 5, 700, "Matern32"), (1100, 12, 300, "Matern52"), (450, 6, 300, "Matern52")])
def test_fused_step_kernel_gives_the_bits_of_the_two_phase_kernel(dtype, math, gen, contraction, n, d, m, kernel):
    """Round 4: the split kernels run the FUSED step (every wave applies step q with the generation of step q + 1 dealt
    into its MFMA shadows, one barrier per step) instead of round 3's two-phase step (generation and apply as two
    stretches, the waves of a SIMD in opposite order).  Same operations on the same operands in the same order --
    means, variances and winners must be the SAME BITS, for float and double generation, every kernel family, ragged
    leaf counts, several row blocks, segments and on-device growth; with the x.x* contraction of the fp16 split on the
    f32 matrix instruction and on the fp16 pipe (GPSO_OPT_CONTRACTION)."""
    from pygpso_amd import HipGPEngine

    X, y, th = _problem(n, d, kernel, noise=1e-3, variance=1.7)
    Xs = synthetic_leaves(m, d, seed=3)
    res = {}
    for which in ("auto", "two-phase"):
        eng = HipGPEngine(dtype, predict_math=math, generation=gen, precision_check=False)
        eng.set_split_kernel(which)
        eng.set_contraction(contraction)
        _fit(eng, X, y, th, grad=False)
        # (N = 600, 300, 1100: a last row block with <= 128 training rows -- the fused kernel applies its first eight row tiles
        # only and stops at the last k-step that holds training points; N = 450: more than 128 rows in the last block)
        if not (gen == "float64" and d >= (24 if math == "bf16x6" else 36)):
            assert eng.precision_info()["predict_math"] == math  # (the split kernel really runs)
        mean, var = eng.predict(Xs)
        seg = np.array([0, 1, m // 3, m // 3, m], dtype=np.int64)
        best = eng.best_ucb(Xs, VS, seg)
        res[which] = (mean, var, best)
        if d <= 6:
            kids = tree.split_bounds([(0.0, 1.0)] * d)
            res[which] += (eng.best_ucb_grow(np.array([kids[0], kids[2]]), 5, VS),)
    a, b = res["auto"], res["two-phase"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a[2], b[2]))
    if len(a) > 3:
        assert all(np.array_equal(p, q) for p, q in zip(a[3], b[3]))
    post = gpr.posterior(th, X, y)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    assert np.max(np.abs(a[0] - mean_ref)) <= 2e-3 * max(1.0, np.max(np.abs(y))) and np.max(np.abs(a[1] - var_ref)) <= 2e-4 * th.variance


@pytest.mark.parametrize("n,d,m,kernel", [(256, 6, 1000, "Matern52"), (2048, 12, 4096, "Matern52"), (768, 20, 700, "Matern32"),
                                          (512, 33, 513, "SquaredExponential"), (1024, 40, 300, "Matern52"), (512, 48, 257, "Matern52"),
                                          (256, 2, 300, "Matern52")])
def test_fp16_contraction_is_in_the_float_class_and_survives_far_leaves(n, d, m, kernel):
    """Round 4: under float generation the fp16-split kernel contracts x.x* on the fp16 pipe (the scaled inputs split
    into fp16 piece pairs like L^-1; GPSO_OPT_CONTRACTION).  Against the float64 oracle its error is in the class of the
    f32 contraction's (within 2x + a floor, both inside the bounds the fused-step test uses); the option is live (other
    bits); and leaves far outside the training range -- where
    the scaled leaf saturates fp16 -- come back finite with the prior's variance, as from the f32 contraction."""
    from pygpso_amd import HipGPEngine

    X, y, th = _problem(n, d, kernel, noise=1e-3, variance=1.7)
    Xs = synthetic_leaves(m, d, seed=5)
    far = np.concatenate([Xs[:64] * 300.0, -Xs[:64] * 1e4, Xs[:64] + 3.0])
    post = gpr.posterior(th, X, y)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    mean_far, var_far = gpr.predict_y(post, far)
    res = {}
    for which in ("f16", "f32"):
        eng = HipGPEngine("float32", predict_math="f16x3", generation="float32", precision_check=False)
        eng.set_contraction(which)
        _fit(eng, X, y, th, grad=False)
        assert eng.precision_info()["predict_math"] == "f16x3"
        res[which] = eng.predict(Xs) + eng.predict(far)
        eng.close()
    err = {w: (np.max(np.abs(r[0] - mean_ref)), np.max(np.abs(r[1] - var_ref))) for w, r in res.items()}
    ymax = max(1.0, np.max(np.abs(y)))
    for w in err:
        assert err[w][0] <= 2e-3 * ymax and err[w][1] <= 2e-4 * th.variance, (w, err)
    assert err["f16"][0] <= 2 * err["f32"][0] + 2e-5 * ymax and err["f16"][1] <= 2 * err["f32"][1] + 2e-6 * th.variance, err
    assert not np.array_equal(res["f16"][1], res["f32"][1]), "the option changes the arithmetic"
    for w, r in res.items():
        assert np.all(np.isfinite(r[2])) and np.all(np.isfinite(r[3])), w
        assert np.max(np.abs(r[2] - mean_far)) <= 2e-3 * ymax and np.max(np.abs(r[3] - var_far)) <= 2e-4 * th.variance, w


@pytest.mark.parametrize("n", [130, 300, 321, 600, 1100])
def test_float_predict_contexts_pad_to_the_split_kernels_row_block(n):
    """Float-predict contexts pad N > 128 to a multiple of 256 (the row block of the split kernels), so the fp16 split
    runs at EVERY N -- with a pad of 128 half of all N fell to the f32 MFMA kernel (N = 1100: 0.89 -> 0.30 ms per 65 536
    leaves).  The single-level factorisation only steps over the 64-row blocks that hold training rows, so the padding
    costs the fit nothing; a double fit on the larger pad (mixed) is the float64 context's fit BIT FOR BIT (factor,
    inverse, alpha, loss, gradient), and the predictions keep their tolerances."""
    from pygpso_amd import HipGPEngine
    from pygpso_amd import _lib as L

    d = 5
    X, y, th = _problem(n, d, noise=1e-3, variance=1.3)
    Xs = synthetic_leaves(1000, d, seed=4)
    post = gpr.posterior(th, X, y)
    mean_ref, var_ref = gpr.predict_y(post, Xs)
    out = {}
    for dtype in ("float64", "mixed", "float32"):
        eng = HipGPEngine(dtype)
        f, g = _fit(eng, X, y, th, grad=True)
        assert eng.padded_n == (-(-n // 128) * 128 if dtype == "float64" else -(-n // 256) * 256)
        out[dtype] = (f, g, eng.get_matrix(L.MAT_CHOL), eng.get_matrix(L.MAT_LINV), eng.get_vector(L.VEC_ALPHA), eng.predict(Xs))
        if dtype != "float64":
            assert eng.precision_info()["predict_math"] == "f16x3"
        eng.close()
    a, b = out["float64"], out["mixed"]
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert all(np.array_equal(p, q) for p, q in zip(a[2:5], b[2:5]))
    assert np.max(np.abs(a[5][0] - mean_ref)) < 1e-9 and np.max(np.abs(a[5][1] - var_ref)) < 1e-9
    ymax = max(1.0, np.max(np.abs(y)))
    for dtype in ("mixed", "float32"):
        mean, var = out[dtype][5]
        assert np.max(np.abs(mean - mean_ref)) <= SMALL_FLOAT_BOUNDS[0] * ymax and np.max(np.abs(var - var_ref)) <= SMALL_FLOAT_BOUNDS[1] * th.variance, dtype


@pytest.mark.parametrize("n,d", [(512, 4), (2048, 3), (2048, 6), (2048, 12), (1024, 20)])
def test_generation_choice_walks_fp16_contraction_then_f32_contraction_then_double(n, d):
    """GPSO_GEN_AUTO (float32 context, default options): the posterior's self-test picks the generation arithmetic --
    float with the contraction on the fp16 pipe where that is comfortably inside the tolerances or as good as double
    generation; else float with the f32 contraction of rounds 1-3 on the same terms (its r^2 AT a training input, where
    the test looks, is closer to zero); else double.  Whatever it picks, the predictions are the BITS of an engine
    pinned to that arithmetic, and at these shapes (round 3 kept float generation on all of them) it is never double."""
    from pygpso_amd import HipGPEngine

    X, y = synthetic_problem(n, d, seed=0)
    th = gpr.Theta("Matern52", 0.25 * np.sqrt(d) * np.ones(1), 1.0, 1e-3, float(y.mean()))
    Xs = synthetic_leaves(777, d, seed=2)

    def run(generation=None, contraction=None):
        eng = HipGPEngine("float32", **({} if generation is None else {"generation": generation}))
        if contraction is not None:
            eng.set_contraction(contraction)
        _fit(eng, X, y, th, grad=False)
        info = eng.precision_info()
        out = eng.predict(Xs)
        eng.close()
        return info, out

    info, auto = run()
    assert info["passed"] and info["predict_math"] == "f16x3"
    pinned = {"fp16 contraction": run("float32", "f16")[1], "f32 contraction": run("float32", "f32")[1], "double": run("float64")[1]}
    same = [k for k, v in pinned.items() if np.array_equal(v[0], auto[0]) and np.array_equal(v[1], auto[1])]
    print(f"generation choice N={n} D={d}: {same}")
    assert len(same) >= 1 and same[0] != "double" and info["generation"] == "float32", (same, info)
    if (n, d) == (512, 4):
        assert same == ["f32 contraction"]  # (the second rung: measured -- the fp16 contraction reads 1.9x double's variance error here)
    if (n, d) == (2048, 12):
        assert same == ["fp16 contraction"]  # (C3's shape keeps the fast path)


@pytest.mark.parametrize("dtype", ["float64", "mixed", "float32"])
@pytest.mark.parametrize("n,d,depth", [(52, 2, 5), (30, 4, 7), (100, 6, 9), (128, 3, 8), (300, 5, 6), (7, 1, 9), (256, 6, 8), (200, 12, 4)])
def test_small_call_sequence_gives_the_bits_of_the_general_one(dtype, n, d, depth):
    """Round 4: best-UCB calls on small batches run growth + input scaling in ONE launch (boxes by value), the tile
    kernel, and finalize + arg-max in one workgroup that writes pinned host memory (GPSO_OPT_SMALL_CALLS, default on).
    Same winners, values, indices and row counts as the general sequence: unit-cube boxes (a third of the rows dropped),
    arbitrary boxes (near-duplicates appended through the counter, twice in a row: it must be back at zero), plain
    batches from the host with ragged and empty segments, and the sharded halves."""
    from pygpso_amd import HipGPEngine

    X, y, th = _problem(n, d, noise=1e-3 if dtype != "float64" else 1e-6, variance=1.3)
    rng = np.random.default_rng(depth)
    kids = tree.split_bounds([(0.0, 1.0)] * d)
    lo = rng.random((2, d)) * 0.5
    arbitrary = np.stack([lo, lo + 0.1 + 0.4 * rng.random((2, d))], axis=2)
    res = {}
    for small in (3, 1, 2, 0):  # one launch wherever it applies | the default choice | three launches | the general sequence
        eng = HipGPEngine(dtype)
        eng.set_small_calls(small)
        _fit(eng, X, y, th, grad=False)
        out = []
        for boxes in (np.array([kids[0], kids[2]]), arbitrary, arbitrary, np.array([kids[1]])):
            out.append(eng.best_ucb_grow(boxes, depth, VS) + (eng.last_count(0), eng.last_count(1)))
        Xs = synthetic_leaves(700, d, seed=depth)
        out.append(eng.best_ucb(Xs, VS, np.array([0, 0, 1, 350, 699, 700], dtype=np.int64)))
        out.append(eng.best_ucb(Xs[:1], VS))
        out.append(tuple(eng.shard_winners_grow(r, 3, arbitrary, depth, VS) for r in range(3)))
        res[small] = out
    for other in (3, 1, 2):
        for a, b in zip(res[other], res[0]):
            for p, q in zip(a, b):
                assert np.array_equal(np.asarray(p), np.asarray(q), equal_nan=True), other
    # and against the full duplicated list scored by predict + numpy (the reference's gp_eval_best_ucb)
    eng = HipGPEngine(dtype)
    _fit(eng, X, y, th, grad=False)
    full = eng.grow(arbitrary, depth)
    for sgm in range(2):
        mean, var = eng.predict(full[sgm])
        ucb = mean + VS * var
        i = int(np.argmax(ucb))
        got = res[1][1]
        assert int(got[0][sgm]) == i and got[3][sgm] == ucb[i] and got[1][sgm] == mean[i] and got[2][sgm] == var[i]


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_the_non_blocking_pair_gives_the_blocking_calls_bits(dtype):
    """gpso_best_ucb_begin / _grow_begin / _end: two calls in flight, ended in order or out of order, return what the
    blocking calls return, bit for bit; a third begin is refused; a ticket is good for one end."""
    from pygpso_amd import HipGPEngine, _lib as L

    n, d = 700, 4
    X, y, th = _problem(n, d, variance=1.0)
    eng = HipGPEngine(dtype)
    _fit(eng, X, y, th, grad=False)
    A, B = synthetic_leaves(5000, d, seed=3), synthetic_leaves(30000, d, seed=4)
    seg = np.array([0, 1000, 1000, 30000])
    ref_a, ref_b = eng.best_ucb(A, VS), eng.best_ucb(B, VS, seg)
    box = np.array([[[0.2, 0.5]] * d, [[0.0, 1.0 / 3.0]] * d])
    ref_g = eng.best_ucb_grow(box, 6, VS)
    for order in ("in order", "reversed"):
        ta = eng.best_ucb_begin(A, VS)
        tb = eng.best_ucb_begin(B, VS, seg)
        with pytest.raises(L.GpsoHipError, match="already in flight"):
            eng.best_ucb_begin(A, VS)
        if order == "in order":
            got_a, got_b = eng.best_ucb_end(ta), eng.best_ucb_end(tb)
        else:
            got_b, got_a = eng.best_ucb_end(tb), eng.best_ucb_end(ta)
        assert all(np.array_equal(u, v) for u, v in zip(got_a, ref_a))
        assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(got_b, ref_b))
    tg = eng.best_ucb_grow_begin(box, 6, VS)
    with pytest.raises(L.GpsoHipError, match="asynchronous"):  # the posterior cannot change under an open ticket
        eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    ta = eng.best_ucb_begin(A, VS)
    assert all(np.array_equal(u, v) for u, v in zip(eng.best_ucb_end(tg), ref_g))
    assert all(np.array_equal(u, v) for u, v in zip(eng.best_ucb_end(ta), ref_a))
    rc = eng._lib.gpso_best_ucb_end(eng._h, ta, None, None, None, None)
    assert rc == L.E_ARG  # (ended already)
    # a long pipeline: K calls, two deep
    t = eng.best_ucb_begin(A, VS)
    for _ in range(20):
        t2 = eng.best_ucb_begin(A, VS)
        assert all(np.array_equal(u, v) for u, v in zip(eng.best_ucb_end(t), ref_a))
        t = t2
    assert all(np.array_equal(u, v) for u, v in zip(eng.best_ucb_end(t), ref_a))
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(eng.best_ucb(B, VS, seg), ref_b))  # the blocking call behind it


@pytest.mark.parametrize("n,d", [(2048, 12), (700, 33), (300, 5)])
def test_leaves_scaled_in_the_kernels_prologue_give_the_prep_kernels_bits(n, d):
    """Float leaves of a one-chunk batch are scaled by the lengthscales in the fp16-contraction kernel's own prologue
    (GPSO_OPT_FUSED_PREP, default on): the same bits as with the separate prep kernel, and as float64 leaves holding the
    same values (which always go through the prep kernel) -- host and device leaves, predict and best-UCB."""
    import torch

    from pygpso_amd import HipGPEngine, _lib as L

    X, y, th = _problem(n, d, variance=1.0)
    Xs = synthetic_leaves(5000, d).astype(np.float32)
    res = []
    for fused in (1, 0):
        eng = HipGPEngine("mixed", predict_math="f16x3")
        eng._check(eng._lib.gpso_set_option(eng._h, L.OPT_FUSED_PREP, fused))
        _fit(eng, X, y, th, grad=False)
        assert eng.precision_info()["predict_math"] == "f16x3"
        dev = torch.from_numpy(Xs).cuda()
        res.append((eng.predict(Xs), eng.predict(dev), eng.best_ucb(dev, VS, np.array([0, 17, 4000, 5000])), eng.predict(Xs.astype(np.float64))))
    for a, b in zip(res[0], res[1]):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert all(np.array_equal(u, v) for u, v in zip(res[0][0], res[0][3]))  # float leaves == the same values as doubles
    mean_ref, var_ref = gpr.predict_y(gpr.posterior(th, X, y), Xs.astype(np.float64))
    assert np.max(np.abs(res[0][0][1] - var_ref)) <= 2e-5 * th.variance


# ---- round 6: the double two-level fit overlaps chains, updates and the inverse (GPSO_OPT_FIT_OVERLAP) ---------------------
@pytest.mark.parametrize("n,d,force_two_level", [(2048, 6, True), (1500, 3, True), (4096, 6, False), (3000, 5, False)])
def test_overlapped_double_fit_gives_the_sequential_schedules_bits(n, d, force_two_level):
    """float64 / mixed fits above the single-level limit look the diagonal chains ahead on a side stream and issue the
    level-doubling inverse pair by pair on a third one as soon as its panels are final (fit.hip: launch_potrf).  The same
    products on the same tiles in the same k order: L, L^-1, alpha, K^-1, NLML and gradient are the sequential schedule's
    bits -- and the oracle's values to 1e-9.  Panel counts: 4 (a power of two: the overlapped inverse) and 3 (look-ahead
    only), at the default limit and forced at small sizes."""
    from pygpso_amd import HipGPEngine, _lib as L

    X, y, th = _problem(n, d, noise=1e-3)
    res = {}
    for overlap in (3, 2, 0):  # look-ahead + overlapped inverse | the default (overlapped inverse) | sequential
        eng = HipGPEngine("float64")
        eng._check(eng._lib.gpso_set_option(eng._h, L.OPT_FIT_OVERLAP, overlap))
        if force_two_level:
            eng.set_fit_single_level_max(0)
        outs = []
        for rep in range(2):  # (twice: stream / event reuse across fits of one context)
            f, g = _fit(eng, X, y, th, grad=True)
            outs.append((f, g.tobytes(), eng.get_matrix(L.MAT_LINV).tobytes(), eng.get_matrix(L.MAT_CHOL).tobytes(),
                         eng.get_vector(L.VEC_ALPHA).tobytes(), eng.get_matrix(L.MAT_KINV).tobytes()))
        assert outs[0] == outs[1]
        res[overlap] = (outs[0], eng)
    assert res[3][0] == res[0][0] and res[2][0] == res[0][0]
    f_ref, g_ref = gpr.nlml_and_grad(th, X, y)
    post = gpr.posterior(th, X, y)
    eng = res[3][1]
    f = res[3][0][0]
    assert abs(f - f_ref) <= 1e-9 * abs(f_ref)
    assert _rel(eng.get_matrix(L.MAT_CHOL), post.L) < 1e-9
    assert _rel(eng.get_matrix(L.MAT_LINV), np.linalg.inv(post.L)) < 1e-8
    assert _rel(eng.get_vector(L.VEC_ALPHA), post.alpha) < 1e-7
    g = np.frombuffer(res[3][0][1], dtype=np.float64)
    assert np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref))) < 1e-7
    # a posterior fit (no gradient) leaves the same factor
    f2, _ = _fit(eng, X, y, th, grad=False)
    assert f2 == f and eng.get_matrix(L.MAT_LINV).tobytes() == res[3][0][2]


# ---- round 6: a workgroup of the split kernels loops over row blocks (GPSO_OPT_ROW_LOOP) ---------------------------------------
@pytest.mark.parametrize("dtype,math", [("float32", "f16x3"), ("float32", "bf16x6"), ("mixed", "f16x3"), ("float32", "bf16x3"),
                                        ("mixed", "bf16x6")])
@pytest.mark.parametrize("n,d,m", [(2048, 12, 65536), (2048, 12, 8192), (512, 6, 2048), (1024, 20, 1000), (2040, 12, 4096),
                                   (4096, 6, 300), (1100, 33, 77000), (300, 5, 4096)])
def test_row_block_loop_gives_the_one_row_block_kernels_bits(dtype, math, n, d, m):
    """A workgroup keeps its leaf tile and loops over the row blocks of its split (the leaf prologue once per tile instead of
    once per row block); the launcher picks how many workgroups share a leaf tile (forced here to 1 ... all of them).  Every (leaf tile, row block)
    is computed by the same operations in the same order: means, variances and winners are the bits of rounds 1-5's kernel,
    with segments, two-phase and fused steps, a last row block of few rows (N = 1100, 2040) and batches of every size class."""
    from pygpso_amd import HipGPEngine

    X, y, th = _problem(n, d, variance=1.0)
    eng = HipGPEngine(dtype, predict_math=math, precision_check=False)
    _fit(eng, X, y, th, grad=False)
    Xs = synthetic_leaves(m, d).astype(np.float32)
    seg = np.array([0, m // 3, m // 3, m - 5, m], dtype=np.int64)
    out = {}
    for on in (1, 0, 2, 3, 4, 1000):  # (2, 3, 4, 1000: that many workgroups per leaf tile, capped at the row blocks)
        eng.set_row_loop(on)
        for which in ("auto", "two-phase"):
            eng.set_split_kernel(which)
            mean, var = eng.predict(Xs)
            out[(on, which)] = (mean.tobytes(), var.tobytes(), tuple(a.tobytes() for a in eng.best_ucb(Xs, VS, seg)))
    assert len(set(out.values())) == 1, [k for k, v in out.items() if v != out[(0, "auto")]]


@pytest.mark.gpu
def test_row_block_split_count_follows_the_makespan_model():
    """gpso_last_count(ctx, 3) = workgroups per leaf tile of the last split launch.  The rule (leaf_row_splits, leaf_split.hpp):
    C3's 256 leaf tiles = one workgroup each on the 256 CUs -> 1; a batch of 32 tiles -> one row block per workgroup (256
    workgroups); 462 tiles (bench.py --leaves grow --depth 11: a coarser grain costs a round of tail, measured +4.7 %) -> one row
    block per workgroup; a grown batch, whose live count only the device knows -> one row block per workgroup."""
    from pygpso_amd import HipGPEngine

    X, y, th = _problem(2048, 12, variance=1.0)
    eng = HipGPEngine("float32", predict_math="f16x3", precision_check=False)
    _fit(eng, X, y, th, grad=False)
    nbi = 2048 // 256
    for m, want in ((65536, 1), (8192, nbi), (118098, nbi), (4 * 65536, 1), (128 * 256, 2)):
        eng.best_ucb(synthetic_leaves(m, 12).astype(np.float32), VS)
        assert eng.last_count(3) == want, (m, eng.last_count(3))
    eng.set_row_loop(0)
    eng.best_ucb(synthetic_leaves(65536, 12).astype(np.float32), VS)
    assert eng.last_count(3) == nbi
    eng.set_row_loop(1)
    boxes = np.array([[[0.0, 1.0 / 3]] + [[0.0, 1.0]] * 11, [[2.0 / 3, 1.0]] + [[0.0, 1.0]] * 11])
    eng.best_ucb_grow(boxes, 9, VS)
    assert eng.last_count(3) == nbi


def _leaf_row_splits(mode, ltiles, nbi, ncu, live_known=True):
    """leaf_row_splits (leaf_split.hpp) restated: workgroups per leaf tile for GPSO_OPT_ROW_LOOP = mode."""
    if mode == 0 or nbi <= 1:
        return nbi
    if mode >= 2:
        return min(mode, nbi)
    if not live_known:
        return nbi
    prologue = 1.2
    total = 4.0 * nbi * (nbi + 1)
    best, best_s = max(ltiles * (total + prologue * nbi) / ncu + 8.0, 8.0 * nbi + prologue), nbi
    S = nbi // 2
    while S >= 1:
        heaviest = 0.0
        for split in range(S):
            w, j = 0.0, 0
            while True:
                rank = j * S + ((S - 1 - split) if j & 1 else split)
                if rank >= nbi:
                    break
                w += 8.0 * (nbi - rank)
                j += 1
            heaviest = max(heaviest, w)
        t = ((ltiles * S + ncu - 1) // ncu) * (heaviest + prologue)
        if t <= best:
            best, best_s = t, S
        S //= 2
    return best_s


# the smallest shape at which the split count can differ: four 256-row blocks, two leaf tiles
_ROW_LOOP_SHAPE = (1024, 6, 300)


def _row_loop_engine(X, y, th, row_loop=None):
    from pygpso_amd import HipGPEngine

    eng = HipGPEngine("float32", predict_math="f16x3", precision_check=False)
    _fit(eng, X, y, th, grad=False)
    if row_loop is not None:
        eng.set_row_loop(row_loop)
    return eng


def test_row_loop_option_and_split_count_belong_to_one_context():
    """GPSO_OPT_ROW_LOOP set on one context steers that context's launches only, and gpso_last_count(ctx, 3) reports the last
    launch that context made: two engines on the same data with different options keep their own counts across interleaved
    calls, and a third that was never given the option launches by the default rule and returns the same bits."""
    import torch

    n, d, m = _ROW_LOOP_SHAPE
    X, y, th = _problem(n, d, variance=1.0)
    Xs = synthetic_leaves(m, d).astype(np.float32)
    A, B = _row_loop_engine(X, y, th, 0), _row_loop_engine(X, y, th, 2)
    A.best_ucb(Xs, VS)
    B.best_ucb(Xs, VS)
    assert A.last_count(3) == 4 and B.last_count(3) == 2, (A.last_count(3), B.last_count(3))
    A.best_ucb(Xs, VS)
    assert A.last_count(3) == 4 and B.last_count(3) == 2, (A.last_count(3), B.last_count(3))
    C = _row_loop_engine(X, y, th)
    out = []
    for eng in (A, B, C):
        mean, var = eng.predict(Xs)
        out.append((mean.tobytes(), var.tobytes(), tuple(a.tobytes() for a in eng.best_ucb(Xs, VS))))
    assert out[0] == out[1] == out[2]
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert C.last_count(3) == _leaf_row_splits(1, (m + 255) // 256, n // 256, ncu)
    assert A.last_count(3) == 4 and B.last_count(3) == 2, (A.last_count(3), B.last_count(3))


def test_row_loop_option_and_split_count_per_context_from_two_threads():
    """The same from one host thread per engine (what HipGPEngineGroup does per device): every call reports its own
    context's split count, every time -- nothing a launch reads or writes is shared between contexts."""
    import threading

    n, d, m = _ROW_LOOP_SHAPE
    X, y, th = _problem(n, d, variance=1.0)
    Xs = synthetic_leaves(m, d).astype(np.float32)
    failures = []

    def work(eng, want):
        try:
            for it in range(20):
                eng.best_ucb(Xs, VS)
                got = eng.last_count(3)
                if got != want:
                    failures.append((want, it, got))
        except Exception as e:  # noqa: BLE001  (reported by the assertion below)
            failures.append((want, repr(e)))

    threads = [threading.Thread(target=work, args=(_row_loop_engine(X, y, th, on), want)) for on, want in ((0, 4), (2, 2))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
