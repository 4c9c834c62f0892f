"""
GPU tests of ``gpso_predict_joint`` and ``gpso_sample_joint`` (the joint predictive: full covariance, draws and their
arg-max) through the C-ABI, against the float64 oracle of tests/joint_oracle.py.

Problems as tests/test_gpu_predict_grad.py builds them (its ``reference``): ``synthetic_problem``, variance 1.3, ARD
lengthscales 0.25 sqrt(D) linspace(0.8, 1.3, D), noise 1e-3 and 1e-1, test points uniform on [-0.2, 1.2]^D; float64 and mixed
engines (the call reads the dense double factor on both).

Stated tolerances (the project's own for float64 stages, as that file states them)
  mean ............ 1e-8 max|y|
  every entry of cov 1e-8 of the kernel variance; cov == cov.T to the bit
  Matern-1/2 ...... 1e-4 on both (the sqrt at r = 0 amplifies the rounding of r^2, which the oracle's Gram and the device's
                    form differently)
  the factor ...... Z = I makes samples - mean the rows of L^T: lower triangular, positive diagonal, and L L^T reproduces
                    the oracle's cov + diag_add I to the covariance tolerance -- the factor is unique, so this pins L whatever
                    the spectrum
  draws ........... generic Z (noise 1e-1 cases: lambda_min >= 0.1): the mean's tolerance + |dL|_F |z|_2 with the first-order
                    bound |dL|_F <= sqrt(lambda_max) M delta / (sqrt 2 lambda_min), delta the covariance tolerance, lambda
                    the eigenvalues of the ORACLE's cov + diag_add I (tests/joint_oracle.py: chol_perturbation_bound)
  installed forms . diag(cov) + noise against gpso_predict's variance on the same float64 context 1e-9 by max(1, |.|)
Shapes, the smallest that reach every path: N = 2 one row; 17 a partial 16-tile; 129 two row blocks with padding; 300 three
row blocks -- three splits of the contraction at every M here (joint_splits: one row block a split up to 16 splits); D = 26
gives D_pad = 28.  M = 1 and 17 a partial tile, 16, 64 exactly one, 65 an off-diagonal tile pair with a 1-point tile, 130 three
tiles and a Cholesky padded to 256; M = 1024 (136 tile pairs) once at N = 129, 1025 refused.  Stale rows of V: a mixed
context (N_pad a multiple of 256) fitted at N = 500, then at N = 300 -- rows 384 .. 511 of V are the first problem's.
The achieved maxima are recorded in profiles/joint_parity.json by tools/joint_errors.py.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import gpr
from tests import joint_oracle as jo
from tests import test_gpu_predict_grad as PG
from tests.helpers import synthetic_problem

pytestmark = pytest.mark.gpu

KERNELS = PG.KERNELS
SHAPES = [(2, 1), (17, 3), (129, 3), (300, 5), (40, 26)]
NOISES = (1.0e-3, 1.0e-1)
MS = (1, 16, 17, 64, 65, 130)
DTYPES = ("float64", "mixed")
JITTER = 1.0e-6
LIMIT = 1024  # kPredictGradChunk


def tolerance(kernel):
    return 1.0e-4 if kernel == "Matern12" else 1.0e-8


_joint_cache = {}


def reference(n, d, kernel, noise):
    """tests/test_gpu_predict_grad.py's case (ARD) with the oracle's joint predictive of the latent f at max(MS) points;
    computed once per case and shared (never modified)."""
    key = (n, d, kernel, noise)
    if key not in _joint_cache:
        r = PG.reference(n, d, True, kernel, noise)
        mean, cov = jo.gpr_predict_joint(r["post"], r["Xs"][:max(MS)], 0.0)
        _joint_cache[key] = dict(r, mean=mean, cov=cov)
    return _joint_cache[key]


def with_diag(cov, diag_add):
    out = cov.copy()
    out[np.diag_indices(out.shape[0])] += diag_add
    return out


def joint_errors(got, mean, cov, r):
    return dict(mean=float(np.max(np.abs(got[0] - mean)) / np.max(np.abs(r["y"]))),
                cov=float(np.max(np.abs(got[1] - cov)) / r["th"].variance))


def _hold(errs, tol, what):
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= tol, (what, k, v, tol)


# ---- 1. parity with the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_parity_with_the_oracle(n, d, kernel):
    tol = tolerance(kernel)
    for noise in NOISES:
        r = reference(n, d, kernel, noise)
        for dtype in DTYPES:
            eng = PG.fitted(r, dtype)
            for m in MS:
                Xs = r["Xs"][:m]
                what = f"N={n} D={d} {kernel} noise {noise:g} s={'yes' if r['s'] is not None else 'no'} {dtype} M={m}"
                mean, cov = eng.predict_joint(Xs)
                assert mean.shape == (m,) and cov.shape == (m, m)
                assert np.array_equal(cov, cov.T), what
                _hold(joint_errors((mean, cov), r["mean"][:m], r["cov"][:m, :m], r), tol, "predict_joint " + what)
                # with the noise on the diagonal: the marginals of gpso_predict_grad on the same context
                mean_y, cov_y = eng.predict_joint(Xs, noise)
                _, var, _, _ = eng.predict_grad(Xs)
                off = ~np.eye(m, dtype=bool)
                assert np.array_equal(mean_y, mean) and np.array_equal(cov_y[off], cov[off])
                e = float(np.max(np.abs(np.diag(cov_y) - var)) / r["th"].variance)
                print(f"diagonal against gpso_predict_grad {what}: {e:.2e}")
                assert e <= tol, (what, e)
            eng.close()


def test_the_largest_batch():
    """M = 1024 at N = 129: sixteen tiles, 136 tile pairs, two splits; the draws' factor at the full size too."""
    r = PG.reference(129, 3, True, "Matern52", 1.0e-1)
    Xs = PG.points_at(LIMIT, 3, seed=8)
    mean, cov = jo.gpr_predict_joint(r["post"], Xs, 0.0)
    eng = PG.fitted(r)
    got = eng.predict_joint(Xs)
    assert np.array_equal(got[1], got[1].T)
    _hold(joint_errors(got, mean, cov, r), tolerance("Matern52"), f"predict_joint N=129 M={LIMIT}")
    z = np.random.default_rng(2).standard_normal((3, LIMIT))
    f, idx, val = eng.sample_joint(Xs, z, 1.0e-1)
    want = jo.draws(mean, with_diag(cov, 1.0e-1), z)
    bound = 1.0e-8 * np.max(np.abs(r["y"])) + jo.chol_perturbation_bound(with_diag(cov, 1.0e-1), 1.0e-8 * r["th"].variance) * \
        np.linalg.norm(z, axis=1)
    err = np.max(np.abs(f - want), axis=1)
    print(f"draws M={LIMIT}: max error {err.max():.2e}, bound {bound.min():.2e}")
    assert np.all(err <= bound)
    assert np.array_equal(idx, np.argmax(f, axis=1)) and np.array_equal(val, np.max(f, axis=1))


# ---- 2. the Cholesky, pinned by Z = I ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", SHAPES)
def test_identity_draws_are_the_factor(n, d):
    tol = tolerance("Matern52")
    for noise in NOISES:
        r = reference(n, d, "Matern52", noise)
        for dtype in DTYPES:
            eng = PG.fitted(r, dtype)
            for m in MS:
                Xs = r["Xs"][:m]
                mean, _ = eng.predict_joint(Xs)
                for diag_add, of in ((JITTER, "f + jitter"), (noise, "y")):
                    what = f"N={n} D={d} noise {noise:g} {dtype} M={m} {of}"
                    f, _, _ = eng.sample_joint(Xs, np.eye(m), diag_add)
                    Lt = f - mean[None, :]  # row s: column s of L
                    Lf = Lt.T
                    assert np.all(np.triu(Lf, 1) == 0.0), what
                    assert np.all(np.diag(Lf) > 0.0), what
                    e = float(np.max(np.abs(Lf @ Lf.T - with_diag(r["cov"][:m, :m], diag_add))) / r["th"].variance)
                    print(f"L L^T against the oracle {what}: {e:.2e}")
                    assert e <= tol, (what, e)
            eng.close()


# ---- 3. draws for generic normals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", SHAPES)
def test_draws_for_seeded_normals(n, d):
    noise, s = 1.0e-1, 7
    r = reference(n, d, "Matern52", noise)
    ymax, variance = np.max(np.abs(r["y"])), r["th"].variance
    for dtype in DTYPES:
        eng = PG.fitted(r, dtype)
        for m in MS:
            Xs = r["Xs"][:m]
            z = np.random.default_rng(100 + m).standard_normal((s, m))
            cov = with_diag(r["cov"][:m, :m], noise)
            want = jo.draws(r["mean"][:m], cov, z)
            bound = tolerance("Matern52") * ymax + jo.chol_perturbation_bound(cov, tolerance("Matern52") * variance) * \
                np.linalg.norm(z, axis=1)
            f, idx, val = eng.sample_joint(Xs, z, noise)
            assert f.shape == (s, m) and idx.shape == (s,) and val.shape == (s,)
            err = np.max(np.abs(f - want), axis=1)
            print(f"draws N={n} D={d} {dtype} M={m}: max error {err.max():.2e}, smallest bound {bound.min():.2e}")
            assert np.all(err <= bound), (n, d, dtype, m, err, bound)
            # the winners are those of the returned draws, to the bit, with and without the draws leaving the device
            assert np.array_equal(idx, np.argmax(f, axis=1)) and np.array_equal(val, np.max(f, axis=1))
            none, idx2, val2 = eng.sample_joint(Xs, z, noise, want_samples=False)
            assert none is None and np.array_equal(idx2, idx) and np.array_equal(val2, val)
        eng.close()


def test_ties_go_to_the_lowest_index_and_duplicated_points_factor_with_jitter():
    """Every test point twice and z = 0: a draw is the mean, whose bits at a point and at its copy are the same -- the
    arg-max is the first of the pair.  The duplicated rows make cov singular: with the jitter the factor exists and every
    draw is finite (no failure is asserted WITHOUT jitter: the sign of a zero pivot is rounding)."""
    r = reference(129, 3, "Matern52", 1.0e-3)
    eng = PG.fitted(r)
    P = r["Xs"][:70]
    Xs = np.vstack([P, P])
    f, idx, val = eng.sample_joint(Xs, np.zeros((2, 140)), JITTER)
    mean, _ = eng.predict_joint(Xs)
    assert np.array_equal(f[0], mean) and np.array_equal(f[1], mean) and np.array_equal(mean[:70], mean[70:])
    assert idx[0] == idx[1] == int(np.argmax(mean)) and idx[0] < 70 and val[0] == mean[idx[0]]
    z = np.random.default_rng(9).standard_normal((5, 140))
    f, idx, val = eng.sample_joint(Xs, z, JITTER)
    assert np.all(np.isfinite(f)) and np.array_equal(idx, np.argmax(f, axis=1)) and np.array_equal(val, np.max(f, axis=1))


# ---- 4. determinism, history, purity -----------------------------------------------------------------------------------------
def test_same_bits_again_and_nothing_else_moves():
    r = reference(300, 5, "Matern52", 1.0e-3)
    eng = PG.fitted(r)
    Xs = r["Xs"][:130]
    z = np.random.default_rng(1).standard_normal((4, 130))
    h0, p0 = eng.posterior_hash(), eng.predict(Xs)
    a, b = eng.predict_joint(Xs), eng.predict_joint(Xs)
    sa, sb = eng.sample_joint(Xs, z, JITTER), eng.sample_joint(Xs, z, JITTER)
    for x, y_ in zip(a + sa, b + sb):
        assert np.array_equal(x, y_)
    assert eng.posterior_hash() == h0
    p1 = eng.predict(Xs)
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])


def _history_against_fresh(dtype, sizes, X, y, th, Xs, z):
    used = PG._engine(dtype)
    for n in sizes:
        used.set_data(X[:n], y[:n])
        used.fit_eval(*th, want_grad=False)
        got = used.predict_joint(Xs) + used.sample_joint(Xs, z, JITTER)
    n = sizes[-1]
    fresh = PG._engine(dtype)
    fresh.set_data(X[:n], y[:n])
    fresh.fit_eval(*th, want_grad=False)
    for a, b in zip(got, fresh.predict_joint(Xs) + fresh.sample_joint(Xs, z, JITTER)):
        assert np.array_equal(a, b)


def test_a_smaller_problem_after_a_larger_one_gives_a_fresh_contexts_bits():
    """N = 300, then N = 17 on the same float64 context: N_pad falls from 384 to 128, the factor, alpha, the scaled rows and
    every workspace keep the larger problem's contents behind the smaller one's.  (V itself is laid out anew by N_pad = 128
    and written whole here: the case that leaves stale ROWS of V is the next test's.)"""
    X, y = synthetic_problem(300, 5, seed=3)
    th = ("Matern52", [0.6], 1.3, 1.0e-3, float(y.mean()))
    _history_against_fresh("float64", (300, 17), X, y, th, PG.points_at(130, 5), np.random.default_rng(1).standard_normal((3, 130)))


def test_stale_rows_of_v_are_never_read():
    """The stale-row rule.  A mixed context pads N > 128 to a multiple of 256: N = 500 and N = 300 both have N_pad = 512, so V
    keeps its layout [tile][512][64].  The first fit's calls write all 512 rows of every tile; after the second fit pg_apply
    writes rows 0 .. 383 = ceil(300 / 128) * 128 and rows 384 .. 511 still hold the V of the 500-point problem for the same
    130 test points.  A contraction that ran to N_pad would add their products; the bits must be a fresh context's."""
    X, y = synthetic_problem(500, 5, seed=3)
    th = ("Matern52", [0.6], 1.3, 1.0e-3, float(y.mean()))
    used = PG._engine("mixed")
    used.set_data(X, y)
    assert used.padded_n == 512
    used.close()
    _history_against_fresh("mixed", (500, 300), X, y, th, PG.points_at(130, 5), np.random.default_rng(1).standard_normal((3, 130)))


def test_device_float32_points_and_device_outputs_equal_the_host_path():
    import torch

    r = reference(129, 3, "SquaredExponential", 1.0e-3)
    eng = PG.fitted(r)
    xs32 = r["Xs"][:100].astype(np.float32)
    host = eng.predict_joint(xs32, 0.25)
    assert np.array_equal(host[0], eng.predict_joint(xs32.astype(np.float64), 0.25)[0])  # (the same values as float64)
    dev = torch.device("cuda", eng.device)
    xt = torch.from_numpy(xs32).to(dev)
    out = (torch.empty(100, dtype=torch.float64, device=dev), torch.full((100, 100), np.nan, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    eng.predict_joint(xt, 0.25, out=out)
    assert np.array_equal(host[0], out[0].cpu().numpy()) and np.array_equal(host[1], out[1].cpu().numpy())
    # the mean is nullable; device points with host outputs, and draws from device points, are the same bits too
    cov_only = torch.empty(100, 100, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.predict_joint(xt, 0.25, out=(None, cov_only))
    assert np.array_equal(host[1], cov_only.cpu().numpy())
    mixed = eng.predict_joint(xt, 0.25)
    assert np.array_equal(host[0], mixed[0]) and np.array_equal(host[1], mixed[1])
    z = np.random.default_rng(4).standard_normal((3, 100))
    for a, b in zip(eng.sample_joint(xs32, z, 0.25), eng.sample_joint(xt, z, 0.25)):
        assert np.array_equal(a, b)


def test_timing_covers_the_call():
    eng = PG.fitted(reference(129, 3, "Matern52", 1.0e-3))
    eng.set_timing(True)
    eng.predict(PG.points_at(7, 3))
    eng.predict_joint(PG.points_at(130, 3))
    assert eng.last_ms(1) > 0.0 and eng.last_count(0) == 130 and eng.last_count(1) == 130
    eng.sample_joint(PG.points_at(65, 3), np.zeros((2, 65)), JITTER)
    assert eng.last_ms(1) > 0.0 and eng.last_count(0) == 65 and eng.last_count(1) == 65


# ---- 5. the failure path and the refusals ---------------------------------------------------------------------------------------
def _joint_code(eng, Xs, diag_add=0.0):
    from pygpso_amd import _lib as L

    xs = np.ascontiguousarray(Xs, dtype=np.float64)
    m = xs.shape[0]
    mean, cov = np.empty(max(m, 1)), np.empty(max(m * m, 1))
    return eng._lib.gpso_predict_joint(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, m, diag_add,
                                       C.c_void_p(mean.ctypes.data), C.c_void_p(cov.ctypes.data), L.MEM_HOST)


def _sample_code(eng, Xs, s, diag_add=JITTER):
    from pygpso_amd import _lib as L

    xs = np.ascontiguousarray(Xs, dtype=np.float64)
    m = xs.shape[0]
    z = np.zeros(max(s * m, 1))
    f, idx, val = np.empty(max(s * m, 1)), np.empty(max(s, 1), dtype=np.int64), np.empty(max(s, 1))
    return eng._lib.gpso_sample_joint(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, m, diag_add, L.dptr(z), s,
                                      L.dptr(f), L.i64ptr(idx), L.dptr(val))


def _too_many_draws_code(eng, Xs):
    """s = 2^20 + 1 with buffers for ONE draw: the call must be refused before it reads z or writes an output."""
    from pygpso_amd import _lib as L

    xs = np.ascontiguousarray(Xs, dtype=np.float64)
    m = xs.shape[0]
    z, f, idx, val = np.zeros(m), np.empty(m), np.empty(1, dtype=np.int64), np.empty(1)
    return eng._lib.gpso_sample_joint(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, m, JITTER, L.dptr(z), 2 ** 20 + 1,
                                      L.dptr(f), L.i64ptr(idx), L.dptr(val))


def _message(eng):
    return eng._lib.gpso_last_error(eng._h).decode()


def test_a_failing_pivot_is_reported_and_the_posterior_still_predicts():
    from pygpso_amd import _lib as L

    r = reference(129, 3, "Matern52", 1.0e-3)
    eng = PG.fitted(r)
    Xs = r["Xs"][:65]
    p0, j0 = eng.predict(Xs), eng.predict_joint(Xs)
    assert _sample_code(eng, Xs, 2, diag_add=-2.0 * r["th"].variance) == L.E_NOTPD
    msg = _message(eng)
    assert "pivot 0" in msg and "diag_add" in msg and "jitter" in msg
    with pytest.raises(np.linalg.LinAlgError):
        eng.sample_joint(Xs, np.zeros((2, 65)), -2.0 * r["th"].variance)
    p1, j1 = eng.predict(Xs), eng.predict_joint(Xs)
    for a, b in zip(p0 + j0, p1 + j1):
        assert np.array_equal(a, b)
    f, _, _ = eng.sample_joint(Xs, np.zeros((1, 65)), JITTER)
    assert np.array_equal(f[0], j0[0])


def test_refusals_and_the_context_works_afterwards():
    from pygpso_amd import _lib as L
    from tests.test_gpu_distributed import _handoff

    r = reference(129, 3, "Matern52", 1.0e-3)
    Xs = r["Xs"][:20]
    # a float32 context
    e32 = PG.fitted(r, "float32")
    assert _joint_code(e32, Xs) == L.E_ARG and '"float64"' in _message(e32) and '"mixed"' in _message(e32)
    assert _sample_code(e32, Xs, 2) == L.E_ARG and '"float64"' in _message(e32)
    with pytest.raises(ValueError):
        e32.predict_joint(Xs)
    e32.predict(Xs)
    # no posterior
    eng = PG._engine()
    eng.set_data(r["X"], r["y"])
    assert _joint_code(eng, Xs) == L.E_STATE and _sample_code(eng, Xs, 2) == L.E_STATE
    th = r["th"]
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    want = eng.predict_joint(Xs) + eng.sample_joint(Xs, np.ones((2, 20)), JITTER)
    # an open best-UCB ticket
    ticket = eng.best_ucb_begin(r["Xs"], gpr.VARSIGMA_DEFAULT)
    assert _joint_code(eng, Xs) == L.E_STATE and "best-UCB" in _message(eng)
    assert _sample_code(eng, Xs, 2) == L.E_STATE
    eng.best_ucb_end(ticket)
    # m = 0, m = 1025, s = 0
    assert _joint_code(eng, np.empty((0, 3))) == L.E_ARG and "m=0" in _message(eng)
    assert _sample_code(eng, np.empty((0, 3)), 2) == L.E_ARG
    big = PG.points_at(LIMIT + 1, 3)
    assert _joint_code(eng, big) == L.E_ARG and "m=1025" in _message(eng)
    assert _sample_code(eng, big, 1) == L.E_ARG
    assert _sample_code(eng, Xs, 0) == L.E_ARG and "s=0" in _message(eng)
    assert _too_many_draws_code(eng, Xs) == L.E_ARG and f"s={2 ** 20 + 1}" in _message(eng)  # (refused before z is read)
    # nothing is left in flight: the same bits as before the refusals
    for a, b in zip(want, eng.predict_joint(Xs) + eng.sample_joint(Xs, np.ones((2, 20)), JITTER)):
        assert np.array_equal(a, b)
    # an adopted posterior (the hand-off replayed with plain copies)
    dst = PG._engine()
    _handoff(eng, dst)
    assert _joint_code(dst, Xs) == L.E_STATE and "adopted" in _message(dst)
    assert _sample_code(dst, Xs, 2) == L.E_STATE
    m0, v0 = eng.predict(Xs)
    m1, v1 = dst.predict(Xs)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


# ---- 6. installed posteriors --------------------------------------------------------------------------------------------------
def _installed_agrees(eng, rows, th, y, what):
    """diag(cov) + noise against gpso_predict's variance (1e-9 by max(1, |.|)) -- the noise the installed predictive adds
    read off gpso_predict itself at a point far from every row, where var = variance + noise --, the mean against
    gpso_predict's, and every entry against the oracle fed with C and alpha read back from the device."""
    from pygpso_amd import _lib as L

    Xs = PG.points_at(40, 3)
    far = np.full((1, 3), 1.0e6)
    noise = float(eng.predict(far)[1][0]) - th.variance
    mean, cov = eng.predict_joint(Xs)
    m0, v0 = eng.predict(Xs)
    e = dict(mean=float(np.max(np.abs(mean - m0) / np.maximum(1.0, np.abs(m0)))),
             var=float(np.max(np.abs(np.diag(cov) + noise - v0) / np.maximum(1.0, np.abs(v0)))))
    _hold(e, 1e-9, what + " against gpso_predict")
    assert np.array_equal(cov, cov.T)
    Cm, alpha = eng.get_matrix(L.MAT_LINV), eng.get_vector(L.VEC_ALPHA)
    want = jo.predictive_joint(np.tril(Cm), alpha, rows, th, Xs, 0.0)
    scale = dict(y=y, th=th)
    _hold(joint_errors((mean, cov), want[0], want[1], scale), 1e-8, what + " against the oracle on the device's C and alpha")


def test_after_a_vgp_posterior():
    from tests import vgp_oracle as V

    X, y = synthetic_problem(60, 3, seed=4)
    u = V.initial_u(0.3 * np.sqrt(3), 1.1, 0.01, 0.05)
    eng = PG._engine()
    eng.set_data(X, y)
    eng.vgp_set_q()
    eng.vgp_natgrad("Matern52", u, 1, True, 0.0, 0.5)
    eng.vgp_posterior("Matern52", u, 1, True, 0.0)
    _installed_agrees(eng, X, gpr.Theta("Matern52", [0.3 * np.sqrt(3)], 1.1, 0.01, 0.05), y, "VGP posterior")


def test_after_an_sgpr_posterior():
    from tests import sgpr_oracle as S

    X, y = synthetic_problem(60, 3, seed=6)
    Z = S.choose_inducing("Matern52", X, 0.3 * np.sqrt(3), 1.1, 20)
    eng = PG._sparse_engine(None)
    u = S.initial_u(0.3 * np.sqrt(3), 1.1, 0.02, 0.15)
    eng.sgpr_bound_u("Matern52", u, 1, True, 0.0, want_grad=False)
    eng.sgpr_posterior("Matern52", u, 1, True, 0.0)
    assert eng.n == 20
    _installed_agrees(eng, Z, gpr.Theta("Matern52", [0.3 * np.sqrt(3)], 1.1, 0.02, 0.15), y, "SGPR posterior (M = 20, N = 60)")


def test_after_an_svgp_posterior():
    from tests import sgpr_oracle as S
    from tests import svgp_oracle as O
    from tests import vgp_studentt_oracle as T

    X, y = synthetic_problem(60, 3, seed=6)
    Z = S.choose_inducing("Matern52", X, 0.3 * np.sqrt(3), 1.1, 20)
    lik = ("StudentT", 4.0)
    eng = PG._sparse_engine((lik[0], lik[1], T.N_GH))
    u = O.initial_u(0.3 * np.sqrt(3), 1.1, 0.3, lik, c=0.05)
    eng.svgp_init_q("Matern52", u, 1, True, 0.0, 0.3 ** 2 * 2.0)
    eng.svgp_natgrad("Matern52", u, 1, True, 0.0, 0.5)
    eng.svgp_posterior("Matern52", u, 1, True, 0.0)
    _installed_agrees(eng, Z, gpr.Theta("Matern52", [0.3 * np.sqrt(3)], 1.1, 0.18, 0.05), y, "SVGP posterior (Student-t)")


# ---- 7. through the classes -----------------------------------------------------------------------------------------------------
def test_through_the_model_and_the_surrogate():
    from pygpso_amd import GPRSurrogate
    from pygpso_amd import kernels as K
    from pygpso_amd.model import HipGPR

    X, y = synthetic_problem(40, 3, seed=4)
    model = HipGPR((X, y[:, None]), K.Matern52(lengthscales=0.5, variance=1.1), K.Constant(0.05), noise_variance=0.02)
    post = gpr.posterior(gpr.Theta("Matern52", [0.5], 1.1, 0.02, 0.05), X, y)
    Xs = PG.points_at(5, 3)
    want = jo.gpr_predict_joint(post, Xs, 0.0)
    mean, cov = model.predict_f(Xs, full_cov=True)
    assert mean.shape == (5, 1) and cov.shape == (5, 5) and np.array_equal(cov, cov.T)
    assert np.max(np.abs(np.asarray(mean)[:, 0] - want[0])) <= 1e-8 * np.max(np.abs(y)) and np.max(np.abs(cov - want[1])) <= 1e-8 * 1.1
    _, cov_y = model.predict_y(Xs, full_cov=True)
    assert np.max(np.abs(cov_y - with_diag(want[1], 0.02))) <= 1e-8 * 1.1
    mean_f, var_f = model.predict_f(Xs)  # (the default path: the marginals it always returned)
    assert var_f.shape == (5, 1) and np.max(np.abs(np.asarray(var_f)[:, 0] - np.diag(cov))) <= 1e-8 * 1.1
    # draws: reproducible from a seed; the empirical mean of 4000 within five standard errors of the mean
    a, b = model.predict_f_samples(Xs, 3, rng=7), model.predict_f_samples(Xs, 3, rng=np.random.default_rng(7))
    assert a.shape == (3, 5) and np.array_equal(a, b)
    f = model.predict_f_samples(Xs, 4000, rng=1)
    se = np.sqrt((np.diag(want[1]) + JITTER) / 4000.0)
    print("empirical mean over 4000 draws, in standard errors:", np.abs(f.mean(axis=0) - want[0]) / se)
    assert np.all(np.abs(f.mean(axis=0) - want[0]) <= 5.0 * se)
    # the surrogate: Thompson's arg-max per draw is gp_sample's for the same seed
    coords = np.random.default_rng(5).random((30, 2))
    scores = np.sin(3.0 * coords[:, 0]) + coords[:, 1] ** 2
    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy())
    surr.append(coords, scores)
    surr.gp_update()
    cand = np.random.default_rng(6).random((65, 2))
    stored = list(surr.points)
    draws = surr.gp_sample(cand, 8, rng=3)
    idx, val = surr.thompson_select(cand, 8, rng=3)
    assert draws.shape == (8, 65) and np.array_equal(idx, np.argmax(draws, axis=1)) and np.array_equal(val, np.max(draws, axis=1))
    m_j, c_j = surr.gp_predict_joint(cand)
    assert m_j.shape == (65,) and c_j.shape == (65, 65) and np.array_equal(c_j, c_j.T)
    assert list(surr.points) == stored
