"""
Multi-start hyper-parameter search on the device: ``gpso_fit_eval_u_batch`` (one launch, one workgroup per theta) against
``gpso_fit_eval_u`` on the same context -- bit for bit -- and against the CPU oracle; the context it must leave alone; failed
entries; limits; and ``Scipy(restarts=R)`` end to end.  Through the C-ABI.  Run on the GPU box with ``pytest -m gpu``.

Stated tolerances (float64 fit, the bounds of tests/test_gpu_parity.py): NLML 1e-9 relative, gradient 1e-7 of max(1, |g|)
(Matern12, as there: 1e-5 / 1e-4 -- its sqrt at r = 0 amplifies the rounding noise of the GEMM-form r^2 on the diagonal).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import gpr
from tests.helpers import synthetic_leaves, synthetic_problem
from tests.multistart_problem import KERNEL, THETA0, oracle_multistart, problem

pytestmark = pytest.mark.gpu

KERNELS = ["Matern52", "Matern32", "Matern12", "SquaredExponential"]


def _engine(dtype="float64"):
    from pygpso_amd import HipGPEngine

    return HipGPEngine(dtype)


def _u_rows(b, d, n_ls, train_mean, seed, y_mean=0.0):
    """b unconstrained vectors around a sane theta (lengthscale 0.25 sqrt(D), variance 1.3, noise 1e-2)."""
    rng = np.random.default_rng(seed)
    nu = n_ls + 2 + (1 if train_mean else 0)
    centre = np.concatenate([np.full(n_ls, gpr.softplus_inv(0.25 * np.sqrt(d))), [gpr.softplus_inv(1.3)],
                             [gpr.softplus_inv(1.0e-2)], [y_mean] if train_mean else []])
    return np.ascontiguousarray(centre + 0.3 * rng.standard_normal((b, nu)))


def _single(eng, kid, u, n_ls, train_mean, c):
    """gpso_fit_eval_u at u: (rc, loss, grad_u)."""
    from pygpso_amd import _lib as L

    u = np.ascontiguousarray(u, dtype=np.float64)
    f, g = C.c_double(np.nan), np.full(u.shape[0], np.nan)
    rc = eng._lib.gpso_fit_eval_u(eng._h, kid, L.dptr(u), n_ls, 1 if train_mean else 0, float(c), C.byref(f), L.dptr(g), None)
    return rc, f.value, g


def _batch(eng, kid, U, n_ls, train_mean, c, b=None):
    """gpso_fit_eval_u_batch at the rows of U: (rc, loss, grad_u, status, pivot)."""
    from pygpso_amd import _lib as L

    U = np.ascontiguousarray(U, dtype=np.float64)
    b = U.shape[0] if b is None else b
    f, g = np.full(U.shape[0], np.nan), np.full(U.shape, np.nan)
    st, pv = np.full(U.shape[0], 99, dtype=np.intc), np.full(U.shape[0], -7, dtype=np.int64)
    rc = eng._lib.gpso_fit_eval_u_batch(eng._h, kid, L.dptr(U), b, n_ls, 1 if train_mean else 0, float(c), L.dptr(f),
                                        L.dptr(g), st.ctypes.data_as(C.POINTER(C.c_int)),
                                        pv.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, f, g, st, pv


def _assert_bits(eng, kid, U, n_ls, train_mean, c, sizes):
    """Entries of batches of the given sizes (prefixes of U) equal the single calls on the same context, bit for bit."""
    from pygpso_amd import _lib as L

    singles = [_single(eng, kid, u, n_ls, train_mean, c) for u in U]
    assert all(rc == L.OK for rc, _, _ in singles)
    f_ref = np.array([f for _, f, _ in singles])
    g_ref = np.stack([g for _, _, g in singles])
    for b in sizes:
        rc, f, g, st, _ = _batch(eng, kid, U[:b], n_ls, train_mean, c)
        assert rc == L.OK, eng.last_message()
        assert np.all(st == L.OK)
        assert f.tobytes() == f_ref[:b].tobytes(), (b, np.flatnonzero(f != f_ref[:b])[:4])
        assert g.tobytes() == g_ref[:b].tobytes(), (b, np.argwhere(g != g_ref[:b])[:4])


@pytest.mark.parametrize("n,d", [(5, 2), (5, 12), (64, 2), (64, 12), (65, 2), (65, 12), (128, 2), (128, 12)])
def test_batch_entries_are_the_single_calls_bit_for_bit_fp64(n, d):
    """N = 5, 64, 65, 128: the edges of the one- and two-block algebra; every kernel, isotropic and ARD, trained and fixed
    mean, B = 1, 3 and 256 (the launch's limit)."""
    from pygpso_amd import _lib as L

    X, y = synthetic_problem(n, d, seed=n + d)
    eng = _engine()
    eng.set_data(X, y)
    assert eng.fit_batch_max() == 256
    for k, kernel in enumerate(KERNELS):
        for n_ls in (1, d):
            for train_mean in (True, False):
                U = _u_rows(256, d, n_ls, train_mean, seed=1000 * n + 10 * d + k, y_mean=float(y.mean()))
                _assert_bits(eng, L.KERNEL_IDS[kernel], U, n_ls, train_mean, 0.1, (1, 3, 256))
    eng.close()


@pytest.mark.parametrize("dtype", ["float32", "mixed"])
@pytest.mark.parametrize("n", [5, 128])
def test_batch_entries_are_the_single_calls_bit_for_bit_float_contexts(dtype, n):
    """The one-launch fit computes in double in LDS whatever the context's matrix type, and its loss and gradient are
    formed from the double values: the batch is bit-identical on float32 and mixed contexts too."""
    from pygpso_amd import _lib as L

    d = 12
    X, y = synthetic_problem(n, d, seed=3)
    eng = _engine(dtype)
    eng.set_data(X, y)
    for n_ls in (1, d):
        U = _u_rows(256, d, n_ls, True, seed=n + n_ls, y_mean=float(y.mean()))
        _assert_bits(eng, L.MATERN52, U, n_ls, True, 0.0, (1, 3, 256))
    eng.close()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,d,ard", [(5, 2, False), (64, 12, True), (65, 2, True), (128, 12, False), (100, 12, True)])
def test_batch_entries_against_the_oracle(kernel, n, d, ard):
    from pygpso_amd import _lib as L

    tol_f, tol_g = (1e-5, 1e-4) if kernel == "Matern12" else (1e-9, 1e-7)
    X, y = synthetic_problem(n, d, seed=7)
    n_ls = d if ard else 1
    U = _u_rows(5, d, n_ls, True, seed=n + d, y_mean=float(y.mean()))
    eng = _engine()
    eng.set_data(X, y)
    rc, f, g, st, _ = _batch(eng, L.KERNEL_IDS[kernel], U, n_ls, True, 0.0)
    assert rc == L.OK and np.all(st == L.OK)
    for b, u in enumerate(U):
        f_ref, g_ref = gpr.loss_and_grad_unconstrained(kernel, u, X, y)
        assert abs(f[b] - f_ref) <= tol_f * abs(f_ref), (b, f[b], f_ref)
        assert np.max(np.abs(g[b] - g_ref) / np.maximum(1.0, np.abs(g_ref))) <= tol_g, (b, g[b], g_ref)
    eng.close()


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_the_batch_leaves_the_context_alone(dtype):
    from pygpso_amd import _lib as L

    n, d = 100, 6
    X, y = synthetic_problem(n, d, seed=0)
    leaves = synthetic_leaves(64, d, seed=1)
    th = gpr.Theta("Matern52", 0.25 * np.sqrt(d), 1.0, 1.0e-3, float(y.mean()))
    eng = _engine(dtype)
    eng.set_data(X, y)
    f0, _ = eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    h0 = eng.posterior_hash()
    mean0, var0 = eng.predict(leaves)
    ucb0 = eng.best_ucb(leaves, gpr.VARSIGMA_DEFAULT)
    U = _u_rows(8, d, 1, True, seed=5, y_mean=float(y.mean()))
    rc, f, _, st, _ = _batch(eng, L.MATERN32, U, 1, True, 0.0)
    assert rc == L.OK and np.all(st == L.OK) and np.all(np.isfinite(f))
    assert eng.posterior_hash() == h0
    mean1, var1 = eng.predict(leaves)  # (no refit: the posterior of theta* is still the resident one)
    assert mean1.tobytes() == mean0.tobytes() and var1.tobytes() == var0.tobytes()
    ucb1 = eng.best_ucb(leaves, gpr.VARSIGMA_DEFAULT)
    for a, b in zip(ucb0, ucb1):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    if dtype == "float64":
        i_ref, mu_ref, var_ref, ucb_ref = gpr.best_ucb(gpr.posterior(th, X, y), leaves)
        assert int(ucb1[0][0]) == i_ref and abs(ucb1[3][0] - ucb_ref) < 1e-9
    eng.close()


def test_failed_entries_are_statuses_and_the_others_keep_their_bits():
    from pygpso_amd import _lib as L

    n, d, n_ls = 40, 3, 1
    X, y = synthetic_problem(n, d, seed=2)
    # (a) NaN in one entry's variance slot, beside ordinary entries
    eng = _engine()
    eng.set_data(X, y)
    U = _u_rows(6, d, n_ls, True, seed=9, y_mean=float(y.mean()))
    U[2, n_ls] = np.nan
    singles = [_single(eng, L.MATERN52, u, n_ls, True, 0.0) for u in U]
    assert singles[2][0] < 0  # the NaN entry does fail in the single call
    rc, f, g, st, pv = _batch(eng, L.MATERN52, U, n_ls, True, 0.0)
    assert rc == L.OK
    assert "entry 2" in eng.last_message()
    for b, (rc1, f1, g1) in enumerate(singles):
        assert st[b] == rc1, (b, st[b], rc1)
        if rc1 == L.OK:
            assert np.float64(f[b]).tobytes() == np.float64(f1).tobytes() and g[b].tobytes() == g1.tobytes()
        else:
            assert np.isnan(f[b]) and np.all(np.isnan(g[b]))
    assert [int(s) for s in st] == [L.OK, L.OK, st[2], L.OK, L.OK, L.OK]
    eng.close()
    # (b) data with a duplicated row; one entry at u_variance = 1e13 (K + noise I = 1e13 (ones) + O(1e-2) there)
    Xd, yd = np.vstack([X, X[7]]), np.concatenate([y, y[7:8]])
    eng = _engine()
    eng.set_data(Xd, yd)
    U = _u_rows(5, d, n_ls, True, seed=10, y_mean=float(y.mean()))
    U[3, n_ls] = 1.0e13
    singles = [_single(eng, L.MATERN52, u, n_ls, True, 0.0) for u in U]
    rc, f, g, st, pv = _batch(eng, L.MATERN52, U, n_ls, True, 0.0)
    assert rc == L.OK
    for b, (rc1, f1, g1) in enumerate(singles):
        assert st[b] == rc1, (b, st[b], rc1)
        if rc1 == L.OK:
            assert np.float64(f[b]).tobytes() == np.float64(f1).tobytes() and g[b].tobytes() == g1.tobytes()
            assert pv[b] == -1
        else:
            assert rc1 == L.E_NOTPD and np.isnan(f[b]) and 0 <= pv[b] <= n
    assert all(singles[b][0] == L.OK for b in (0, 1, 2, 4))
    eng.close()


def test_limits():
    from pygpso_amd import _lib as L

    def ctx(n, d):
        X, y = synthetic_problem(n, d, seed=4)
        e = _engine()
        assert e.fit_batch_max() == 0  # no data yet
        e.set_data(X, y)
        return e, X, y

    eng, X, y = ctx(100, 12)
    assert eng.fit_batch_max() == 256
    U = _u_rows(257, 12, 1, True, seed=1)
    rc, f, _, st, _ = _batch(eng, L.MATERN52, U, 1, True, 0.0)
    assert rc == L.E_ARG and "256" in eng.last_message()
    assert np.all(np.isnan(f)) and np.all(st == 99)  # refused before anything was done
    rc, *_ = _batch(eng, L.MATERN52, U, 1, True, 0.0, b=0)
    assert rc == L.E_ARG
    assert eng._lib.gpso_fit_eval_u_batch(eng._h, L.MATERN52, None, 1, 1, 1, 0.0, None, None, None, None) == L.E_ARG
    eng.close()

    eng, _, _ = ctx(100, 40)
    assert eng.fit_batch_max() == 0
    eng.close()

    eng, X, y = ctx(200, 3)
    assert eng.fit_batch_max() == 0
    U = _u_rows(3, 3, 1, True, seed=2, y_mean=float(y.mean()))
    rc, *_ = _batch(eng, L.MATERN52, U, 1, True, 0.0)
    assert rc == L.E_ARG and "N > 128" in eng.last_message()
    # HipGPEngine.fit_eval_u_batch at N = 200: the rows one after another, same answers
    loss, grad, ok = eng.fit_eval_u_batch("Matern52", U, 1, True)
    assert np.all(ok)
    for b, u in enumerate(U):
        f1, g1, _ = eng.fit_eval_u("Matern52", u, 1, True)
        assert np.float64(loss[b]).tobytes() == np.float64(f1).tobytes() and grad[b].tobytes() == g1.tobytes()
    eng.close()


def test_engine_batch_of_300_is_chunked_and_agrees_with_the_single_calls():
    n, d = 52, 2
    X, y = synthetic_problem(n, d, seed=6)
    eng = _engine()
    eng.set_data(X, y)
    U = _u_rows(300, d, d, True, seed=3, y_mean=float(y.mean()))
    loss, grad, ok = eng.fit_eval_u_batch("Matern52", U, d, True)
    assert loss.shape == (300,) and grad.shape == (300, d + 3) and np.all(ok)
    for b in (0, 1, 255, 256, 257, 299):
        f1, g1, _ = eng.fit_eval_u("Matern52", U[b], d, True)
        assert np.float64(loss[b]).tobytes() == np.float64(f1).tobytes() and grad[b].tobytes() == g1.tobytes()
    eng.close()


def test_multistart_surrogate_end_to_end_against_the_oracle_run():
    """GPRSurrogate(optimiser=Scipy(restarts=4, starts=...)) on the multimodal problem of tests/multistart_problem.py: every
    search's record is the oracle-backed CPU run's, the winner is the same (a restart, not the warm start), and the
    leaf-UCB afterwards is the oracle's at the winner's theta."""
    from pygpso_amd.gp_surrogate import GPRSurrogate
    from pygpso_amd.kernels import Constant, Matern52, Scipy

    X, y, u0, starts = problem()
    ref = oracle_multistart()
    surr = GPRSurrogate(gp_kernel=Matern52(lengthscales=THETA0["lengthscales"], variance=THETA0["variance"]),
                        gp_meanf=Constant(THETA0["mean_c"]), gauss_likelihood_sigma=THETA0["noise"],
                        optimiser=Scipy(restarts=4, starts=starts))
    surr.append(np.array(X), np.array(y))
    surr.gp_update()
    res = surr.optimiser.last_result
    model = surr.gpflow_model
    assert model.num_loss_evals == sum(r["nfev"] for r in res.restarts)
    assert len(res.restarts) == 4 and res.winner == ref.winner != 0
    for got, want in zip(res.restarts, ref.restarts):
        assert got["nfev"] == want["nfev"] and got["status"] == want["status"]
        assert abs(got["fun"] - want["fun"]) <= 1e-9 * abs(want["fun"])
    th = gpr.Theta.unpack(KERNEL, res.x)
    leaves = synthetic_leaves(512, 2, seed=1)
    mu, var, ucb = surr.gp_eval_best_ucb(leaves)
    i_ref, mu_ref, var_ref, ucb_ref = gpr.best_ucb(gpr.posterior(th, X, y), leaves)
    assert abs(mu - mu_ref) < 1e-9 and abs(var - var_ref) < 1e-9 and abs(ucb - ucb_ref) < 1e-9
    model.engine.close()
