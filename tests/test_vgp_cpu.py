"""
CPU checks of the variational GP: the float64 oracle (tests/vgp_oracle.py) against the reference's known answer and
against itself (central differences, the GPR limit, the triangular predictive), the surrogate's constructor limits, and
that without a GPU the surrogate raises instead of falling back to the CPU.
"""
import json
import os

import numpy as np
import pytest

from oracle import gpr
from tests import vgp_oracle as V
from tests.helpers import kat_training_data, synthetic_problem

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "reference_goldens_vgp.json")) as fh:
    GV = json.load(fh)["VG1"]


def _kat_run():
    X, y = kat_training_data()
    n = X.shape[0]
    r = GV["recipe"]
    u0 = V.initial_u(r["lengthscales"], r["variance"], r["likelihood_variance"], r["c"])
    u, mu, S, _ = V.train(r["kernel"], u0, 1, True, 0.0, X, y, np.zeros(n), np.eye(n), r["train_iterations"],
                          r["natgrad_learning_rate"], V.Adam(r["optimiser"][1]))
    return V.Posterior(r["kernel"], u, 1, True, 0.0, X, mu, S)


def test_oracle_hits_the_reference_kat():
    m, v = _kat_run().predict_y(GV["predict_at"])
    assert float(np.around(m[0], GV["decimals"])) == GV["mean"]
    assert float(np.around(v[0], GV["decimals"])) == GV["var"]


def _problem(n, d, seed):
    X, y = synthetic_problem(n, d, seed=seed)
    rng = np.random.default_rng(seed + 100)
    mu = 0.3 * rng.normal(size=n)
    S = np.tril(0.1 * rng.normal(size=(n, n)), -1) + np.diag(0.5 + rng.random(n))
    return X, y, mu, S


@pytest.mark.parametrize("kernel", gpr.KERNELS)
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("train_mean", [False, True])
def test_oracle_gradient_matches_central_differences(kernel, ard, train_mean, monkeypatch):
    # (Matern-1/2: k = s2 exp(-sqrt(r^2)) turns the ~1e-16 GEMM-form r^2 of the diagonal into ~1e-8 of k, noise that a
    # difference quotient amplifies; the analytic gradient takes dk there as 0.  The quotient here sees an exact diagonal.)
    sqd = gpr.scaled_sqdist

    def exact_diagonal(X, X2, ls):
        r2 = sqd(X, X2, ls)
        if X2 is None or X2 is X:
            np.fill_diagonal(r2, 0.0)
        return r2

    monkeypatch.setattr(gpr, "scaled_sqdist", exact_diagonal)
    n, d = 12, 3
    X, y, mu, S = _problem(n, d, seed=3)
    ls = np.array([0.6, 0.9, 1.3]) if ard else 0.8
    u = V.initial_u(ls, 1.3, 0.05, 0.2 if train_mean else None)
    n_ls = d if ard else 1
    f, g, _ = V.neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, 0.1, X, y, mu, S)
    assert np.isclose(f, V.neg_elbo(kernel, u, n_ls, train_mean, 0.1, X, y, mu, S), rtol=1e-13)
    h, tol = 1e-6, 1e-6
    for k in range(u.shape[0]):
        up, um = u.copy(), u.copy()
        up[k] += h
        um[k] -= h
        fd = (V.neg_elbo(kernel, up, n_ls, train_mean, 0.1, X, y, mu, S)
              - V.neg_elbo(kernel, um, n_ls, train_mean, 0.1, X, y, mu, S)) / (2 * h)
        assert abs(fd - g[k]) <= tol * max(1.0, abs(fd)), (k, fd, g[k])


def test_full_natgrad_step_gives_the_gpr_posterior():
    """gamma = 1 at fixed theta: q is the exact posterior, and the predictive is GPR's with K + 1e-6 I and noise s2."""
    X, y, mu, S = _problem(40, 2, seed=5)
    u = V.initial_u(0.4, 1.1, 0.01, 0.05)
    mu1, S1 = V.natgrad("Matern32", u, 1, True, 0.0, X, y, mu, S, 1.0)
    post = V.Posterior("Matern32", u, 1, True, 0.0, X, mu1, S1)
    ls, var, s2, c = V.unpack(u, 1, True)
    theta = gpr.Theta("Matern32", ls[0], var, s2 + V.JITTER, c)
    Xs = np.random.default_rng(0).random((50, 2))
    m_ref, v_ref = gpr.predict_y(gpr.posterior(theta, X, y), Xs)
    m, v = post.predict_f(Xs)
    np.testing.assert_allclose(m, m_ref, rtol=0, atol=1e-10)
    # GPR's latent variance with K + (1e-6 + s2) I and VGP's with K + 1e-6 I and noise s2 are the same quantity
    np.testing.assert_allclose(v + s2 + V.JITTER, v_ref, rtol=0, atol=1e-10)


def test_triangular_predictive_equals_two_term_form():
    X, y, _, _ = _problem(30, 3, seed=7)
    u = V.initial_u(0.7, 0.9, 0.02, 0.0)
    mu1, S1 = V.natgrad("Matern52", u, 1, True, 0.0, X, y, np.zeros(30), np.eye(30), 1.0)
    u2 = V.initial_u(0.5, 1.2, 0.05, 0.1)  # a step of half length at other hyper-parameters: still Lambda > I
    mu1, S1 = V.natgrad("Matern52", u2, 1, True, 0.0, X, y, mu1, S1, 0.5)
    post = V.Posterior("Matern52", u, 1, True, 0.0, X, mu1, S1)
    Xs = np.random.default_rng(1).random((64, 3))
    m2, v2 = post.predict_y(Xs)
    m3, v3 = post.predict_y(Xs, triangular=True)
    np.testing.assert_allclose(m3, m2, rtol=0, atol=1e-13)
    np.testing.assert_allclose(v3, v2, rtol=0, atol=1e-13)


def test_constructor_limits():
    from pygpso_amd import VGPSurrogate
    from pygpso_amd import kernels as K

    class Bernoulli:
        pass

    with pytest.raises(NotImplementedError):
        VGPSurrogate(gp_kernel=K.Matern52(), likelihood=Bernoulli())
    for gamma in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            VGPSurrogate(gp_kernel=K.Matern52(), natgrad_learning_rate=gamma)
    with pytest.raises(ValueError):
        VGPSurrogate(gp_kernel=K.Matern52(), dtype="float32")
    for dtype in ("float64", "mixed"):
        s = VGPSurrogate(gp_kernel=K.Matern52(), gp_meanf=K.Constant(), dtype=dtype)
        assert s.dtype == dtype and isinstance(s.optimiser, K.Adam) and s.likelihood.variance == 1e-3
        assert s.train_iters == 10 and s.natgrad_gamma == 1.0


def test_adam_spec_matches_the_oracle_adam():
    from pygpso_amd.kernels import Adam

    rng = np.random.default_rng(2)
    a, b = Adam(0.01), V.Adam(0.01)
    u1 = u2 = rng.normal(size=4)
    for _ in range(7):
        g = rng.normal(size=4)
        u1, u2 = a.step(u1, g), b.step(u2, g)
    np.testing.assert_array_equal(u1, u2)


def test_rows_carried_in_order_of_arrival():
    from pygpso_amd.vgp import carried_order

    rng = np.random.default_rng(4)
    x, y = rng.random((6, 2)), rng.random((6, 1))
    perm = np.array([3, 0, 5, 1, 4, 2])
    order = carried_order(x[:4], y[:4], x[perm], y[perm])
    np.testing.assert_array_equal(x[perm][order][:4], x[:4])
    y2 = y.copy()
    y2[2] += 1.0
    assert carried_order(x[:4], y[:4], x, y2) is None


def test_no_cpu_fallback_without_gpu():
    import ctypes as C

    from pygpso_amd import _lib
    from pygpso_amd import kernels as K
    from pygpso_amd import VGPSurrogate

    lib = _lib.load()
    h = C.c_void_p()
    if lib.gpso_create(C.byref(h), 0, _lib.F64) == _lib.OK:
        lib.gpso_destroy(h)
        pytest.skip("a HIP device is present: this test checks the behaviour without one")
    s = VGPSurrogate(gp_kernel=K.Matern52(), gp_meanf=K.Constant())
    X, y = kat_training_data()
    with pytest.raises(_lib.GpsoHipError):
        s._gp_train(X, y[:, None])
