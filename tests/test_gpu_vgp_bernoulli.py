"""
The variational GP's Bernoulli likelihood (exact probit) on the MI355X: the device's quadrature sequence
under GPSO_LIK_BERNOULLI against the float64 oracle of tests/vgp_bernoulli_oracle.py, the install (the LATENT predictive:
noise slot 0, shift 0), ``gpso_predict_prob`` against the host entry of the same header, and the refusals.

Cases (n, d, kernel, ard): (7, 1, Matern12, no), (60, 2, Matern52, yes), (128, 3, SquaredExponential, yes) and (129, 12,
Matern32, no) -- one row past the 128 padding, training only.  Labels are the sign of a smooth function of X about its median,
seed fixed per case: every case has at least 20 % of each label, and the oracle's Lambda of both steps keeps its smallest
eigenvalue >= 1 (asserted here, checked on the CPU in tests/test_vgp_bernoulli_cpu.py).

Tolerances: those tests/test_gpu_vgp_studentt.py states for the same quantities -- 2e-9, and 1e-5 / 1e-4 under Matern-1/2
(r = sqrt(r^2) on the diagonal).
"""
import numpy as np
import pytest

from tests import vgp_bernoulli_oracle as B
from tests import vgp_oracle as V
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu
ULP = float(np.finfo(np.float64).eps)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _engine(X, y, dtype="float64"):
    from pygpso_amd import HipGPEngine

    eng = HipGPEngine(dtype, device=0)
    eng.set_data(X, y)
    eng.vgp_set_likelihood("Bernoulli", 0.0, B.N_GH)
    eng.vgp_set_q()
    return eng


def _tols(kernel):
    return (1e-5, 1e-4) if kernel == "Matern12" else (2e-9, 2e-9)


@pytest.mark.parametrize("n,d,kernel,ard", B.CASES)
def test_device_natgrad_elbo_against_oracle(n, d, kernel, ard):
    X, y, u, n_ls = B.case_problem(n, d, kernel, ard)
    assert 0.2 <= y.mean() <= 0.8  # at least 20 % of each label
    tol, tol_g = _tols(kernel)
    eng = _engine(X, y)
    mu, S = np.zeros(n), np.eye(n)
    for gamma, shift in B.STEPS:
        uu = u + shift
        lam, _ = B.natural_params(kernel, uu, n_ls, True, 0.0, X, y, mu, S, gamma)
        ev = np.linalg.eigvalsh(lam)
        assert ev.min() >= 1.0 - 4.0 * n * ULP * ev.max()  # log-concave: Lambda >= I (up to the eigensolver's rounding)
        eng.vgp_natgrad(kernel, uu, n_ls, True, 0.0, gamma)
        mu, S = B.natgrad(kernel, uu, n_ls, True, 0.0, X, y, mu, S, gamma)
        dmu, dS = eng.vgp_get_q()
        print(f"BERNOULLI_PARITY n={n} gamma={gamma}: mu {_rel(dmu, mu):.2e}, Sigma {_rel(dS @ dS.T, S @ S.T):.2e} (bound {tol:.0e})")
        assert _rel(dmu, mu) <= tol, (gamma, _rel(dmu, mu))
        assert _rel(dS @ dS.T, S @ S.T) <= tol, (gamma, _rel(dS @ dS.T, S @ S.T))
        eng.vgp_set_q(mu, S)
        f, g, th = eng.vgp_elbo_u(kernel, uu, n_ls, True, 0.0)
        f_ref, g_ref, th_ref = B.neg_elbo_and_grad_u(kernel, uu, n_ls, True, 0.0, X, y, mu, S)
        print(f"BERNOULLI_PARITY n={n} gamma={gamma}: loss {abs(f - f_ref) / abs(f_ref):.2e}, grad {_rel(g, g_ref):.2e} (bound {tol_g:.0e})")
        assert abs(f - f_ref) <= tol * abs(f_ref), (f, f_ref)
        assert _rel(g, g_ref) <= tol_g, (g, g_ref)
        assert g[n_ls + 1] == 0.0 and not np.signbit(g[n_ls + 1])  # the likelihood slot: exactly 0.0
        np.testing.assert_allclose(th, th_ref, rtol=1e-15)  # (the slot is decoded as the Gaussian's, and read by nothing)
    eng.close()


_INSTALLED = {}


def _installed(n, d, kernel, ard):
    """A Bernoulli install on the device after the oracle's two steps: made once per case, shared, read-only."""
    key = (n, d, kernel, ard)
    if key not in _INSTALLED:
        X, y, u, n_ls = B.case_problem(n, d, kernel, ard)
        mu, S = np.zeros(n), np.eye(n)
        for gamma, shift in B.STEPS:
            mu, S = B.natgrad(kernel, u + shift, n_ls, True, 0.0, X, y, mu, S, gamma)
        uu = u + B.STEPS[-1][1]
        eng = _engine(X, y)
        eng.vgp_set_q(mu, S)
        eng.vgp_posterior(kernel, uu, n_ls, True, 0.0)
        post = B.Posterior(kernel, uu, n_ls, True, 0.0, X, mu, S)
        xs = synthetic_leaves(200, d, seed=31)
        _INSTALLED[key] = (eng, post, xs, eng.predict(xs), eng.predict_prob(xs, want_latent=True))
    return _INSTALLED[key]


@pytest.mark.parametrize("n,d,kernel,ard", B.CASES[:3])
def test_install_serves_the_latent_predictive(n, d, kernel, ard):
    from pygpso_amd import acquisition as A

    eng, post, xs, (m, v), _ = _installed(n, d, kernel, ard)
    tol, _ = _tols(kernel)
    m_ref, v_ref = post.predict_f(xs)
    print(f"BERNOULLI_PARITY n={n} install: mean {_rel(m, m_ref):.2e}, var {_rel(v, v_ref):.2e} (bound {tol:.0e})")
    assert _rel(m, m_ref) <= tol and _rel(v, v_ref) <= tol
    # predictive variance minus latent variance is exactly 0.0 -- noise slot 0 and delta = 0: a latent kind subtracts the
    # installed noise slot (noise + delta * variance) from the same column, and gives the bits of the kind that does not
    lat = eng.acq_values(xs, A.UCBStd(2.0, latent=True))
    obs = eng.acq_values(xs, A.UCBStd(2.0, latent=False))
    assert np.array_equal(_bits(lat[1]), _bits(obs[1])) and np.array_equal(_bits(lat[2]), _bits(obs[2]))
    # ... and the hyper block a push copies reports the slot itself
    from pygpso_amd import HipGPEngine

    other = HipGPEngine("float64", device=0)
    other.success_push(eng)
    present, n_m, theta = other.success_info()
    assert present and n_m == n and theta[49] == 0.0 and not np.signbit(theta[49])
    assert theta[48] == pytest.approx(post.var, rel=1e-14) and theta[50] == post.c
    other.close()


@pytest.mark.parametrize("n,d,kernel,ard", B.CASES[:3])
def test_predict_prob_is_the_host_map_of_the_devices_own_columns(n, d, kernel, ard):
    from pygpso_amd import HipGPEngine

    eng, post, xs, (m, v), (prob, logprob, lm, lv) = _installed(n, d, kernel, ard)
    h_prob, h_lp = HipGPEngine.success_prob_host(lm, lv)
    assert np.array_equal(_bits(logprob), _bits(h_lp)) and np.array_equal(_bits(prob), _bits(h_prob))
    # its columns are gpso_predict's within DESIGN.md 2.1's float64 row: 1e-9 of max(1, max |targets|) on the mean, of the kernel
    # variance on the variance (Matern-1/2: 1e-5)
    tol = 1e-5 if kernel == "Matern12" else 1e-9
    em, ev = float(np.max(np.abs(lm - m))), float(np.max(np.abs(lv - v))) / post.var
    print(f"BERNOULLI_PARITY n={n} predict_prob columns vs gpso_predict: mean {em:.2e}, var {ev:.2e} (bound {tol:.0e})")
    assert em <= tol and ev <= tol
    p_ref, lp_ref = post.predict_prob(xs)
    assert np.max(np.abs(prob - p_ref)) <= 10.0 * tol
    # one output alone, and a float32 leaf array
    only = eng.predict_prob(xs[:5])
    assert np.array_equal(_bits(only[0]), _bits(prob[:5])) and np.array_equal(_bits(only[1]), _bits(logprob[:5]))
    # the same call gives the same bits
    again = eng.predict_prob(xs, want_latent=True)
    for a, b in zip(again, (prob, logprob, lm, lv)):
        assert np.array_equal(_bits(a), _bits(b))


def _refused(fn, code, word):
    from pygpso_amd import _lib

    with pytest.raises(ValueError if code == _lib.E_ARG else _lib.GpsoHipError) as err:  # (the engine raises GPSO_E_ARG as ValueError)
        fn()
    assert (code == _lib.E_ARG or err.value.code == code) and word in str(err.value), str(err.value)


def test_predict_prob_refusals():
    from pygpso_amd import HipGPEngine, _lib

    X, y, u, n_ls = B.case_problem(60, 2, "Matern52", False)
    xs = synthetic_leaves(10, 2, seed=2)
    who = "gpso_predict_prob"
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    _refused(lambda: eng.predict_prob(xs), _lib.E_STATE, who)  # no posterior
    eng.vgp_set_q()  # a Gaussian VGP install
    eng.vgp_natgrad("Matern52", u, n_ls, True, 0.0, 1.0)
    eng.vgp_posterior("Matern52", u, n_ls, True, 0.0)
    _refused(lambda: eng.predict_prob(xs), _lib.E_STATE, who)
    eng.fit_eval("Matern52", 0.4, 1.0, 1e-2, 0.0, want_grad=False)  # a fitted GPR
    _refused(lambda: eng.predict_prob(xs), _lib.E_STATE, who)
    # n = 129
    X9, y9, u9, n9 = B.case_problem(*B.CASES[3])
    e9 = _engine(X9, y9)
    e9.vgp_natgrad("Matern32", u9, n9, True, 0.0, 1.0)
    e9.vgp_posterior("Matern32", u9, n9, True, 0.0)
    _refused(lambda: e9.predict_prob(synthetic_leaves(10, 12, seed=2)), _lib.E_ARG, who)
    assert e9.predict(synthetic_leaves(10, 12, seed=2))[0].shape == (10,)  # (the install itself is served at any N)
    e9.close()
    # a float32 context has no variational GP at all, and no success probability
    e32 = HipGPEngine("float32", device=0)
    e32.set_data(X, y)
    e32.fit_eval("Matern52", 0.4, 1.0, 1e-2, 0.0, want_grad=False)
    _refused(lambda: e32.predict_prob(xs), _lib.E_ARG, who)
    e32.close()
    # a Bernoulli install: served; a later natgrad step drops it again; an open ticket refuses
    eb = _engine(X, y)
    eb.vgp_natgrad("Matern52", u, n_ls, True, 0.0, 1.0)
    eb.vgp_posterior("Matern52", u, n_ls, True, 0.0)
    assert eb.predict_prob(xs)[0].shape == (10,)
    ticket = eb.best_ucb_begin(xs, 2.0)
    _refused(lambda: eb.predict_prob(xs), _lib.E_STATE, who)
    eb.best_ucb_end(ticket)
    eb.vgp_natgrad("Matern52", u, n_ls, True, 0.0, 0.5)
    _refused(lambda: eb.predict_prob(xs), _lib.E_STATE, who)
    # the kind takes df = 0 alone
    x, w = np.polynomial.hermite.hermgauss(20)
    assert _lib.load().gpso_vgp_set_likelihood(eb._h, _lib.LIK_BERNOULLI, 3.0, 20, _lib.dptr(x), _lib.dptr(w)) == _lib.E_ARG
    assert _lib.load().gpso_vgp_set_likelihood(eb._h, _lib.LIK_BERNOULLI, 0.0, 20, _lib.dptr(x), _lib.dptr(w)) == _lib.OK
    eb.close()
    eng.close()


def test_svgp_calls_refuse_the_bernoulli_kind():
    from pygpso_amd import _lib

    X, y, u, n_ls = B.case_problem(60, 2, "Matern52", False)
    eng = _engine(X, y)
    eng.sgpr_set_inducing(X[:16])
    z = np.ascontiguousarray(X[:16])
    for name, fn in (("gpso_svgp_init_q", lambda: eng.svgp_init_q("Matern52", u, n_ls, True, 0.0, 0.1)),
                     ("gpso_svgp_set_q", lambda: eng.svgp_set_q()),
                     ("gpso_svgp_get_q", lambda: eng.svgp_get_q()),
                     ("gpso_svgp_natgrad", lambda: eng.svgp_natgrad("Matern52", u, n_ls, True, 0.0, 0.5)),
                     ("gpso_svgp_elbo_u", lambda: eng.svgp_elbo_u("Matern52", u, n_ls, True, 0.0)),
                     ("gpso_svgp_posterior", lambda: eng.svgp_posterior("Matern52", u, n_ls, True, 0.0)),
                     ("gpso_svgp_elbo_uz", lambda: eng.svgp_elbo_uz("Matern52", u, n_ls, True, 0.0, z))):
        _refused(fn, _lib.E_ARG, name)
    # back under the Gaussian kind the family serves the same context
    eng.vgp_set_likelihood("Gaussian")
    eng.svgp_init_q("Matern52", V.initial_u(0.4, 1.0, 0.1, 0.0), 1, True, 0.0, 0.1)
    eng.close()


def test_hipvgp_bernoulli_trains_and_predicts_on_the_device():
    from pygpso_amd import kernels as K
    from pygpso_amd.vgp import HipVGP

    X, y, _, _ = B.case_problem(60, 2, "Matern52", False)
    model = HipVGP(data=(X, y[:, None]), kernel=K.Matern52(lengthscales=0.3, variance=1.2), mean_function=K.Constant(0.1),
                   likelihood=K.Bernoulli())
    adam_dev, adam_ref = K.Adam(0.05), V.Adam(0.05)
    u_ref, mu, S = B.initial_u(0.3, 1.2, 0.1), np.zeros(60), np.eye(60)
    for _ in range(3):
        model.natgrad(0.5)
        adam_dev.minimize(model.training_loss, model.trainable_variables)
    u_ref, mu, S, _ = B.train("Matern52", u_ref, 1, True, 0.0, X, y, mu, S, 3, 0.5, adam_ref)
    np.testing.assert_allclose(model._device_u(), u_ref, rtol=1e-8, atol=1e-10)
    xs = synthetic_leaves(50, 2, seed=5)
    post = B.Posterior("Matern52", u_ref, 1, True, 0.0, X, mu, S)
    prob, logprob = model.predict_prob(xs)
    np.testing.assert_allclose(np.asarray(prob)[:, 0], post.predict_prob(xs)[0], rtol=1e-6, atol=1e-9)
    mean, var = model.predict_f(xs)
    np.testing.assert_allclose(np.asarray(mean)[:, 0], post.predict_f(xs)[0], rtol=1e-6, atol=1e-9)
    with pytest.raises(NotImplementedError):
        model.predict_y(xs)
    model.engine.close()


@pytest.mark.parametrize("lik", ("Bernoulli", "StudentT", "Gaussian"))
def test_hipvgp_save_and_from_saved_on_the_device(lik):
    """The model's own save / from_saved (new with this likelihood, for every kind): ARD lengthscales, the kind and its
    parameters, the data and q come back, and the restored model predicts the same bits."""
    import os
    from shutil import rmtree

    from pygpso_amd import kernels as K
    from pygpso_amd.vgp import HipVGP

    tmp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_tmp_vgp_bernoulli")
    X, labels, _, _ = B.case_problem(60, 2, "Matern52", True)
    _, y = synthetic_problem(60, 2, seed=9)
    spec = {"Bernoulli": K.Bernoulli(), "StudentT": K.StudentT(scale=0.7, df=4.5), "Gaussian": K.Gaussian(0.02)}[lik]
    model = HipVGP(data=(X, (labels if lik == "Bernoulli" else y)[:, None]), kernel=K.SquaredExponential(lengthscales=np.array([0.3, 0.5]), variance=1.1),
                   mean_function=K.Constant(0.05), likelihood=spec, dtype="mixed")
    adam = K.Adam(0.02)
    for _ in range(2):
        model.natgrad(0.5)
        adam.minimize(model.training_loss, model.trainable_variables)
    model.save(tmp)
    try:
        back = HipVGP.from_saved(tmp)
        assert type(back.likelihood_spec()) is type(spec) and back.kernel.name == "SquaredExponential" and back.kernel.ard
        assert back.engine.dtype_name == "mixed"
        if lik == "StudentT":
            assert back.likelihood.df == 4.5 and back.likelihood.scale == model.likelihood.scale
        a, b = model.parameter_dict(), back.parameter_dict()
        assert sorted(a) == sorted(b)
        for k in a:
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]))
        xs = synthetic_leaves(64, 2, seed=6)
        for p, q in zip(model.predict_f(xs), back.predict_f(xs)):
            np.testing.assert_array_equal(np.asarray(p), np.asarray(q))
        if lik == "Bernoulli":
            for p, q in zip(model.predict_prob(xs), back.predict_prob(xs)):
                np.testing.assert_array_equal(np.asarray(p), np.asarray(q))
        back.engine.close()
    finally:
        rmtree(tmp, ignore_errors=True)
        model.engine.close()

