"""
CPU checks of the variational GP's Student-t likelihood: the float64 oracle (tests/vgp_studentt_oracle.py) against scipy's
Student-t density and adaptive quadrature, against itself (central differences, the natural gradient's fixed point) and
against the closed-form Gaussian oracle (tests/vgp_oracle.py); the constructor limits of the specs and the surrogate.
"""
import numpy as np
import pytest
import scipy.integrate
import scipy.stats

from oracle import gpr
from tests import vgp_oracle as V
from tests import vgp_studentt_oracle as T
from tests.helpers import synthetic_problem

ST = ("StudentT", 3.0)
GH = ("GaussianGH", None)


def _problem(n, d, seed):
    X, y = synthetic_problem(n, d, seed=seed)
    rng = np.random.default_rng(seed + 100)
    mu = 0.3 * rng.normal(size=n)
    S = np.tril(0.1 * rng.normal(size=(n, n)), -1) + np.diag(0.5 + rng.random(n))
    return X, y, mu, S


@pytest.mark.parametrize("nu", [2.5, 3.0, 7.0, 40.0])
def test_log_density_is_scipys_student_t(nu):
    rng = np.random.default_rng(1)
    y, f = 3.0 * rng.normal(size=50), rng.normal(size=50)
    for s in (0.05, 1.0, 4.0):
        psi, _, _ = T.logdensity(("StudentT", nu), y, f, s)
        np.testing.assert_allclose(psi, scipy.stats.t.logpdf(y, nu, loc=f, scale=s), rtol=1e-13, atol=1e-13)


def test_log_density_derivatives():
    rng = np.random.default_rng(2)
    y, f = 3.0 * rng.normal(size=20), rng.normal(size=20)
    for lik, p in ((ST, 0.7), (("StudentT", 5.5), 1.3), (GH, 0.4)):
        _, dpsi, dp = T.logdensity(lik, y, f, p)
        h = 1e-6
        fd_f = (T.logdensity(lik, y, f + h, p)[0] - T.logdensity(lik, y, f - h, p)[0]) / (2 * h)
        fd_p = (T.logdensity(lik, y, f, p + h)[0] - T.logdensity(lik, y, f, p - h)[0]) / (2 * h)
        np.testing.assert_allclose(dpsi, fd_f, rtol=1e-7, atol=1e-7)
        np.testing.assert_allclose(dp, fd_p, rtol=1e-7, atol=1e-7)


def test_twenty_point_quadrature_against_adaptive_quadrature():
    # the 20-point Gauss-Hermite rule integrates log(1 + z^2 / df) against N(m, v) to within ~1e-5 of its value here (the
    # integrand is analytic but no polynomial); scipy's adaptive quadrature is exact to 1e-10
    rng = np.random.default_rng(3)
    y = np.array([0.0, 0.5, -1.0, 2.0, 8.0])
    m = rng.normal(size=5)
    v = np.array([0.01, 0.1, 0.5, 1.0, 0.3])
    s = 0.8
    ve, _, _, _ = T.quadrature(ST, y, m, v, s)
    for i in range(5):
        sd = np.sqrt(v[i])
        ref, _ = scipy.integrate.quad(
            lambda f: scipy.stats.norm.pdf(f, m[i], sd) * scipy.stats.t.logpdf(y[i], 3.0, loc=f, scale=s),
            m[i] - 12 * sd, m[i] + 12 * sd, epsabs=1e-12, epsrel=1e-12, limit=200)
        assert abs(ve[i] - ref) <= 2e-4 * max(1.0, abs(ref)), (i, ve[i], ref)


@pytest.mark.parametrize("kernel", gpr.KERNELS)
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("train_mean", [False, True])
@pytest.mark.parametrize("lik", [ST, GH], ids=["studentt", "gaussian_gh"])
def test_oracle_gradient_matches_central_differences(kernel, ard, train_mean, lik, monkeypatch):
    # (an exact diagonal of r^2, as in tests/test_vgp_cpu.py: Matern-1/2's sqrt amplifies the GEMM-form rounding there)
    sqd = gpr.scaled_sqdist

    def exact_diagonal(X, X2, ls):
        r2 = sqd(X, X2, ls)
        if X2 is None or X2 is X:
            np.fill_diagonal(r2, 0.0)
        return r2

    monkeypatch.setattr(gpr, "scaled_sqdist", exact_diagonal)
    n, d = 12, 3
    X, y, mu, S = _problem(n, d, seed=3)
    y = y.copy()
    y[4] += 6.0  # one outlier: the Student-t's tails at work
    ls = np.array([0.6, 0.9, 1.3]) if ard else 0.8
    c = 0.2 if train_mean else None
    u = T.initial_u(ls, 1.3, 0.3, c) if lik == ST else V.initial_u(ls, 1.3, 0.05, c)
    n_ls = d if ard else 1
    args = (kernel, u, n_ls, train_mean, 0.1, X, y, mu, S, lik)
    f, g, th = T.neg_elbo_and_grad_u(*args)
    assert np.isclose(f, T.neg_elbo(*args), rtol=1e-13)
    assert th[n_ls + 1] == pytest.approx(0.3 if lik == ST else 0.05, rel=1e-12)
    h, tol = 1e-6, 1e-6
    for k in range(u.shape[0]):
        up, um = u.copy(), u.copy()
        up[k] += h
        um[k] -= h
        fd = (T.neg_elbo(kernel, up, *args[2:]) - T.neg_elbo(kernel, um, *args[2:])) / (2 * h)
        assert abs(fd - g[k]) <= tol * max(1.0, abs(fd)), (k, fd, g[k])


def test_gaussian_through_the_quadrature_is_the_closed_form():
    """Twenty Gauss-Hermite points integrate a quadratic exactly: loss, gradient and natgrad steps equal tests/vgp_oracle.py."""
    X, y, mu, S = _problem(30, 3, seed=4)
    for kernel, train_mean in (("Matern52", True), ("SquaredExponential", False)):
        u = V.initial_u(0.7, 1.1, 0.03, 0.2 if train_mean else None)
        f0, g0, th0 = V.neg_elbo_and_grad_u(kernel, u, 1, train_mean, 0.1, X, y, mu, S)
        f1, g1, th1 = T.neg_elbo_and_grad_u(kernel, u, 1, train_mean, 0.1, X, y, mu, S, GH)
        assert abs(f1 - f0) <= 1e-12 * abs(f0), (f0, f1)
        np.testing.assert_allclose(g1, g0, rtol=1e-12, atol=1e-12 * np.max(np.abs(g0)))
        np.testing.assert_array_equal(th1, th0)
        for gamma in (1.0, 0.5):
            m0, S0 = V.natgrad(kernel, u, 1, train_mean, 0.1, X, y, mu, S, gamma)
            m1, S1 = T.natgrad(kernel, u, 1, train_mean, 0.1, X, y, mu, S, GH, gamma)
            np.testing.assert_allclose(m1, m0, rtol=0, atol=1e-12 * np.max(np.abs(m0)))
            np.testing.assert_allclose(S1, S0, rtol=0, atol=1e-12)
        p0 = V.Posterior(kernel, u, 1, train_mean, 0.1, X, mu, S)
        p1 = T.Posterior(kernel, u, 1, train_mean, 0.1, X, mu, S, GH)
        assert p0.s2 == p1.s2


def test_natgrad_fixed_point_is_a_stationary_point_of_the_elbo():
    """gamma = 0.2 at fixed theta until q stops moving: there the ELBO's gradient in mu (central differences) vanishes --
    an independent check of the non-conjugate natural gradient's derivation."""
    X, y = synthetic_problem(25, 2, seed=6)
    y = y.copy()
    y[[3, 11]] += 5.0
    n = y.shape[0]
    u = T.initial_u(0.4, 1.0, 0.2, 0.0)
    mu, S = np.zeros(n), np.eye(n)
    for it in range(400):
        m2, S2 = T.natgrad("Matern52", u, 1, True, 0.0, X, y, mu, S, ST, 0.2)
        step = max(np.max(np.abs(m2 - mu)), np.max(np.abs(S2 - S)))
        mu, S = m2, S2
        if step < 1e-13:
            break
    assert step < 1e-11, (it, step)
    f0 = T.neg_elbo("Matern52", u, 1, True, 0.0, X, y, mu, S, ST)
    h = 1e-5
    for i in range(n):
        mp, mm = mu.copy(), mu.copy()
        mp[i] += h
        mm[i] -= h
        fd = (T.neg_elbo("Matern52", u, 1, True, 0.0, X, y, mp, S, ST)
              - T.neg_elbo("Matern52", u, 1, True, 0.0, X, y, mm, S, ST)) / (2 * h)
        assert abs(fd) <= 1e-7 * max(1.0, abs(f0)), (i, fd)
    # ... and in the diagonal of S (the covariance's stationarity)
    for i in range(0, n, 5):
        Sp, Sm = S.copy(), S.copy()
        Sp[i, i] += h
        Sm[i, i] -= h
        fd = (T.neg_elbo("Matern52", u, 1, True, 0.0, X, y, mu, Sp, ST)
              - T.neg_elbo("Matern52", u, 1, True, 0.0, X, y, mu, Sm, ST)) / (2 * h)
        assert abs(fd) <= 1e-7 * max(1.0, abs(f0)), (i, fd)


def test_outlier_makes_the_full_step_indefinite():
    """g_v > 0 where |y - f| > sqrt(df) scale: a gross outlier at gamma = 1 gives Lambda* an eigenvalue < 0 (GPflow then
    fails in natural_to_meanvarsqrt) -- the situation the device must answer with NOTPD and q untouched."""
    X, y = synthetic_problem(40, 2, seed=8)
    y = y.copy()
    y[7] += 30.0
    u = T.initial_u(0.3, 1.0, 0.05, 0.0)
    lam, _ = T.natural_params("Matern52", u, 1, True, 0.0, X, y, np.zeros(40), np.eye(40), ST, 1.0)
    assert np.linalg.eigvalsh(lam).min() < -0.1
    with pytest.raises(np.linalg.LinAlgError):
        T.natgrad("Matern52", u, 1, True, 0.0, X, y, np.zeros(40), np.eye(40), ST, 1.0)


def test_constructor_limits():
    from pygpso_amd import VGPSurrogate
    from pygpso_amd import kernels as K

    s = VGPSurrogate(gp_kernel=K.Matern52(), gp_meanf=K.Constant(), likelihood=K.StudentT(), natgrad_learning_rate=0.1)
    assert s.likelihood.name == "StudentT" and s.likelihood.scale == 1.0 and s.likelihood.df == 3.0
    assert s.natgrad_gamma == 0.1
    for df in (2.0, 1.5, 0.0, -3.0):
        with pytest.raises(ValueError):
            K.StudentT(df=df)
    for scale in (0.0, -1.0):
        with pytest.raises(ValueError):
            K.StudentT(scale=scale)

    class Bernoulli:
        pass

    with pytest.raises(NotImplementedError):
        VGPSurrogate(gp_kernel=K.Matern52(), likelihood=Bernoulli())
    # the default learning rate stays the reference's 1.0
    assert VGPSurrogate(gp_kernel=K.Matern52(), likelihood=K.StudentT(0.5, 4.0)).natgrad_gamma == 1.0


def test_likelihood_ids_match_the_header():
    from pygpso_amd import _lib

    assert (_lib.LIK_GAUSSIAN, _lib.LIK_STUDENT_T, _lib.LIK_GAUSSIAN_GH) == (0, 1, 2)
    assert "gpso_vgp_set_likelihood" in _lib.SIGNATURES
