"""
CPU checks of the SVGP's float64 oracle (tests/svgp_oracle.py) and of SVGPSurrogate's argument checking: the closed-form
-ELBO gradient against central differences, the Titsias identity (a Gaussian gamma = 1 step from the prior lands on the
SGPR's optimal q: -ELBO equals the collapsed -bound and the predictive the SGPR's), and the constructor's limits.
"""
import numpy as np
import pytest

from oracle import gpr
from tests import sgpr_oracle as S_
from tests import svgp_oracle as O
from tests.helpers import synthetic_problem

KERNELS = ["Matern52", "Matern32", "Matern12", "SquaredExponential"]
LIKS = [("Gaussian", None), ("StudentT", 4.0)]


def _problem(n, d, m, seed):
    X, y = synthetic_problem(n, d, seed=seed)
    rng = np.random.default_rng(seed + 1)
    return X, y, rng.random((m, d))  # (Z away from X: no coincident pairs in Kuf, where Matern-1/2 has its kink)


def _q(m, seed):
    rng = np.random.default_rng(seed)
    S = np.tril(0.2 * rng.standard_normal((m, m)), -1) + np.diag(0.5 + 0.4 * rng.random(m))
    return 0.5 * rng.standard_normal(m), S


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("lik", LIKS, ids=["gauss", "studentt"])
@pytest.mark.parametrize("ard", [False, True])
def test_oracle_gradient_matches_central_differences(kernel, lik, ard, monkeypatch):
    # (as tests/test_sgpr_cpu.py: Matern-1/2 turns the ~1e-16 GEMM-form r^2 of Kuu's diagonal into ~1e-8 of k, noise that a
    # difference quotient amplifies; the analytic gradient takes dk there as 0, so the quotient sees an exact diagonal)
    sqd = gpr.scaled_sqdist

    def exact_diagonal(X, X2, ls):
        r2 = sqd(X, X2, ls)
        if X2 is None or X2 is X:
            np.fill_diagonal(r2, 0.0)
        return r2

    monkeypatch.setattr(gpr, "scaled_sqdist", exact_diagonal)
    n, d, m = 40, 3, 9
    X, y, Z = _problem(n, d, m, seed=7)
    mu, S = _q(m, 3)
    n_ls = d if ard else 1
    ls = np.array([0.6, 0.8, 1.1]) if ard else 0.8
    u = O.initial_u(ls, 1.3, 0.3 if lik[0] == "StudentT" else 0.05, lik, c=0.2)
    f0, g, _ = O.neg_elbo_and_grad_u(kernel, u, n_ls, True, 0.0, X, y, Z, mu, S, lik)
    assert f0 == pytest.approx(O.neg_elbo(kernel, u, n_ls, True, 0.0, X, y, Z, mu, S, lik), rel=1e-13)
    h = 1e-6
    fd = np.empty_like(g)
    for k in range(u.shape[0]):
        e = np.zeros_like(u)
        e[k] = h
        fd[k] = (O.neg_elbo(kernel, u + e, n_ls, True, 0.0, X, y, Z, mu, S, lik)
                 - O.neg_elbo(kernel, u - e, n_ls, True, 0.0, X, y, Z, mu, S, lik)) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=2e-6, atol=2e-6 * max(1.0, np.max(np.abs(fd))))


def test_titsias_identity():
    """Gaussian likelihood, one gamma = 1 step from the prior: q is the SGPR's optimum, -ELBO = -bound (<= 1e-12 relative)
    and the predictive is sgpr_oracle.Posterior's."""
    n, d, m, kernel = 300, 3, 40, "Matern52"
    X, y = synthetic_problem(n, d, seed=11)
    ls, var, s2, c = 0.7, 1.1, 0.02, 0.15
    Z = S_.choose_inducing(kernel, X, ls, var, m)
    lik = ("Gaussian", None)
    u = O.initial_u(ls, var, s2, lik, c=c)
    mu, S = O.natgrad(kernel, u, 1, True, 0.0, X, y, Z, np.zeros(m), np.eye(m), lik, 1.0)
    loss = O.neg_elbo(kernel, u, 1, True, 0.0, X, y, Z, mu, S, lik)
    bound, _, _ = S_.neg_bound_and_grad_u(kernel, u, 1, True, 0.0, X, y, Z)
    assert abs(loss - bound) / abs(bound) <= 1e-12
    Xs = synthetic_problem(64, d, seed=12)[0]
    m_s, v_s = S_.Posterior(kernel, u, 1, True, 0.0, X, y, Z).predict_f(Xs)
    m_v, v_v = O.Posterior(kernel, u, 1, True, 0.0, X, Z, mu, S, lik).predict_f(Xs)
    np.testing.assert_allclose(m_v, m_s, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(v_v, v_s, rtol=1e-9, atol=1e-11)


def test_conjugate_start_is_the_gaussian_step():
    n, d, m, kernel = 60, 2, 12, "Matern32"
    X, y, Z = _problem(n, d, m, seed=5)
    lik = ("StudentT", 3.0)
    u = O.initial_u(0.5, 1.0, 0.2, lik, c=0.0)
    s2 = 0.2 ** 2 * 3.0
    mu, S = O.conjugate_start(kernel, u, 1, True, 0.0, X, y, Z, lik, s2)
    ug = O.initial_u(0.5, 1.0, s2, ("Gaussian", None), c=0.0)
    mu2, S2 = O.natgrad(kernel, ug, 1, True, 0.0, X, y, Z, np.zeros(m), np.eye(m), ("Gaussian", None), 1.0)
    np.testing.assert_allclose(mu, mu2, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(S, S2, rtol=1e-6, atol=1e-9)


def test_surrogate_arguments():
    from pygpso_amd import SVGPSurrogate
    from pygpso_amd import kernels as K

    kern = K.Matern52(lengthscales=0.3, variance=1.0)

    class Bernoulli:
        name = "Bernoulli"

    with pytest.raises(NotImplementedError):
        SVGPSurrogate(gp_kernel=kern, likelihood=Bernoulli())
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            SVGPSurrogate(gp_kernel=kern, natgrad_learning_rate=bad)
    with pytest.raises(ValueError):
        SVGPSurrogate(gp_kernel=kern, dtype="float32")
    with pytest.raises(ValueError):
        SVGPSurrogate(gp_kernel=kern, inducing="random")
    with pytest.raises(ValueError):
        SVGPSurrogate(gp_kernel=kern, num_inducing=0)
    with pytest.raises(ValueError):
        SVGPSurrogate(gp_kernel=kern, inducing=np.array([[np.nan, 0.0]]))
    s = SVGPSurrogate(gp_kernel=kern, likelihood=K.StudentT(scale=0.2, df=3.0), natgrad_learning_rate=0.1,
                      num_inducing=64)
    assert s.natgrad_gamma == 0.1 and s.num_inducing == 64 and s.train_iters == 10
    assert type(s.optimiser).__name__ == "Adam"
    s = SVGPSurrogate(gp_kernel=kern, inducing=np.zeros((5, 2)), optimiser=K.Scipy(), dtype="mixed")
    assert s.num_inducing == 5 and type(s.optimiser).__name__ == "Scipy"


def test_model_refuses_float32():
    from pygpso_amd.svgp import HipSVGP
    from pygpso_amd import kernels as K

    with pytest.raises(ValueError):
        HipSVGP(data=(np.zeros((4, 2)), np.zeros((4, 1))), kernel=K.Matern52(lengthscales=0.3, variance=1.0),
                dtype="float32")
