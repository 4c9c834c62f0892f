"""
CPU tests of the joint predictive: the float64 oracle of tests/joint_oracle.py against the textbook
form K** - K*^T (K + noise I)^-1 K* (a dense solve that never forms C) and against the marginals of
tests/predict_grad_oracle.py, and the Python surface -- ``predict_f`` / ``predict_y(full_cov=True)``, ``predict_f_samples``,
``gp_predict_joint``, ``gp_sample``, ``thompson_select`` -- over a stub engine whose arithmetic is that oracle.  (That
``gpso_predict_joint`` and ``gpso_sample_joint`` are declared, exported and bound is tests/test_cabi_cpu.py's.)
"""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gpr
from pygpso_amd import GPRSurrogate
from pygpso_amd import kernels as K
from pygpso_amd.model import HipGPR
from tests import joint_oracle as jo
from tests import predict_grad_oracle as po
from tests.helpers import synthetic_problem
from tests.test_loo_cpu import RecordingEngine

KERNELS = ("Matern52", "Matern32", "Matern12", "SquaredExponential")
SHAPES = [(2, 1), (17, 3), (129, 3), (300, 5), (40, 26)]
NOISES = (1.0e-3, 1.0e-1)


def _case(n, d, kernel, noise, m=40):
    """Problem, theta, test points, and the predictive's C and alpha from the direct-difference Gram (the textbook form's)."""
    X, y = synthetic_problem(n, d, seed=17 + n)
    th = gpr.Theta(kernel, 0.25 * np.sqrt(d) * np.linspace(0.8, 1.3, d), 1.3, noise, float(y.mean()))
    Ky = jo._kernel_direct(th, X, X)
    Ky[np.diag_indices(n)] += noise
    L = np.linalg.cholesky(Ky)
    C = po.linv_of(L)
    alpha = C.T @ (C @ (y - th.mean_c))
    return X, y, th, C, alpha, np.random.default_rng(5).uniform(-0.2, 1.2, size=(m, d))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_oracle_against_the_textbook_form_and_the_marginals(n, d, kernel):
    for noise in NOISES:
        X, y, th, C, alpha, Xs = _case(n, d, kernel, noise)
        mean, cov = jo.predictive_joint(C, alpha, X, th, Xs, 0.0)
        m0, c0 = jo.textbook_joint(th, X, y, Xs, 0.0)
        e_cov = np.max(np.abs(cov - c0)) / th.variance
        e_mean = np.max(np.abs(mean - m0)) / max(1.0, np.max(np.abs(y)))
        gm, gv, _, _ = po.predictive_grad(C, alpha, X, th, Xs)
        e_diag = np.max(np.abs(np.diag(cov) + noise - gv))
        print(f"N={n} D={d} {kernel} noise={noise:g}: cov {e_cov:.2e}, mean {e_mean:.2e}, diag {e_diag:.2e}")
        assert e_cov <= 1e-10 and e_mean <= 1e-10
        assert e_diag <= 1e-12 and np.max(np.abs(mean - gm)) <= 1e-12 * max(1.0, np.max(np.abs(gm)))
        assert np.array_equal(cov, cov.T)
        # diag_add lands on the diagonal and nowhere else
        _, cov_y = jo.predictive_joint(C, alpha, X, th, Xs, noise)
        off = ~np.eye(Xs.shape[0], dtype=bool)
        assert np.array_equal(cov_y[off], cov[off]) and np.array_equal(np.diag(cov_y), np.diag(cov) + noise)


def test_draws_and_the_perturbation_bound():
    X, y, th, C, alpha, Xs = _case(40, 26, "Matern52", 1.0e-1, m=30)
    mean, cov = jo.predictive_joint(C, alpha, X, th, Xs, 1.0e-1)
    z = np.random.default_rng(3).standard_normal((7, 30))
    f = jo.draws(mean, cov, z)
    Lc = np.linalg.cholesky(cov)
    assert f.shape == (7, 30) and np.allclose(f[2], mean + Lc @ z[2], rtol=0, atol=1e-13)
    # a symmetric perturbation of size delta moves the factor by less than the first-order bound
    delta = 1e-8 * th.variance
    E = np.random.default_rng(4).uniform(-delta, delta, size=cov.shape)
    E = np.tril(E) + np.tril(E, -1).T
    moved = np.linalg.norm(np.linalg.cholesky(cov + E) - Lc)
    assert 0.0 < moved <= jo.chol_perturbation_bound(cov, delta)


# ---- the Python surface over a stub engine ----------------------------------------------------------------------------------
class JointEngine(RecordingEngine):
    """``RecordingEngine`` with the two joint calls answered by tests/joint_oracle.py."""

    def predict(self, xs, out=None):
        self.calls.append("predict")
        return super().predict(xs, out)

    def predict_joint(self, xs, diag_add=0.0):
        self.calls.append(("predict_joint", float(diag_add)))
        return jo.gpr_predict_joint(self.post, xs, diag_add)

    def sample_joint(self, xs, z, diag_add, want_samples=True):
        self.calls.append(("sample_joint", float(diag_add), bool(want_samples)))
        mean, cov = jo.gpr_predict_joint(self.post, xs, diag_add)
        f = jo.draws(mean, cov, z)
        return (f if want_samples else None), np.argmax(f, axis=1), np.max(f, axis=1)


class Float32JointEngine(JointEngine):
    dtype_name = "float32"

    def predict_joint(self, xs, diag_add=0.0):
        raise ValueError('gpso_predict_joint needs a GPSO_F64 or GPSO_MIXED context -- dtype="float64" or "mixed"')


def _model(engine=None, n=12):
    X, y = synthetic_problem(n, 2, seed=2)
    return HipGPR(data=(X, y[:, None]), kernel=K.Matern52(lengthscales=0.4, variance=1.0), mean_function=K.Constant(0.0),
                  noise_variance=1.0e-2, engine=engine or JointEngine())


def test_full_cov_shapes_and_noise_on_the_diagonal():
    m = _model()
    Xs = np.random.default_rng(1).random((9, 2))
    mean, cov = m.predict_f(Xs, full_cov=True)
    assert mean.shape == (9, 1) and cov.shape == (9, 9) and np.array_equal(cov, cov.T)
    mean_y, cov_y = m.predict_y(Xs, full_cov=True)
    assert mean_y.shape == (9, 1) and np.array_equal(np.asarray(mean_y), np.asarray(mean))
    assert np.allclose(cov_y - cov, 1.0e-2 * np.eye(9), rtol=0, atol=1e-15)
    assert ("predict_joint", 0.0) in m.engine.calls and ("predict_joint", 1.0e-2) in m.engine.calls
    # the marginals of the default path are the diagonal
    _, var = m.predict_f(Xs)
    assert np.max(np.abs(np.asarray(var)[:, 0] - np.diag(cov))) <= 1e-10


def test_default_paths_make_the_calls_they_made_before():
    m = _model()
    Xs = np.random.default_rng(1).random((5, 2))
    m.predict_y(Xs)
    m.predict_f(Xs)
    m.predict_f(Xs, full_cov=False)
    m.predict_y(Xs, full_cov=False)
    assert m.engine.calls == ["fit_eval", "predict", "predict", "predict", "predict"]
    a, b = m.predict_f(Xs), m.predict_f(Xs, False)
    assert a[0].shape == (5, 1) and a[1].shape == (5, 1) and np.array_equal(a[1], b[1])


def test_predict_f_samples_is_reproducible_from_a_seed():
    m = _model()
    Xs = np.random.default_rng(1).random((6, 2))
    a = m.predict_f_samples(Xs, 4, rng=11)
    b = m.predict_f_samples(Xs, num_samples=4, rng=np.random.default_rng(11))
    c = m.predict_f_samples(Xs, 4, rng=12)
    assert a.shape == (4, 6) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert m.predict_f_samples(Xs).shape == (1, 6)
    assert ("sample_joint", 1e-6, True) in m.engine.calls  # (GPflow's default_jitter)
    with pytest.raises(ValueError):
        m.predict_f_samples(Xs, 0)


def test_a_float32_engine_raises_the_argument_error_that_names_the_dtypes():
    m = _model(Float32JointEngine())
    with pytest.raises(ValueError, match='"float64".*"mixed"'):
        m.predict_f(np.zeros((3, 2)), full_cov=True)


def _surrogate(monkeypatch):
    monkeypatch.setattr(GPRSurrogate, "engine_factory", JointEngine)
    rng = np.random.default_rng(5)
    coords = rng.random((14, 2))
    scores = np.sin(3.0 * coords[:, 0]) + coords[:, 1] ** 2
    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.3, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy())
    surr.append(coords, scores)
    surr.gp_update()
    return surr, rng.random((11, 2))


def test_thompson_select_is_the_argmax_of_gp_sample_and_nothing_is_stored(monkeypatch):
    surr, cand = _surrogate(monkeypatch)
    stored = list(surr.points)
    f = surr.gp_sample(cand, 6, rng=21)
    idx, val = surr.thompson_select(cand, 6, rng=21)
    assert f.shape == (6, 11) and idx.shape == (6,) and val.shape == (6,)
    assert np.array_equal(idx, np.argmax(f, axis=1)) and np.array_equal(val, np.max(f, axis=1))
    calls = surr.gpflow_model.engine.calls
    assert calls[-2] == ("sample_joint", 1e-6, True) and calls[-1] == ("sample_joint", 1e-6, False)  # (the draws stay on the device)
    # noise=True: the model's predictive noise joins the jitter on the diagonal
    noise = surr.gpflow_model.predictive_noise()
    surr.gp_sample(cand, 2, rng=1, noise=True, jitter=1e-5)
    assert calls[-1] == ("sample_joint", 1e-5 + noise, True)
    mean, cov = surr.gp_predict_joint(cand)
    mean_y, cov_y = surr.gp_predict_joint(cand, noise=True)
    assert mean.shape == (11,) and cov.shape == (11, 11) and np.array_equal(mean, mean_y)
    assert np.allclose(cov_y - cov, noise * np.eye(11), rtol=0, atol=1e-15)
    assert list(surr.points) == stored
