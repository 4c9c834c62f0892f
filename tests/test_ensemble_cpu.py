"""CPU checks of the hyper-parameter ensemble's host side: the fold of csrc/ensemble.hpp through
``gpso_ensemble_fold_host`` against tests/ensemble_oracle.py, and the priors of pygpso_amd/priors.py in the training loss."""
import numpy as np
import pytest

from tests import acq_oracle, ensemble_oracle as eo

KS = (1, 2, 7, 32)
M = 96


@pytest.fixture(scope="module")
def fold():
    import __graft_entry__ as entry
    from pygpso_amd import HipGPEngine, _lib

    import os
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return HipGPEngine.ensemble_fold_host


def _columns(k, seed):
    rng = np.random.default_rng([seed, k])
    mean = rng.normal(0.0, 1.0, (k, M))
    var = rng.uniform(1e-4, 2.0, (k, M)) ** 2
    noise = rng.uniform(1e-6, 1e-4, k)
    return mean, var, noise


def _spec(kind, **kw):
    from pygpso_amd import acquisition as A

    return {eo.UCB_VAR: lambda: A.UCBVar(kw.get("varsigma", 1.7)), eo.UCB_STD: lambda: A.UCBStd(kw.get("varsigma", 1.7), latent=kw.get("latent", False)),
            eo.EI: lambda: A.EI(xi=kw.get("xi", 0.0), latent=kw.get("latent", False)),
            eo.LOGEI: lambda: A.LogEI(xi=kw.get("xi", 0.0), latent=kw.get("latent", False)),
            eo.PI: lambda: A.PI(xi=kw.get("xi", 0.0), latent=kw.get("latent", False))}[kind]()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", (eo.UCB_VAR, eo.UCB_STD))
def test_ucb_kinds_and_moments_are_the_written_out_expression_bitwise(fold, kind, k):
    mean, var, noise = _columns(k, 1)
    got = fold(_spec(kind, varsigma=1.7), mean, var, noise)
    want = eo.fold_numpy(kind, mean, var, 1.7)
    for g, w, name in zip(got, want, ("mean_mix", "var_mix", "value")):
        assert np.array_equal(g, w), (name, k, np.max(np.abs(g - w)))


@pytest.mark.parametrize("k", KS)
def test_var_mix_is_the_two_pass_moment_match(fold, k):
    mean, var, noise = _columns(k, 2)
    mean_mix, var_mix, _ = fold(_spec(eo.UCB_VAR), mean, var, noise)
    # the mixture's moments: E[y] and E[var] + Var[mean], to rounding
    assert np.allclose(mean_mix, mean.mean(axis=0), rtol=1e-14, atol=1e-15)
    assert np.allclose(var_mix, var.mean(axis=0) + mean.var(axis=0), rtol=1e-13)
    w_mean, w_var = eo.moments_numpy(mean, var)
    assert np.array_equal(mean_mix, w_mean) and np.array_equal(var_mix, w_var)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("latent", (False, True))
@pytest.mark.parametrize("kind", (eo.EI, eo.PI, eo.LOGEI))
def test_improvement_kinds_within_the_acquisition_oracles_tolerance(fold, kind, latent, k):
    mean, var, noise = _columns(k, 3)
    inc = 0.8
    _, _, got = fold(_spec(kind, latent=latent, xi=0.01), mean, var, noise, incumbent=inc)
    want = eo.fold_truth(kind, mean, var, noise, latent=latent, incumbent=inc, xi=0.01)
    tol, yard = acq_oracle.tolerance(kind)
    err = acq_oracle.error(kind, got, want)
    print(f"kind {kind} latent {latent} K {k}: error {err:.3e}, tolerance {tol:.3e} (yardstick {yard:.3e})")
    assert err <= tol


def test_logei_is_finite_where_every_members_ei_is_zero_in_float64(fold):
    from pygpso_amd import HipGPEngine

    k = 7
    s = np.full((k, 5), 1.0e-2)
    mean = -np.linspace(0.5, 3.0, k * 5).reshape(k, 5)  # z from -50 to -300
    ei = np.array([HipGPEngine.acq_eval_host(_spec(eo.EI), mean[i], s[i] ** 2, 0.0, 0.0) for i in range(k)])
    assert np.all(ei == 0.0)
    _, _, got = fold(_spec(eo.LOGEI), mean, s ** 2, np.zeros(k), incumbent=0.0)
    assert np.all(np.isfinite(got)) and np.all(got < -1000.0)
    want = eo.fold_truth(eo.LOGEI, mean, s ** 2, incumbent=0.0)
    assert acq_oracle.error(eo.LOGEI, got, want) <= acq_oracle.tolerance(eo.LOGEI)[0]


def test_minus_infinity_nan_and_a_single_member(fold):
    from pygpso_amd import HipGPEngine

    k = 4
    # s == 0 and d < 0 in every member: EI = 0, LOGEI = log 0 = -inf -> the fold is -inf, not NaN
    mean, var = np.full((k, 3), -1.0), np.zeros((k, 3))
    _, _, v = fold(_spec(eo.LOGEI), mean, var, np.zeros(k), incumbent=0.0)
    assert np.all(np.isneginf(v))
    # ... and -inf in some members only is their EI of zero in the mean
    var2 = var.copy()
    var2[0] = 1.0
    _, _, v2 = fold(_spec(eo.LOGEI), mean, var2, np.zeros(k), incumbent=0.0)
    one = HipGPEngine.acq_eval_host(_spec(eo.LOGEI), mean[0], var2[0], 0.0, 0.0)
    assert np.allclose(v2, one - np.log(k), rtol=0, atol=1e-14 * np.abs(one).max())
    # a NaN member: NaN, for every kind
    mean3, var3, noise3 = _columns(k, 5)
    mean3[2, 1] = np.nan
    for kind in (eo.UCB_VAR, eo.UCB_STD, eo.EI, eo.LOGEI, eo.PI):
        mm, vm, val = fold(_spec(kind), mean3, var3, noise3, incumbent=0.0)
        assert np.isnan(val[1]) and np.isnan(mm[1]) and np.isnan(vm[1])
        assert not np.any(np.isnan(np.delete(val, 1)))
    # K = 1: the member's own three numbers, bit for bit
    mean1, var1, noise1 = _columns(1, 6)
    for kind in (eo.UCB_VAR, eo.UCB_STD, eo.EI, eo.LOGEI, eo.PI):
        for latent in (False, True):
            spec = _spec(kind, latent=latent) if kind != eo.UCB_VAR else _spec(kind)
            mm, vm, val = fold(spec, mean1, var1, noise1, incumbent=0.3)
            own = HipGPEngine.acq_eval_host(spec, mean1[0], var1[0], noise1[0], 0.3)
            assert np.array_equal(mm, mean1[0]) and np.array_equal(vm, var1[0]) and np.array_equal(val, own), (kind, latent)


def test_mes_and_bad_arguments_are_refused(fold):
    from pygpso_amd import _lib, acquisition as A

    mean, var, noise = _columns(2, 7)
    with pytest.raises(_lib.GpsoHipError) as err:
        fold(A.MES(), mean, var, noise)
    assert err.value.code == _lib.E_ARG
    with pytest.raises(_lib.GpsoHipError):
        fold(A.EI(latent=True), mean, var, None, incumbent=0.0)  # a latent kind reads the members' noise
    with pytest.raises(_lib.GpsoHipError):
        fold(A.UCBVar(1.0), np.zeros((33, 2)), np.ones((33, 2)), np.zeros(33))  # more members than GPSO_ENSEMBLE_MAX
    assert _lib.ENSEMBLE_MAX == 32 and _lib.ENSEMBLE_THETA == 51


# ---- priors -----------------------------------------------------------------------------------------------------------
class _DoubleEngine:
    """A test-double engine: returns fixed arrays and counts what it was asked."""

    dtype_name = "float64"

    def __init__(self, nu):
        self.f, self.g = 3.25, np.arange(1.0, nu + 1.0)
        self.theta = np.ones(nu + 1)

    def set_data(self, x, y):
        pass

    def fit_eval_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        return self.f, self.g, self.theta

    def fit_batch_max(self):
        return 256

    def fit_eval_u_batch(self, kernel, U, n_ls, train_mean, mean_c_fixed=0.0):
        self.loss, self.grad, self.ok = np.full(U.shape[0], self.f), np.tile(self.g, (U.shape[0], 1)), np.ones(U.shape[0], dtype=bool)
        return self.loss, self.grad, self.ok


def _model(train_mean=True, ard=False):
    from pygpso_amd.kernels import Constant, Matern52
    from pygpso_amd.model import HipGPR

    d = 3
    ls = np.array([0.3, 0.6, 1.2]) if ard else 0.4
    x = np.random.default_rng(0).random((6, d))
    nu = (d if ard else 1) + 2 + (1 if train_mean else 0)
    eng = _DoubleEngine(nu)
    m = HipGPR((x, x[:, :1]), Matern52(variance=1.3, lengthscales=ls), Constant(0.2) if train_mean else None, noise_variance=2e-3, engine=eng)
    return m, eng


def test_without_priors_the_loss_is_the_engines_numbers_untouched():
    m, eng = _model()
    u = m._pack()
    f, g = m._loss_and_grad(u)
    assert f == eng.f and g is eng.g
    loss, grad, ok = m._loss_and_grad_batch(np.stack([u, u + 0.1]))
    assert loss is eng.loss and grad is eng.grad and ok is eng.ok
    assert m.neg_log_prior() == 0.0 and m._prior_slots() is None


@pytest.mark.parametrize("ard", (False, True))
def test_prior_density_jacobian_and_gradient(ard):
    from pygpso_amd import priors as P

    m, eng = _model(ard=ard)
    P.attach(m, {"lengthscales": P.LogNormal(0.5, 1.0), "variance": P.LogNormal(1.0, 1.5), "noise": P.LogNormal(1e-3, 2.0),
                 "mean": P.Normal(0.1, 2.0)})
    n_ls = 3 if ard else 1
    slots = [(("lognormal", 0.5, 1.0), "softplus")] * n_ls + [(("lognormal", 1.0, 1.5), "softplus"), (("lognormal", 1e-3, 2.0), "softplus"),
                                                               (("normal", 0.1, 2.0), "identity")]
    rng = np.random.default_rng(3)
    for trial in range(5):
        u = m._pack() + rng.normal(0.0, 1.0, n_ls + 3)
        f, g = m._loss_and_grad(u)
        want = eo.neg_log_prior(u, slots)
        assert abs((f - eng.f) - want) <= 1e-12 * max(1.0, abs(want))
        # the Jacobian term is there: without it the value differs by sum log sigmoid(u) over the softplus slots
        no_jac = want - float(np.sum(np.logaddexp(0.0, -u[: n_ls + 2])))
        assert abs((f - eng.f) - no_jac) > 1e-3
        num = np.empty_like(u)
        for i in range(u.shape[0]):
            h = 1e-5
            e = np.zeros_like(u)
            e[i] = h
            num[i] = (eo.neg_log_prior(u + e, slots) - eo.neg_log_prior(u - e, slots)) / (2 * h)
        assert np.allclose(g - eng.g, num, rtol=1e-7, atol=1e-8), (g - eng.g, num)
        # the batch form adds the same term row by row
        loss, grad, ok = m._loss_and_grad_batch(np.stack([u, u]))
        assert np.array_equal(loss, np.array([f, f])) and np.array_equal(grad[1], g) and ok.all()
    # the noise prior applies to the part above NOISE_FLOOR, and a partial set of priors leaves the other slots alone
    m2, eng2 = _model(train_mean=False)
    P.attach(m2, {"noise": P.LogNormal(1e-3, 2.0)})
    u = m2._pack()
    f, g = m2._loss_and_grad(u)
    above = m2.likelihood.variance - 1.0e-6
    assert abs(np.logaddexp(0.0, u[2]) - above) < 1e-15
    assert abs((f - eng2.f) - eo.neg_log_prior(u, [(None, "softplus"), (None, "softplus"), (("lognormal", 1e-3, 2.0), "softplus")])) < 1e-12
    assert g[0] == eng2.g[0] and g[1] == eng2.g[1] and g[2] != eng2.g[2]


def test_training_loss_carries_the_prior_and_the_marginal_likelihood_does_not():
    from pygpso_amd import priors as P

    m, eng = _model()
    m._last_nlml = 5.0
    m._ensure_resident = lambda: None
    assert m.training_loss() == 5.0
    P.attach(m, P.default_priors())
    assert m.training_loss() == 5.0 + m.neg_log_prior() and m.neg_log_prior() != 0.0
    assert m.log_marginal_likelihood() == -5.0
    with pytest.raises(ValueError):
        P.attach(m, {"lengthscale": P.LogNormal(1.0, 1.0)})
    with pytest.raises(ValueError):
        P.LogNormal(-1.0, 1.0)
