"""
CPU checks of the trained inducing points: the oracle's dloss/dZ (tests/inducing_oracle.py) against central differences of
the oracles' own losses, the coincident-pair convention, and the host plumbing of ``train_inducing`` -- the optimiser's
vector, the policy at a change of the data, save / from_saved -- on a stub engine that answers from the oracles.
"""
import json
import os

import numpy as np
import pytest

from oracle import gpr
from tests import inducing_oracle as I
from tests import sgpr_oracle as S
from tests import svgp_oracle as V
from tests.helpers import synthetic_problem

KERNELS = ["Matern52", "Matern32", "Matern12", "SquaredExponential"]
LIKS = [("Gaussian", None), ("StudentT", 4.0)]
H = 1e-6  # the project's difference-quotient step (tests/test_sgpr_cpu.py, tests/test_svgp_cpu.py)


@pytest.fixture
def exact_diagonal(monkeypatch):
    # (as tests/test_sgpr_cpu.py: the quotient sees an exact diagonal of Kuu; the analytic gradient takes dk there as 0)
    sqd = gpr.scaled_sqdist

    def patched(X, X2, ls):
        r2 = sqd(X, X2, ls)
        if X2 is None or X2 is X:
            np.fill_diagonal(r2, 0.0)
        return r2

    monkeypatch.setattr(gpr, "scaled_sqdist", patched)


def _problem(n, d, m, seed, coincident=False):
    X, y = synthetic_problem(n, d, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    Z = rng.random((m, d))  # (away from X: no coincident pairs in Kuf, where Matern-1/2 has its kink)
    if coincident:
        Z[: m // 2] = X[3: 3 + m // 2]
    return X, y, Z


def _q(m, seed):
    rng = np.random.default_rng(seed)
    Sq = np.tril(0.2 * rng.standard_normal((m, m)), -1) + np.diag(0.5 + 0.4 * rng.random(m))
    return 0.5 * rng.standard_normal(m), Sq


def _quotient(loss, Z):
    fd = np.empty_like(Z)
    for i in range(Z.shape[0]):
        for k in range(Z.shape[1]):
            Zp, Zm = Z.copy(), Z.copy()
            Zp[i, k] += H
            Zm[i, k] -= H
            fd[i, k] = (loss(Zp) - loss(Zm)) / (2 * H)
    return fd


def _hyper(d, ard):
    return (np.array([0.6, 0.9, 1.3])[:d] if ard else 0.8), (d if ard else 1)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ard", [False, True])
def test_sgpr_grad_z_matches_central_differences(kernel, ard, exact_diagonal):
    n, d, m = 40, 3, 9
    X, y, Z = _problem(n, d, m, seed=3)
    ls, n_ls = _hyper(d, ard)
    u = S.initial_u(ls, 1.3, 0.05, 0.2)
    gz = I.sgpr_grad_z(kernel, u, n_ls, True, 0.0, X, y, Z)
    fd = _quotient(lambda Zq: -S.bound(kernel, u, n_ls, True, 0.0, X, y, Zq), Z)
    err = np.max(np.abs(gz - fd) / np.maximum(1.0, np.abs(fd)))
    print(f"SGPR {kernel} ard={ard}: max |grad_z - fd| / max(1, |fd|) = {err:.3g}")
    assert err <= 1e-6
    # the device's ordering of the same sum agrees to rounding
    gg = I.sgpr_grad_z(kernel, u, n_ls, True, 0.0, X, y, Z, contract=I.contract_z_gemm)
    assert np.max(np.abs(gg - gz)) <= 1e-10 * max(1.0, np.max(np.abs(gz)))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("lik", LIKS, ids=["gauss", "studentt"])
@pytest.mark.parametrize("ard", [False, True])
def test_svgp_grad_z_matches_central_differences(kernel, lik, ard, exact_diagonal):
    n, d, m = 40, 3, 9
    X, y, Z = _problem(n, d, m, seed=7)
    mu, Sq = _q(m, 3)  # (a non-trivial q)
    ls, n_ls = _hyper(d, ard)
    u = V.initial_u(ls, 1.3, 0.3 if lik[0] == "StudentT" else 0.05, lik, c=0.2)
    gz = I.svgp_grad_z(kernel, u, n_ls, True, 0.0, X, y, Z, mu, Sq, lik)
    fd = _quotient(lambda Zq: V.neg_elbo(kernel, u, n_ls, True, 0.0, X, y, Zq, mu, Sq, lik), Z)
    print(f"SVGP {kernel} {lik[0]} ard={ard}: max |grad_z - fd| = {np.max(np.abs(gz - fd)):.3g} of {np.max(np.abs(fd)):.3g}")
    np.testing.assert_allclose(gz, fd, rtol=2e-6, atol=2e-6 * max(1.0, np.max(np.abs(fd))))


@pytest.mark.parametrize("kernel", KERNELS)
def test_coincident_pairs_contribute_zero(kernel, exact_diagonal):
    """Rows of Z copied from X: the gradient is finite for every kernel, and for the kernels that are differentiable at
    r = 0 it is still the derivative of the loss (the Matern-1/2 has a kink there: 0 is the convention, not a limit)."""
    n, d, m = 40, 3, 8
    X, y, Z = _problem(n, d, m, seed=5, coincident=True)
    assert np.sum(I.r2_direct(Z, X, np.ones(d)) == 0.0) == m // 2
    u = S.initial_u(0.8, 1.3, 0.05, 0.2)
    gz = I.sgpr_grad_z(kernel, u, 1, True, 0.0, X, y, Z)
    mu, Sq = _q(m, 4)
    lik = ("StudentT", 4.0)
    uv = V.initial_u(0.8, 1.3, 0.3, lik, c=0.2)
    gv = I.svgp_grad_z(kernel, uv, 1, True, 0.0, X, y, Z, mu, Sq, lik)
    assert np.all(np.isfinite(gz)) and np.all(np.isfinite(gv))
    if kernel == "Matern12":
        return
    fd = _quotient(lambda Zq: -S.bound(kernel, u, 1, True, 0.0, X, y, Zq), Z)
    assert np.max(np.abs(gz - fd) / np.maximum(1.0, np.abs(fd))) <= 1e-6
    fdv = _quotient(lambda Zq: V.neg_elbo(kernel, uv, 1, True, 0.0, X, y, Zq, mu, Sq, lik), Z)
    np.testing.assert_allclose(gv, fdv, rtol=2e-6, atol=2e-6 * max(1.0, np.max(np.abs(fdv))))


# ---- host plumbing on a stub engine ------------------------------------------------------------------------------------
class StubEngine:
    """The engine calls HipSGPR / HipSVGP make, answered by the oracles in float64 on the host."""

    dtype_name = "float64"

    def __init__(self, dtype="float64", device=0, **options):
        self.calls = []
        self.n = self.d = 0
        self.lik = ("Gaussian", None)
        self.Z = self.q = self.post = None

    def set_timing(self, on):
        pass

    def close(self):
        pass

    def set_data(self, x, y):
        self.calls.append("set_data")
        self.X, self.y = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)
        self.n, self.d = self.X.shape
        self.Z = self.q = self.post = None

    def sgpr_set_inducing(self, Z):
        self.calls.append("sgpr_set_inducing")
        self.Z = np.array(Z, dtype=np.float64)
        self.n = self.Z.shape[0]
        self.q = (np.zeros(self.n), np.eye(self.n))

    def sgpr_select_inducing(self, kernel, u, n_ls, m):
        self.calls.append("sgpr_select_inducing")
        idx = S.greedy_select(kernel, self.X, gpr.softplus(np.asarray(u)[:n_ls]), float(gpr.softplus(u[n_ls])), m)
        self.sgpr_set_inducing(self.X[idx])
        self.calls.pop()
        return idx

    def sgpr_get_inducing(self):
        return self.Z.copy(), self.X.shape[0]

    def sgpr_move_inducing(self, Z):
        self.calls.append("sgpr_move_inducing")
        assert np.shape(Z) == self.Z.shape
        self.Z = np.array(Z, dtype=np.float64)

    def sgpr_bound_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, want_grad=True):
        self.calls.append("sgpr_bound_u")
        f, g, th = S.neg_bound_and_grad_u(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, self.Z)
        return f, (g if want_grad else None), th

    def sgpr_bound_uz(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, Z=None, want_grad=True):
        self.calls.append("sgpr_bound_uz")
        assert len(u) == n_ls + 2 + (1 if train_mean else 0)
        if Z is not None:
            assert np.shape(Z) == self.Z.shape
            self.Z = np.array(Z, dtype=np.float64)
        f, g, gz = I.sgpr_loss_and_grads(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, self.Z)
        return f, (g if want_grad else None), (gz if want_grad else None), None

    def sgpr_posterior(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        self.calls.append("sgpr_posterior")
        self.post = S.Posterior(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, self.Z)
        return 0.0

    def predict(self, Xnew):
        return self.post.predict_y(np.asarray(Xnew, dtype=np.float64))

    # the SVGP's
    def vgp_set_likelihood(self, kind, df=0.0, n_gh=20):
        self.lik = (kind, df if kind == "StudentT" else None)

    def svgp_init_q(self, kernel=None, u=None, n_ls=1, train_mean=False, mean_c_fixed=0.0, noise_variance=0.0):
        if noise_variance > 0.0:
            self.q = V.conjugate_start(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, self.Z, self.lik, noise_variance)
        else:
            self.q = (np.zeros(self.n), np.eye(self.n))

    def svgp_set_q(self, mu=None, S=None):
        self.q = (np.array(mu, dtype=np.float64), np.array(S, dtype=np.float64))

    def svgp_get_q(self):
        return self.q[0].copy(), self.q[1].copy()

    def svgp_natgrad(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, gamma=1.0):
        self.calls.append("svgp_natgrad")
        self.q = V.natgrad(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, self.Z, *self.q, self.lik, gamma)

    def svgp_elbo_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, want_grad=True):
        self.calls.append("svgp_elbo_u")
        f, g, th = V.neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, self.Z, *self.q, self.lik)
        return f, (g if want_grad else None), th

    def svgp_elbo_uz(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, Z=None, want_grad=True):
        self.calls.append("svgp_elbo_uz")
        assert len(u) == n_ls + 2 + (1 if train_mean else 0)
        if Z is not None:
            self.Z = np.array(Z, dtype=np.float64)
        f, g, gz = I.svgp_loss_and_grads(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, self.Z, *self.q, self.lik)
        return f, (g if want_grad else None), (gz if want_grad else None), None

    def svgp_posterior(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        self.calls.append("svgp_posterior")
        self.post = V.Posterior(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.Z, *self.q, self.lik)
        return 0.0


def test_train_inducing_is_accepted_and_validated():
    from pygpso_amd import SGPRSurrogate, SVGPSurrogate
    from pygpso_amd import kernels as K
    from pygpso_amd.sgpr import HipSGPR

    assert SGPRSurrogate(gp_kernel=K.Matern52()).train_inducing is False
    assert SVGPSurrogate(gp_kernel=K.Matern52()).train_inducing is False
    assert SGPRSurrogate(gp_kernel=K.Matern52(), train_inducing=True, num_inducing=16).train_inducing is True
    assert SVGPSurrogate(gp_kernel=K.Matern52(), train_inducing=True, likelihood=K.StudentT(0.3, 4.0)).train_inducing is True
    assert SGPRSurrogate.default(num_inducing=32, train_inducing=True).train_inducing is True
    for cls in (SGPRSurrogate, SVGPSurrogate):
        with pytest.raises(TypeError):
            cls(gp_kernel=K.Matern52(), train_inducing="yes")
        with pytest.raises(TypeError):
            cls(gp_kernel=K.Matern52(), train_inducing=1)
    X, y = synthetic_problem(20, 2, seed=0)
    with pytest.raises(TypeError):
        HipSGPR((X, y[:, None]), K.Matern52(), num_inducing=4, engine=StubEngine(), train_inducing=None)


def test_pack_and_assign_carry_z_through_the_optimisers_vector():
    from pygpso_amd import kernels as K
    from pygpso_amd.sgpr import HipSGPR
    from pygpso_amd.svgp import HipSVGP

    X, y = synthetic_problem(60, 3, seed=1)
    m = 8
    for ard in (False, True):
        ls = np.array([0.5, 0.7, 0.9]) if ard else 0.6
        for make in (lambda e, t: HipSGPR((X, y[:, None]), K.Matern52(lengthscales=ls), K.Constant(0.1), num_inducing=m,
                                          engine=e, train_inducing=t),
                     lambda e, t: HipSVGP((X, y[:, None]), K.Matern52(lengthscales=ls), K.Constant(0.1),
                                          likelihood=K.StudentT(0.3, 4.0), num_inducing=m, engine=e, train_inducing=t)):
            fixed, eng = make(StubEngine(), False), StubEngine()
            model = make(eng, True)
            nt = (3 if ard else 1) + 3
            u0 = model._pack()
            assert fixed._pack().shape == (nt,) and u0.shape == (nt + m * 3,)
            np.testing.assert_array_equal(u0[:nt], fixed._pack())
            np.testing.assert_array_equal(u0[nt:].reshape(m, 3), eng.Z)  # (Z starts at the greedy picks)
            np.testing.assert_array_equal(model.trainable_variables, u0)
            assert "(trained)" in model.summary() and "(not trained)" in fixed.summary()
            # an evaluation goes through the moving-Z entry point with theta and Z split, and returns the long gradient
            f, g = model._loss_and_grad(u0)
            assert eng.calls[-1] in ("sgpr_bound_uz", "svgp_elbo_uz") and g.shape == u0.shape and np.isfinite(f)
            f_fixed, g_fixed = fixed._loss_and_grad(fixed._pack())
            assert fixed.engine.calls[-1] in ("sgpr_bound_u", "svgp_elbo_u")
            assert f == pytest.approx(f_fixed, rel=1e-12)
            np.testing.assert_allclose(g[:nt], g_fixed, rtol=1e-9, atol=1e-12)
            # _assign splits the vector: the hyper-parameters into the model, Z onto the device
            u1 = u0 + 0.01 * np.arange(u0.shape[0]) / u0.shape[0]
            model._assign(u1)
            np.testing.assert_allclose(model._pack(), u1, rtol=1e-12, atol=1e-14)
            np.testing.assert_array_equal(eng.Z, u1[nt:].reshape(m, 3))
            assert eng.calls[-1] == "sgpr_move_inducing"
            np.testing.assert_array_equal(model.parameter_dict()[".inducing_variable.Z"], eng.Z)


def test_policy_at_a_change_of_the_data():
    """N <= M: Z is the data and is not trained; the first time N > M the selection runs; afterwards the trained Z is
    kept and nothing is selected.  Without train_inducing every change of the data selects again."""
    from pygpso_amd import kernels as K
    from pygpso_amd.sgpr import HipSGPR

    X, y = synthetic_problem(90, 2, seed=2)
    m = 16
    for train, want in ((True, 1), (False, 3)):
        eng = StubEngine()
        model = HipSGPR((X[:10], y[:10, None]), K.Matern52(lengthscales=0.5), K.Constant(0.0), num_inducing=m, engine=eng,
                        train_inducing=train)
        assert model._pack().shape == (4,) and "(not trained)" in model.summary()  # N <= M
        np.testing.assert_array_equal(eng.Z, X[:10])
        for n in (40, 60, 90):
            model.data = (X[:n], y[:n, None])
            assert model._pack().shape == ((4 + m * 2,) if train else (4,))
            if train:
                z_before = eng.Z.copy()
                K.Scipy().minimize(model.training_loss, model.trainable_variables)
                assert not np.array_equal(eng.Z, z_before)  # (the search moved Z, and the model holds what the device holds)
                np.testing.assert_array_equal(model._pack()[4:].reshape(m, 2), eng.Z)
                z_trained = eng.Z.copy()
        assert eng.calls.count("sgpr_select_inducing") == want
        if train:  # the kept Z is the trained one, and a smaller data set ends the training of Z
            model.data = (X, y[:, None])
            np.testing.assert_array_equal(eng.Z, z_trained)
            model.data = (X[:12], y[:12, None])
            assert model._pack().shape == (4,)
            np.testing.assert_array_equal(eng.Z, X[:12])


# the end-to-end problem of tests/test_gpu_inducing.py (END_TO_END, Y_NOISE there), restated: picked here, on the oracle alone
END_TO_END = {"SGPR": dict(kernel="Matern32", m=16, maxiter=5), "SVGP": dict(kernel="Matern52", m=24, maxiter=10)}


def _end_to_end_surrogate(which, train):
    from pygpso_amd import SGPRSurrogate, SVGPSurrogate
    from pygpso_amd import kernels as K

    cfg = END_TO_END[which]
    kernel = getattr(K, cfg["kernel"])(lengthscales=0.5)
    optimiser = K.Scipy(options={"maxiter": cfg["maxiter"]})
    if which == "SGPR":
        return SGPRSurrogate(gp_kernel=kernel, gp_meanf=K.Constant(0.0), gauss_likelihood_sigma=1e-2, num_inducing=cfg["m"],
                             optimiser=optimiser, train_inducing=train)
    return SVGPSurrogate(gp_kernel=kernel, gp_meanf=K.Constant(0.0), num_inducing=cfg["m"], likelihood=K.StudentT(0.3, 4.0),
                         natgrad_learning_rate=0.5, train_iterations=3, optimiser=optimiser, train_inducing=train)


@pytest.mark.parametrize("d", [2, 12])
@pytest.mark.parametrize("which", ["SGPR", "SVGP"])
def test_joint_search_on_the_oracle_is_no_worse_than_the_fixed_z_search(which, d, monkeypatch):
    """The end-to-end problem of tests/test_gpu_inducing.py on the oracle alone (the surrogates on the stub engine): from
    the same start the capped L-BFGS-B search ends lower with Z trained than with Z fixed, with room to spare against the
    device test's slack, and it ends where the comparison with the device means something -- the oracle's two float64
    restatements of the gradient (GEMM-form r^2 against direct differences throughout) agree to a tenth of the 2e-9 the
    device is held to."""
    import pygpso_amd.model as model_module

    monkeypatch.setattr(model_module, "HipGPEngine", StubEngine)
    X, y = synthetic_problem(300, d, seed=11)
    y = y + 0.1 * np.random.default_rng(12).standard_normal(300)
    final = {}
    for train in (False, True):
        s = _end_to_end_surrogate(which, train)
        s.append(X, y)
        s.gp_update()
        final[train] = s.gpflow_model.training_loss()
    model, cfg = s.gpflow_model, END_TO_END[which]
    uz, nt = model._pack(), model._n_theta()
    u, Z = uz[:nt], uz[nt:].reshape(cfg["m"], d)

    def reference():
        if which == "SGPR":
            return I.sgpr_loss_and_grads(cfg["kernel"], u, 1, True, 0.0, X, y, Z)
        mu, Sq = model.get_q()
        return I.svgp_loss_and_grads(cfg["kernel"], u, 1, True, 0.0, X, y, Z, mu, Sq, ("StudentT", 4.0))

    _, gu, gz = reference()
    with I.direct_r2_everywhere():
        _, gu2, gz2 = reference()
    spread = (np.max(np.abs(gu2 - gu)) / np.max(np.abs(gu)), np.max(np.abs(gz2 - gz)) / np.max(np.abs(gz)))
    print(f"{which} D={d}: fixed Z {final[False]:.6f}; trained Z {final[True]:.6f}; spread grad_u {spread[0]:.3g} grad_z {spread[1]:.3g}")
    assert final[True] <= final[False] - 1.0  # (room to spare: the device test allows +max(1e-3, 1e-6 |loss|))
    assert max(spread) <= 2e-10


def test_z_travels_once_and_comes_back_after_a_failed_evaluation():
    """The device's Z follows the model's: an evaluation at the Z the device already holds sends none, ``_assign`` moves Z
    only when it differs, and an evaluation that raises after it replaced the device's rows (Kuu not positive definite
    where rows of Z collapse) puts the model's Z back before the error leaves."""
    from pygpso_amd import kernels as K
    from pygpso_amd.sgpr import HipSGPR

    class Engine(StubEngine):
        fail = False

        def sgpr_bound_uz(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, Z=None, want_grad=True):
            self.sent = Z is not None
            if self.fail:
                self.Z = np.array(Z, dtype=np.float64)
                raise np.linalg.LinAlgError("Kuu = k(Z, Z) + 1e-6 I is not positive definite")
            return super().sgpr_bound_uz(kernel, u, n_ls, train_mean, mean_c_fixed, Z, want_grad)

    X, y = synthetic_problem(60, 2, seed=1)
    eng = Engine()
    model = HipSGPR((X, y[:, None]), K.Matern52(lengthscales=0.6), K.Constant(0.1), num_inducing=8, engine=eng,
                    train_inducing=True)
    u0 = model._pack()
    model._loss_and_grad(u0)
    assert not eng.sent  # (the device holds the picks already)
    u1 = u0.copy()
    u1[4:] += 0.01
    model._loss_and_grad(u1)
    assert eng.sent
    moves = eng.calls.count("sgpr_move_inducing")
    model._assign(u1)  # (the point of the last evaluation: nothing to move)
    assert eng.calls.count("sgpr_move_inducing") == moves
    model._assign(u0)
    assert eng.calls.count("sgpr_move_inducing") == moves + 1
    model._loss_and_grad(u0)
    assert not eng.sent  # (as under Adam: the step after _assign evaluates at the Z that call moved)
    eng.fail = True
    with pytest.raises(np.linalg.LinAlgError):
        model._loss_and_grad(u1)
    np.testing.assert_array_equal(eng.Z, u0[4:].reshape(8, 2))  # the device is back at the Z the model holds
    np.testing.assert_array_equal(model.inducing_points, model._pack()[4:].reshape(8, 2))


@pytest.mark.parametrize("which", ["SGPR", "SVGP"])
def test_save_and_from_saved_keep_the_policy_and_z(which, tmp_path, monkeypatch):
    import pygpso_amd.model as model_module
    from pygpso_amd import SGPRSurrogate, SVGPSurrogate
    from pygpso_amd import kernels as K

    monkeypatch.setattr(model_module, "HipGPEngine", StubEngine)
    X, y = synthetic_problem(50, 2, seed=4)
    Xs = np.random.default_rng(5).random((20, 2))

    def make(train):
        if which == "SGPR":
            return SGPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.5), gp_meanf=K.Constant(0.0), num_inducing=8,
                                 optimiser=K.Scipy(options={"maxiter": 8}) if train else None, train_inducing=train)
        return SVGPSurrogate(gp_kernel=K.Matern52(lengthscales=0.5), gp_meanf=K.Constant(0.0), num_inducing=8,
                             likelihood=K.StudentT(0.3, 4.0), natgrad_learning_rate=0.5, train_iterations=3,
                             optimiser=K.Scipy(options={"maxiter": 8}) if train else None, train_inducing=train)

    s = make(True)
    s.append(X, y)
    s.gp_update()
    z = s.gpflow_model.inducing_points
    mean, var = s.gpflow_model.predict_y(Xs)
    folder = str(tmp_path / "trained")
    s.save(folder)
    with open(os.path.join(folder, s.GPR_INFO)) as fh:
        info = json.load(fh)
    assert info["train_inducing"] is True and info["inducing"] == "greedy"
    r = type(s).from_saved(folder)
    assert r.train_inducing is True and r.gpflow_model.train_inducing is True
    assert isinstance(r.optimiser, K.Scipy) and r.optimiser.options == {"maxiter": 8}  # (the cap travels with the run)
    np.testing.assert_array_equal(r.gpflow_model.inducing_points, z)
    mean_r, var_r = r.gpflow_model.predict_y(Xs)
    np.testing.assert_allclose(mean_r, mean, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(var_r, var, rtol=1e-9, atol=1e-12)
    # the resumed run continues from the trained Z: one more update, no selection
    eng = r.gpflow_model.engine
    eng.calls.clear()
    Xn, yn = synthetic_problem(10, 2, seed=6)
    r.append(Xn, yn)
    r.gp_update()
    assert "sgpr_select_inducing" not in eng.calls and ("sgpr_bound_uz" in eng.calls or "svgp_elbo_uz" in eng.calls)
    # a surrogate that does not train Z writes no key, and a directory without the key loads as train_inducing=False
    s0 = make(False)
    s0.append(X, y)
    s0.gp_update()
    folder0 = str(tmp_path / "fixed")
    s0.save(folder0)
    with open(os.path.join(folder0, s0.GPR_INFO)) as fh:
        assert "train_inducing" not in json.load(fh)
    r0 = type(s0).from_saved(folder0)
    assert r0.train_inducing is False and r0.gpflow_model.train_inducing is False
    assert r0.gpflow_model._pack().shape == (4,)


def test_product_modules_do_not_import_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("sgpr.py", "svgp.py", "gp_surrogate.py", "engine.py"):
        with open(os.path.join(root, "pygpso_amd", name)) as fh:
            assert "oracle" not in fh.read(), name


def test_the_two_restatements_agree_where_the_problem_is_well_conditioned():
    """``direct_r2_everywhere`` swaps the GEMM-form r^2 for direct differences in every kernel matrix and puts it back; at
    a well-conditioned point both restatements give the same gradient to rounding (their distance is what the device tests
    use as the size of float64 rounding at an ill-conditioned one)."""
    X, y, Z = _problem(40, 3, 9, seed=3)
    u = S.initial_u(0.8, 1.3, 0.05, 0.2)
    before = gpr.scaled_sqdist
    f0, gu0, gz0 = I.sgpr_loss_and_grads("Matern52", u, 1, True, 0.0, X, y, Z)
    with I.direct_r2_everywhere():
        assert gpr.scaled_sqdist is not before
        f1, gu1, gz1 = I.sgpr_loss_and_grads("Matern52", u, 1, True, 0.0, X, y, Z)
    assert gpr.scaled_sqdist is before
    assert abs(f1 - f0) <= 1e-12 * abs(f0)
    assert np.max(np.abs(gu1 - gu0)) <= 1e-10 * np.max(np.abs(gu0))
    assert np.max(np.abs(gz1 - gz0)) <= 1e-10 * np.max(np.abs(gz0))
