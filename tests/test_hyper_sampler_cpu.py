"""CPU checks of pygpso_amd/hyper_sampler.py: the lockstep HMC sampler on targets given as callables -- a known density, a
callable whose rows fail, and the multimodal toy problem's posterior over the float64 oracle's NLML."""
import numpy as np
import pytest

from pygpso_amd.hyper_sampler import sample_theta


class _Normal3:
    """-log density of a 3-D standard normal, as a batch callable; counts its calls."""

    def __init__(self, fail_every=0):
        self.calls = self.rows = 0
        self.fail_every = fail_every

    def __call__(self, U):
        self.calls += 1
        ok = np.ones(U.shape[0], dtype=bool)
        loss, grad = 0.5 * np.sum(U * U, axis=1), U.copy()
        if self.fail_every:
            for b in range(U.shape[0]):
                self.rows += 1
                if self.rows % self.fail_every == 0:  # a row that reports "not positive definite": its numbers mean nothing
                    ok[b], loss[b], grad[b] = False, np.nan, np.nan
        return loss, grad, ok


# Seed 11 was chosen so that the moment checks below hold (they are 4-standard-error statements about ONE deterministic
# run, not about the sampler's distribution over seeds); the run is the same on every machine: numpy's generator and float64
# arithmetic on the host only.
SEED = 11


@pytest.fixture(scope="module")
def normal_run():
    target = _Normal3()
    U, info = sample_theta(target, np.zeros(3), 800, proper=True, chains=8, burn=60, leapfrog=10, step=0.1, thin=4, rng=SEED)
    return target, U, info


def test_known_target_moments_within_four_standard_errors(normal_run):
    target, U, info = normal_run
    n = U.shape[0]
    assert U.shape == (800, 3) and np.all(np.isfinite(U))
    mean, var = U.mean(axis=0), U.var(axis=0, ddof=1)
    # independent draws would have SE(mean) = 1 / sqrt(n), SE(var) = sqrt(2 / (n - 1))
    print("mean", mean, "var", var, "accept", info["accept_rate"], "step", info["step"])
    assert np.all(np.abs(mean) <= 4.0 / np.sqrt(n)), mean
    assert np.all(np.abs(var - 1.0) <= 4.0 * np.sqrt(2.0 / (n - 1))), var
    assert info["accept_rate"].shape == (8,) and np.all(info["accept_rate"] > 0.5)
    # one batch call per leapfrog step, whatever the number of chains: 1 start + (burn + thin * 100) * leapfrog
    assert info["batch_calls"] == target.calls == 1 + (60 + 4 * 100) * 10
    assert info["restarted"] == 0 and info["failed_rows"] == 0


def test_the_same_seed_gives_the_same_samples_and_the_rng_is_the_callers(normal_run):
    _, U, info = normal_run
    U2, info2 = sample_theta(_Normal3(), np.zeros(3), 800, proper=True, chains=8, burn=60, leapfrog=10, step=0.1, thin=4,
                             rng=np.random.default_rng(SEED))
    assert np.array_equal(U, U2) and info["step"] == info2["step"]
    U3, _ = sample_theta(_Normal3(), np.zeros(3), 800, proper=True, chains=8, burn=60, leapfrog=10, step=0.1, thin=4, rng=SEED + 1)
    assert not np.array_equal(U, U3)


def test_samples_need_not_divide_by_the_chains():
    U, info = sample_theta(_Normal3(), np.zeros(3), 13, proper=True, chains=8, burn=5, leapfrog=4, rng=0)
    assert U.shape == (13, 3)
    U, _ = sample_theta(_Normal3(), np.zeros(3), 3, proper=True, chains=8, burn=5, leapfrog=4, rng=0)
    assert U.shape == (3, 3)


def test_a_tiny_frozen_step_accepts_nearly_everything():
    U, info = sample_theta(_Normal3(), np.ones(3), 64, proper=True, chains=8, burn=0, leapfrog=5, step=1e-3, thin=5, rng=1)
    assert info["step"] == pytest.approx(1e-3, rel=1e-12)  # burn = 0: nothing adapts
    assert np.all(info["accept_rate"] >= 0.99)


def test_failing_rows_are_rejected_proposals_never_exceptions():
    target = _Normal3(fail_every=3)
    U, info = sample_theta(target, np.zeros(3), 40, proper=True, chains=8, burn=10, leapfrog=4, rng=2)
    assert U.shape == (40, 3) and np.all(np.isfinite(U))
    assert info["failed_rows"] > 0 and info["restarted"] > 0
    assert np.all(info["accept_rate"] <= 1.0)


def test_an_improper_target_is_refused():
    with pytest.raises(ValueError, match="prior"):
        sample_theta(_Normal3(), np.zeros(3), 4, proper=False)
    with pytest.raises(TypeError):
        sample_theta(_Normal3(), np.zeros(3), 4)  # the caller must say


def test_sample_hyper_refuses_a_model_without_priors_and_samples_one_with():
    from pygpso_amd import priors as P
    from pygpso_amd.kernels import Matern52
    from pygpso_amd.model import HipGPR
    from tests.multistart_problem import KERNEL, problem
    from oracle import gpr

    X, y, u0, _ = problem()

    class OracleBatchEngine:
        """Engine double over the oracle's NLML in u (no mean trained: 3 variables)."""
        dtype_name = "float64"

        def set_data(self, x, y_):
            pass

        def fit_batch_max(self):
            return 256

        def fit_eval_u_batch(self, kernel, U, n_ls, train_mean, mean_c_fixed=0.0):
            loss, grad, ok = np.full(U.shape[0], np.nan), np.full(U.shape, np.nan), np.zeros(U.shape[0], dtype=bool)
            for b, u in enumerate(U):
                try:
                    f, g = gpr.loss_and_grad_unconstrained(kernel, np.append(u, mean_c_fixed), X, y)
                    loss[b], grad[b], ok[b] = f, g[:3], True
                except np.linalg.LinAlgError:
                    pass
            return loss, grad, ok

    m = HipGPR((X, y), Matern52(variance=1.0, lengthscales=0.25), noise_variance=1e-3, engine=OracleBatchEngine())
    with pytest.raises(ValueError, match="prior"):
        m.sample_hyper(4, rng=0)
    P.attach(m, P.default_priors())
    before = m._pack()
    U, info = m.sample_hyper(6, rng=0, chains=4, burn=5, leapfrog=3)
    assert U.shape == (6, 3) and np.all(np.isfinite(U)) and np.array_equal(m._pack(), before)


def test_the_toy_problems_posterior_visits_both_optima():
    """tests/multistart_problem.py: two local optima of the NLML 0.137 nats apart at N = 10.  With the default priors on
    lengthscale, variance and noise and N(0, 1) on the mean, the chains started at the first optimum reach the basin of the
    second.  A sample is IN a basin when its distance in u to that optimum is below 1.0 and smaller than to the other (the
    optima lie 5.4 apart in u)."""
    from pygpso_amd import priors as P
    from tests.multistart_problem import KERNEL, OracleModel, oracle_multistart, problem

    X, y, u0, starts = problem()
    res = oracle_multistart()
    from pygpso_amd.kernels import Scipy

    opt_a = Scipy().minimize(OracleModel(X, y, u0).training_loss).x          # the warm start's optimum (10.2897)
    opt_b = np.asarray(res.x)                                                # the multi-start's winner (10.1524)
    sep = float(np.linalg.norm(opt_a - opt_b))
    assert sep > 2.0, sep
    model = OracleModel(X, y, u0)
    pri = P.default_priors()
    slots = [(pri["lengthscales"], P.SOFTPLUS), (pri["variance"], P.SOFTPLUS), (pri["noise"], P.SOFTPLUS), (P.Normal(0.0, 1.0), P.IDENTITY)]

    def target(U):
        loss, grad, ok = model._loss_and_grad_batch(U)
        p, gp = P.neg_log_prior_u(U, slots)
        return loss + p, grad + gp, ok

    U, info = sample_theta(target, opt_a, 256, proper=True, chains=8, burn=60, leapfrog=10, step=0.1, thin=5, rng=4)
    da, db = np.linalg.norm(U - opt_a, axis=1), np.linalg.norm(U - opt_b, axis=1)
    in_a, in_b = int(np.sum((da < 1.0) & (da < db))), int(np.sum((db < 1.0) & (db < da)))
    print(f"optima {sep:.2f} apart in u; samples in basin a: {in_a}, in basin b: {in_b}; accept {info['accept_rate']}")
    assert in_a > 0 and in_b > 0
