"""
CPU tests of pathwise posterior draws: the float64 oracle of tests/paths_oracle.py against its
dense-solve twin and the posterior mean; the draws' moments against the exact posterior; the random-feature frequencies of
``pygpso_amd.paths``; the conditioning of the cases tests/test_gpu_paths.py runs on the device; and the Python surface --
``HipGPR.sample_paths`` / ``eval_paths``, ``GPSurrogate.gp_sample_paths`` / ``gp_eval_paths`` / ``thompson_select_leaves`` --
over a stub engine whose arithmetic is that oracle.  (That the three entry points are declared, exported and bound is
tests/test_cabi_cpu.py's.)
"""
import numpy as np
import pytest

from oracle import gpr
from pygpso_amd import GPRSurrogate
from pygpso_amd import kernels as K
from pygpso_amd import paths as P
from pygpso_amd.model import HipGPR
from tests import hetero_oracle as ho
from tests import joint_oracle as jo
from tests import paths_cases as pc
from tests import paths_oracle as po
from tests.helpers import synthetic_problem
from tests.test_loo_cpu import RecordingEngine

KERNELS = ("Matern52", "Matern32", "Matern12", "SquaredExponential")


# ---- 1. the oracle against its twin and the posterior mean ---------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,d", [(2, 1), (17, 3), (129, 3), (40, 26)])
def test_oracle_against_the_dense_solve_and_the_posterior_mean(n, d, kernel):
    X, y = synthetic_problem(n, d, seed=17 + n)
    th = gpr.Theta(kernel, 0.25 * np.sqrt(d) * np.linspace(0.8, 1.3, d), 1.3, 1.0e-2, float(y.mean()))
    Xs = pc.points_at(30, d)
    for s in (None, ho.draw_s(n, th.variance, seed=n + d)):
        # (L from the direct-difference Gram, the textbook form's: the two differ in how K_y is solved and in nothing else)
        Ky = jo._kernel_direct(th, X, X)
        Ky[np.diag_indices(n)] += th.noise + (0.0 if s is None else s)
        post = gpr.Posterior()
        post.theta, post.X, post.y, post.L = th, X, y, np.linalg.cholesky(Ky)
        omega, phase, w, eps = pc.inputs(kernel, 5, 64, n, d, seed=3)
        got = po.path_values(post, s, omega, phase, w, eps, Xs)
        want = po.textbook_values(th, X, y, s, omega, phase, w, eps, Xs)
        scale = max(np.max(np.abs(y)), np.sqrt(th.variance) * np.max(np.abs(w)))
        err = np.max(np.abs(got - want)) / scale
        print(f"N={n} D={d} {kernel} s={'yes' if s is not None else 'no'}: oracle against the dense solve {err:.2e}")
        assert got.shape == (5, 30) and err <= 1e-10
        # w = 0, eps = 0: every path is the posterior mean
        mean = po.path_values(post, s, omega, phase, np.zeros_like(w), None, Xs)
        post.alpha = np.linalg.solve(Ky, y - th.mean_c)
        ref = jo._kernel_direct(th, Xs, X) @ post.alpha + th.mean_c
        assert np.max(np.abs(mean - ref[None, :])) <= 1e-10 * scale
    # ... and oracle.gpr's own mean (its Gram in the GEMM form) for the plain posterior
    plain = gpr.posterior(th, X, y)
    mean = po.path_values(plain, None, omega, phase, np.zeros_like(w), np.zeros_like(eps), Xs)
    tol = (1e-5 if kernel == "Matern12" else 1e-9) * max(1.0, np.max(np.abs(y)))
    assert np.max(np.abs(mean - gpr.predict_y(plain, Xs)[0][None, :])) <= tol


def test_segmented_first_argmax():
    v = np.array([[1.0, 3.0, 3.0, 2.0, 5.0, 5.0], [0.0, -1.0, 2.0, 2.0, 2.0, 1.0]])
    idx, val = po.seg_argmax(v, [0, 1, 1, 4, 6])
    assert idx.tolist() == [[0, -1, 0, 0], [0, -1, 1, 0]]
    assert val[:, [0, 2, 3]].tolist() == [[1.0, 3.0, 5.0], [0.0, 2.0, 2.0]] and np.all(np.isnan(val[:, 1]))
    idx, val = po.seg_argmax(v)
    assert idx.tolist() == [[4], [2]] and val.tolist() == [[5.0], [2.0]]
    assert po.top_two_gap(v, [0, 1, 4, 6]).tolist() == [[np.inf, 0.0, 0.0], [np.inf, 0.0, 1.0]]


# ---- 2. statistics --------------------------------------------------------------------------------------------------------
N_DRAWS, N_FEATURES, BLOCK = 4000, 512, 4
MEAN_MULTIPLE, COV_MULTIPLE = 4.5, 5.0


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_draws_moments_are_the_exact_posteriors(kernel):
    """(N, D) = (40, 3), 20 test points, S = 4000 draws in blocks of 4 with FRESH features (F = 512) per block, fixed seed.
    Given the features, a draw's mean is the exact posterior mean (w and eps have mean zero) and its covariance is linear in
    the feature Gram, whose expectation is the kernel: over fresh features the draws have exactly the posterior's mean and
    covariance, so the sample moments miss them by Monte-Carlo error alone.
      mean:  |error_a| <= 4.5 sqrt(Sigma_aa / S): two-sided normal tail 6.8e-6 a point, 1.4e-4 over the 20 points.
      cov:   |error_ab| <= 5 sqrt((Sigma_aa Sigma_bb + Sigma_ab^2) / S), a Gaussian sample covariance's standard error:
             tail 5.7e-7 an entry, 1.2e-4 over the 210 distinct entries.
    Achieved (this seed), in standard errors, mean | cov: Matern52 2.40 | 3.15, Matern32 2.33 | 2.82, Matern12 1.86 | 2.49,
    SquaredExponential 1.45 | 2.42."""
    X, y = synthetic_problem(40, 3, seed=57)
    th = gpr.Theta(kernel, 0.25 * np.sqrt(3) * np.linspace(0.8, 1.3, 3), 1.3, 1.0e-2, float(y.mean()))
    post = gpr.posterior(th, X, y)
    Xs = pc.points_at(20, 3, seed=9)
    mean, cov = po.exact_posterior(post, Xs)
    rng = np.random.default_rng(2024 + KERNELS.index(kernel))
    f = np.empty((N_DRAWS, 20))
    for b in range(0, N_DRAWS, BLOCK):
        omega, phase, w, eps = P.draw_path_inputs(kernel, BLOCK, N_FEATURES, 40, 3, rng)
        f[b:b + BLOCK] = po.path_values(post, None, omega, phase, w, eps, Xs)
    var = np.diag(cov)
    e_mean = np.max(np.abs(f.mean(axis=0) - mean) / np.sqrt(var / N_DRAWS))
    e_cov = np.max(np.abs(np.cov(f, rowvar=False) - cov) / np.sqrt((np.outer(var, var) + cov * cov) / N_DRAWS))
    print(f"{kernel}: mean {e_mean:.2f}, cov {e_cov:.2f} standard errors (S = {N_DRAWS}, F = {N_FEATURES})")
    assert e_mean <= MEAN_MULTIPLE and e_cov <= COV_MULTIPLE


@pytest.mark.parametrize("kernel", KERNELS)
def test_spectral_frequencies_reproduce_the_kernel_at_the_root_f_rate(kernel):
    """Phi(X) Phi(X)^T against k(X, X), N = 40: a term 2 variance cos(a) cos(b) = variance (cos(a - b) + cos(a + b)) has
    variance at most variance^2, so an entry's standard error is at most variance / sqrt(F); five of them over the 820
    distinct entries (tail 5.7e-7 each).  At sixteen times the features the error is a quarter: it falls between F = 1024 and
    F = 16384 by more than a factor of two."""
    X, _ = synthetic_problem(40, 3, seed=57)
    th = gpr.Theta(kernel, 0.25 * np.sqrt(3) * np.linspace(0.8, 1.3, 3), 1.3, 1.0e-2, 0.0)
    Kxx = jo._kernel_direct(th, X, X)
    errs = []
    for f in (1024, 16384):
        gen = np.random.default_rng(31)
        omega = P.spectral_frequencies(kernel, f, 3, gen)
        assert omega.shape == (f, 3)
        phase = gen.uniform(0.0, 2.0 * np.pi, f)
        phi = po.features(th, omega, phase, X)
        errs.append(float(np.max(np.abs(phi @ phi.T - Kxx))))
        print(f"{kernel} F={f}: max |Phi Phi^T - K| = {errs[-1]:.3e} (bound {5.0 * th.variance / np.sqrt(f):.3e})")
        assert errs[-1] <= 5.0 * th.variance / np.sqrt(f)
    assert errs[1] < 0.5 * errs[0]
    # a seed and a generator give the same frequencies; the kernels differ
    assert np.array_equal(P.spectral_frequencies(kernel, 8, 2, 5), P.spectral_frequencies(kernel, 8, 2, np.random.default_rng(5)))
    with pytest.raises(ValueError):
        P.spectral_frequencies("Cosine", 8, 2, 5)
    with pytest.raises(ValueError):
        P.spectral_frequencies(kernel, 0, 2, 5)


# ---- 3. the GPU cases are well conditioned ----------------------------------------------------------------------------------
@pytest.mark.parametrize("index", list(range(len(pc.CASES))) + ["append"])
def test_gpu_cases_float64_and_extended_oracles_agree_to_a_tenth_of_the_tolerance(index):
    """Every (case, omega, phase, w, eps) the GPU suite holds to the oracle within a tolerance."""
    r = pc.append_case() if index == "append" else pc.reference(index)
    wide = po.path_values(r["post"], r["s"], r["omega"], r["phase"], r["w"], r["eps"], r["Xs"], dtype=np.longdouble)
    diff = float(np.max(np.abs(wide - r["values"])))
    print(f"{index if index == 'append' else pc.name(index)}: float64 against extended {diff:.2e} (a tenth of the tolerance {0.1 * r['tol']:.2e})")
    assert np.max(np.abs(r["omega"])) <= pc.OMEGA_CLIP
    assert diff <= 0.1 * r["tol"]


def test_gpu_cases_gap_rule_excludes_at_most_one_pair_in_ten():
    excluded = total = 0
    for r in [pc.reference(index) for index in range(len(pc.CASES))] + [pc.append_case()]:
        layouts = [None] + ([pc.SEGMENTS] if r["Xs"].shape[0] == 130 else [])
        for seg in layouts:
            gap = po.top_two_gap(r["values"], seg)
            excluded += int(np.sum(gap <= 2.0 * r["tol"]))
            total += gap.size
    print(f"gap rule: {excluded} of {total} (draw, segment) pairs excluded")
    assert 10 * excluded <= total


# ---- 4. the Python surface over a stub engine ---------------------------------------------------------------------------------
class PathsEngine(RecordingEngine):
    """``RecordingEngine`` with the path calls answered by tests/paths_oracle.py."""

    path_set = None

    def fit_eval(self, *a, **kw):
        self.path_set = None  # (every fit ends the set)
        return super().fit_eval(*a, **kw)

    def paths_draw(self, omega, phase, w, eps=None):
        self.calls.append(("paths_draw", w.shape, None if eps is None else eps.shape))
        v = po.solve_v(self.post, po.residual(self.post, None, omega, phase, w, eps))
        self.path_set = (omega, phase, w, v)

    def paths_info(self):
        return (0, 0) if self.path_set is None else (self.path_set[2].shape[0], self.path_set[2].shape[1])

    def paths_eval(self, xs, seg_off=None, want_values=True, out=None):
        self.calls.append(("paths_eval", bool(want_values)))
        if self.path_set is None:
            raise RuntimeError("no path set resident")
        values = po.evaluate(self.post, *self.path_set, xs)
        idx, val = po.seg_argmax(values, seg_off)
        return (values if want_values else None), idx, val


def _surrogate(monkeypatch):
    monkeypatch.setattr(GPRSurrogate, "engine_factory", PathsEngine)
    rng = np.random.default_rng(5)
    coords = rng.random((14, 2))
    scores = np.sin(3.0 * coords[:, 0]) + coords[:, 1] ** 2
    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.3, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy())
    surr.append(coords, scores)
    surr.gp_update()
    return surr, rng.random((1500, 2))


def test_thompson_select_leaves_is_the_segmented_argmax_of_gp_eval_paths_and_nothing_is_stored(monkeypatch):
    surr, cand = _surrogate(monkeypatch)
    stored = list(surr.points)
    surr.gp_sample_paths(6, n_features=64, rng=21)
    f = surr.gp_eval_paths(cand)
    idx, val = surr.thompson_select_leaves(cand)
    assert f.shape == (6, 1500) and idx.shape == (6, 1) and val.shape == (6, 1)
    assert np.array_equal(idx[:, 0], np.argmax(f, axis=1)) and np.array_equal(val[:, 0], np.max(f, axis=1))
    seg = [0, 10, 10, 900, 1500]
    idx, val = surr.thompson_select_leaves(cand, seg_off=seg)
    want_i, want_v = po.seg_argmax(f, seg)
    assert idx.shape == (6, 4) and np.array_equal(idx, want_i) and np.array_equal(val, want_v, equal_nan=True)
    calls = surr.gpflow_model.engine.calls
    assert calls[-3:] == [("paths_eval", True), ("paths_eval", False), ("paths_eval", False)]  # (the values stay on the device)
    assert ("paths_draw", (6, 64), (6, 14)) in calls
    # the same seed: the same set; another seed: another
    surr.gp_sample_paths(6, n_features=64, rng=np.random.default_rng(21))
    assert np.array_equal(surr.gp_eval_paths(cand), f)
    surr.gp_sample_paths(6, n_features=64, rng=22)
    assert not np.array_equal(surr.gp_eval_paths(cand), f)
    assert list(surr.points) == stored
    with pytest.raises(ValueError):
        surr.gp_sample_paths(0)


def test_the_model_methods_and_an_engine_group_raises(monkeypatch):
    from pygpso_amd.distributed import HipGPEngineGroup

    X, y = synthetic_problem(12, 2, seed=2)
    m = HipGPR(data=(X, y[:, None]), kernel=K.Matern32(lengthscales=0.4, variance=1.0), mean_function=K.Constant(0.0),
               noise_variance=1.0e-2, engine=PathsEngine())
    Xs = np.random.default_rng(1).random((9, 2))
    m.sample_paths(3, n_features=32, rng=4)
    values, idx, val = m.eval_paths(Xs, seg_off=[0, 4, 9])
    assert values.shape == (3, 9) and idx.shape == (3, 2) and val.shape == (3, 2)
    assert m.engine.paths_info() == (3, 32)
    # the inputs are paths.draw_path_inputs' for the model's kernel, data shape and seed
    omega, phase, w, eps = P.draw_path_inputs("Matern32", 3, 32, 12, 2, rng=4)
    assert np.array_equal(values, po.path_values(m.engine.post, None, omega, phase, w, eps, Xs))
    surr, cand = _surrogate(monkeypatch)
    surr.gpflow_model.engine = object.__new__(HipGPEngineGroup)
    for call in (lambda: surr.gp_sample_paths(2), lambda: surr.gp_eval_paths(cand), lambda: surr.thompson_select_leaves(cand)):
        with pytest.raises(NotImplementedError):
            call()
