"""
CPU tests of the pathwise draws of the variational posteriors: the float64 oracle of
tests/paths_q_oracle.py against each family's predictive mean and against the closed form of a draw's moments; 4000 draws'
moments against that form; the conditioning of the cases tests/test_gpu_paths_q.py runs on the device; and the Python
surface -- ``HipVGP`` / ``HipSGPR`` / ``HipSVGP.sample_paths``, the surrogates' ``gp_sample_paths`` / ``gp_eval_paths`` /
``thompson_select_leaves`` -- over a stub engine whose arithmetic is that oracle.
"""
import copy
import re

import numpy as np
import pytest

from pygpso_amd import kernels as K
from pygpso_amd import paths as P
from tests import paths_cases as pc
from tests import paths_oracle as po
from tests import paths_q_cases as qc
from tests import paths_q_oracle as pq
from tests import sgpr_oracle as SG
from tests import svgp_oracle as SV
from tests import vgp_oracle as V
from tests import vgp_studentt_oracle as T
from tests.helpers import synthetic_problem
from tests.joint_oracle import _kernel_direct
from tests.test_inducing_cpu import StubEngine

FAMILIES = ("vgp", "sgpr", "svgp")


def _problem(family, kernel="Matern52", lik=pq.GAUSSIAN, n=40, big_n=90, d=3, seed=57):
    """One posterior of ``family`` over n resident rows (N = n for the VGP) after a natural-gradient step, and the family
    oracle's own ``predict_f``."""
    X, y = synthetic_problem(n if family == "vgp" else big_n, d, seed=seed)
    p = 0.3 if lik[0] == "StudentT" else 0.05
    u = SV.initial_u(0.25 * np.sqrt(d), 1.3, p, lik, float(y.mean()))
    if family == "vgp":
        a = (kernel, u, 1, True, 0.0, X, y, np.zeros(n), np.eye(n))
        mu, S = T.natgrad(*a, lik, 0.7) if lik[0] == "StudentT" else V.natgrad(*a, 0.7)
        family_post = T.Posterior(kernel, u, 1, True, 0.0, X, mu, S, lik) if lik[0] == "StudentT" else V.Posterior(kernel, u, 1, True, 0.0, X, mu, S)
        return pq.vgp_posterior(kernel, u, 1, True, 0.0, X, mu, S, lik), family_post.predict_f, y
    Z = X[:n]
    if family == "sgpr":
        return pq.sgpr_posterior(kernel, u, 1, True, 0.0, X, y, Z), SG.Posterior(kernel, u, 1, True, 0.0, X, y, Z).predict_f, y
    mu, S = SV.natgrad(kernel, u, 1, True, 0.0, X, y, Z, np.zeros(n), np.eye(n), lik, 0.7)
    return pq.svgp_posterior(kernel, u, 1, True, 0.0, X, Z, mu, S, lik), SV.Posterior(kernel, u, 1, True, 0.0, X, Z, mu, S, lik).predict_f, y


# ---- 1. the oracle against the families' own predictives --------------------------------------------------------------------
@pytest.mark.parametrize("family,lik", [("vgp", pq.GAUSSIAN), ("vgp", qc.STUDENT), ("sgpr", pq.GAUSSIAN), ("svgp", pq.GAUSSIAN),
                                        ("svgp", qc.STUDENT)])
@pytest.mark.parametrize("kernel", ("Matern52", "Matern12", "SquaredExponential"))
def test_zero_weights_and_zero_normals_give_the_familys_predictive_mean(family, lik, kernel):
    post, predict_f, y = _problem(family, kernel, lik)
    Xs = pc.points_at(30, 3)
    omega, phase, w, eps = pc.inputs(kernel, 5, 64, post.X.shape[0], 3, seed=3)
    assert eps.shape == (5, post.X.shape[0])
    scale = max(1.0, float(np.max(np.abs(y))))
    for e in (np.zeros_like(eps), None):
        values = pq.path_values(post, omega, phase, np.zeros_like(w), e, Xs)
        assert values.shape == (5, 30)
        # the same k (direct differences): to rounding
        assert np.max(np.abs(values - pq.predictive_mean(post, Xs)[None, :])) <= 1e-12 * scale
        # the family oracle's own mean (its Gram in the GEMM form)
        err = float(np.max(np.abs(values - predict_f(Xs)[0][None, :])))
        print(f"{family} {lik[0]} {kernel}: zero-weight paths against the family's predict_f {err:.2e}")
        assert err <= (1e-5 if kernel == "Matern12" else 1e-9) * scale


@pytest.mark.parametrize("family,lik", [("vgp", pq.GAUSSIAN), ("vgp", qc.STUDENT), ("sgpr", pq.GAUSSIAN), ("svgp", qc.STUDENT)])
def test_closed_form_of_a_draws_moments_given_exact_k(family, lik):
    """With the prior path an exact GP draw g ~ GP(0, k), a path is LINEAR in (g(Xs), g(Zr), eps):
        f(Xs) = c + k*^T beta + g(Xs) - k*^T K~^-1 g(Zr) + k*^T Lu^-T Q eps,
    so its covariance is T J T^T + G G^T with J the prior's joint covariance of (g(Xs), g(Zr)) -- K, without jitter, on the
    rows -- , T = [I, -k*^T K~^-1] and G = k*^T Lu^-T Q.  ``expected_moments`` states it as the section's formula; its diagonal
    is the family's var_f less 1e-6 |K~^-1 k*|^2, a gap between -k*^T K~^-1 k* and 0."""
    post, predict_f, y = _problem(family, "Matern52", lik)
    th, Zr = post.theta, post.X
    Xs = pc.points_at(25, 3, seed=9)
    mean, cov, var_f, gap = pq.expected_moments(post, Xs)
    ks = _kernel_direct(th, Zr, Xs)
    Kt = post.L @ post.L.T
    W = np.linalg.solve(Kt, ks)                      # K~^-1 k*
    Tm = np.hstack([np.eye(25), -W.T])
    J = np.block([[_kernel_direct(th, Xs, Xs), ks.T], [ks, Kt - pq.JITTER * np.eye(Zr.shape[0])]])
    G = np.linalg.solve(post.L, ks).T @ post.Q
    assert np.max(np.abs(cov - (Tm @ J @ Tm.T + G @ G.T))) <= 1e-10 * th.variance
    assert np.max(np.abs(mean - pq.predictive_mean(post, Xs))) <= 1e-12 * max(1.0, np.max(np.abs(y)))
    fam_mean, fam_var = predict_f(Xs)
    assert np.max(np.abs(var_f - fam_var)) <= 1e-9 * th.variance and np.max(np.abs(mean - fam_mean)) <= 1e-9 * max(1.0, np.max(np.abs(y)))
    bound = np.sum(ks * W, axis=0)
    print(f"{family} {lik[0]}: cov_aa - var_f in [{gap.min():.2e}, {gap.max():.2e}] (bound -{bound.max():.2e})")
    assert np.all(gap <= 1e-14) and np.all(gap >= -bound - 1e-14)
    np.testing.assert_allclose(gap, -pq.JITTER * np.sum(W * W, axis=0), rtol=1e-6, atol=1e-13)


# ---- 2. statistics --------------------------------------------------------------------------------------------------------
N_DRAWS, N_FEATURES, BLOCK = 4000, 512, 4
MEAN_MULTIPLE, COV_MULTIPLE = 4.5, 5.0  # tests/test_paths_cpu.py's


@pytest.mark.parametrize("family", FAMILIES)
def test_the_draws_moments_are_the_closed_forms(family):
    """n = 40 resident rows (N = 90 behind the sparse two), D = 3, Matern-5/2, 20 test points, S = 4000 draws in blocks of 4
    with FRESH features (F = 512) per block, fixed seed: over fresh features the draws have exactly ``expected_moments``'
    mean and covariance, so the sample moments miss them by Monte-Carlo error alone -- tests/test_paths_cpu.py's argument and
    its multiples: 4.5 standard errors of the mean over 20 points (tail 1.4e-4), 5 of the covariance over 210 entries (1.2e-4).
    Achieved (this seed), in standard errors, mean | cov: vgp 2.67 | 2.88, sgpr 2.15 | 2.97, svgp 2.20 | 3.06.  cov_aa - var_f
    reaches -4.9e-6 here (the three share their resident rows), 3e-3 standard errors of the covariance: this test cannot tell
    the closed form from var_f -- test_closed_form_of_a_draws_moments_given_exact_k does that."""
    post, _, _ = _problem(family)
    n = post.X.shape[0]
    Xs = pc.points_at(20, 3, seed=9)
    mean, cov, var_f, gap = pq.expected_moments(post, Xs)
    rng = np.random.default_rng(4100 + FAMILIES.index(family))
    f = np.empty((N_DRAWS, 20))
    for b in range(0, N_DRAWS, BLOCK):
        omega, phase, w, eps = P.draw_path_inputs("Matern52", BLOCK, N_FEATURES, n, 3, rng)
        f[b:b + BLOCK] = pq.path_values(post, omega, phase, w, eps, Xs)
    var = np.diag(cov)
    se_cov = np.sqrt((np.outer(var, var) + cov * cov) / N_DRAWS)
    e_mean = np.max(np.abs(f.mean(axis=0) - mean) / np.sqrt(var / N_DRAWS))
    e_cov = np.max(np.abs(np.cov(f, rowvar=False) - cov) / se_cov)
    print(f"{family}: mean {e_mean:.2f}, cov {e_cov:.2f} standard errors (S = {N_DRAWS}, F = {N_FEATURES}); cov_aa - var_f "
          f"down to {gap.min():.2e} ({np.max(-gap / np.diag(se_cov)):.1e} standard errors)")
    assert e_mean <= MEAN_MULTIPLE and e_cov <= COV_MULTIPLE


# ---- 3. the GPU cases are well conditioned ----------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(qc.CASES)))
def test_gpu_cases_agree_with_the_extended_oracle_ten_times_tighter_than_the_bar(index):
    """Every case the GPU suite holds to the oracle: float64 against extended precision from the same (Lu, mu, Q), and float64
    against itself with Lu from another rounding of the same Gram (direct differences for the GEMM form)."""
    r = qc.reference(index)
    post = r["post"]
    cols = slice(0, 300)  # (the chunk-crossing case: its first 300 points)
    a = (r["omega"], r["phase"], r["w"], r["eps"], r["Xs"][cols])
    wide = float(np.max(np.abs(pq.path_values(post, *a, dtype=np.longdouble) - r["values"][:, cols])))
    other = copy.copy(post)
    other.L = np.linalg.cholesky(_kernel_direct(post.theta, post.X, post.X) + pq.JITTER * np.eye(post.X.shape[0]))
    gram = float(np.max(np.abs(pq.path_values(other, *a) - r["values"][:, cols])))
    print(f"{qc.name(index)}: float64 against extended {wide:.2e}, against the other Gram's Lu {gram:.2e} (a tenth of the bar "
          f"{0.1 * r['tol']:.2e}); cond K~ {np.linalg.cond(post.L) ** 2:.1e}")
    assert np.max(np.abs(r["omega"])) <= pc.OMEGA_CLIP
    assert wide <= 0.1 * r["tol"] and gram <= 0.1 * r["tol"]


def test_gpu_cases_cover_what_they_claim_and_the_gap_rule_leaves_out_no_pair():
    left_out = total = 0
    for index in range(len(qc.CASES)):
        r = qc.reference(index)
        for seg in qc.segment_layouts(r):
            u = qc.undecided(r, seg)
            left_out += int(np.sum(u))
            total += u.size
    print(f"gap rule: {left_out} of {total} (draw, segment) pairs left out")
    assert left_out == 0
    col = lambda k: {c[k] for c in qc.CASES}
    assert {(c[1], c[2]) for c in qc.CASES} >= {(2, 1), (17, 3), (33, 5), (129, 3), (40, 26)}
    assert {(c[3], c[1]) for c in qc.CASES if c[0] != "vgp"} >= {(130, 17), (300, 33), (300, 129)}
    assert col(4) == {"Matern52", "Matern32", "Matern12", "SquaredExponential"}
    assert col(5) >= {1, 5, 64, 257} and col(6) >= {1, 17, 129} and col(7) >= {1, 65, 130, qc.CHUNK + 3}
    assert {(c[0], c[8][0]) for c in qc.CASES} == {("vgp", "Gaussian"), ("vgp", "StudentT"), ("sgpr", "Gaussian"),
                                                   ("svgp", "Gaussian"), ("svgp", "StudentT")}


# ---- 4. the Python surface over a stub engine ---------------------------------------------------------------------------------
class PathsQEngine(StubEngine):
    """tests/test_inducing_cpu.py's stub with the VGP's calls and the path calls answered by tests/paths_q_oracle.py."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.qpost = self.path_set = self.vq = None

    def set_data(self, x, y):
        super().set_data(x, y)
        self.qpost = self.path_set = None

    def vgp_set_q(self, mu=None, S=None):
        self.vq = (np.zeros(self.n), np.eye(self.n)) if mu is None else (np.array(mu), np.array(S))

    def vgp_natgrad(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, gamma=1.0):
        self.vq = V.natgrad(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, *self.vq, gamma)

    def vgp_elbo_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, want_grad=True):
        f, g, th = V.neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, *self.vq)
        return f, (g if want_grad else None), th

    def vgp_posterior(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        self.qpost, self.path_set = pq.vgp_posterior(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, *self.vq), None

    def sgpr_posterior(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        self.qpost, self.path_set = pq.sgpr_posterior(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, self.Z), None
        return super().sgpr_posterior(kernel, u, n_ls, train_mean, mean_c_fixed)

    def svgp_posterior(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        self.qpost, self.path_set = pq.svgp_posterior(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.Z, *self.q, self.lik), None
        return super().svgp_posterior(kernel, u, n_ls, train_mean, mean_c_fixed)

    def paths_draw(self, omega, phase, w, eps=None):
        raise RuntimeError("GPSO_E_STATE: gpso_paths_draw needs a posterior fitted with targets")

    def paths_draw_q(self, omega, phase, w, eps=None):
        self.calls.append(("paths_draw_q", w.shape, None if eps is None else eps.shape))
        self.path_set = (omega, phase, w, pq.solve_v(self.qpost, omega, phase, w, eps))

    def paths_info(self):
        return (0, 0) if self.path_set is None else self.path_set[2].shape

    def paths_eval(self, xs, seg_off=None, want_values=True, out=None):
        self.calls.append(("paths_eval", bool(want_values)))
        if self.path_set is None:
            raise RuntimeError("no path set resident")
        values = po.evaluate(self.qpost, *self.path_set, xs)
        idx, val = po.seg_argmax(values, seg_off)
        return (values if want_values else None), idx, val


def _model(family):
    from pygpso_amd.sgpr import HipSGPR
    from pygpso_amd.svgp import HipSVGP
    from pygpso_amd.vgp import HipVGP

    X, y = synthetic_problem(30, 2, seed=2)
    common = dict(data=(X, y[:, None]), kernel=K.Matern32(lengthscales=0.4, variance=1.0), mean_function=K.Constant(0.0),
                  engine=PathsQEngine())
    if family == "vgp":
        m = HipVGP(likelihood=K.Gaussian(1.0e-2), **common)
        m.natgrad(0.7)
    elif family == "sgpr":
        m = HipSGPR(noise_variance=1.0e-2, num_inducing=9, **common)
    else:
        m = HipSVGP(likelihood=K.Gaussian(1.0e-2), num_inducing=9, **common)
        m.start_q()
        m.natgrad(0.7)
    return m, (30 if family == "vgp" else 9)


@pytest.mark.parametrize("family", FAMILIES)
def test_sample_paths_draws_the_normals_over_the_resident_rows_and_a_seed_reproduces_the_set(family):
    m, rows = _model(family)
    Xs = np.random.default_rng(1).random((9, 2))
    m.sample_paths(3, n_features=32, rng=4)
    assert ("paths_draw_q", (3, 32), (3, rows)) in m.engine.calls and m.engine.paths_info() == (3, 32)
    values, idx, val = m.eval_paths(Xs, seg_off=[0, 4, 9])
    assert values.shape == (3, 9) and idx.shape == (3, 2) and val.shape == (3, 2)
    # the inputs are paths.draw_path_inputs' for the model's kernel, the RESIDENT row count and the seed: the same generator
    # in the same order as the exact GP's
    omega, phase, w, eps = P.draw_path_inputs("Matern32", 3, 32, rows, 2, rng=4)
    assert np.array_equal(values, pq.path_values(m.engine.qpost, omega, phase, w, eps, Xs))
    m.sample_paths(3, n_features=32, rng=np.random.default_rng(4))
    assert np.array_equal(m.eval_paths(Xs)[0], values)
    m.sample_paths(3, n_features=32, rng=5)
    assert not np.array_equal(m.eval_paths(Xs)[0], values)
    with pytest.raises(ValueError):
        m.sample_paths(0)


@pytest.mark.parametrize("which", ["VGP", "SGPR", "SVGP"])
def test_the_surrogates_thompson_select_leaves_and_an_engine_group_raises(which, monkeypatch):
    import pygpso_amd.model as model_module
    from pygpso_amd import SGPRSurrogate, SVGPSurrogate, VGPSurrogate
    from pygpso_amd.distributed import HipGPEngineGroup

    monkeypatch.setattr(model_module, "HipGPEngine", PathsQEngine)
    rng = np.random.default_rng(5)
    coords = rng.random((24, 2))
    scores = np.sin(3.0 * coords[:, 0]) + coords[:, 1] ** 2
    kw = dict(gp_kernel=K.Matern52(lengthscales=0.4, variance=1.0), gp_meanf=K.Constant(0.0))
    surr = {"VGP": lambda: VGPSurrogate(train_iterations=2, **kw), "SGPR": lambda: SGPRSurrogate(num_inducing=8, **kw),
            "SVGP": lambda: SVGPSurrogate(num_inducing=8, train_iterations=2, **kw)}[which]()
    surr.append(coords, scores)
    surr.gp_update()
    stored = list(surr.points)
    cand = rng.random((1500, 2))
    surr.gp_sample_paths(6, n_features=64, rng=21)
    f = surr.gp_eval_paths(cand)
    seg = [0, 10, 10, 900, 1500]
    idx, val = surr.thompson_select_leaves(cand, seg_off=seg)
    want_i, want_v = po.seg_argmax(f, seg)
    assert f.shape == (6, 1500) and np.array_equal(idx, want_i) and np.array_equal(val, want_v, equal_nan=True)
    assert not np.array_equal(f[0], f[1])
    calls = surr.gpflow_model.engine.calls
    assert calls[-2:] == [("paths_eval", True), ("paths_eval", False)]  # (the values stay on the device)
    assert ("paths_draw_q", (6, 64), (6, 24 if which == "VGP" else 8)) in calls
    surr.gp_sample_paths(6, n_features=64, rng=np.random.default_rng(21))
    assert np.array_equal(surr.gp_eval_paths(cand), f)
    assert list(surr.points) == stored
    surr.gpflow_model.engine = object.__new__(HipGPEngineGroup)
    for call in (lambda: surr.gp_sample_paths(2), lambda: surr.gp_eval_paths(cand), lambda: surr.thompson_select_leaves(cand)):
        with pytest.raises(NotImplementedError):
            call()


# ---- 5. the C-ABI symbol -----------------------------------------------------------------------------------------------------
def test_gpso_paths_draw_q_is_declared_in_the_header_and_bound():
    import os

    from pygpso_amd import _lib as L

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpso_hip.h")).read()
    assert re.search(r"\bint\s+gpso_paths_draw_q\s*\(\s*gpso_ctx\s*\*", header)
    table = next(v for v in vars(L).values() if isinstance(v, dict) and "gpso_paths_draw" in v)
    assert table["gpso_paths_draw_q"] == table["gpso_paths_draw"]  # (the same signature)
