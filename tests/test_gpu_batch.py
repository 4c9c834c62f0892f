"""GPU checks of the latent cross-covariance (gpso_cross_cov) and of greedy batch selection under hallucinated updates
(gpso_best_batch) through the Python engine: against the dense-solve oracle of tests/batch_oracle.py, against the calls the
library already has (gpso_predict, gpso_predict_grad, gpso_predict_joint, gpso_best_acq, gpso_append_noise), the bit rules,
the end rules, the state rules and the refusals.

Tolerances.  gpso_cross_cov is double arithmetic on the dense double factor on both engines: 1e-8 of the kernel variance for
the smooth kernels and 1e-4 for the Matern-1/2 against the oracle (what sections 7h and 7i assert), 1e-12 against
gpso_predict_joint (two summation orders of the same products), 1e-13 for the transpose.  gpso_best_batch on a float64
context: picks identical to the oracle's on the decidable cases (tests/test_batch_cpu.py asserts the gaps), var and value
within the same 1e-8, var_after within 1e-8.  On a mixed context round 0 goes through the float predict path, whose var
tolerance (1e-4, GPSO_OPTF_TOL_VAR) exceeds the gaps: exact picks are not asked; every round is replayed instead -- the
oracle is conditioned on the device's earlier picks and the device's pick must have an oracle value within the value
tolerance of the oracle's maximum over the live rows.  That tolerance follows from GPSO_OPTF_TOL_MEAN / GPSO_OPTF_TOL_VAR:
    ucb_var:  tol_mean max|y - c| + varsigma tol_var variance
    ucb_std:  tol_mean max|y - c| + varsigma tol_var variance / (2 sqrt(noise))     (s2 >= noise; d sqrt(s2) = d s2 / (2 s))
The Matern-1/2 case is replayed the same way on both engines, with its 1e-4."""
import ctypes as C
import filecmp
import functools

import numpy as np
import pytest

from oracle import gpr
from pygpso_amd import HipGPEngine
from pygpso_amd import _lib as L
from pygpso_amd import acquisition as A
from tests import batch_oracle as B
from tests import hetero_oracle as H
from tests import joint_oracle as J
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

VS = gpr.VARSIGMA_DEFAULT
DTYPES = ["float64", "mixed"]
KINDS = ["ucb_var", "ucb_std", "ei", "logei", "pi"]
TOL64 = 1.0e-8
TOL_CTX = 1.0e-4  # GPSO_OPTF_TOL_VAR / GPSO_OPTF_TOL_MEAN of a mixed context


def _spec(name, incumbent=None, latent=False):
    if name == "ucb_var":
        return A.UCBVar(VS)
    if name == "ucb_std":
        return A.UCBStd(VS, latent=latent)
    return {"ei": A.EI, "logei": A.LogEI, "pi": A.PI}[name](incumbent=incumbent, latent=latent)


class Case:
    """One of the five problems of tests/batch_oracle.py under a kernel, with or without ARD and a per-point noise vector."""

    def __init__(self, i, kernel="Matern52", ard=False, with_s=False):
        n, d, seed = B.PROBLEMS[i]
        self.X, self.y = synthetic_problem(n, d, seed=seed)
        ls = 0.25 * np.sqrt(d) * (np.linspace(0.8, 1.3, d) if ard else np.ones(1))
        self.theta = gpr.Theta(kernel, ls, 1.0, 1.0e-3, float(self.y.mean()))
        self.s = H.draw_s(n, self.theta.variance, seed=n + d) if with_s else None
        self.leaves = synthetic_leaves(B.LEAVES_M[i], d, seed=seed + 1)
        self.d = d
        self.incumbent = float(np.max(self.y))
        self.tol = 1.0e-4 if kernel == "Matern12" else TOL64
        self._engines = {}

    def joint(self, Xs):
        """(mean, latent Sigma) of the oracle at the rows Xs."""
        if self.s is None:
            return J.textbook_joint(self.theta, self.X, self.y, Xs)
        return J.gpr_predict_joint(H.posterior(self.theta, self.X, self.y, self.s), Xs)

    @functools.lru_cache(maxsize=None)
    def oracle(self):
        return self.joint(self.leaves)

    def fit(self, eng, n=None):
        n = len(self.y) if n is None else n
        eng.set_data(self.X[:n], self.y[:n])
        if self.s is not None:
            eng.set_noise_diag(self.s[:n])
        th = self.theta
        eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
        return eng

    def engine(self, dtype):
        if dtype not in self._engines:
            self._engines[dtype] = self.fit(HipGPEngine(dtype, device=0))
        return self._engines[dtype]


@functools.lru_cache(maxsize=None)
def case(i, kernel="Matern52", ard=False, with_s=False):
    return Case(i, kernel, ard, with_s)


# the four kernels over the five problems; ARD once; half of them with a noise vector
COV_CASES = [(0, "Matern52", False, False), (1, "Matern32", False, True), (2, "SquaredExponential", True, False),
             (3, "Matern12", False, True), (4, "Matern52", False, True), (1, "SquaredExponential", False, False)]
SHAPES = [(1, 1), (17, 16), (65, 17), (300, 64), (300, 1)]  # (m, b)


# ---- 1. gpso_cross_cov ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", range(len(COV_CASES)))
def test_cross_cov_against_the_oracle_and_the_joint_predictive(which, dtype):
    c = case(*COV_CASES[which])
    eng = c.engine(dtype)
    _, Sigma = c.oracle()
    worst = worst_joint = 0.0
    for m, b in SHAPES:
        m = min(m, len(c.leaves))
        b = min(b, len(c.leaves))
        xa, xb = c.leaves[:m], c.leaves[len(c.leaves) - b:]
        got = eng.cross_cov(xa, xb)
        assert got.shape == (b, m)
        worst = max(worst, float(np.max(np.abs(got - Sigma[len(c.leaves) - b:, :m]))))
        union = np.vstack([xa, xb])
        _, cov = eng.predict_joint(union)
        worst_joint = max(worst_joint, float(np.max(np.abs(got - cov[m:, :m]))))
    print(f"{COV_CASES[which]} {dtype}: |cov - oracle| {worst:.2e} (tolerance {c.tol:.0e}), |cov - predict_joint| {worst_joint:.2e}")
    assert worst <= c.tol * c.theta.variance
    assert worst_joint <= 1e-12 * c.theta.variance


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_cov_transpose_diagonal_and_row_independence(dtype):
    c = case(2, "SquaredExponential", True, False)
    eng = c.engine(dtype)
    xa, xb = c.leaves[:64], c.leaves[100:117]
    ab, ba = eng.cross_cov(xa, xb), eng.cross_cov(xb, xa)
    assert float(np.max(np.abs(ab - ba.T))) <= 1e-13 * c.theta.variance
    # cov(t, t) + noise is the predictive variance
    pts = c.leaves[:40]
    diag = np.array([eng.cross_cov(pts[j:j + 1], pts[j:j + 1])[0, 0] for j in range(0, 40, 7)])
    var = eng.predict_grad(pts)[1][::7]
    assert float(np.max(np.abs(diag + c.theta.noise - var))) <= 1e-12 * c.theta.variance
    # a row's bits depend neither on the rest of its batch nor on the other batch
    full = eng.cross_cov(c.leaves, xb)
    assert np.array_equal(eng.cross_cov(c.leaves[:17], xb), full[:, :17])
    assert np.array_equal(eng.cross_cov(c.leaves, xb[3:4])[0], full[3])
    # float32 points: the same call on the rounded coordinates
    x32 = c.leaves[:33].astype(np.float32)
    assert np.array_equal(eng.cross_cov(x32, xb), eng.cross_cov(x32.astype(np.float64), xb))
    # a NaN coordinate gives NaNs, in its row or column only
    bad = c.leaves[:5].copy()
    bad[2, 1] = np.nan
    got = eng.cross_cov(bad, xb)
    assert np.all(np.isnan(got[:, 2])) and np.all(np.isfinite(np.delete(got, 2, axis=1)))
    got = eng.cross_cov(xb, bad)
    assert np.all(np.isnan(got[2])) and np.all(np.isfinite(np.delete(got, 2, axis=0)))


def test_cross_cov_across_the_chunk_boundary_has_the_bits_of_the_rows_alone():
    c = case(2)
    eng = c.engine("float64")
    m = 16384 + 17
    xa = synthetic_leaves(m, c.d, seed=11)
    xb = c.leaves[:3]
    eng.set_timing(True)
    full = eng.cross_cov(xa, xb)
    assert eng.last_count(0) == eng.last_count(1) == m and eng.last_ms(1) > 0.0
    for lo, hi in ((0, 17), (16384 - 5, 16384 + 17), (16000, 16100)):
        assert np.array_equal(eng.cross_cov(xa[lo:hi], xb), full[:, lo:hi])


# ---- 2. gpso_best_batch: bits ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large():  # (the batch past the small-call limit of tests/test_gpu_acq.py: 16 640 rows on N = 200, D = 3)
    X, y = synthetic_problem(200, 3, seed=1)
    theta = gpr.Theta("Matern52", 0.25 * np.sqrt(3), 1.0, 1.0e-3, float(y.mean()))
    return X, y, theta, synthetic_leaves(16640, 3, seed=2)


@functools.lru_cache(maxsize=None)
def large_engine(dtype):
    X, y, th, _ = large()
    eng = HipGPEngine(dtype, device=0)
    eng.set_data(X, y)
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    return eng


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", ["small", "large"])
def test_the_first_pick_has_the_bits_of_best_acq(size, dtype):
    if size == "small":
        c = case(0)
        eng, leaves, inc, noise = c.engine(dtype), c.leaves, c.incumbent, c.theta.noise
    else:
        X, y, th, leaves = large()
        eng, inc, noise = large_engine(dtype), float(np.max(y)), th.noise
    pm, _ = eng.predict(leaves)
    for name in KINDS:
        for latent in (False, True):
            if latent and name == "ucb_var":
                continue
            spec = _spec(name, inc, latent)
            want = eng.best_acq(leaves, spec, incumbent=inc)
            one = eng.best_batch(leaves, spec, 1, noise, incumbent=inc)
            for w, g in zip(want, one):
                np.testing.assert_array_equal(w, g)
            q = 5 if size == "small" else 2
            many = eng.best_batch(leaves, spec, q, noise, incumbent=inc)
            assert len(many[0]) == q and len(set(many[0].tolist())) == q
            for w, g in zip(want, many):
                np.testing.assert_array_equal(w[0], g[0])
            np.testing.assert_array_equal(many[1], pm[many[0]])  # mean[t]: gpso_predict's bits at that row


# ---- 3. gpso_best_batch: parity --------------------------------------------------------------------------------------------
def _value_tol(c, name, tol):
    scale = float(np.max(np.abs(c.y - c.theta.mean_c)))
    dv = VS * tol * c.theta.variance
    return tol * scale + (dv if name == "ucb_var" else dv / (2.0 * np.sqrt(c.theta.noise)))


def _replay(c, eng, name, obs, tol):
    """Every round of the device's batch against the oracle conditioned on the device's earlier picks."""
    mean, Sigma = c.oracle()
    noise = c.theta.noise
    idx, mu, var, val, after = eng.best_batch(c.leaves, _spec(name), B.ROUNDS, obs, want_var_after=True)
    assert len(idx) == B.ROUNDS and len(set(idx.tolist())) == B.ROUNDS
    vtol = _value_tol(c, name, tol)
    for t in range(B.ROUNDS):
        var_o, val_o = B.round_state(mean, Sigma, noise, obs, name, idx[:t])
        live = np.ones(len(mean), dtype=bool)
        live[idx[:t]] = False
        best = float(np.max(val_o[live]))
        print(f"  round {t}: pick {idx[t]}, oracle value {val_o[idx[t]]:.6f} (maximum {best:.6f}), |d var| {abs(var[t] - var_o[idx[t]]):.1e}")
        assert live[idx[t]] and val_o[idx[t]] >= best - vtol, (t, idx[t], val_o[idx[t]], best, vtol)
        assert abs(var[t] - var_o[idx[t]]) <= tol * c.theta.variance
        assert abs(val[t] - val_o[idx[t]]) <= vtol
    var_o, _ = B.round_state(mean, Sigma, noise, obs, name, idx)
    err = float(np.max(np.abs(after - var_o)))
    print(f"  var_after: {err:.2e} (tolerance {tol:.0e})")
    assert err <= tol * c.theta.variance


@pytest.mark.parametrize("name", ["ucb_var", "ucb_std"])
@pytest.mark.parametrize("i", range(len(B.PROBLEMS)))
def test_float64_picks_equal_the_oracles_on_the_decidable_cases(i, name):
    c = case(i)
    eng = c.engine("float64")
    mean, Sigma = c.oracle()
    noise = c.theta.noise
    want = B.greedy(mean, Sigma, c.leaves, noise, noise, name, B.ROUNDS)
    assert np.all(want.gaps > B.GAP_FLOOR)
    idx, mu, var, val, after = eng.best_batch(c.leaves, _spec(name), B.ROUNDS, noise, want_var_after=True)
    errs = [float(np.max(np.abs(a - b))) for a, b in ((var, want.var), (val, want.value), (after, want.var_after), (mu, want.mean))]
    print(f"case {i} {name}: picks {idx.tolist()}, |d var| {errs[0]:.1e}, |d value| {errs[1]:.1e}, |d var_after| {errs[2]:.1e}")
    assert idx.tolist() == want.idx.tolist()
    assert max(errs) <= TOL64 * c.theta.variance


@pytest.mark.parametrize("name", ["ucb_var", "ucb_std"])
@pytest.mark.parametrize("i", range(len(B.PROBLEMS)))
def test_mixed_rounds_replayed_against_the_oracle(i, name):
    c = case(i)
    _replay(c, c.engine("mixed"), name, c.theta.noise, TOL_CTX)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [1, 2, 3, 4])
def test_other_kernels_ard_and_noise_vectors_replayed(which, dtype):
    c = case(*COV_CASES[which])
    _replay(c, c.engine(dtype), "ucb_var", 2.0 * c.theta.noise, max(c.tol, TOL_CTX if dtype == "mixed" else 0.0))


# ---- 4. against the device's own fantasised posterior --------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_var_after_is_the_variance_of_a_context_the_picks_were_appended_to(which):
    c = case(*COV_CASES[which])
    eng = c.engine("float64")
    obs = 3.0 * c.theta.noise
    idx, mu, var, val, after = eng.best_batch(c.leaves, A.UCBVar(VS), 5, obs, want_var_after=True)
    m0, _ = eng.predict(c.leaves)
    other = c.fit(HipGPEngine("float64", device=0))
    other.append(c.leaves[idx], mu, s=np.full(len(idx), obs - c.theta.noise))
    m1, v1 = other.predict(c.leaves)
    assert float(np.max(np.abs(m1 - m0))) <= 1e-8 and float(np.max(np.abs(v1 - after))) <= 1e-8
    other.close()


# ---- 5. other posteriors and states ------------------------------------------------------------------------------------------
def test_installed_sgpr_posterior_with_logei():
    from tests import sgpr_oracle as S

    c = case(0)
    Z = c.X[:16].copy()
    u = S.initial_u(0.5, 1.0, 0.01, 0.0)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(c.X, c.y)
    eng.sgpr_set_inducing(Z)
    eng.sgpr_posterior("Matern52", u, 1, True, 0.0)
    spec = _spec("logei", c.incumbent)
    want = eng.best_acq(c.leaves, spec, incumbent=c.incumbent)
    idx, mu, var, val, after = eng.best_batch(c.leaves, spec, 4, 0.01, incumbent=c.incumbent, want_var_after=True)
    for w, g in zip(want, (idx, mu, var, val)):
        np.testing.assert_array_equal(w[0], g[0])
    # the SGPR oracle's predictive at the leaves, then var_after against the joint covariance of that predictive (C, alpha)
    # conditioned on the picks by a dense solve
    post = S.Posterior("Matern52", u, 1, True, 0.0, c.X, c.y, Z)
    mean_o, var_o = (np.asarray(a).reshape(-1) for a in post.predict_y(c.leaves))
    m_dev, v_dev = eng.predict(c.leaves)
    assert float(np.max(np.abs(v_dev - var_o))) <= 1e-8 and float(np.max(np.abs(m_dev - mean_o))) <= 1e-8
    _, cov = eng.predict_joint(c.leaves)
    noise = float(np.median(var_o - np.diag(cov)))  # (the likelihood variance of initial_u)
    assert float(np.max(np.abs(np.diag(cov) + noise - var_o))) <= 1e-8
    cond_var, cond_val = B.round_state(mean_o, cov, noise, 0.01, "logei", idx, incumbent=c.incumbent)
    assert float(np.max(np.abs(after - cond_var))) <= 1e-8
    for t in range(1, 4):  # every later pick is the oracle's arg-max over the live rows, given the earlier ones
        _, val_t = B.round_state(mean_o, cov, noise, 0.01, "logei", idx[:t], incumbent=c.incumbent)
        live = np.ones(len(mean_o), dtype=bool)
        live[idx[:t]] = False
        assert val_t[idx[t]] >= np.max(val_t[live]) - 1e-6 and abs(val[t] - val_t[idx[t]]) <= 1e-6
    assert len(set(idx.tolist())) == 4
    eng.close()


def test_vgp_context_var_after_agrees_with_conditioning_on_cross_cov_rows():
    from tests import paths_q_cases as qc
    from tests.test_gpu_paths_q import installed

    r = qc.reference(1)
    eng = installed(r)
    Xs = r["Xs"][:130]
    obs = 0.05
    idx, mu, var, val, after = eng.best_batch(Xs, A.UCBStd(VS), 4, obs, want_var_after=True)
    assert len(idx) == 4 and len(set(idx.tolist())) == 4
    _, v0 = eng.predict(Xs)
    K = eng.cross_cov(Xs, Xs[idx])  # [4, M]
    S = K[:, idx] + obs * np.eye(4)
    want = v0 - np.sum(K * np.linalg.solve(S, K), axis=0)
    assert float(np.max(np.abs(after - want))) <= 1e-8
    np.testing.assert_array_equal(var[0], v0[idx[0]])
    eng.close()


def test_stale_rows_of_a_larger_fit_change_no_bit():
    c = case(3)  # N = 300: fitted at 300 after an unrelated fit at 500 on the same context
    Xb, yb = synthetic_problem(500, c.d, seed=9)
    used = HipGPEngine("mixed", device=0)
    used.set_data(Xb, yb)
    th = c.theta
    used.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, float(yb.mean()), want_grad=False)
    used.best_batch(c.leaves, A.UCBVar(VS), 3, th.noise, want_var_after=True)
    c.fit(used)
    fresh = c.fit(HipGPEngine("mixed", device=0))
    for a, b in zip(used.best_batch(c.leaves, A.UCBVar(VS), 6, th.noise, want_var_after=True),
                    fresh.best_batch(c.leaves, A.UCBVar(VS), 6, th.noise, want_var_after=True)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(used.cross_cov(c.leaves, c.leaves[:17]), fresh.cross_cov(c.leaves, c.leaves[:17]))
    used.close()
    fresh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_calls_are_stateless(dtype):
    from pygpso_amd.paths import draw_path_inputs

    c = case(0)
    eng = c.fit(HipGPEngine(dtype, device=0))
    omega, phase, w, eps = draw_path_inputs(c.theta.kernel, 3, 64, len(c.y), c.d, 5)
    eng.paths_draw(omega, phase, w, eps)
    before = (eng.posterior_hash(), eng.predict(c.leaves), eng.paths_eval(c.leaves)[0])
    eng.set_timing(True)
    first = eng.best_batch(c.leaves, A.UCBStd(VS), 6, c.theta.noise, want_var_after=True)
    assert eng.last_count(0) == eng.last_count(1) == len(c.leaves) and eng.last_ms(1) > 0.0
    cov = eng.cross_cov(c.leaves, c.leaves[:16])
    assert eng.posterior_hash() == before[0] and eng.paths_info() == (3, 64)
    for a, b in zip(before[1], eng.predict(c.leaves)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(before[2], eng.paths_eval(c.leaves)[0])
    for a, b in zip(first, eng.best_batch(c.leaves, A.UCBStd(VS), 6, c.theta.noise, want_var_after=True)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(cov, eng.cross_cov(c.leaves, c.leaves[:16]))
    # q smaller, and without var_after: the same leading picks
    for a, b in zip(first[:4], eng.best_batch(c.leaves, A.UCBStd(VS), 3, c.theta.noise)):
        np.testing.assert_array_equal(a[:3], b)
    eng.close()


def _raw_batch(eng, leaves, spec, q, obs, incumbent=None):
    """gpso_best_batch itself with sentinel-filled outputs: (rc, n_picked, idx, mean, var, value)."""
    xs = np.ascontiguousarray(leaves, dtype=np.float64)
    rec = spec.c_struct(incumbent)
    idx = np.full(64, -99, dtype=np.int64)
    mean, var, val = (np.full(64, -99.0) for _ in range(3))
    n = C.c_int(-99)
    rc = eng._lib.gpso_best_batch(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, xs.shape[0], C.byref(rec), float(obs), int(q),
                                  L.i64ptr(idx), L.dptr(mean), L.dptr(var), L.dptr(val), C.byref(n), None, L.MEM_HOST)
    return rc, n.value, idx, mean, var, val


def _untouched_beyond(k, idx, mean, var, val):
    return np.all(idx[k:] == -99) and all(np.all(a[k:] == -99.0) for a in (mean, var, val))


def test_end_rules_on_the_device():
    c = case(1)
    eng = c.engine("float64")
    noise = c.theta.noise
    # q beyond the distinct rows; every row twice: a twin is retired with its pick
    rows = np.vstack([c.leaves[:10], c.leaves[:10][::-1]])
    rc, n, idx, mean, var, val = _raw_batch(eng, rows, A.UCBVar(VS), 15, noise)
    assert rc == L.OK and n == 10 and _untouched_beyond(10, idx, mean, var, val)
    assert len({tuple(rows[i]) for i in idx[:10]}) == 10 and np.all(idx[:10] < 10)  # (the first of each pair wins the tie)
    out = eng.best_batch(rows, A.UCBVar(VS), 15, noise, want_var_after=True)
    np.testing.assert_array_equal(out[4][:10], out[4][10:][::-1])  # a retired row's var_after is still updated
    single = eng.best_batch(c.leaves[:10], A.UCBVar(VS), 10, noise, want_var_after=True)
    np.testing.assert_array_equal(single[0], out[0])
    # a NaN row is picked first and ends the batch
    bad = c.leaves[:30].copy()
    bad[17, 2] = np.nan
    for name in KINDS:
        rc, n, idx, mean, var, val = _raw_batch(eng, bad, _spec(name, c.incumbent), 4, noise, c.incumbent)
        assert rc == L.OK and n == 1 and idx[0] == 17 and np.isnan(val[0]) and np.isnan(mean[0]), name
        assert _untouched_beyond(1, idx, mean, var, val)
    # a pick whose d is not positive ends the batch after it: an installed posterior whose factor overstates the data
    # (L / 2: |C k*|^2 four times too large, the latent variance near the data negative), ranked by the mean alone
    post = gpr.posterior(c.theta, c.X, c.y)
    over = HipGPEngine("float64", device=0)
    th = c.theta
    over.set_posterior(c.X, 0.5 * post.L, post.alpha, th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    at = c.X[:12].copy()  # (training inputs: |C k*|^2 = 4 (variance - O(noise)) at every one of them)
    mu, vv = over.predict(at)
    p = int(np.argmax(mu))
    lat = over.cross_cov(at[p:p + 1], at[p:p + 1])[0, 0]
    assert lat < 0.0, "the case needs a pick whose latent variance is negative"
    rc, n, idx, mean, var, val = _raw_batch(over, at, A.UCBVar(0.0), 4, 0.0)
    assert rc == L.OK and n == 1 and idx[0] == p and val[0] == mu[p] and _untouched_beyond(1, idx, mean, var, val)
    after = over.best_batch(at, A.UCBVar(0.0), 4, 0.0, want_var_after=True)[4]
    np.testing.assert_array_equal(after, vv)  # that pick changes no variance
    over.close()


def _codes(eng, leaves, q=2, obs=1e-3, b=1):
    xs = np.ascontiguousarray(leaves, dtype=np.float64)
    rc_batch = _raw_batch(eng, xs, A.UCBVar(VS), q, obs)[0]
    xb = np.ascontiguousarray(np.resize(xs, (max(b, 1), xs.shape[1])))
    cov = np.empty((max(b, 1), xs.shape[0]))
    rc_cov = eng._lib.gpso_cross_cov(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, xs.shape[0], L.dptr(xb), int(b),
                                     C.c_void_p(cov.ctypes.data), L.MEM_HOST)
    return rc_batch, rc_cov


def test_refusals_and_the_context_works_afterwards():
    from tests.test_gpu_distributed import _handoff

    c = case(1)
    Xs = c.leaves[:20]
    e32 = c.fit(HipGPEngine("float32", device=0))
    assert _codes(e32, Xs) == (L.E_ARG, L.E_ARG)
    e32.predict(Xs)
    e32.close()
    eng = HipGPEngine("float64", device=0)
    eng.set_data(c.X, c.y)
    assert _codes(eng, Xs) == (L.E_STATE, L.E_STATE)  # no posterior
    c.fit(eng)
    want = eng.best_batch(Xs, A.UCBVar(VS), 3, 1e-3)
    assert _codes(eng, Xs, q=0)[0] == L.E_ARG and _codes(eng, Xs, q=65)[0] == L.E_ARG
    assert _codes(eng, Xs, b=0)[1] == L.E_ARG and _codes(eng, Xs, b=65)[1] == L.E_ARG
    assert _codes(eng, Xs, q=64) == (L.OK, L.OK) and _codes(eng, Xs, b=64)[1] == L.OK
    for obs in (-1e-3, np.nan, np.inf):
        assert _codes(eng, Xs, obs=obs)[0] == L.E_ARG
    assert _codes(eng, np.empty((0, c.d))) == (L.E_ARG, L.E_ARG)
    with pytest.raises(ValueError, match="must be finite"):
        eng.best_batch(Xs, A.UCBStd(np.nan), 2, 1e-3)
    xs = np.ascontiguousarray(Xs)
    n = C.c_int(0)
    idx = np.zeros(4, dtype=np.int64)
    rec = A.UCBVar(VS).c_struct(None)
    args = (C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, 20, C.byref(rec), 1e-3, 2)
    assert eng._lib.gpso_best_batch(eng._h, *args, None, None, None, None, C.byref(n), None, L.MEM_HOST) == L.E_ARG
    assert eng._lib.gpso_best_batch(eng._h, *args, L.i64ptr(idx), None, None, None, None, None, L.MEM_HOST) == L.E_ARG
    assert eng._lib.gpso_best_batch(eng._h, None, L.F64, L.MEM_HOST, 20, C.byref(rec), 1e-3, 2, L.i64ptr(idx), None, None, None,
                                    C.byref(n), None, L.MEM_HOST) == L.E_ARG
    assert eng._lib.gpso_best_batch(eng._h, *args[:4], None, 1e-3, 2, L.i64ptr(idx), None, None, None, C.byref(n), None,
                                    L.MEM_HOST) == L.E_ARG
    assert eng._lib.gpso_best_batch(eng._h, *args, L.i64ptr(idx), None, None, None, C.byref(n), None, L.MEM_HOST) == L.OK and n.value == 2
    assert eng._lib.gpso_cross_cov(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, 20, None, 1, C.c_void_p(xs.ctypes.data),
                                   L.MEM_HOST) == L.E_ARG
    # an open best-UCB ticket
    ticket = eng.best_ucb_begin(c.leaves, VS)
    assert _codes(eng, Xs) == (L.E_STATE, L.E_STATE)
    eng.best_ucb_end(ticket)
    for a, b in zip(want, eng.best_batch(Xs, A.UCBVar(VS), 3, 1e-3)):
        np.testing.assert_array_equal(a, b)
    # an adopted posterior (the hand-off replayed with plain copies)
    dst = HipGPEngine("float64", device=0)
    _handoff(eng, dst)
    assert _codes(dst, Xs) == (L.E_STATE, L.E_STATE)
    dst.predict(Xs)
    dst.close()
    eng.close()


# ---- 6. the surrogate ------------------------------------------------------------------------------------------------------
def test_surrogate_select_batch_on_a_small_run(tmp_path):
    from pygpso_amd import GPRSurrogate, GPSOptimiser, ParameterSpace
    from pygpso_amd import kernels as K
    from tests.helpers import rotated_peaks

    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0))
    opt = GPSOptimiser(parameter_space=ParameterSpace(parameter_names=["x", "y"], parameter_bounds=[[-3, 5], [-3, 3]]),
                       gp_surrogate=surr, exploration_method="tree", exploration_depth=3, budget=12,
                       stopping_condition="evaluations", update_cycle=1, n_workers=1)
    opt.run(rotated_peaks)
    coords = synthetic_leaves(200, 2, seed=3)
    stored = list(surr.points)
    surr.save(str(tmp_path / "before"))
    idx, mean, var, value, after = surr.select_batch(coords, 5, return_var_after=True)
    surr.save(str(tmp_path / "after"))
    assert len(idx) == 5 and len(set(idx.tolist())) == 5 and after.shape == (200,)
    first = surr.gp_eval_best_acq(coords, "ucb_var")
    assert idx[0] == first[0][0] and mean[0] == first[1][0] and var[0] == first[2][0] and value[0] == first[3][0]
    m0, v0 = surr.gpflow_model.predict_y(coords)
    assert np.all(after <= np.asarray(v0)[:, 0] + 1e-12) and after[idx[1]] < np.asarray(v0)[idx[1], 0]
    for name in ("ucb_std", "ei", "logei", "pi"):
        got = surr.select_batch(coords, 3, acquisition=name)
        want = surr.gp_eval_best_acq(coords, name)
        assert len(set(got[0].tolist())) == 3 and got[0][0] == want[0][0] and got[3][0] == want[3][0]
    cc = surr.gp_cross_cov(coords[:7], coords[5:9])
    assert cc.shape == (4, 7) and cc[0, 5] > 0.0 and abs(cc[1, 6] + surr.gpflow_model.predictive_noise() - np.asarray(v0)[6, 0]) <= 1e-10
    assert list(surr.points) == stored
    cmp = filecmp.dircmp(str(tmp_path / "before"), str(tmp_path / "after"))
    assert not cmp.left_only and not cmp.right_only and not cmp.diff_files and cmp.common_files
