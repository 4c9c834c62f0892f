"""GPU checks of max-value entropy search through the Python engine: GPSO_ACQ_MES on every route a best-acquisition call
can take (the route shapes of tests/test_gpu_acq.py), its accuracy on the device, gpso_best_batch under it, the state rules
of the maxima, gpso_max_logcdf, and ``mes_select`` end to end.

Tolerances (tests/mes_oracle.py).  A value: 8 x the float64 restatement's own worst error on the fixed grid, floor 16 ulp,
against the 60-digit truth on the call's OWN (mean, var).  A max-logcdf sum: 8 x the restatement's own error on the rows
that go to 60 digits, floor (16 + log2 m) ulp.  gpso_best_batch: tests/test_gpu_batch.py's 1e-8 of the kernel variance.

``test_value_has_the_bits_of_the_host_map`` asks for the bits of ``gpso_acq_mes_eval_host`` on the call's own (mean, var):
the same header compiled for the host and for the device, its exp / log / log1p / erfc written out in it."""
import functools

import mpmath as mp
import numpy as np
import pytest

from oracle import gpr, tree
from pygpso_amd import HipGPEngine
from pygpso_amd import _lib as L
from pygpso_amd import acquisition as A
from tests import mes_oracle as MO
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

E = HipGPEngine
VS = gpr.VARSIGMA_DEFAULT
DTYPES = ["float64", "mixed"]
N, D = 40, 3


class Problem:
    def __init__(self, n=N, d=D, seed=0):
        self.X, self.y = synthetic_problem(n, d, seed=seed)
        self.d = d
        self.theta = gpr.Theta("Matern52", 0.25 * np.sqrt(d), 1.0, 1.0e-3, float(self.y.mean()))
        self.post = gpr.posterior(self.theta, self.X, self.y)
        top = float(np.max(self.y))
        self.ystar = top + np.array([0.0, 0.125, 0.3, 0.75, 1.5])  # K = 5
        self._engines = {}

    def fit(self, eng):
        eng.set_data(self.X, self.y)
        th = self.theta
        eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
        return eng

    def engine(self, dtype, small_calls=True):
        key = (dtype, small_calls)
        if key not in self._engines:
            eng = self.fit(HipGPEngine(dtype, device=0))
            if not small_calls:
                eng.set_small_calls(False)
            self._engines[key] = eng
        return self._engines[key]


@functools.lru_cache(maxsize=None)
def prob():
    return Problem()


LEAVES_A = synthetic_leaves(300, D, seed=1)
SEG_A = np.array([0, 90, 201, 300])
LEAVES_C = synthetic_leaves(16640, D, seed=2)  # (the smallest batch tests/test_gpu_acq.py sends past the small-call limit)
SEG_C = np.array([0, 8001, 16640])
BOXES = np.array([[[0.0, 1.0 / 3], [0.0, 1.0], [0.0, 1.0]], [[1.0 / 3, 2.0 / 3], [1.0 / 3, 2.0 / 3], [0.0, 1.0 / 3]],
                  [[2.0 / 3, 1.0], [0.0, 1.0 / 3], [2.0 / 3, 1.0]]])


def _spec(latent=False, maxima=None):
    return A.MES(latent=latent, maxima=prob().ystar if maxima is None else maxima)


def _check_values(ystar, mean, var, val):
    rows = np.arange(len(val)) if len(val) <= 512 else np.unique(np.linspace(0, len(val) - 1, 256).astype(int))
    tol = MO.tolerance()[0]
    err = MO.error(val[rows], MO.truth(ystar, mean[rows], var[rows]))
    assert err <= tol, (err / MO.ULP, tol / MO.ULP)
    assert np.all(val[~np.isnan(val)] >= 0.0) and np.all(np.isfinite(val[~np.isnan(mean)]))
    return err


def _check_winner(got, seg, mean, var, val):
    idx, mu, vv, best = got
    for s, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        i = int(np.argmax(val[a:b]))  # the first maximum, NaN first
        assert idx[s] == i, (s, idx[s], i)
        np.testing.assert_array_equal([mu[s], vv[s], best[s]], [mean[a + i], var[a + i], val[a + i]])


def _route(dtype, leaves, seg, small_calls=True):
    """mean / var: gpso_predict's bits; the column: within the tolerance of truth; idx: np.argmax of the column."""
    eng = prob().engine(dtype, small_calls)
    pm, pv = eng.predict(leaves)
    mean, var, val = eng.acq_values(leaves, _spec())
    np.testing.assert_array_equal(pm, mean)
    np.testing.assert_array_equal(pv, var)
    err = _check_values(prob().ystar, mean, var, val)
    got = eng.best_acq(leaves, _spec(), seg_off=seg)
    _check_winner(got, seg, mean, var, val)
    print(f"{dtype}: value error {err / MO.ULP:.1f} ulp (tolerance {MO.tolerance()[0] / MO.ULP:.1f} ulp)")
    return got, (mean, var, val)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_a_small_call_kernel(dtype):
    _route(dtype, LEAVES_A, SEG_A)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_b_two_stage_argmax_finalising_in_stage_1(dtype):
    _route(dtype, LEAVES_A, SEG_A, small_calls=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_c_past_the_small_call_limit(dtype):
    _route(dtype, LEAVES_C, SEG_C)


def _grown(dtype, depth):
    eng = prob().engine(dtype)
    rows = tree.grow_count(depth)
    coords = eng.grow(BOXES, depth).reshape(-1, D)
    seg = np.arange(4) * rows
    pm, pv = eng.predict(coords)
    mean, var, val = eng.acq_values(coords, _spec())
    np.testing.assert_array_equal(pm, mean)
    np.testing.assert_array_equal(pv, var)
    _check_values(prob().ystar, mean, var, val)
    got = eng.best_acq_grow(BOXES, depth, _spec())
    _check_winner(got, seg, mean, var, val)  # (the first maximum over the full duplicated list)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("depth", [4, 9])  # the small keyed route: 3 x 40 rows; the large one: 3 x 9841
def test_routes_d_e_grown(dtype, depth):
    _grown(dtype, depth)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_f_two_tickets_of_different_kinds(dtype):
    p = prob()
    eng = p.engine(dtype)
    inc = float(np.max(p.y))
    logei = A.LogEI(incumbent=inc)
    eng.acq_set_maxima(p.ystar)
    block_mes = eng.best_acq(LEAVES_A, A.MES(latent=False), seg_off=SEG_A)
    block_le = eng.best_acq(LEAVES_A, logei, seg_off=SEG_A)
    block_grown = eng.best_acq_grow(BOXES, 4, A.MES(latent=False))
    t1 = eng.best_acq_begin(LEAVES_A, A.MES(latent=False), seg_off=SEG_A)
    t2 = eng.best_acq_begin(LEAVES_A, logei, seg_off=SEG_A)
    got_le = eng.best_ucb_end(t2)  # (ended out of order)
    got_mes = eng.best_ucb_end(t1)
    t3 = eng.best_acq_grow_begin(BOXES, 4, A.MES(latent=False))
    t4 = eng.best_ucb_begin(LEAVES_A, VS, seg_off=SEG_A)
    got_grown, got_ucb = eng.best_ucb_end(t3), eng.best_ucb_end(t4)
    for want, got in ((block_mes, got_mes), (block_le, got_le), (block_grown, got_grown),
                      (eng.best_ucb(LEAVES_A, VS, seg_off=SEG_A), got_ucb)):
        for w, g in zip(want, got):
            np.testing.assert_array_equal(w, g)
    mean, var, val = eng.acq_values(LEAVES_A, A.MES(latent=False))
    _check_winner(got_mes, SEG_A, mean, var, val)


ROUTES = {"a": lambda dt: _route(dt, LEAVES_A, SEG_A)[0], "b": lambda dt: _route(dt, LEAVES_A, SEG_A, small_calls=False)[0],
          "c": lambda dt: _route(dt, LEAVES_C, SEG_C)[0], "d": lambda dt: _grown(dt, 4), "e": lambda dt: _grown(dt, 9)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_value_has_the_bits_of_the_host_map(route, dtype):
    """Every route's ``value`` against ``gpso_acq_mes_eval_host`` on the call's own (mean, var), bit for bit; and the whole
    column of ``gpso_acq_values`` on the small batch.

    The map calls no math-library function: exp, log, log1p and erfc are written out in csrc/acq.hpp (DESIGN.md section
    7p), because the host's and the device's differ in the last place (38 of these 300 values did, by up to 3 ulp)."""
    idx, mu, vv, best = ROUTES[route](dtype)
    host = E.acq_mes_eval_host(prob().ystar, mu, vv, latent=False)
    ulps = np.abs(best - host) / np.spacing(host)
    print(f"route {route} {dtype}: winners differ from the host map by {ulps.tolist()} ulp")
    mean, var, val = prob().engine(dtype).acq_values(LEAVES_A, _spec())
    col = E.acq_mes_eval_host(prob().ystar, mean, var, latent=False)
    off = np.abs(val - col) / np.spacing(col)
    print(f"  column of 300: {int(np.sum(off > 0))} rows differ, at most {float(np.max(off)):.0f} ulp")
    np.testing.assert_array_equal(best, host)
    np.testing.assert_array_equal(val, col)


def test_latent_reads_the_variance_before_the_noise():
    p = prob()
    eng = p.engine("float64")
    mean, var, val = eng.acq_values(LEAVES_A, _spec(latent=True))
    pm, pv = eng.predict(LEAVES_A)
    np.testing.assert_array_equal(pm, mean)
    np.testing.assert_array_equal(pv, var)
    # the device reads variance - sum BEFORE the noise is added; var is that plus the noise rounded once: truth's s2 is
    # known to half an ulp of var, so the value lies between truth at both ends of that interval, widened by the tolerance
    noise, tol = p.theta.noise, MO.tolerance()[0]
    half = 0.5 * np.spacing(var)
    lo = MO.truth(p.ystar, mean, var, s2_add=(-noise, -half))
    hi = MO.truth(p.ystar, mean, var, s2_add=(-noise, half))
    worst = 0.0
    for g, a, b in zip(val, lo, hi):
        a, b = min(a, b), max(a, b)
        if not (a <= mp.mpf(float(g)) <= b):
            worst = max(worst, min(MO.error([g], [a]), MO.error([g], [b])))
    assert worst <= tol, (worst / MO.ULP, tol / MO.ULP)
    assert not np.array_equal(val, eng.acq_values(LEAVES_A, _spec(latent=False))[2])
    _check_winner(eng.best_acq(LEAVES_A, _spec(latent=True), seg_off=SEG_A), SEG_A, mean, var, val)


# ---- accuracy where the map is hard -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_accuracy_at_gamma_8_m6_m38_m100_on_an_installed_posterior(dtype):
    p = prob()
    eng = HipGPEngine(dtype, device=0)
    th = p.theta
    eng.set_posterior(p.X, p.post.L, p.post.alpha, th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
    leaves = LEAVES_A[:64]
    mean, var = eng.predict(leaves)
    j = 7
    gammas = np.array([8.0, -6.0, -38.0, -100.0])
    ystar = mean[j] + gammas * np.sqrt(var[j])  # leaf j sits at these gammas; the other leaves around them
    tol = MO.tolerance()[0]
    worst = 0.0
    for k in range(4):  # one maximum at a time: no large term hides a small one's error
        m1, v1, val = eng.acq_values(leaves, A.MES(latent=False, maxima=ystar[k:k + 1]))
        np.testing.assert_array_equal(m1, mean)
        np.testing.assert_array_equal(v1, var)
        g = (ystar[k] - mean) / np.sqrt(var)
        assert abs(g[j] - gammas[k]) <= 1e-9 * abs(gammas[k])
        err = MO.error(val, MO.truth(ystar[k:k + 1], mean, var))
        print(f"{dtype} gamma {gammas[k]}: gammas of the batch {g.min():.1f} .. {g.max():.1f}, error {err / MO.ULP:.1f} ulp")
        worst = max(worst, err)
        assert np.all(np.isfinite(val)) and np.all(val >= 0.0)
    assert worst <= tol, (worst / MO.ULP, tol / MO.ULP)
    m4, v4, val = eng.acq_values(leaves, A.MES(latent=False, maxima=ystar))
    assert MO.error(val, MO.truth(ystar, mean, var)) <= tol
    eng.close()


def test_float32_context_on_the_small_route():
    p = prob()
    eng = p.fit(HipGPEngine("float32", device=0))
    pm, pv = eng.predict(LEAVES_A)
    mean, var, val = eng.acq_values(LEAVES_A, _spec())
    np.testing.assert_array_equal(pm, mean)
    np.testing.assert_array_equal(pv, var)
    _check_values(p.ystar, mean, var, val)
    _check_winner(eng.best_acq(LEAVES_A, _spec(), seg_off=SEG_A), SEG_A, mean, var, val)
    eng.close()


def test_installed_sgpr_posterior():
    from tests import sgpr_oracle as S

    X, y = synthetic_problem(64, D, seed=3)
    Z = X[:16].copy()
    u = S.initial_u(0.5, 1.0, 0.01, 0.0)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    eng.sgpr_set_inducing(Z)
    eng.sgpr_posterior("Matern52", u, 1, True, 0.0)
    ystar = float(np.max(y)) + np.array([0.0, 0.2, 0.5, 1.0, 2.0])
    spec = A.MES(latent=False, maxima=ystar)
    mean, var, val = eng.acq_values(LEAVES_A, spec)
    pm, pv = eng.predict(LEAVES_A)
    np.testing.assert_array_equal(pm, mean)
    np.testing.assert_array_equal(pv, var)
    _check_values(ystar, mean, var, val)
    _check_winner(eng.best_acq(LEAVES_A, spec, seg_off=SEG_A), SEG_A, mean, var, val)
    eng.close()


# ---- gpso_best_batch ----------------------------------------------------------------------------------------------------
def test_best_batch_against_a_numpy_greedy_loop_over_cross_cov():
    p = prob()
    eng = p.engine("float64")
    noise, q = p.theta.noise, 3
    spec = _spec(latent=True)
    idx, mu, var, val, after = eng.best_batch(LEAVES_A, spec, q, noise, want_var_after=True)
    mean, s2, _ = eng.acq_values(LEAVES_A, spec)
    s2 = s2.copy()
    cols, picks, vals, vars_ = [], [], [], []
    live = np.ones(len(mean), dtype=bool)
    for t in range(q):
        score = E.acq_mes_eval_host(p.ystar, mean, s2, noise=noise, latent=True)
        score[~live] = -np.inf
        pick = int(np.argmax(score))
        picks.append(pick)
        vals.append(score[pick])
        vars_.append(s2[pick])
        c = eng.cross_cov(LEAVES_A, LEAVES_A[pick:pick + 1])[0]
        for g in cols:
            c = c - g * g[pick]
        g = c / np.sqrt(c[pick] + noise)
        cols.append(g)
        s2 = s2 - g * g
        live[pick] = False
    print(f"picks {idx.tolist()} (numpy {picks}); |d value| {np.max(np.abs(val - vals)):.1e}; |d var| {np.max(np.abs(var - vars_)):.1e}")
    assert idx.tolist() == picks
    tol = 1.0e-8 * p.theta.variance
    assert np.max(np.abs(val - vals)) <= tol and np.max(np.abs(var - vars_)) <= tol and np.max(np.abs(after - s2)) <= tol
    np.testing.assert_array_equal(mu, mean[idx])
    first = eng.best_acq(LEAVES_A, spec)
    for w, g in zip(first, (idx, mu, var, val)):
        np.testing.assert_array_equal(w[0], g[0])
    np.testing.assert_array_equal(eng.acq_get_maxima(), p.ystar)  # (fixed over the rounds, and still there)


# ---- state and bits -------------------------------------------------------------------------------------------------------
def test_state_rules_of_the_maxima():
    p = prob()
    eng = p.fit(HipGPEngine("float64", device=0))
    fresh = p.fit(HipGPEngine("float64", device=0))
    want_hash, want_ucb = fresh.posterior_hash(), fresh.best_ucb(LEAVES_A, VS, seg_off=SEG_A)
    assert eng.acq_get_maxima().size == 0
    with pytest.raises(L.GpsoHipError) as err:  # MES with no set
        eng.best_acq(LEAVES_A, A.MES())
    assert err.value.code == L.E_STATE
    with pytest.raises(L.GpsoHipError) as err:
        eng.acq_values(LEAVES_A, A.MES())
    assert err.value.code == L.E_STATE
    for bad in (np.arange(65.0), [0.5, np.nan], [np.inf]):
        with pytest.raises(ValueError):  # (GPSO_E_ARG)
            eng.acq_set_maxima(bad)
    assert eng.acq_get_maxima().size == 0
    # setting, replacing, clearing: the posterior's hash and a best-UCB call's four outputs stay a fresh context's bits
    for ys in (p.ystar, p.ystar[:2] + 1.0, None, np.linspace(1.0, 3.0, 64)):
        eng.acq_set_maxima(ys)
        np.testing.assert_array_equal(eng.acq_get_maxima(), np.zeros(0) if ys is None else ys)
        assert eng.posterior_hash() == want_hash
        for w, g in zip(want_ucb, eng.best_ucb(LEAVES_A, VS, seg_off=SEG_A)):
            np.testing.assert_array_equal(w, g)
    # a ticket open
    eng.acq_set_maxima(p.ystar)
    ticket = eng.best_acq_begin(LEAVES_A, A.MES(latent=False), seg_off=SEG_A)
    with pytest.raises(L.GpsoHipError) as err:
        eng.acq_set_maxima(p.ystar + 1.0)
    assert err.value.code == L.E_STATE
    got = eng.best_ucb_end(ticket)
    np.testing.assert_array_equal(eng.acq_get_maxima(), p.ystar)
    for w, g in zip(eng.best_acq(LEAVES_A, A.MES(latent=False), seg_off=SEG_A), got):
        np.testing.assert_array_equal(w, g)
    # the set survives a refit (and an append), and the call after it reads it
    before = eng.acq_values(LEAVES_A, A.MES(latent=False))
    p.fit(eng)
    np.testing.assert_array_equal(eng.acq_get_maxima(), p.ystar)
    for w, g in zip(before, eng.acq_values(LEAVES_A, A.MES(latent=False))):
        np.testing.assert_array_equal(w, g)
    eng.append(LEAVES_A[:2], np.array([0.1, -0.2]))
    np.testing.assert_array_equal(eng.acq_get_maxima(), p.ystar)
    mean, var, val = eng.acq_values(LEAVES_A, A.MES(latent=False))
    _check_values(p.ystar, mean, var, val)
    eng.close()
    fresh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_coordinate_wins_its_segment(dtype):
    leaves = LEAVES_A.copy()
    leaves[137, 1] = np.nan  # a row of the second segment
    for small_calls in (True, False):
        eng = prob().engine(dtype, small_calls)
        idx, mu, vv, best = eng.best_acq(leaves, _spec(), seg_off=SEG_A)
        assert idx[1] == 137 - SEG_A[1] and np.isnan(mu[1]) and np.isnan(vv[1]) and np.isnan(best[1])
        assert not np.isnan(best[0]) and not np.isnan(best[2])


# ---- gpso_max_logcdf --------------------------------------------------------------------------------------------------------
def _columns(m):
    rng = np.random.default_rng(m)
    mean, var = rng.normal(0.0, 1.0, m), rng.uniform(0.01, 2.0, m)
    if m >= 63:
        mean[5], var[9] = np.nan, np.nan
        var[17], mean[17] = 0.001, -7.5  # (var - var_sub < 0: s = 0, below every threshold but the lowest)
    return mean, var


VAR_SUB = 0.005
Y64 = np.concatenate([np.linspace(-40.0, 8.0, 61), [-7.5, 0.125, 40.0]])


@functools.lru_cache(maxsize=None)
def _logcdf_truth(m, g):
    mean, var = _columns(m)
    y = Y64 if g == 64 else np.array([0.125])
    if m * g <= 8192:
        want, n = MO.truth_logcdf(mean, var, y, VAR_SUB)
        own = MO.error(MO.restatement_logcdf(mean, var, y, VAR_SUB)[0], want)
    else:  # (a spread of rows at 60 digits, math.fsum of the restatement for the others: 2 000 rows at m = 70 001)
        want, n, own = MO.truth_logcdf_sampled(mean, var, y, VAR_SUB, n_exact=2000 if m > 1000 else 128)
    return y, want, n, own


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("g", [1, 64])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 70001])  # (70 001: 137 workgroups, the second stage folds them)
def test_max_logcdf_against_truth(m, g, mem):
    eng = prob().engine("float64")
    mean, var = _columns(m)
    y, want, n, own = _logcdf_truth(m, g)
    if mem == "device":
        import torch

        mean, var = torch.tensor(mean, device="cuda:0"), torch.tensor(var, device="cuda:0")
    got, used = eng.max_logcdf(mean, var, y, VAR_SUB, want_used=True)
    again = eng.max_logcdf(mean, var, y, VAR_SUB)
    np.testing.assert_array_equal(got, again)  # the same call: the same bits
    assert used == n == m - (2 if m >= 63 else 0)
    tol = MO.logcdf_tolerance(m, own)
    err = MO.error(got, want)
    print(f"m={m} g={g} {mem}: {err / MO.ULP:.1f} ulp (restatement {own / MO.ULP:.1f}, tolerance {tol / MO.ULP:.1f})")
    assert err <= tol
    host = E.max_logcdf_host(*_columns(m), y, VAR_SUB)
    assert np.array_equal(np.isneginf(got), np.isneginf(host))
    if g == 64 and m >= 63:
        assert np.isneginf(got[y < -7.5]).all() and np.isfinite(got[y >= -7.5]).all()


def test_max_logcdf_far_below_every_mean_is_finite_and_refusals():
    eng = prob().engine("float64")
    mean, var = np.full(600, 2.0), np.full(600, 0.25)
    got = eng.max_logcdf(mean, var, [-100.0, -1e4], 0.0)  # z = -204 and about -2e4: Phi underflows, the tail form does not
    assert np.all(np.isfinite(got)) and np.all(got < -1e6)
    want = [600 * w for w in MO.truth_logcdf(mean[:1], var[:1], [-100.0, -1e4])[0]]
    assert MO.error(got, want) <= MO.logcdf_tolerance(600)
    for bad_y in (np.zeros(0), np.zeros(65), [np.nan]):
        with pytest.raises(ValueError):
            eng.max_logcdf(mean, var, bad_y)
    ticket = eng.best_ucb_begin(LEAVES_A, VS)
    with pytest.raises(L.GpsoHipError) as err:
        eng.max_logcdf(mean, var, [0.0])
    assert err.value.code == L.E_STATE
    eng.best_ucb_end(ticket)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _surrogate():
    from pygpso_amd import GPRSurrogate, GPSOptimiser, ParameterSpace
    from pygpso_amd import kernels as K
    from tests.helpers import rotated_peaks

    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0))
    opt = GPSOptimiser(parameter_space=ParameterSpace(parameter_names=["x", "y"], parameter_bounds=[[-3, 5], [-3, 3]]),
                       gp_surrogate=surr, exploration_method="tree", exploration_depth=3, budget=30,
                       stopping_condition="evaluations", update_cycle=1, n_workers=1)
    opt.run(rotated_peaks)
    return surr


@pytest.mark.parametrize("method", ["paths", "gumbel"])
def test_mes_select_on_a_one_dimensional_slice(method):
    surr = _surrogate()
    model = surr.gpflow_model
    assert len(model._data[1]) >= 30  # (the budget of 30 evaluations, and the initial points)
    # a 1-D slice of 2 000 leaves through the best training input: the maximum over it is not settled by the clamp alone
    x_best = np.asarray(model._data[0])[int(np.argmax(model._data[1]))]
    coords = np.column_stack([np.linspace(0.0, 1.0, 2000), np.full(2000, x_best[1])])
    stored = list(surr.points)
    idx, mean, var, value = surr.mes_select(coords, k=16, method=method, rng=5)
    maxima = model.engine.acq_get_maxima()
    assert maxima.shape == (16,) and np.all(maxima >= float(np.max(model._data[1])))  # (the clamp)
    print(f"{method}: maxima {np.sort(maxima)[[0, 8, 15]]} over a best target of {float(np.max(model._data[1])):.6f}; pick {idx[0]}")
    assert np.any(maxima > float(np.max(model._data[1])))
    m_all, v_all, val_all = surr.gp_acq_values(coords, A.MES(latent=True))
    host = E.acq_mes_eval_host(maxima, m_all, v_all, noise=model.predictive_noise(), latent=True)
    assert idx[0] == int(np.argmax(host)) == int(np.argmax(val_all))
    assert mean[0] == m_all[idx[0]] and var[0] == v_all[idx[0]] and value[0] == val_all[idx[0]] and value[0] > 0.0
    again = surr.mes_select(coords, k=16, method=method, rng=5)  # the same seed: the same maxima, the same pick
    np.testing.assert_array_equal(model.engine.acq_get_maxima(), maxima)
    for a, b in zip((idx, mean, var, value), again):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(surr.max_value_samples(coords, k=16, method=method, rng=5), maxima)
    assert not np.array_equal(surr.max_value_samples(coords, k=16, method=method, rng=6), maxima)
    seg = surr.mes_select(coords, k=4, method=method, rng=1, seg_off=np.array([0, 700, 2000]))
    assert len(seg[0]) == 2 and 0 <= seg[0][0] < 700 and 0 <= seg[0][1] < 1300
    got = surr.select_batch(coords, 3, acquisition=A.MES(maxima=maxima))
    assert len(set(got[0].tolist())) == 3 and got[0][0] == idx[0]
    assert list(surr.points) == stored
    with pytest.raises(ValueError):
        surr.polish(coords[:2], objective="mes")
    with pytest.raises(ValueError):
        surr.acq_value_and_grad(coords[:2], "mes")
