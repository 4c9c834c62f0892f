"""GPU checks of the acquisition functions through the C-ABI (gpso_best_acq*, gpso_acq_values): every route a best-UCB
call can take serves every kind, GPSO_ACQ_UCB_VAR has the bits of the gpso_best_ucb* calls, the value column agrees with
the 60-digit truth evaluated on the call's OWN mean / var (the map's error apart from the posterior's), the winner is the
first maximum of that column and truth's winner on the float64 oracle posterior.

Tolerance of a value: tests/acq_oracle.py (8 x the float64 yardstick's own worst error on the fixed grid, floor 16 ulp).
Winners against the oracle are only asked where they are decidable: the seeds are chosen so that in every segment truth's
gap between the best and the runner-up exceeds 100 x that tolerance -- asserted here, no segment excused."""
import functools

import mpmath as mp
import numpy as np
import pytest

from oracle import gpr, tree
from pygpso_amd import HipGPEngine
from pygpso_amd import acquisition as A
from tests import acq_oracle as AO
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

VS = gpr.VARSIGMA_DEFAULT
DTYPES = ["float64", "mixed"]
NAMES = ["ucb_std", "ei", "logei", "pi"]
TOP = 24  # candidates per segment that go to the 60-digit evaluation (the yardstick ranks the rest out: its error is
          # orders of magnitude below the spread of the top values)


def _spec(name, incumbent=None, latent=False):
    if name == "ucb_var":
        return A.UCBVar(VS)
    if name == "ucb_std":
        return A.UCBStd(VS, latent=latent)
    return {"ei": A.EI, "logei": A.LogEI, "pi": A.PI}[name](incumbent=incumbent, latent=latent)


class Problem:
    def __init__(self, n, d, seed):
        self.X, self.y = synthetic_problem(n, d, seed=seed)
        self.d = d
        self.theta = gpr.Theta("Matern52", 0.25 * np.sqrt(d), 1.0, 1.0e-3, float(self.y.mean()))
        self.post = gpr.posterior(self.theta, self.X, self.y)
        self.incumbent = float(np.max(self.y))
        self._engines = {}

    def engine(self, dtype, small_calls=True):
        key = (dtype, small_calls)
        if key not in self._engines:
            eng = HipGPEngine(dtype, device=0)
            eng.set_data(self.X, self.y)
            th = self.theta
            eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
            if not small_calls:
                eng.set_small_calls(False)
            self._engines[key] = eng
        return self._engines[key]


@functools.lru_cache(maxsize=None)
def small():  # routes (a), (b), (d), (e), (f)
    return Problem(52, 2, seed=0)


@functools.lru_cache(maxsize=None)
def large():  # route (c)
    return Problem(200, 3, seed=1)


LEAVES_A = synthetic_leaves(300, 2, seed=1)
SEG_A = np.array([0, 90, 201, 300])
LEAVES_C = synthetic_leaves(16640, 3, seed=2)
SEG_C = np.array([0, 8001, 16640])
BOXES = np.array([[[0.0, 1.0 / 3], [0.0, 1.0]], [[1.0 / 3, 2.0 / 3], [1.0 / 3, 2.0 / 3]], [[2.0 / 3, 1.0], [0.0, 1.0 / 3]]])


def _truth_vals(name, mean, var, incumbent):
    return AO.truth(AO.KINDS[name], mean, var, varsigma=VS, incumbent=incumbent)


def _value_tol(name):
    return 16.0 * AO.ULP if name == "ucb_std" else AO.tolerance(AO.KINDS[name])[0]


def _truth_winners(name, mean, var, seg, incumbent):
    """Per segment: (truth's arg-max, its gap to the runner-up in the error measure of the kind).  The float64 yardstick
    picks TOP candidates, the 60-digit truth ranks them."""
    kind = AO.KINDS[name]
    yard = AO.yardstick(kind, mean, var, varsigma=VS, incumbent=incumbent)
    out = []
    for a, b in zip(seg[:-1], seg[1:]):
        cand = a + np.argsort(-yard[a:b], kind="stable")[:TOP]
        vals = _truth_vals(name, mean[cand], var[cand], incumbent)
        order = sorted(range(len(cand)), key=lambda i: (-vals[i], cand[i]))
        best, second = vals[order[0]], vals[order[1]]
        scale = max(mp.mpf(1), abs(best)) if name == "logei" else abs(best)
        out.append((int(cand[order[0]] - a), float((best - second) / scale)))
    return out


def _assert_decidable(name, winners):
    for seg, (_, gap) in enumerate(winners):
        assert gap > 100.0 * _value_tol(name), (name, seg, gap)


def _check_values(name, mean, var, val, incumbent, noise=None):
    """The value column against truth on the call's own (mean, var).  ``noise``: the latent variant -- the device reads
    variance - sum BEFORE the noise is added, the returned var is that plus the noise rounded once, so truth's s^2 is known
    to half an ulp of var only: the value has to lie between truth at both ends of that interval, widened by the tolerance."""
    kind, tol = AO.KINDS[name], _value_tol(name)
    if noise is None:
        if name == "ucb_std":
            assert np.array_equal(val, mean + VS * np.sqrt(np.maximum(var, 0.0)))
            return 0.0
        err = AO.error(kind, val, _truth_vals(name, mean, var, incumbent))
        assert err <= tol, (name, err, tol)
        return err
    half = 0.5 * np.spacing(var)
    lo = AO.truth(kind, mean, var, varsigma=VS, incumbent=incumbent, s2_add=(-noise, -half))
    hi = AO.truth(kind, mean, var, varsigma=VS, incumbent=incumbent, s2_add=(-noise, half))
    worst = 0.0
    for g, a, b in zip(val, lo, hi):
        a, b = min(a, b), max(a, b)
        if not (a <= mp.mpf(float(g)) <= b):
            worst = max(worst, min(AO.error(kind, [g], [a]), AO.error(kind, [g], [b])))
    assert worst <= tol, (name, "latent", worst, tol)
    return worst


def _check_winner(eng, leaves, seg, spec, mean, var, val, incumbent):
    idx, mu, vv, best = eng.best_acq(leaves, spec, seg_off=seg, incumbent=incumbent)
    for s, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        i = int(np.argmax(val[a:b]))  # the first maximum, NaN first: np.argmax's rule is the library's
        assert idx[s] == i, (spec.name, s, idx[s], i)
        np.testing.assert_array_equal([mu[s], vv[s], best[s]], [mean[a + i], var[a + i], val[a + i]])
    return idx


def _route(prob, dtype, leaves, seg, small_calls=True):
    """Every kind on one batch: UCB_VAR's bits, the value column, the winners."""
    eng = prob.engine(dtype, small_calls)
    inc = prob.incumbent
    # the reference's rule: bits of gpso_best_ucb and gpso_predict
    ref = eng.best_ucb(leaves, VS, seg_off=seg)
    got = eng.best_acq(leaves, A.UCBVar(VS), seg_off=seg)
    for r, g in zip(ref, got):
        np.testing.assert_array_equal(r, g)
    pm, pv = eng.predict(leaves)
    mean, var, val = eng.acq_values(leaves, A.UCBVar(VS))
    np.testing.assert_array_equal(pm, mean)
    np.testing.assert_array_equal(pv, var)
    np.testing.assert_array_equal(val, mean + VS * var)
    mean_ref, var_ref = gpr.predict_y(prob.post, leaves)
    for name in NAMES:
        spec = _spec(name, inc)
        mean, var, val = eng.acq_values(leaves, spec, incumbent=inc)
        np.testing.assert_array_equal(pm, mean)
        np.testing.assert_array_equal(pv, var)
        # (the 60-digit comparison of the whole column where it is a few hundred rows; of a spread of rows otherwise)
        rows = np.arange(len(val)) if len(val) <= 512 else np.unique(np.linspace(0, len(val) - 1, 256).astype(int))
        err = _check_values(name, mean[rows], var[rows], val[rows], inc)
        idx = _check_winner(eng, leaves, seg, spec, mean, var, val, inc)
        winners = _truth_winners(name, mean_ref, var_ref, seg, inc)
        _assert_decidable(name, winners)
        print(f"{dtype} {name}: value error {err:.2e} (tolerance {_value_tol(name):.2e}); gaps {[f'{g:.1e}' for _, g in winners]}")
        assert [int(i) for i in idx] == [w for w, _ in winners], (name, idx, winners)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_a_small_call_kernel(dtype):
    _route(small(), dtype, LEAVES_A, SEG_A)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_b_two_stage_argmax_finalising_in_stage_1(dtype):
    _route(small(), dtype, LEAVES_A, SEG_A, small_calls=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_c_past_the_small_call_limit(dtype):
    _route(large(), dtype, LEAVES_C, SEG_C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_route_a_latent(dtype, name):
    prob = small()
    eng = prob.engine(dtype)
    spec = _spec(name, prob.incumbent, latent=True)
    mean, var, val = eng.acq_values(LEAVES_A, spec, incumbent=prob.incumbent)
    pm, pv = eng.predict(LEAVES_A)
    np.testing.assert_array_equal(pm, mean)
    np.testing.assert_array_equal(pv, var)
    if name == "ucb_std":  # (not bitwise here: sqrt of the unrounded latent variance; within the interval, at 16 ulp)
        _check_values("ucb_std", mean, var, val, prob.incumbent, noise=prob.theta.noise)
    else:
        _check_values(name, mean, var, val, prob.incumbent, noise=prob.theta.noise)
    _check_winner(eng, LEAVES_A, SEG_A, spec, mean, var, val, prob.incumbent)
    # the latent variance is smaller: the value differs from the predictive variant's
    assert not np.array_equal(val, eng.acq_values(LEAVES_A, _spec(name, prob.incumbent), incumbent=prob.incumbent)[2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("depth", [4, 9])  # (d) the small keyed route: 3 x 40 rows; (e) the large one: 3 x 9841 = 29 523
def test_routes_d_e_grown(dtype, depth):
    prob = small()
    eng = prob.engine(dtype)
    inc = prob.incumbent
    rows = tree.grow_count(depth)
    coords = eng.grow(BOXES, depth).reshape(-1, 2)
    seg = np.arange(4) * rows
    for r, g in zip(eng.best_ucb_grow(BOXES, depth, VS), eng.best_acq_grow(BOXES, depth, A.UCBVar(VS))):
        np.testing.assert_array_equal(r, g)
    mean_ref, var_ref = gpr.predict_y(prob.post, coords)
    firsts = [seg[s] + np.sort(np.unique(coords[seg[s]:seg[s + 1]], axis=0, return_index=True)[1]) for s in range(3)]
    keep = np.concatenate(firsts)
    kseg = np.concatenate([[0], np.cumsum([len(f) for f in firsts])])
    for name in NAMES:
        spec = _spec(name, inc)
        mean, var, val = eng.acq_values(coords, spec, incumbent=inc)
        idx, mu, vv, best = eng.best_acq_grow(BOXES, depth, spec, incumbent=inc)
        for s in range(3):
            i = int(np.argmax(val[seg[s]:seg[s + 1]]))  # (the first maximum over the full duplicated list)
            assert idx[s] == i, (name, s, idx[s], i)
            np.testing.assert_array_equal([mu[s], vv[s], best[s]], [mean[seg[s] + i], var[seg[s] + i], val[seg[s] + i]])
        # truth's winner: a centre child repeats its parent bit for bit, so the best value occurs more than once in the
        # duplicated list -- ranked over the distinct rows of each box, reported by the first occurrence
        winners = _truth_winners(name, mean_ref[keep], var_ref[keep], kseg, inc)
        _assert_decidable(name, winners)
        want = [int(keep[kseg[s] + w] - seg[s]) for s, (w, _) in enumerate(winners)]
        assert [int(i) for i in idx] == want, (name, idx, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_f_two_tickets_of_different_kinds(dtype):
    prob = small()
    eng = prob.engine(dtype)
    inc = prob.incumbent
    ei, logei, std = _spec("ei", inc), _spec("logei", inc), _spec("ucb_std")
    block_ei = eng.best_acq(LEAVES_A, ei, seg_off=SEG_A)
    block_le = eng.best_acq(LEAVES_A, logei, seg_off=SEG_A)
    block_gs = eng.best_acq_grow(BOXES, 4, std)
    t1 = eng.best_acq_begin(LEAVES_A, ei, seg_off=SEG_A)
    t2 = eng.best_acq_begin(LEAVES_A, logei, seg_off=SEG_A)
    got_le = eng.best_ucb_end(t2)  # (ended out of order)
    got_ei = eng.best_ucb_end(t1)
    t3 = eng.best_acq_grow_begin(BOXES, 4, std)
    t4 = eng.best_ucb_begin(LEAVES_A, VS, seg_off=SEG_A)
    got_gs, got_ucb = eng.best_ucb_end(t3), eng.best_ucb_end(t4)
    for want, got in ((block_ei, got_ei), (block_le, got_le), (block_gs, got_gs), (eng.best_ucb(LEAVES_A, VS, seg_off=SEG_A), got_ucb)):
        for w, g in zip(want, got):
            np.testing.assert_array_equal(w, g)


def test_route_g_installed_sgpr_posterior_scored_with_logei():
    from tests import sgpr_oracle as S

    prob = small()
    Z = prob.X[:16].copy()
    u = S.initial_u(0.5, 1.0, 0.01, 0.0)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(prob.X, prob.y)
    eng.sgpr_set_inducing(Z)
    eng.sgpr_posterior("Matern52", u, 1, True, 0.0)
    post = S.Posterior("Matern52", u, 1, True, 0.0, prob.X, prob.y, Z)
    inc = prob.incumbent
    spec = _spec("logei", inc)
    mean, var, val = eng.acq_values(LEAVES_A, spec, incumbent=inc)
    pm, pv = eng.predict(LEAVES_A)
    np.testing.assert_array_equal(pm, mean)
    np.testing.assert_array_equal(pv, var)
    _check_values("logei", mean, var, val, inc)
    idx = _check_winner(eng, LEAVES_A, SEG_A, spec, mean, var, val, inc)
    mean_ref, var_ref = post.predict_y(LEAVES_A)
    winners = _truth_winners("logei", np.asarray(mean_ref).reshape(-1), np.asarray(var_ref).reshape(-1), SEG_A, inc)
    _assert_decidable("logei", winners)
    assert [int(i) for i in idx] == [w for w, _ in winners]
    for r, g in zip(eng.best_ucb(LEAVES_A, VS, seg_off=SEG_A), eng.best_acq(LEAVES_A, A.UCBVar(VS), seg_off=SEG_A)):
        np.testing.assert_array_equal(r, g)


@pytest.mark.parametrize("dtype", DTYPES)
def test_logei_ranks_on_the_device_where_ei_is_zero(dtype):
    prob = small()
    eng = prob.engine(dtype)
    tau = prob.incumbent + 60.0 * np.sqrt(prob.theta.variance)
    mean_ref, var_ref = gpr.predict_y(prob.post, LEAVES_A)
    assert np.all(AO.yardstick(AO.EI, mean_ref, var_ref, incumbent=tau) == 0.0)  # float64 EI is dead on every row
    idx, _, _, best = eng.best_acq(LEAVES_A, A.EI(incumbent=tau), seg_off=SEG_A)
    assert list(idx) == [0, 0, 0] and np.all(best == 0.0)  # every row ties: the first maximum is row 0
    eng.set_timing(True)
    eng.predict(LEAVES_A[:7])  # (another count: what is read below describes the acq_values call)
    mean, var, val = eng.acq_values(LEAVES_A, A.LogEI(incumbent=tau))
    assert eng.last_count(0) == eng.last_count(1) == len(LEAVES_A) and eng.last_ms(1) > 0.0
    assert np.all(np.isfinite(val))
    _check_values("logei", mean, var, val, tau)
    idx = _check_winner(eng, LEAVES_A, SEG_A, A.LogEI(incumbent=tau), mean, var, val, tau)
    winners = _truth_winners("logei", mean_ref, var_ref, SEG_A, tau)
    _assert_decidable("logei", winners)
    assert [int(i) for i in idx] == [w for w, _ in winners] and any(w != 0 for w, _ in winners)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_coordinate_wins_its_segment_under_every_kind(dtype):
    prob = small()
    leaves = LEAVES_A.copy()
    leaves[137, 1] = np.nan  # a row of the second segment
    for small_calls in (True, False):
        eng = prob.engine(dtype, small_calls)
        for name in ["ucb_var"] + NAMES:
            idx, mu, vv, best = eng.best_acq(leaves, _spec(name, prob.incumbent), seg_off=SEG_A, incumbent=prob.incumbent)
            assert idx[1] == 137 - SEG_A[1] and np.isnan(mu[1]) and np.isnan(vv[1]) and np.isnan(best[1]), (name, idx)
            assert not np.isnan(best[0]) and not np.isnan(best[2])


def test_bad_records_and_states():
    from pygpso_amd import _lib as L

    prob = small()
    eng = prob.engine("float64")
    for bad in (A.EI(incumbent=np.inf), A.PI(incumbent=0.0, xi=np.nan), A.UCBStd(np.nan)):
        with pytest.raises(ValueError, match="must be finite"):  # (GPSO_E_ARG: the engine raises ValueError with the message)
            eng.best_acq(LEAVES_A, bad)
        with pytest.raises(ValueError, match="must be finite"):
            eng.acq_values(LEAVES_A, bad)
    fresh = HipGPEngine("float64", device=0)
    fresh.d = 2
    with pytest.raises(L.GpsoHipError) as err:
        fresh.best_acq(LEAVES_A, A.UCBStd(VS))
    assert err.value.code == L.E_STATE
    t1 = eng.best_acq_begin(LEAVES_A, A.UCBStd(VS))
    t2 = eng.best_acq_begin(LEAVES_A, A.UCBStd(VS))
    with pytest.raises(L.GpsoHipError) as err:
        eng.best_acq_begin(LEAVES_A, A.UCBStd(VS))
    assert err.value.code == L.E_STATE
    eng.best_ucb_end(t1), eng.best_ucb_end(t2)


def test_surrogate_on_ucb_std_reproduces_the_stand_in_run():
    """GPRSurrogate(gp_acquisition="ucb_std"): 20 evaluations of the toy objective on the GPU against the same run on the CPU
    stand-in (tests/test_acq_cpu.py), the ``score_ucb`` column within the float64 tolerance of tests/test_gpu_goldens.py
    (1e-8, through the L-BFGS-B fits of both platforms)."""
    from pygpso_amd import GPRSurrogate, GPSOptimiser, ParameterSpace
    from pygpso_amd import kernels as K
    from tests.helpers import rotated_peaks
    from tests.acq_oracle import AcqOracleEngine

    def run(factory):
        old = GPRSurrogate.engine_factory
        GPRSurrogate.engine_factory = factory
        try:
            # (GPRSurrogate.default()'s specification -- the one the golden runs of tests/test_gpu_goldens.py reproduce
            # across platforms -- with the acquisition keyword)
            surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0),
                                gp_acquisition="ucb_std")
            opt = GPSOptimiser(parameter_space=ParameterSpace(parameter_names=["x", "y"], parameter_bounds=[[-3, 5], [-3, 3]]),
                               gp_surrogate=surr, exploration_method="tree", exploration_depth=3, budget=20,
                               stopping_condition="evaluations", update_cycle=1, n_workers=1)
            opt.run(rotated_peaks)
            return surr.points
        finally:
            GPRSurrogate.engine_factory = old

    cpu, gpu = run(AcqOracleEngine), run(None)
    assert len(cpu) == len(gpu) and [p.label for p in cpu] == [p.label for p in gpu]
    np.testing.assert_allclose([p.score_ucb for p in gpu], [p.score_ucb for p in cpu], rtol=0, atol=1e-8)
    vs = float(gpr.VARSIGMA_DEFAULT)
    for p in gpu:
        if p.label.name == "gp_based":
            assert p.score_ucb == p.score_mu + vs * np.sqrt(p.score_sigma)
