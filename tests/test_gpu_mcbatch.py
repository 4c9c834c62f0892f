"""
GPU tests of ``gpso_paths_best_batch`` (Monte-Carlo batch acquisition over the path draws) through the
C-ABI, and of ``GPSurrogate.select_batch_mc`` on top of it.
  bits ....... the device rounds against ``gpso_paths_batch_host`` on the values ``gpso_paths_eval`` returns for the same rows:
               the same idx and n_picked, and bitwise the same gain, batch_value and gain0
  parity ..... the same calls against tests/mcbatch_oracle.py fed by the float64 path oracle's values (tests/paths_cases.py,
               tests/paths_q_cases.py): the same idx, gains within the case's float64 stage tolerance (1e-8 of its scale, 1e-4
               for the Matern-1/2).  A value off by at most tol moves a QEI gain by at most 2 tol and a QPI count not at all
               while no value lies within tol of its threshold; the bars and margins of every case are CHOSEN, with the oracle
               alone (tests/mcbatch_cases.py; asserted here before anything runs on the device and, on the CPU,
               in tests/test_mcbatch_cpu.py), so that every round's gap exceeds four times the tolerance.  No case is
               dropped on the device
Shapes: (N, D) = (2, 1), (17, 3), (129, 3); S = 1, 17, 129 (a second block of draws); m = 1, 64, 65 and 16384 + 3 (stage A's
chunk boundary, the round-0 winner moved into the last chunk); b = 0, 3; q = 1, 2, 64; both kinds; scalar and per-draw bars;
float64 and mixed engines; host and device leaves.
"""
import ctypes as C

import numpy as np
import pytest

from tests import mcbatch_cases as mc
from tests import mcbatch_oracle as mo
from tests import paths_cases as pc
from tests import paths_q_cases as qc
from tests.test_gpu_paths import drawn, fitted

pytestmark = pytest.mark.gpu

CONFIGS, config_inputs = mc.CONFIGS, mc.config_inputs


def _leaves(eng, rows, on_device):
    if not on_device:
        return rows
    import torch

    t = torch.from_numpy(np.ascontiguousarray(rows)).to(torch.device("cuda", eng.device))
    torch.cuda.synchronize()
    return t


def both_routes(eng, rows, pend, q, kind, inc, bars, xi, on_device=False):
    """The device call and the host rounds on ``gpso_paths_eval``'s values of the same rows: asserts the bits, returns the
    device's (idx, gain, batch_value, gain0)."""
    from pygpso_amd import HipGPEngine

    b = 0 if pend is None else pend.shape[0]
    V = eng.paths_eval(rows if pend is None else np.vstack([rows, pend]))[0]
    kw = dict(incumbent=inc) if bars is None else dict(incumbent_s=bars)
    want = HipGPEngine.paths_batch_host(V, q, kind, n_pending=b, xi=xi, **kw)
    got = eng.paths_best_batch(_leaves(eng, rows, on_device), q, kind, pending=pend, xi=xi, want_gain0=True, **kw)
    assert np.array_equal(got[0], want[0]), (kind, q, got[0], want[0])
    for a, w in zip(got[1:], want[1:]):
        assert a.shape == w.shape and a.tobytes() == w.tobytes(), (kind, q)
    return got


# ---- 1. bits, and parity with the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_bits_of_the_host_rounds_and_parity_with_the_oracle(ci):
    index, m, b, dtype, on_device = CONFIGS[ci]
    r, rows, pend, V, chosen = config_inputs(ci)
    assert len(chosen) == 4
    eng = drawn(r, dtype)
    worst = 0.0
    for (kind, per_draw), (inc, bars, xi) in sorted(chosen.items()):
        for q in (1, 2, 64):
            idx, gain, value, gain0 = both_routes(eng, rows, pend, q, kind, inc, bars, xi, on_device)
            want = mo.greedy(V, m, q, kind, bars if per_draw else inc, xi)
            assert np.array_equal(idx, want[0]), (pc.name(index), kind, per_draw, q, idx, want[0])
            err = max(float(np.max(np.abs(gain - want[1]))), float(np.max(np.abs(gain0 - want[3]))))
            worst = max(worst, err)
            assert err <= (r["tol"] if kind == "qei" else 0.0)
            assert np.all(np.abs(value - want[2]) <= len(idx) * r["tol"])
    if m > pc.CHUNK:
        assert int(eng.paths_best_batch(rows, 1, "qei", incumbent=float(np.median(V[:, :m])))[0][0]) == m - 2  # in the last chunk
    print(f"mc batch {pc.name(index)} m={m} b={b} {dtype}: largest gain error {worst:.2e} (tolerance {r['tol']:.2e})")
    eng.close()


# ---- 2. every posterior family ---------------------------------------------------------------------------------------------------
def test_the_exact_gp_after_an_append():
    from tests.test_gpu_paths import _engine

    r = pc.append_case()
    X, y, th = r["X"], r["y"], r["th"]
    eng = _engine()
    eng.set_data(X[:300], y[:300])
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    _, in_place = eng.append(X[300:], y[300:])
    assert in_place
    eng.paths_draw(r["omega"], r["phase"], r["w"], r["eps"])
    inc = float(np.median(r["values"]))
    for kind in ("qei", "qpi"):
        idx = both_routes(eng, r["Xs"], None, 4, kind, inc, None, 0.0)[0]
        if mo.decided_by(r["values"], 70, 4, kind, inc) > 2.0 * r["tol"]:
            assert np.array_equal(idx, mo.greedy(r["values"], 70, 4, kind, inc)[0])
    eng.close()


@pytest.mark.parametrize("index", (1, 5, 10))  # a VGP, an SGPR, a Student-t SVGP: S = 17, 65 / 65 / 130 rows
def test_the_variational_families(index):
    from tests.test_gpu_paths_q import drawn as drawn_q

    r = qc.reference(index)
    eng = drawn_q(r)
    m = r["Xs"].shape[0] - 3
    rows, pend = r["Xs"][:m], r["Xs"][m:]
    bars = np.median(r["values"], axis=1)
    for kind in ("qei", "qpi"):
        idx, gain, _, _ = both_routes(eng, rows, pend, 5, kind, None, bars, 0.0)
        if mo.decided_by(r["values"], m, 5, kind, bars) > 2.0 * r["tol"]:
            want = mo.greedy(r["values"], m, 5, kind, bars)
            assert np.array_equal(idx, want[0]) and np.all(np.abs(gain - want[1]) <= r["tol"])
    eng.close()


# ---- 3. the call only reads --------------------------------------------------------------------------------------------------------
def test_read_only_repeatable_and_a_rows_gain0_is_its_own():
    r = pc.reference(7)  # N = 300, D = 5, S = 16, M = 130
    eng = drawn(r)
    Xs = r["Xs"]
    inc = float(np.median(r["values"]))
    h0, before = eng.posterior_hash(), eng.paths_eval(Xs)
    first = eng.paths_best_batch(Xs, 6, "qei", incumbent=inc, pending=Xs[:2], want_gain0=True)
    again = eng.paths_best_batch(Xs, 6, "qei", incumbent=inc, pending=Xs[:2], want_gain0=True)
    after = eng.paths_eval(Xs)
    assert eng.posterior_hash() == h0 and eng.paths_info() == (16, 257)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    # a row's round-0 gain: alone, in a sub-batch, in a permuted batch, with another q and with device outputs
    g0 = eng.paths_best_batch(Xs, 1, "qei", incumbent=inc, want_gain0=True)[3]
    assert eng.paths_best_batch(Xs[77:78], 1, "qei", incumbent=inc, want_gain0=True)[3][0] == g0[77]
    assert np.array_equal(eng.paths_best_batch(Xs[60:70], 3, "qei", incumbent=inc, want_gain0=True)[3], g0[60:70])
    perm = np.random.default_rng(1).permutation(130)
    assert np.array_equal(eng.paths_best_batch(Xs[perm], 64, "qei", incumbent=inc, want_gain0=True)[3], g0[perm])
    for kind in ("qei", "qpi"):
        p1 = eng.paths_best_batch(Xs, 1, kind, incumbent=inc, want_gain0=True)
        assert int(p1[0][0]) == int(np.argmax(p1[3])) and p1[1][0] == p1[3].max() == p1[2][0]
    # timing and counts describe the call
    eng.set_timing(True)
    eng.paths_best_batch(Xs, 2, "qei", incumbent=inc)
    assert eng.last_ms(1) > 0.0 and eng.last_count(0) == 130 and eng.last_count(1) == 130
    # gain0 into device memory
    import torch

    from pygpso_amd import _lib as L

    out = torch.empty(130, dtype=torch.float64, device=torch.device("cuda", eng.device))
    torch.cuda.synchronize()
    xs = np.ascontiguousarray(Xs)
    rec, idx, n = L.GpsoMcAcq(L.MC_QEI, 0.0, inc), np.zeros(4, dtype=np.int64), C.c_int(0)
    rc = eng._lib.gpso_paths_best_batch(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, 130, C.byref(rec), None, None, 0, 4,
                                        L.i64ptr(idx), None, None, C.byref(n), C.c_void_p(out.data_ptr()), L.MEM_DEVICE)
    assert rc == L.OK and n.value == 4 and np.array_equal(out.cpu().numpy(), g0)
    eng.close()


# ---- 4. statuses -------------------------------------------------------------------------------------------------------------------
def _code(eng, Xs, kind=0, xi=0.0, inc=0.0, bars=None, pend=None, b=0, q=2, m=None, xs_null=False, rec_null=False, idx_null=False,
          n_null=False, out_mem=0):
    from pygpso_amd import _lib as L

    xs = np.ascontiguousarray(Xs, dtype=np.float64)
    rec, idx, n = L.GpsoMcAcq(kind, xi, inc), np.zeros(64, dtype=np.int64), C.c_int(0)
    bars = None if bars is None else np.ascontiguousarray(bars, dtype=np.float64)
    pend = None if pend is None else np.ascontiguousarray(pend, dtype=np.float64)
    return eng._lib.gpso_paths_best_batch(eng._h, None if xs_null else C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST,
                                          xs.shape[0] if m is None else m, None if rec_null else C.byref(rec),
                                          None if bars is None else L.dptr(bars), None if pend is None else L.dptr(pend), b, q,
                                          None if idx_null else L.i64ptr(idx), None, None, None if n_null else C.byref(n), None, out_mem)


def test_statuses():
    from pygpso_amd import _lib as L
    from tests.test_gpu_paths import _engine

    r = pc.reference(3)  # N = 17, D = 3, S = 16
    th, Xs = r["th"], r["Xs"]
    eng = fitted(r)
    assert _code(eng, Xs) == L.E_STATE  # no path set
    eng.paths_draw(r["omega"], r["phase"], r["w"], r["eps"])
    assert _code(eng, Xs) == L.OK
    want = eng.paths_eval(Xs)[0]
    for bad in (dict(m=0), dict(q=0), dict(q=65), dict(b=-1), dict(b=65, pend=np.zeros((65, 3))), dict(b=2), dict(xs_null=True),
                dict(rec_null=True), dict(idx_null=True), dict(n_null=True), dict(kind=2), dict(kind=-1), dict(xi=np.nan),
                dict(inc=np.nan), dict(bars=np.r_[np.zeros(15), np.nan]), dict(out_mem=7), dict(m=(1 << 22) + 1)):
        assert _code(eng, Xs, **bad) == L.E_ARG, bad
    for fine in (dict(inc=np.inf), dict(inc=-np.inf), dict(inc=np.nan, bars=np.zeros(16)), dict(bars=np.full(16, -np.inf)),
                 dict(b=2, pend=Xs[:2]), dict(q=64), dict(kind=1, xi=np.inf)):
        assert _code(eng, Xs, **fine) == L.OK, fine
    ticket = eng.best_ucb_begin(Xs, 2.0)
    assert _code(eng, Xs) == L.E_STATE  # an asynchronous best-UCB ticket open
    eng.best_ucb_end(ticket)
    assert np.array_equal(eng.paths_eval(Xs)[0], want)  # refused calls left the set serving the same bits
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    assert _code(eng, Xs) == L.E_STATE  # a stale set after a fit
    eng.close()
    e32 = _engine("float32")
    e32.set_data(r["X"], r["y"])
    e32.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    assert _code(e32, Xs) == L.E_ARG
    e32.close()


# ---- 5. the Python layer -------------------------------------------------------------------------------------------------------------
def _small_run(poke=None):
    from pygpso_amd import GPRSurrogate, GPSOptimiser, ParameterSpace
    from pygpso_amd import kernels as K
    from tests.helpers import rotated_peaks

    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0))
    opt = GPSOptimiser(parameter_space=ParameterSpace(parameter_names=["x", "y"], parameter_bounds=[[-3, 5], [-3, 3]]),
                       gp_surrogate=surr, exploration_method="tree", exploration_depth=3, budget=12,
                       stopping_condition="evaluations", update_cycle=1, n_workers=1)

    def objective(point):
        if poke is not None and surr.gpflow_model is not None and len(surr.current_training_data[1]) >= 6:
            poke(surr)
        return rotated_peaks(point)

    opt.run(objective)
    return surr, [(tuple(p.normed_coord), p.score_mu, p.score_sigma, p.score_ucb, p.label) for p in surr.points]


def test_select_batch_mc_and_the_loop_is_unchanged():
    from tests.helpers import synthetic_leaves

    leaves = synthetic_leaves(500, 2, seed=3)
    surr, plain = _small_run()
    stored = list(surr.points)
    idx, gain, value = surr.select_batch_mc(leaves, 6, n_paths=32, n_features=256, rng=7)
    model = surr.gpflow_model
    assert len(idx) == 6 and len(set(idx.tolist())) == 6 and np.all(np.diff(gain) <= 0.0) and np.all(gain > 0.0)
    assert model.engine.paths_info() == (32, 256)
    # the bars are eval_paths' best_val over the evaluated points
    x_train = np.ascontiguousarray(surr.current_training_data[0])
    bars = model.eval_paths(x_train, want_values=False)[2][:, 0]
    direct = model.mc_batch(leaves, 6, "qnei", incumbent_s=bars)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((idx, gain, value), direct))
    V = model.eval_paths(leaves)[0]
    assert np.array_equal(idx, mo.greedy(V, 500, 6, "qei", bars)[0]) or mo.decided_by(V, 500, 6, "qei", bars) < 1e-12
    for kind in ("qnei", "qei", "qpi"):
        i1, g1, _, g0 = surr.select_batch_mc(leaves, 1, kind=kind, return_gain0=True)
        assert int(i1[0]) == int(np.argmax(g0)) and g1[0] == g0.max()
    pend = leaves[idx[:2]]
    i2 = surr.select_batch_mc(leaves, 4, pending=pend)[0]
    assert not (set(i2.tolist()) & set(idx[:2].tolist()))
    assert list(surr.points) == stored
    # the loop: a run during which the surrogate is asked for batches equals the plain run bit for bit
    _, poked = _small_run(lambda s: s.select_batch_mc(leaves, 3, n_paths=8, n_features=64, rng=1))
    assert poked == plain
