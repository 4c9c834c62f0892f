"""
CPU tests of the Monte-Carlo batch acquisition over path draws: ``gpso_paths_batch_host`` -- the host
restatement of csrc/mcbatch.hpp that the device rounds are held to bit for bit in tests/test_gpu_mcbatch.py -- against the
independent numpy oracle of tests/mcbatch_oracle.py, the rules of the rounds, every refusal of the host call, and the Python
surface over a stub engine.

Tolerance of a QEI gain.  A gain is the mean of S non-negative terms, each at most ``scale`` = max|V| + max|bar| + |xi|.  A
term carries at most three roundings on either side (two subtractions in the header, three in the oracle, which subtracts the
held improvement instead of moving the bar), each at most eps scale: the numbers rounded are below 2 scale.  The header sums
the terms in draw order, numpy's ``mean`` pairwise: either sum is within (S - 1) eps/2 of the exact sum of its terms, relative
to a sum of at most S scale, and the division adds one rounding.  So two gains of the same row differ by at most
2 (S + 3) eps scale =: BOUND(S, scale).  It is not tuned.  A QPI gain is an integer count divided once by S: exact on both
sides, bound zero, and a tie is decided by the shared rule (the first maximum).  The inputs are chosen -- and checked here
with the oracle alone -- so that the two highest QEI gains of every round that reports a pick differ by more than twice
BOUND; no case is skipped.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from pygpso_amd import _lib as L
from tests import mcbatch_oracle as mo

EPS = float(np.finfo(np.float64).eps)
KINDS = {"qei": L.MC_QEI, "qpi": L.MC_QPI}


def bound(s, scale):
    return 2.0 * (s + 3) * EPS * scale


@pytest.fixture(scope="module")
def lib():
    import os

    import __graft_entry__ as entry

    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.load()


def host(lib, V, m, q, kind, incumbent=0.0, bars=None, xi=0.0, want=(True, True, True)):
    """The raw C call -> (rc, idx, gain, batch_value, gain0, n_picked)."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    s, b = V.shape[0], V.shape[1] - m
    rec = L.GpsoMcAcq(KINDS[kind], float(xi), float(incumbent))
    idx = np.full(max(q, 1), -7, dtype=np.int64)
    gain, value = np.full(max(q, 1), -7.0), np.full(max(q, 1), -7.0)
    gain0 = np.full(max(m, 1), -7.0)
    n = C.c_int(-1)
    bars = None if bars is None else np.ascontiguousarray(bars, dtype=np.float64)
    rc = lib.gpso_paths_batch_host(C.byref(rec), L.dptr(V), s, m, b, None if bars is None else L.dptr(bars), q, L.i64ptr(idx),
                                   L.dptr(gain) if want[0] else None, L.dptr(value) if want[1] else None, C.byref(n),
                                   L.dptr(gain0) if want[2] else None)
    k = max(n.value, 0)
    return rc, idx[:k], gain[:k], value[:k], gain0[:m], n.value


def random_case(s, m, b, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((s, m + b)) + 0.3 * rng.standard_normal((1, m + b))
    bars = V[:, :m].mean(axis=1) - 0.5 + 0.1 * rng.standard_normal(s)  # per draw: a bar most rows of the draw clear
    return V, float(V.mean() - 1.0), bars


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,m", list(itertools.product((1, 17, 129), (1, 5, 65))))
def test_host_rounds_equal_the_oracle(lib, s, m):
    for b, q, kind, per_draw in itertools.product((0, 3), (1, 2, 64), ("qei", "qpi"), (False, True)):
        V, inc, bars = random_case(s, m, b, seed=1000 * s + 10 * m + b)
        xi = 0.01 if per_draw else 0.0
        start = bars if per_draw else inc
        want_i, want_g, want_v, want_g0, margins = mo.greedy(V, m, q, kind, start, xi)
        tol = bound(s, float(np.max(np.abs(V)) + np.max(np.abs(start)) + xi)) if kind == "qei" else 0.0
        what = f"S={s} m={m} b={b} q={q} {kind} {'per-draw' if per_draw else 'scalar'}"
        # the case is decided: checked with the oracle alone
        assert margins.size == want_i.size and (kind == "qpi" or np.all(margins > 2.0 * tol)), (what, margins, tol)
        rc, idx, gain, value, gain0, n = host(lib, V, m, q, kind, inc, bars if per_draw else None, xi)
        assert rc == L.OK and n == want_i.size and 1 <= n <= min(q, m), what
        assert np.array_equal(idx, want_i), what
        assert np.all(np.abs(gain - want_g) <= tol) and np.all(np.abs(gain0 - want_g0) <= tol), what
        assert np.all(np.abs(value - want_v) <= n * tol), what
        assert gain[0] == gain0[idx[0]] and len(set(idx.tolist())) == n
        if kind == "qei":
            assert np.all(np.diff(gain) <= 0.0), (what, gain)  # submodular: the gains never rise
            assert abs(value[-1] - mo.batch_value_qei(V, m, idx, start, xi)) <= (n + 1) * tol, what
        # outputs are optional one by one, and the picks do not depend on which are asked for
        rc2, idx2, _, _, _, n2 = host(lib, V, m, q, kind, inc, bars if per_draw else None, xi, want=(False, False, False))
        assert rc2 == L.OK and n2 == n and np.array_equal(idx2, idx)


def test_every_gpu_configuration_is_decided():
    """tests/mcbatch_cases.py: for each configuration of the GPU suite, each kind and each bar type a margin of the grid exists
    at which every round of q = 1, 2 and 64 is decided by more than two tolerances (a gap of four) -- so the GPU suite drops no case."""
    from tests import mcbatch_cases as mc

    for ci in range(len(mc.CONFIGS)):
        chosen = mc.config_inputs(ci)[4]
        assert sorted(chosen) == [("qei", False), ("qei", True), ("qpi", False), ("qpi", True)], (mc.CONFIGS[ci], sorted(chosen))


# ---- 2. the rules ------------------------------------------------------------------------------------------------------------
def test_a_duplicated_column_is_never_picked_twice(lib):
    V, inc, bars = random_case(17, 12, 0, seed=3)
    for kind, xi in (("qei", 0.0), ("qei", 0.05), ("qei", -0.05), ("qpi", 0.0), ("qpi", 0.05)):
        first = int(mo.greedy(V, 12, 1, kind, inc, xi)[0][0])
        V2 = np.hstack([V, V[:, first:first + 1], V[:, first:first + 1]])  # two copies of the winner behind the batch
        rc, idx, gain, _, gain0, n = host(lib, V2, 14, 14, kind, inc, xi=xi)
        assert rc == L.OK and n >= 2 and int(idx[0]) == first  # (the first of the tie wins)
        assert not (set(idx[1:].tolist()) & {first, 12, 13}) and np.all(gain[1:] > 0.0)
        assert gain0[first] == gain0[12] == gain0[13]


def test_a_nan_column_wins_and_ends_the_batch(lib):
    V, inc, bars = random_case(17, 9, 0, seed=4)
    V[5, 6] = np.nan
    for kind in ("qei", "qpi"):
        rc, idx, gain, value, gain0, n = host(lib, V, 9, 4, kind, inc)
        assert rc == L.OK and n == 1 and idx[0] == 6 and np.isnan(gain[0]) and np.isnan(value[0])
        assert np.isnan(gain0[6]) and not np.isnan(np.delete(gain0, 6)).any()
    # ... in a later round: row 6 is a NaN only in a draw whose term is reached -- every round sees it, so it wins round 0;
    # a NaN that shows up among the PENDING columns moves no bar
    V2, inc, _ = random_case(17, 9, 2, seed=5)
    ref = host(lib, np.delete(V2, 10, axis=1), 9, 3, "qei", inc)
    V2[:, 10] = np.nan
    got = host(lib, V2, 9, 3, "qei", inc)
    pend_only = host(lib, np.hstack([V2[:, :9], V2[:, 9:10]]), 9, 3, "qei", inc)
    assert np.array_equal(got[1], pend_only[1]) and np.array_equal(got[2], pend_only[2]) and np.array_equal(ref[1], got[1])


def test_q_above_m_ends_at_m_or_earlier(lib):
    V, inc, bars = random_case(129, 5, 0, seed=6)
    for kind in ("qei", "qpi"):
        rc, idx, gain, _, _, n = host(lib, V, 5, 64, kind, inc)
        assert rc == L.OK and 1 <= n <= 5 and len(set(idx.tolist())) == n
    # a bar far below everything: every row improves every draw, and every later gain is still > 0 until the rows run out
    V = np.arange(1.0, 21.0).reshape(4, 5)
    V = V[:, ::-1] + 10.0 * np.eye(4, 5)[:, ::-1]  # each of the first picks is best in some draw
    rc, idx, gain, _, _, n = host(lib, V, 5, 64, "qei", -100.0)
    assert rc == L.OK and n <= 5 and np.all(gain > 0.0)


def test_a_batch_ends_when_no_draw_can_improve(lib):
    V, _, _ = random_case(17, 30, 0, seed=7)
    top = float(V.max())
    for kind in ("qei", "qpi"):
        # nothing clears the bar: round 0's pick is still reported -- the first row, gain 0 --, and the batch ends
        rc, idx, gain, value, gain0, n = host(lib, V, 30, 8, kind, top + 1.0)
        assert rc == L.OK and n == 1 and idx[0] == 0 and gain[0] == 0.0 and value[0] == 0.0 and not gain0.any()
        # +inf bars likewise
        rc, idx, gain, _, _, n = host(lib, V, 30, 8, kind, np.inf)
        assert rc == L.OK and n == 1 and idx[0] == 0 and gain[0] == 0.0
    # one row holds every draw's maximum: after it nothing can improve
    V[:, 11] = V.max(axis=1) + 0.5
    rc, idx, gain, _, _, n = host(lib, V, 30, 8, "qei", float(V.mean()))
    assert rc == L.OK and n == 1 and idx[0] == 11 and gain[0] > 0.0
    rc, idx, _, _, _, n = host(lib, V, 30, 8, "qpi", float(V.min()) - 1.0)  # (every row clears every draw: gain 1, first row)
    assert rc == L.OK and n == 1 and idx[0] == 0


def test_pending_columns_raise_the_bars_and_are_never_returned(lib):
    V, inc, bars = random_case(17, 20, 3, seed=8)
    best = int(host(lib, V[:, :20], 20, 1, "qei", inc)[1][0])
    Vp = V.copy()
    Vp[:, 20] = V[:, best]  # the round-0 winner is already being evaluated
    for kind in ("qei", "qpi"):
        rc, idx, gain, _, gain0, n = host(lib, Vp, 20, 20, kind, inc)
        assert rc == L.OK and best not in idx.tolist() and np.all(idx < 20) and gain0[best] == 0.0 and gain0.shape == (20,)
        free = host(lib, V[:, :20], 20, 1, kind, inc)
        assert np.all(gain0 <= free[4]) and np.any(gain0 < free[4])
    # QEI at xi = 0: the same as starting from the raised bars without pending columns
    t0 = np.maximum(inc, Vp[:, 20:].max(axis=1))
    a = host(lib, Vp, 20, 6, "qei", inc)
    b = host(lib, Vp[:, :20], 20, 6, "qei", 0.0, bars=t0)
    assert all(np.array_equal(x, y) for x, y in zip(a[1:5], b[1:5]))


def test_minus_infinity_bars(lib):
    V, _, bars = random_case(17, 9, 0, seed=9)
    rc, idx, gain, value, gain0, n = host(lib, V, 9, 3, "qei", -np.inf)
    assert rc == L.OK and idx[0] == 0 and np.all(np.isposinf(gain0)) and np.isposinf(gain[0]) and np.all(np.isposinf(value))
    # ... and from round 1 on the bars are the first pick's values: finite gains, the oracle's picks
    # (the oracle from those bars: its definition by improvements over t0 has no meaning at t0 = -inf)
    want = mo.greedy(V, 9, 2, "qei", V[:, 0])
    assert n == 1 + want[0].size and np.array_equal(idx[1:], want[0]) and np.all(np.isfinite(gain[1:]))
    assert np.all(np.abs(gain[1:] - want[1]) <= bound(17, 2.0 * float(np.max(np.abs(V)))))
    some = bars.copy()
    some[::2] = -np.inf
    rc, idx, gain, _, _, n = host(lib, V, 9, 3, "qei", 0.0, bars=some)
    assert rc == L.OK and idx[0] == 0 and np.isposinf(gain[0])
    rc, idx, gain, _, _, n = host(lib, V, 9, 3, "qpi", -np.inf)  # every row clears every draw: gain 1, then nothing is left to improve
    assert rc == L.OK and n == 1 and idx[0] == 0 and gain[0] == 1.0


def test_every_refusal_of_the_host_call(lib):
    V, inc, bars = random_case(4, 6, 2, seed=10)
    rec = L.GpsoMcAcq(L.MC_QEI, 0.0, inc)
    idx, gain, n = np.zeros(64, dtype=np.int64), np.zeros(64), C.c_int(0)

    def call(rec_p=C.byref(rec), values=L.dptr(V), s=4, m=6, b=2, bars_p=None, q=2, idx_p=L.i64ptr(idx), n_p=C.byref(n)):
        return lib.gpso_paths_batch_host(rec_p, values, s, m, b, bars_p, q, idx_p, L.dptr(gain), None, n_p, None)

    assert call() == L.OK
    for bad in (dict(rec_p=None), dict(values=None), dict(idx_p=None), dict(n_p=None), dict(s=0), dict(s=257), dict(m=0), dict(m=-1),
                dict(q=0), dict(q=65), dict(b=-1), dict(b=65), dict(s=256, m=(1 << 18) - 1, b=2), dict(s=1, m=(1 << 26), b=1)):
        assert call(**bad) == L.E_ARG, bad
    for kind, xi, incumbent in ((2, 0.0, 0.0), (-1, 0.0, 0.0), (L.MC_QEI, np.nan, 0.0), (L.MC_QPI, 0.0, np.nan)):
        assert call(rec_p=C.byref(L.GpsoMcAcq(kind, xi, incumbent))) == L.E_ARG, (kind, xi, incumbent)
    nan_bars = bars.copy()
    nan_bars[3] = np.nan
    assert call(bars_p=L.dptr(nan_bars)) == L.E_ARG
    # what is allowed: a NaN incumbent that is not read, infinite bars, a negative xi
    assert call(rec_p=C.byref(L.GpsoMcAcq(L.MC_QEI, -0.5, np.nan)), bars_p=L.dptr(bars)) == L.OK
    inf_bars = np.array([np.inf, -np.inf, 0.0, 1.0])
    assert call(bars_p=L.dptr(inf_bars)) == L.OK and call(rec_p=C.byref(L.GpsoMcAcq(L.MC_QPI, np.inf, -np.inf))) == L.OK
    assert call(s=256, m=(1 << 18) - 2, b=2, q=1, values=L.dptr(np.zeros((256, 1 << 18)))) == L.OK  # exactly 2^26 cells


def test_the_stand_alone_host_check_builds_and_passes(lib, tmp_path):
    """tools/mcbatch_host_check.cpp -- the program the host sanitizers are run on (its header says how) -- built here by the
    host compiler against the product library, without sanitizers: every check of its own holds."""
    import os
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe, libdir = str(tmp_path / "mcbatch_host_check"), os.path.dirname(L.LIB_PATH)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(root, "tools", "mcbatch_host_check.cpp"),
                    "-I" + os.path.join(root, "include"), "-L" + libdir, "-lgpso_hip", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "mcbatch_host_check: ok\n", (r.returncode, r.stdout, r.stderr)


# ---- 3. the Python surface ---------------------------------------------------------------------------------------------------
def test_the_ctypes_wrapper(lib):
    from pygpso_amd import HipGPEngine

    V, inc, bars = random_case(17, 20, 3, seed=11)
    for kind, kw in (("qei", dict(incumbent=inc)), ("qnei", dict(incumbent_s=bars)), ("qpi", dict(incumbent=inc, xi=0.1))):
        idx, gain, value, gain0 = HipGPEngine.paths_batch_host(V, 5, kind, n_pending=3, **kw)
        raw = host(lib, V, 20, 5, "qpi" if kind == "qpi" else "qei", kw.get("incumbent", 0.0), kw.get("incumbent_s"), kw.get("xi", 0.0))
        assert all(np.array_equal(a, b) for a, b in zip((idx, gain, value, gain0), raw[1:5]))
    with pytest.raises(ValueError):
        HipGPEngine.paths_batch_host(V, 5, "ucb", incumbent=0.0)
    with pytest.raises(ValueError):
        HipGPEngine.paths_batch_host(V, 5, "qei")
    with pytest.raises(ValueError):
        HipGPEngine.paths_batch_host(V, 5, "qnei", incumbent_s=bars[:3])
    with pytest.raises(L.GpsoHipError):
        HipGPEngine.paths_batch_host(V, 65, "qei", incumbent=0.0)


def _stub_engine():
    from pygpso_amd import HipGPEngine
    from tests.test_paths_cpu import PathsEngine

    class McEngine(PathsEngine):
        """``PathsEngine`` with ``paths_best_batch`` answered by the host rounds on the oracle's path values."""

        def paths_best_batch(self, xs, q, kind="qei", incumbent=None, incumbent_s=None, pending=None, xi=0.0, want_gain0=False):
            self.calls.append(("paths_best_batch", kind, None if incumbent_s is None else np.array(incumbent_s), incumbent))
            rows = xs if pending is None else np.vstack([xs, np.atleast_2d(pending)])
            values = self.paths_eval(rows)[0]
            self.calls.pop()
            out = HipGPEngine.paths_batch_host(values, q, kind, incumbent, incumbent_s, rows.shape[0] - xs.shape[0], xi)
            return out if want_gain0 else out[:3]

    return McEngine


def test_select_batch_mc_over_a_stub_engine(lib, monkeypatch):
    from pygpso_amd import GPRSurrogate
    from pygpso_amd import kernels as K

    monkeypatch.setattr(GPRSurrogate, "engine_factory", _stub_engine())
    rng = np.random.default_rng(5)
    coords = rng.random((14, 2))
    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.3, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy())
    surr.append(coords, np.sin(3.0 * coords[:, 0]) + coords[:, 1] ** 2)
    surr.gp_update()
    cand = rng.random((300, 2))
    stored = list(surr.points)
    idx, gain, value = surr.select_batch_mc(cand, 4, n_paths=16, n_features=64, rng=3)
    eng = surr.gpflow_model.engine
    assert eng.paths_info() == (16, 64) and len(set(idx.tolist())) == len(idx) >= 1 and np.all(np.diff(gain) <= 0.0)
    # qnei: the bars are eval_paths' best_val over the evaluated points, and the values stayed on the device
    x_train = surr.current_training_data[0]
    want_bars = eng.paths_eval(x_train, want_values=False)[2][:, 0]
    call = [c for c in eng.calls if c[0] == "paths_best_batch"][-1]
    assert call[1] == "qnei" and np.array_equal(call[2], want_bars) and call[3] is None
    assert ("paths_eval", False) in eng.calls
    # a resident set is kept (no second draw); q = 1 with gain0: the pick is its arg-max
    draws = sum(c[0] == "paths_draw" for c in eng.calls)
    i1, g1, _, gain0 = surr.select_batch_mc(cand, 1, kind="qei", return_gain0=True)
    assert sum(c[0] == "paths_draw" for c in eng.calls) == draws
    assert int(i1[0]) == int(np.argmax(gain0)) and g1[0] == gain0.max() and gain0.shape == (300,)
    call = [c for c in eng.calls if c[0] == "paths_best_batch"][-1]
    assert call[1] == "qei" and call[2] is None and call[3] == float(np.max(surr.current_training_data[1]))
    # pending points are never returned and only lower the gains
    _, _, _, g0p = surr.select_batch_mc(cand, 1, kind="qei", pending=cand[int(i1[0])], return_gain0=True)
    # (the stub's numpy values of a row are not bit-identical from batch to batch as the device's are: rounding, not zero)
    assert np.all(g0p <= gain0 + 1e-12) and g0p[int(i1[0])] <= 1e-12 < gain0[int(i1[0])]
    assert list(surr.points) == stored  # nothing is stored
    with pytest.raises(ValueError):
        surr.select_batch_mc(cand, 2, kind="ucb")


def test_engine_groups_and_served_surrogates_refuse(lib, monkeypatch):
    from pygpso_amd import GPRSurrogate
    from pygpso_amd.model import HipGPR
    from pygpso_amd import kernels as K
    from pygpso_amd.distributed import HipGPEngineGroup
    from tests.helpers import synthetic_problem

    monkeypatch.setattr(GPRSurrogate, "engine_factory", _stub_engine())
    rng = np.random.default_rng(6)
    coords = rng.random((10, 2))
    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.3, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy())
    surr.append(coords, coords.sum(axis=1))
    surr.gp_update()
    surr.gpflow_model.engine = object.__new__(HipGPEngineGroup)
    with pytest.raises(NotImplementedError, match="engine group"):
        surr.select_batch_mc(coords, 2)
    # the model on an engine without the call
    from tests.test_loo_cpu import RecordingEngine

    X, y = synthetic_problem(12, 2, seed=2)
    m = HipGPR(data=(X, y[:, None]), kernel=K.Matern32(lengthscales=0.4, variance=1.0), mean_function=K.Constant(0.0),
               noise_variance=1.0e-2, engine=RecordingEngine())
    with pytest.raises(NotImplementedError, match="mc_batch"):
        m.mc_batch(X, 2, "qei")
    # what a constraint set, a success member or an ensemble does not serve is refused in words
    for kw, word in ((dict(constraints=["c"]), "constraints"), (dict(failures="classify"), "failures"), (dict(hyper="marginal"), "marginal")):
        s2 = object.__new__(GPRSurrogate)
        s2.hyper, s2.constraints, s2.failures = kw.get("hyper", "point"), kw.get("constraints"), kw.get("failures")
        with pytest.raises(ValueError, match=word):
            s2.select_batch_mc(coords, 2)
