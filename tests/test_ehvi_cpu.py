"""CPU-only checks of the bi-objective calls: ``pygpso_amd.pareto`` against brute force, the fold of
csrc/ehvi.hpp through ``gpso_ehvi_fold_host`` against 60 digits and against the independent numpy oracle of
tests/ehvi_oracle.py, its value maps and its logpof to the bit, every refusal of the front validation, and the surrogate's
``pareto_front`` / ``ehvi_select`` over the CPU stand-in engine.

Tolerances.  The EHVI is a sum of P + 1 strip terms (g(a_k) - g(a_{k+1})) e_k; the differences are formed from numbers of
size g(a_k), so the rounding error of the sum scales with B = sum_k g(a_k) e_k, the sum BEFORE the subtraction, not with the
EHVI itself.  Errors are therefore measured as c = |value - truth| / (2^-52 B + 2^-1000), truth and B from mpmath at 60
digits (the floor 2^-1000: below it a double is in or near the subnormal range and carries fewer than 53 bits).
  C_HOST_MEASURED = 5.521   the worst c of gpso_ehvi_fold_host over the full grid (P in {0, 1, 2, 31, 32, 63}, means from 40
                            standard deviations above to 40 below the front, s from 1e-6 to 1e3), measured on the CPU; the
                            test allows twice it
  C_ORACLE_MEASURED = 91.625  the worst c of the numpy oracle itself (plain scipy pdf + z cdf) on the moderate grid
                            (|z| <= 6); host against oracle is allowed 2 C_HOST_MEASURED + 4 C_ORACLE_MEASURED: the two errors
                            add, the oracle's with a margin of four
"""
import warnings

import numpy as np
import pytest

from pygpso_amd import GPRSurrogate, HipGPEngine
from pygpso_amd import _lib as L
from pygpso_amd import acquisition as A
from pygpso_amd import kernels as K
from pygpso_amd import pareto
from pygpso_amd.constraints import Constraint
from tests import ehvi_oracle as eo

C_HOST_MEASURED, C_HOST, C_ORACLE_MEASURED, C_VS_ORACLE = eo.C_HOST_MEASURED, eo.C_HOST, eo.C_ORACLE_MEASURED, eo.C_VS_ORACLE


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fold(front, ref, m1, v1, m2, v2, **kw):
    return HipGPEngine.ehvi_fold_host(front, ref, m1, v1, kw.pop("noise1", 0.0), m2, v2, kw.pop("noise2", 0.0), **kw)


# ---- (a) pareto.py against brute force ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_pareto_front_and_hypervolume_against_brute_force(seed):
    rng = np.random.default_rng([31, seed])
    n = int(rng.integers(1, 40))
    Y = rng.integers(0, 7, size=(n, 2)).astype(np.float64) * 0.5 if seed % 2 == 0 else rng.normal(size=(n, 2))
    if n > 3:
        Y[n // 2] = Y[0]  # a duplicate
        Y[n - 1, 0] = Y[1, 0]  # a tie in one objective
    front, rows = pareto.pareto_front(Y)
    want, want_rows = eo.front_brute(Y)
    assert np.array_equal(front, want) and np.array_equal(rows, want_rows) and np.array_equal(Y[rows], front)
    assert np.all(np.diff(front[:, 0]) > 0) and np.all(np.diff(front[:, 1]) < 0)
    ref = pareto.default_reference(Y)
    assert np.all(ref < Y.min(axis=0))
    for r in (ref, np.array([0.25, 0.25]), Y.max(axis=0) + 1.0):
        hv, brute = pareto.hypervolume_2d(front, r), eo.hypervolume_brute(Y, r)
        assert abs(hv - brute) <= 1e-12 * max(1.0, brute), (hv, brute)
        assert abs(pareto.hypervolume_2d(Y, r) - brute) <= 1e-12 * max(1.0, brute)  # (any point set, not a front alone)


def test_default_reference_and_truncate_front():
    Y = np.array([[1.0, 5.0], [3.0, 5.0], [2.0, 5.0]])
    assert np.array_equal(pareto.default_reference(Y), [1.0 - 0.2, 4.0])  # (a zero range subtracts 1)
    f = eo.make_front(80)
    ref = np.array(eo.REF)
    with pytest.warns(RuntimeWarning, match="upper bound"):
        t = pareto.truncate_front(f, ref)
    assert t.shape == (63, 2) and np.all(np.diff(t[:, 0]) > 0) and np.all(np.diff(t[:, 1]) < 0)
    assert {tuple(r) for r in t} <= {tuple(r) for r in f}
    # the first drop is the point of least exclusive hypervolume; the thinned front dominates less, so the EHVI over it is larger
    first = int(np.argmin(pareto.exclusive_hypervolumes(f, ref)))
    with pytest.warns(RuntimeWarning):
        t79 = pareto.truncate_front(f, ref, 79)
    assert np.array_equal(t79, np.delete(f, first, axis=0))
    excl = pareto.exclusive_hypervolumes(f, ref)
    assert abs(pareto.hypervolume_2d(f, ref) - pareto.hypervolume_2d(t79, ref) - excl[first]) <= 1e-12
    assert pareto.hypervolume_2d(t, ref) < pareto.hypervolume_2d(f, ref)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.array_equal(pareto.truncate_front(f[:63], ref), f[:63])  # (63 points: served as they are, no warning)
    m1, m2 = np.array([0.8, 1.5]), np.array([0.9, 0.2])
    full = eo.ehvi_numpy(f, ref, m1, 0.3, m2, 0.3)
    thin, _ = _fold(t, ref, m1, np.full(2, 0.09), m2, np.full(2, 0.09))
    assert np.all(thin >= full * (1.0 - 1e-9))


# ---- (b) the fold against 60 digits -----------------------------------------------------------------------------------------
def test_decomposition_is_the_expectation_of_the_brute_force_improvement():
    """Monte Carlo over the brute-force hypervolume growth (what the EHVI is the expectation of), within the sampling error."""
    rng = np.random.default_rng(5)
    f, ref = eo.make_front(5), eo.REF
    for m1, s1, m2, s2 in ((1.0, 0.5, 0.8, 0.4), (0.2, 0.3, 1.2, 0.2), (2.2, 0.1, 0.1, 0.6)):
        Y = np.column_stack([rng.normal(m1, s1, 1500), rng.normal(m2, s2, 1500)])
        draws = np.array([eo.hvi_brute(y, f, ref) for y in Y])
        v, _ = _fold(f, ref, [m1], [s1 * s1], [m2], [s2 * s2])
        assert abs(v[0] - draws.mean()) <= 5.0 * draws.std() / np.sqrt(len(draws)), (v[0], draws.mean())


@pytest.mark.parametrize("p", eo.GRID_P)
def test_host_fold_against_60_digits_on_the_grid(p):
    front, (m1, v1, m2, v2) = eo.grid(p)
    value, logpof = _fold(front, eo.REF, m1, v1, m2, v2)
    assert np.all(value >= 0.0) and np.all(np.isfinite(value)) and np.array_equal(_bits(logpof), _bits(np.zeros_like(logpof)))
    c = eo.worst_c(value, eo.grid_truth(p))
    print(f"EHVI_ACCURACY P={p}: worst c {c:.3f} over {len(m1)} leaves (measured {C_HOST_MEASURED}, allowed {C_HOST:.3f})")
    assert c <= C_HOST, (p, c)
    # the latent switch is the subtraction of each model's own noise variance, and nothing else
    lat, _ = HipGPEngine.ehvi_fold_host(front, eo.REF, m1, v1 + 0.25, 0.25, m2, v2 + 0.5, 0.5, latent=True)
    pred, _ = HipGPEngine.ehvi_fold_host(front, eo.REF, m1, v1, 0.25, m2, v2, 0.5, latent=False)
    exact = ((v1 + 0.25) - 0.25 == v1) & ((v2 + 0.5) - 0.5 == v2)
    assert np.array_equal(_bits(pred), _bits(value)) and np.array_equal(_bits(lat[exact]), _bits(value[exact])) and exact.any()


def test_exact_results_at_s_zero_nan_and_infinite_means():
    front, ref = eo.make_front(4), (0.0, 0.0)
    a, b = front[:, 0], front[:, 1]
    # s = 0 on both objectives: the hypervolume growth of the outcome itself, max(mu - x, 0) strips
    pts = np.array([[a[1] + 0.1, b[1] + 0.05], [a[3] + 1.0, b[0] + 1.0], [a[0] - 0.01, b[3] - 0.01], [-1.0, 5.0], [a[2], b[2]]])
    v, lp = _fold(front, ref, pts[:, 0], np.zeros(5), pts[:, 1], np.zeros(5))
    want = np.array([eo.hvi_brute(y, front, ref) for y in pts])
    assert np.allclose(v, want, rtol=1e-14, atol=1e-15) and v[2] == 0.0 and v[3] == 0.0 and v[4] == 0.0
    # a variance at or below the noise is s = 0 under latent=True; a negative predictive variance is clamped too
    v2, _ = HipGPEngine.ehvi_fold_host(front, ref, pts[:, 0], np.full(5, 1e-3), 1e-3, pts[:, 1], np.full(5, 5e-4), 1e-3, latent=True)
    v3, _ = HipGPEngine.ehvi_fold_host(front, ref, pts[:, 0], np.full(5, -1e-3), 0.0, pts[:, 1], np.full(5, -0.0), 0.0, latent=False)
    assert np.array_equal(_bits(v2), _bits(v)) and np.array_equal(_bits(v3), _bits(v))
    # s = 0 on one objective alone: g exact, e a plain expectation
    v4, _ = _fold(front, ref, [a[1] + 0.1], [0.0], [0.7], [0.04])
    want4 = eo.ehvi_numpy(front, ref, np.array([a[1] + 0.1]), np.array([0.0]), np.array([0.7]), np.array([0.2]))
    assert abs(v4[0] - want4[0]) <= 1e-13 * want4[0]
    # NaN in: NaN out, whichever entry; -inf mean: +0.0; +inf mean: +inf (a -inf beside it: 0)
    nan, inf = np.nan, np.inf
    for k in range(4):
        cols = [np.array([1.0]), np.array([0.1]), np.array([1.0]), np.array([0.1])]
        cols[k] = np.array([nan])
        assert np.isnan(_fold(front, ref, *cols)[0][0]), k
    v5, _ = _fold(front, ref, [-inf, 1.0, inf, 1.0, inf, -inf], np.full(6, 0.1), [1.0, -inf, 1.0, inf, -inf, inf], np.full(6, 0.1))
    assert np.array_equal(_bits(v5), _bits(np.array([0.0, 0.0, inf, inf, 0.0, 0.0])))
    # far behind the front float64 EHVI is exactly 0 (the tie the header speaks of); far ahead it is the area itself
    v6, _ = _fold(front, ref, [-50.0, 60.0], [1.0, 1.0], [-50.0, 60.0], [1.0, 1.0])
    assert v6[0] == 0.0 and abs(v6[1] - (3600.0 - pareto.hypervolume_2d(front, ref))) <= 1e-12 * 3600.0


# ---- (c) the independent oracle against the host entry ---------------------------------------------------------------------
@pytest.mark.parametrize("p", eo.GRID_P)
def test_numpy_oracle_against_the_host_fold_on_moderate_inputs(p):
    front, (m1, v1, m2, v2) = eo.grid(p, moderate=True)
    truth = eo.grid_truth(p, moderate=True)
    oracle = eo.ehvi_numpy(front, eo.REF, m1, np.sqrt(v1), m2, np.sqrt(v2))
    c_oracle = eo.worst_c(oracle, truth)
    value, _ = _fold(front, eo.REF, m1, v1, m2, v2)
    scale = eo.scale_numpy(front, eo.REF, m1, np.sqrt(v1), m2, np.sqrt(v2))
    c_pair = float(np.max(np.abs(value - oracle) / (eo.ULP * scale)))
    print(f"EHVI_ORACLE P={p}: oracle's own worst c {c_oracle:.3f} (measured {C_ORACLE_MEASURED}), host against oracle {c_pair:.3f} "
          f"(allowed {C_VS_ORACLE:.1f})")
    assert c_oracle <= 2.0 * C_ORACLE_MEASURED and c_pair <= C_VS_ORACLE, (p, c_oracle, c_pair)


# ---- (d) the value maps, the skipped member and the success term ------------------------------------------------------------
def _columns(m=40, k=3, seed=2):
    rng = np.random.default_rng([41, seed])
    front = eo.make_front(7)
    m1, m2 = rng.uniform(-0.5, 2.5, m), rng.uniform(-0.5, 2.0, m)
    v1, v2 = rng.uniform(0.01, 0.5, m), rng.uniform(0.01, 0.5, m)
    om, ov = rng.normal(size=(k, m)), rng.uniform(0.05, 1.0, (k, m))
    onoise, thr, sense = rng.uniform(1e-3, 1e-2, k), rng.normal(size=k) * 0.3, np.array([1, -1, 1][:k])
    sm, sv = rng.normal(size=m) + 0.5, rng.uniform(0.1, 2.0, m)
    return front, m1, v1, m2, v2, om, ov, onoise, thr, sense, sm, sv


def test_logpof_is_the_constrained_fold_without_objective_two_to_the_bit():
    front, m1, v1, m2, v2, om, ov, onoise, thr, sense, sm, sv = _columns()
    ei = A.EI(xi=0.0)
    # with a success member: gpso_constrained_success_fold_host on the same columns, objective 2 removed (k = 3, 1, 0)
    for k in (3, 1, 0):
        _, lp = _fold(front, eo.REF, m1, v1, m2, v2, other_mean=om[:k] if k else None, other_var=ov[:k] if k else None,
                      other_noise=onoise[:k], threshold=thr[:k], sense=sense[:k], success_mean=sm, success_var=sv)
        _, want = HipGPEngine.constrained_success_fold_host(ei, m1, v1, 0.0, om[:k] if k else None, ov[:k] if k else None, onoise[:k], thr[:k],
                                                            sense[:k], sm, sv, "gate", -np.inf, incumbent=0.0)
        assert np.array_equal(_bits(lp), _bits(want)), k
    # without one: gpso_constrained_fold_host; the order of the members matters to the last bit and is kept
    _, lp = _fold(front, eo.REF, m1, v1, m2, v2, other_mean=om, other_var=ov, other_noise=onoise, threshold=thr, sense=sense)
    _, want = HipGPEngine.constrained_fold_host(ei, m1, v1, 0.0, om, ov, onoise, thr, sense, "gate", -np.inf, incumbent=0.0)
    assert np.array_equal(_bits(lp), _bits(want))
    # no other member and no success member: +0.0
    _, lp0 = _fold(front, eo.REF, m1, v1, m2, v2)
    assert np.array_equal(_bits(lp0), _bits(np.zeros_like(m1)))
    # a NaN member column: a NaN logpof, and a NaN value in every mode but the open gate
    om2 = om.copy()
    om2[1, 3] = np.nan
    for mode, lpm, is_nan in (("weight", -np.inf, True), ("gate", np.log(0.5), True), ("gate", -np.inf, False)):
        v, lp = _fold(front, eo.REF, m1, v1, m2, v2, other_mean=om2, other_var=ov, other_noise=onoise, threshold=thr, sense=sense, mode=mode,
                      log_pof_min=lpm)
        assert np.isnan(lp[3]) and np.isnan(v[3]) == is_nan, mode


def test_weight_and_gate_maps():
    front, m1, v1, m2, v2, om, ov, onoise, thr, sense, sm, sv = _columns()
    kw = dict(other_mean=om, other_var=ov, other_noise=onoise, threshold=thr, sense=sense, success_mean=sm, success_var=sv)
    ehvi, lp = _fold(front, eo.REF, m1, v1, m2, v2, **kw)  # (no cspec: value = EHVI, logpof still reported)
    plain, _ = _fold(front, eo.REF, m1, v1, m2, v2)
    assert np.array_equal(_bits(ehvi), _bits(plain)) and np.all(lp < 0.0)
    gate = float(np.median(lp))
    g, lpg = _fold(front, eo.REF, m1, v1, m2, v2, mode="gate", log_pof_min=gate, **kw)
    keep = lp >= gate
    assert keep.any() and (~keep).any() and np.array_equal(_bits(lpg), _bits(lp))
    assert np.array_equal(_bits(g[keep]), _bits(ehvi[keep])) and np.all(np.isneginf(g[~keep]))
    g_open, _ = _fold(front, eo.REF, m1, v1, m2, v2, mode="gate", **kw)
    assert np.array_equal(_bits(g_open), _bits(ehvi))
    w, _ = _fold(front, eo.REF, m1, v1, m2, v2, mode="weight", log_pof_min=gate, **kw)
    expl = HipGPEngine.acq_math_host("exp", lp)  # (the library's written-out exp: the product has its bits)
    assert np.all(np.isneginf(w[~keep])) and np.array_equal(_bits(w[keep]), _bits(ehvi[keep] * expl[keep]))
    assert np.allclose(w[keep], eo.value_numpy(ehvi, lp, "weight", gate)[keep], rtol=1e-15)
    # every other member's column set so that logpof = 0 (s2 = 0 on the feasible side): the value has the EHVI's bits
    easy = dict(other_mean=np.zeros((2, len(m1))), other_var=np.zeros((2, len(m1))), other_noise=[0.0, 0.0], threshold=[1.0, -1.0], sense=[1, -1])
    for mode in ("weight", "gate"):
        v, lp0 = _fold(front, eo.REF, m1, v1, m2, v2, mode=mode, log_pof_min=np.log(0.5), **easy)
        assert np.array_equal(_bits(lp0), _bits(np.zeros_like(m1))) and np.array_equal(_bits(v), _bits(ehvi)), mode
    # against the independent oracle, values and logpof
    o_lp = eo.logpof_numpy(om, ov, onoise, thr, sense, sm, sv)
    assert np.allclose(lp, o_lp, rtol=1e-12)
    o = eo.ehvi_numpy(front, eo.REF, m1, np.sqrt(v1), m2, np.sqrt(v2))
    scale = eo.scale_numpy(front, eo.REF, m1, np.sqrt(v1), m2, np.sqrt(v2))
    assert np.all(np.abs(ehvi - o) <= C_VS_ORACLE * eo.ULP * scale)


# ---- (e) the refusals of the host entry ---------------------------------------------------------------------------------------
def test_every_front_refusal_of_the_host_entry():
    ok = eo.make_front(3)
    one = (np.array([1.0]), np.array([0.1]), np.array([1.0]), np.array([0.1]))
    assert _fold(ok, eo.REF, *one)[0].shape == (1,)
    bad_fronts = {
        "64 points": (eo.make_front(64), eo.REF),
        "NaN entry": (np.array([[0.5, np.nan]]), eo.REF),
        "infinite entry": (np.array([[np.inf, 0.5]]), eo.REF),
        "NaN reference": (ok, (np.nan, 0.0)),
        "infinite reference": (ok, (0.0, -np.inf)),
        "a not ascending": (ok[::-1], eo.REF),
        "a tied": (np.array([[0.5, 1.0], [0.5, 0.5]]), eo.REF),
        "b not descending": (np.array([[0.5, 0.5], [1.0, 1.0]]), eo.REF),
        "b tied": (np.array([[0.5, 0.5], [1.0, 0.5]]), eo.REF),
        "point on the reference in f1": (np.array([[0.0, 0.5]]), eo.REF),
        "point below the reference in f2": (ok, (0.0, float(ok[-1, 1]))),
    }
    for name, (front, ref) in bad_fronts.items():
        with pytest.raises(L.GpsoHipError) as err:
            _fold(front, ref, *one)
        assert err.value.code == L.E_ARG, name
    # p > 0 with a NULL front, a negative p: through the raw entry
    import ctypes as C

    lib = L.load()
    val = np.zeros(1)
    args = [L.dptr(a) for a in one]

    def raw(rec, cs=None):
        return lib.gpso_ehvi_fold_host(C.byref(rec), None if cs is None else C.byref(cs), args[0], args[1], 0.0, args[2], args[3], 0.0, None, None,
                                       None, None, None, 0, 1, None, None, L.dptr(val), None)

    ref2 = (C.c_double * 2)(0.0, 0.0)
    assert raw(L.GpsoEhvi(0, 1, 0, None, ref2)) == L.OK  # (P = 0 is served, with a NULL front)
    assert raw(L.GpsoEhvi(99, 1, 0, None, ref2)) == L.OK  # (member is ignored by the host entry)
    assert raw(L.GpsoEhvi(0, 1, 2, None, ref2)) == L.E_ARG and raw(L.GpsoEhvi(0, 1, -1, None, ref2)) == L.E_ARG
    # the cspec: feasibility mode is the constrained calls', an unknown mode and a bad log_pof_min are refused
    for cs in (L.GpsoCspec(L.CON_FEASIBILITY, -np.inf), L.GpsoCspec(7, -np.inf), L.GpsoCspec(L.CON_GATE, 0.5), L.GpsoCspec(L.CON_WEIGHT, np.nan)):
        assert raw(L.GpsoEhvi(0, 1, 0, None, ref2), cs) == L.E_ARG
    assert raw(L.GpsoEhvi(0, 1, 0, None, ref2), L.GpsoCspec(L.CON_WEIGHT, -np.inf)) == L.OK
    # the columns: 16 other members is one too many (the set holds 16, one of them is objective 2); a success mean without its variance
    with pytest.raises(L.GpsoHipError):
        _fold(ok, eo.REF, *one, other_mean=np.zeros((16, 1)), other_var=np.ones((16, 1)), other_noise=np.zeros(16), threshold=np.zeros(16),
              sense=np.ones(16, dtype=int))
    with pytest.raises(L.GpsoHipError):
        _fold(ok, eo.REF, *one, success_mean=[0.0])


# ---- (f) the surrogate over the CPU stand-in engine -------------------------------------------------------------------------
@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(GPRSurrogate, "engine_factory", eo.EhviOracleEngine)


def _surrogate(cons, **kw):
    return GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy(), constraints=cons,
                        **kw)


def _toy(x):
    """Two outputs in conflict over the unit square, and a third that bounds the first coordinate."""
    x = np.atleast_2d(x)
    return -np.sum((x - 0.25) ** 2, axis=1), -np.sum((x - 0.75) ** 2, axis=1), x[:, 0]


def test_surrogate_pareto_front_and_ehvi_select_on_the_stand_in(stand_in):
    cons = [Constraint("cap", upper=0.9), Constraint("f2", lower=-0.6)]
    surr = _surrogate(cons)
    rng = np.random.default_rng(9)
    x = rng.uniform(0.0, 1.0, (14, 2))
    f1, f2, cap = _toy(x)
    leaves = rng.uniform(0.0, 1.0, (60, 2))
    with pytest.raises(ValueError, match="no constraint models"):
        surr.ehvi_select(leaves, "f2")  # no model yet
    surr.append(x, f1, constraint_values=np.column_stack([cap, f2]))
    # the refusals that need no model
    with pytest.raises(ValueError, match="lower="):
        surr.pareto_front("cap")
    with pytest.raises(ValueError, match="no constraint named"):
        surr.pareto_front("nope")
    with pytest.raises(ValueError):
        surr.pareto_front(2)
    # the default reference: default_reference of the scores, and the constraint's own bound
    xt, yt = surr.current_training_data
    r1 = pareto.default_reference(np.asarray(yt).reshape(-1, 1))[0]
    assert np.array_equal(surr._ehvi_reference(1, np.asarray(yt), None), [r1, -0.6])
    assert np.array_equal(surr._ehvi_reference(1, np.asarray(yt), (None, -2.0)), [r1, -2.0])
    coords, front = surr.pareto_front("f2")
    ct = surr.current_training_constraints
    ok = (ct[:, 0] <= 0.9) & (np.asarray(yt) > r1) & (ct[:, 1] > -0.6)
    want, rows = eo.front_brute(np.column_stack([np.asarray(yt), ct[:, 1]])[ok])
    assert front.shape[0] >= 2 and np.array_equal(front, want) and np.array_equal(coords, np.asarray(xt)[np.flatnonzero(ok)[rows]])
    assert np.array_equal(surr.pareto_front(1)[1], front)  # (by index)
    # a point that breaks the OTHER bound leaves the front; one at the reference does not count (strictly above)
    tight = surr.pareto_front("f2", ref=(float(front[0, 0]), None))[1]
    assert tight.shape[0] == front.shape[0] - 1
    with pytest.raises(ValueError, match="no constraint models"):
        surr.ehvi_select(leaves, "f2")  # data, but no gp_update yet
    surr.gp_update()
    with pytest.raises(ValueError, match="lower="):
        surr.ehvi_select(leaves, "cap")
    with pytest.raises(ValueError, match="mode"):
        surr.ehvi_select(leaves, "f2", mode="feasibility")
    n_points = len(surr.points)
    idx, value, logpof, mean, var = surr.ehvi_select(leaves, "f2", mode=None)
    assert len(surr.points) == n_points and idx.shape == (1,) and mean.shape == (2, 1) and value[0] > 0.0 and logpof[0] <= 0.0
    # ... the stand-in's columns through the library's fold: the arg-max of the values it reports
    vals = surr.gpflow_model.ehvi_values(leaves, 1, front, [r1, -0.6])[0]
    assert int(idx[0]) == int(np.argmax(vals)) and value[0] == vals.max()
    # weight mode ranks by EHVI x P(cap <= 0.9): never above the plain EHVI of the same leaf
    iw, vw, lw, _, _ = surr.ehvi_select(leaves, "f2", mode="weight", seg_off=[0, 30, 60])
    assert iw.shape == (2,) and np.all(vw <= vals[np.array([0, 30]) + iw] * (1 + 1e-15))
    # an engine group is refused in words (the stand-in's own class plays the group)
    import pygpso_amd.distributed as dist

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(dist, "HipGPEngineGroup", type(surr.gpflow_model.engine))
        with pytest.raises(NotImplementedError, match="engine group"):
            surr.ehvi_select(leaves, "f2")
    assert surr.ehvi_select(leaves, "f2", mode=None)[0][0] == idx[0]  # (and served again once it is no group)
    # weight mode keeps the surrogate's gate as well: a leaf whose P(feasible) is below pof_min is worth -inf in both modes
    lp_all = surr.gpflow_model.ehvi_values(leaves, 1, front, [r1, -0.6])[1]
    surr.pof_min = float(np.exp(np.median(lp_all)))
    for mode in ("weight", "gate"):
        iw, vw, lw, _, _ = surr.ehvi_select(leaves, "f2", mode=mode)
        assert lw[0] >= np.log(surr.pof_min) and np.isfinite(vw[0]), mode
        from pygpso_amd.constraints import ConstrainedAcq

        gated = surr.gpflow_model.ehvi_values(leaves, 1, front, [r1, -0.6], cspec=ConstrainedAcq(None, mode, surr.pof_min))[0]
        assert np.array_equal(np.isneginf(gated), lp_all < np.log(surr.pof_min)) and np.isneginf(gated).any(), mode
    surr.close_constraint_models()
