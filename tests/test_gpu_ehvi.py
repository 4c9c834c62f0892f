"""
Bi-objective search on the device: ``gpso_ehvi_values`` / ``gpso_best_ehvi`` -- the exact EHVI of the
pair (objective, one member of the constraint set) over a given front, weighted or gated by the logpof of the remaining members
and of the success member -- against the library's own host fold (bit for bit), the constrained calls' columns (bit for bit),
and the independent numpy oracle of tests/ehvi_oracle.py.

Shapes: N = 20, D = 2; Matern-5/2 on a float64 context and the squared exponential on a "mixed" one; three sets -- "alone"
(J = 1: objective 2 is the set), "middle" (J = 3, objective 2 at index 1: a skip in the middle) and "success" (J = 2 plus a
success member, set up as tests/test_gpu_failures.py does); M in {1, 5, 162} (one leaf, a partly filled block of four, the
loop's size -- the 5 and the 1 are rows of the 162, so a leaf meets three batches and three slots); P in {0, 1, 31, 32, 63}.
The models are fitted at given hyper-parameters, as tests/test_gpu_constraints.py does; the fronts are synthetic, scaled into
the range of the oracle's leaf means so that leaves lie ahead of, on and behind them.  Every case is built once and shared.

Tolerances.  Device against the host fold: bits.  Device against the numpy oracle: tests/ehvi_oracle.py's C_VS_ORACLE (the
host's measured worst c twice, plus the oracle's own four times) in units of 2^-52 B, B = sum_k g(a_k) e_k -- on the DEVICE's
columns for every leaf whose strips all have |z| <= 6 (the range the oracle's error was measured in); on the ORACLE's columns
the same plus what the columns' own tolerance (1e-9 of max(1, |targets|) on a mean, of the kernel variance on a
variance) can move an EHVI: it is Lipschitz in mu_1 with constant e_P = E[(Y_2 - r_2)+], in mu_2 with g(r_1), and in s_i with
0.4 times those (|dE[(Y - x)+]/ds| = phi <= 0.4), s moving by dvar / (2 s).  That last term grows without limit as s -> 0: it is
applied to moderate leaves with s > 0 on both objectives only (s = 0 is an infinite z, so no moderate leaf has it; the mask
states s > 0 explicitly as well), and the share of such leaves is asserted.
"""
import numpy as np
import pytest

from oracle import gpr
from tests import ehvi_oracle as eo
from tests import vgp_bernoulli_oracle as B
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

C_VS_ORACLE = eo.C_VS_ORACLE

N, D = 20, 2
MS = (1, 5, 162)
PS = (0, 1, 31, 32, 63)
SUB5 = np.array([7, 3, 100, 161, 50])  # the rows of the 162 that make the batch of 5; the batch of 1 is row 100
SUB1 = np.array([100])
CONFIGS = {"m52_f64": ("Matern52", "float64"), "se_mixed": ("SquaredExponential", "mixed")}
SETS = {"alone": (1, 0, False), "middle": (3, 1, False), "success": (2, 1, True)}  # J, objective 2's index, success member
CASES = [(cfg, st) for cfg in CONFIGS for st in SETS]
N_CLS, CLS_KERNEL = 30, "SquaredExponential"
_BUILT, _PROBLEMS = {}, {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _rows(m):
    return {1: SUB1, 5: SUB5, 162: np.arange(162)}[m]


def _segments(m):
    """Three segments, the middle one empty."""
    return np.array({1: [0, 1, 1, 1], 5: [0, 2, 2, 5], 162: [0, 60, 60, 162]}[m], dtype=np.int64)


def _classifier_posterior():
    X, y, u, n_ls = B.case_problem(N_CLS, D, CLS_KERNEL, True)
    mu, S = np.zeros(N_CLS), np.eye(N_CLS)
    for gamma, shift in B.STEPS:
        mu, S = B.natgrad(CLS_KERNEL, u + shift, n_ls, True, 0.0, X, y, mu, S, gamma)
    return X, y, u + B.STEPS[-1][1], n_ls, mu, S


def problem(cfg, st):
    """The inputs of a case and what the oracle says of them: no GPU."""
    if (cfg, st) in _PROBLEMS:
        return _PROBLEMS[cfg, st]
    kernel, dtype = CONFIGS[cfg]
    j, member, suc = SETS[st]
    X, y = synthetic_problem(N, D, seed=3)
    leaves = synthetic_leaves(162, D, seed=4)
    rng = np.random.default_rng([8, j, len(kernel)])
    w, ph = rng.normal(size=(j, D)), rng.uniform(0.0, 2.0 * np.pi, j)
    cY = np.array([np.sin(2.0 * X @ w[i] + ph[i]) + 0.25 * np.cos(3.0 * X[:, 0] + i) for i in range(j)])
    th_obj = gpr.Theta(kernel, 0.22, 1.2, 2e-3, float(y.mean()))
    thetas = [gpr.Theta(kernel, 0.2 + 0.03 * i, 1.0 + 0.2 * i, 1e-3 * (i + 1), float(cY[i].mean())) for i in range(j)]
    o_obj = gpr.predict_y(gpr.posterior(th_obj, X, y), leaves)
    cols = [gpr.predict_y(gpr.posterior(th, X, cY[i]), leaves) for i, th in enumerate(thetas)]
    om, ov = np.array([c[0] for c in cols]), np.array([c[1] for c in cols])
    sense = np.array([1 if i % 2 == 0 else -1 for i in range(j)], dtype=np.int64)
    sense[member] = -1  # objective 2 is a lower= constraint
    thr = np.median(om, axis=1)
    # the reference point below the leaves' means, the fronts scaled into their range
    lo = np.array([o_obj[0].min(), om[member].min()])
    hi = np.array([o_obj[0].max(), om[member].max()])
    ref = lo - 0.1 * (hi - lo)
    thr[member] = ref[1]
    fronts = {p: ref + eo.make_front(p) * ((hi - ref) / np.array([2.0, 1.5])) for p in PS}
    for f in fronts.values():
        assert np.all(np.diff(f[:, 0]) > 0) and np.all(np.diff(f[:, 1]) < 0) and np.all(f > ref)
    noise = np.array([th.noise for th in thetas])
    others = [i for i in range(j) if i != member]
    o_suc = None
    if suc:
        Xc, yc, uu, n_ls, mu, S = _classifier_posterior()
        o_suc = B.Posterior(CLS_KERNEL, uu, n_ls, True, 0.0, Xc, mu, S).predict_f(leaves)
    o_lp = eo.logpof_numpy(om[others] if others else None, ov[others] if others else None, noise[others], thr[others], sense[others],
                           None if o_suc is None else o_suc[0], None if o_suc is None else o_suc[1], m=162)
    s1, s2 = eo.sigmas(o_obj[1], th_obj.noise, ov[member], noise[member])
    c = dict(cfg=cfg, st=st, kernel=kernel, dtype=dtype, j=j, member=member, suc=suc, X=X, y=y, leaves=leaves, cY=cY, th_obj=th_obj,
             thetas=thetas, o_obj=o_obj, o_mean=om, o_var=ov, thr=thr, sense=sense, noise=noise, others=others, ref=ref, fronts=fronts,
             o_suc=o_suc, o_logpof=o_lp, o_s=(s1, s2), gate=float(np.median(o_lp)) if (others or suc) else -np.inf)
    _PROBLEMS[cfg, st] = c
    return c


def moderate(c, p, mean1, s1, mean2, s2):
    """[m] bool: the leaves all of whose strips have |z| <= 6 on both objectives."""
    f, ref = c["fronts"][p], c["ref"]
    a, h = np.concatenate([[ref[0]], f[:, 0]]), np.concatenate([f[:, 1], [ref[1]]])
    with np.errstate(divide="ignore"):
        z1 = np.abs(mean1[:, None] - a[None]) / s1[:, None]
        z2 = np.abs(mean2[:, None] - h[None]) / s2[:, None]
    return (z1.max(axis=1) <= 6.0) & (z2.max(axis=1) <= 6.0)


def _fit(eng, th):
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)


def built(cfg, st):
    """The case's engine with its set installed and the device's outputs: made once, shared, read-only."""
    if (cfg, st) in _BUILT:
        return _BUILT[cfg, st]
    from pygpso_amd import HipGPEngine
    from pygpso_amd import acquisition as A

    c = dict(problem(cfg, st))
    eng, src = HipGPEngine(c["dtype"]), HipGPEngine("float64")
    for i, th in enumerate(c["thetas"]):
        src.set_data(c["X"], c["cY"][i])
        _fit(src, th)
        assert eng.constraint_push(src, c["thr"][i], int(c["sense"][i])) == i
    src.close()
    if c["suc"]:
        Xc, yc, uu, n_ls, mu, S = _classifier_posterior()
        cls = HipGPEngine("float64")
        cls.set_data(Xc, yc)
        cls.vgp_set_likelihood("Bernoulli", 0.0, B.N_GH)
        cls.vgp_set_q(mu, S)
        cls.vgp_posterior(CLS_KERNEL, uu, n_ls, True, 0.0)
        eng.success_push(cls)
        cls.close()
    eng.set_data(c["X"], c["y"])
    _fit(eng, c["th_obj"])
    c.update(eng=eng, hash=eng.posterior_hash(), info=eng.constraint_info(), held=eng.last_count(4))
    ei = A.EI(xi=0.0)
    c["con"] = {m: eng.constrained_acq_values(c["leaves"][_rows(m)], ei, "gate", -np.inf, incumbent=0.0, want_members=True) for m in MS}
    c["con_best"] = eng.constrained_best_acq(c["leaves"], ei, "weight", c["gate"], _segments(162), incumbent=0.0)
    c["dev"] = {}
    for m in MS:
        for p in PS:
            for mode in (None, "weight", "gate"):
                c["dev"][m, p, mode] = eng.ehvi_values(c["leaves"][_rows(m)], c["member"], c["fronts"][p], c["ref"], True, mode, c["gate"])
    for a in (c["X"], c["y"], c["leaves"]):
        a.setflags(write=False)
    _BUILT[cfg, st] = c
    return c


def _host(c, m, p, mode, mean, var, latent=True):
    """The library's host fold on the DEVICE's columns of the batch of m."""
    from pygpso_amd import HipGPEngine

    mm, mv = c["con"][m][4], c["con"][m][5]
    o, j = c["others"], c["j"]
    return HipGPEngine.ehvi_fold_host(c["fronts"][p], c["ref"], mean[0], var[0], c["th_obj"].noise, mean[1], var[1], c["noise"][c["member"]],
                                      mm[o] if o else None, mv[o] if o else None, c["noise"][o], c["thr"][o], c["sense"][o],
                                      mm[j] if c["suc"] else None, mv[j] if c["suc"] else None, latent=latent, mode=mode,
                                      log_pof_min=c["gate"])


@pytest.mark.parametrize("cfg,st", CASES)
def test_fronts_and_gates_are_not_vacuous_under_the_oracle(cfg, st):
    """From the oracle alone (no GPU needed for the claim): leaves lie ahead of and behind every front, at least a fifth of them has
    moderate strips (|z| <= 6), the EHVI is positive and varies over the leaves, and both sides of the gate are populated."""
    c = problem(cfg, st)
    m1, m2 = c["o_obj"][0], c["o_mean"][c["member"]]
    s1, s2 = c["o_s"]
    for p in PS:
        f = c["fronts"][p]
        if p:
            dominated = np.array([np.any((f[:, 0] >= a) & (f[:, 1] >= b)) for a, b in zip(m1, m2)])
            assert dominated.any() and (~dominated).any(), p
        mod = moderate(c, p, m1, s1, m2, s2)
        assert mod.mean() >= 0.2, (p, mod.mean())
        e = eo.ehvi_numpy(f, c["ref"], m1, s1, m2, s2)
        assert np.all(e > 0.0) and e.max() / e.min() > 3.0, (p, e.min(), e.max())
    if c["others"] or c["suc"]:
        assert np.mean(c["o_logpof"] >= c["gate"]) >= 0.25 and np.mean(c["o_logpof"] < c["gate"]) >= 0.25


@pytest.mark.parametrize("cfg,st", CASES)
def test_device_fold_is_the_host_fold_of_the_devices_own_columns(cfg, st):
    c = built(cfg, st)
    for (m, p, mode), (value, logpof, mean, var) in c["dev"].items():
        h_val, h_lp = _host(c, m, p, mode, mean, var)
        assert np.array_equal(_bits(logpof), _bits(h_lp)), (m, p, mode)
        assert np.array_equal(_bits(value), _bits(h_val)), (m, p, mode)
        if mode is None:
            assert np.all(value > 0.0) and np.all(np.isfinite(value))
        if mode == "gate" and np.isfinite(c["gate"]):
            assert np.array_equal(np.isneginf(value), ~(logpof >= c["gate"])), (m, p)
            keep = logpof >= c["gate"]
            assert np.array_equal(_bits(value[keep]), _bits(c["dev"][m, p, None][0][keep]))  # the EHVI's own bits behind the gate
        if not c["others"] and not c["suc"]:
            assert np.array_equal(_bits(logpof), _bits(np.zeros(m)))  # no term at all: +0.0
    # the predictive variance (latent = 0) is another value, and the host's too
    m, p = 162, 31
    val, lp, mean, var = c["eng"].ehvi_values(c["leaves"], c["member"], c["fronts"][p], c["ref"], False, None)
    assert np.array_equal(_bits(val), _bits(_host(c, m, p, None, mean, var, latent=False)[0]))
    assert not np.array_equal(_bits(val), _bits(c["dev"][m, p, None][0]))


@pytest.mark.parametrize("cfg,st", CASES)
def test_columns_are_the_constrained_calls_columns(cfg, st):
    c = built(cfg, st)
    for (m, p, mode), (value, logpof, mean, var) in c["dev"].items():
        cm, cv, _, clp, mm, mv = c["con"][m]
        assert mean.shape == (2, m) and var.shape == (2, m)
        assert np.array_equal(_bits(mean[0]), _bits(cm)) and np.array_equal(_bits(var[0]), _bits(cv)), (m, p, mode)
        assert np.array_equal(_bits(mean[1]), _bits(mm[c["member"]])) and np.array_equal(_bits(var[1]), _bits(mv[c["member"]])), (m, p, mode)
    # against the oracle's columns: DESIGN.md 2.1's float64 row
    value, logpof, mean, var = c["dev"][162, 31, None]
    for k, (got_m, got_v, want, targets, variance) in enumerate(((mean[0], var[0], c["o_obj"], c["y"], c["th_obj"].variance),
                                                                 (mean[1], var[1], (c["o_mean"][c["member"]], c["o_var"][c["member"]]),
                                                                  c["cY"][c["member"]], c["thetas"][c["member"]].variance))):
        assert np.max(np.abs(got_m - want[0])) <= 1e-9 * max(1.0, float(np.max(np.abs(targets)))), k
        assert np.max(np.abs(got_v - want[1])) <= 1e-9 * variance, k


@pytest.mark.parametrize("cfg,st", CASES)
def test_same_call_twice_and_a_leaf_in_another_batch_give_the_same_bits(cfg, st):
    c = built(cfg, st)
    eng = c["eng"]
    for p, mode in ((63, "weight"), (0, None)):
        again = eng.ehvi_values(c["leaves"], c["member"], c["fronts"][p], c["ref"], True, mode, c["gate"])
        for a, b in zip(again, c["dev"][162, p, mode]):
            assert np.array_equal(_bits(a), _bits(b)), (p, mode)
    # a leaf's bits do not change with its position in the batch or with the batch around it
    for p in PS:
        for mode in (None, "weight", "gate"):
            full = c["dev"][162, p, mode]
            for m in (1, 5):
                part = c["dev"][m, p, mode]
                for a, b in zip(part, full):
                    assert np.array_equal(_bits(a), _bits(b[..., _rows(m)])), (p, mode, m)
    # ... nor with the rows in another order
    perm = np.random.default_rng(1).permutation(162)
    val, lp, mean, var = eng.ehvi_values(c["leaves"][perm], c["member"], c["fronts"][32], c["ref"], True, "weight", c["gate"])
    full = c["dev"][162, 32, "weight"]
    assert np.array_equal(_bits(val), _bits(full[0][perm])) and np.array_equal(_bits(lp), _bits(full[1][perm]))


@pytest.mark.parametrize("cfg,st", CASES)
def test_best_ehvi_is_numpys_first_argmax_of_the_values(cfg, st):
    c = built(cfg, st)
    eng = c["eng"]
    for m in MS:
        so = _segments(m)
        for p, mode in ((0, None), (1, "gate"), (31, "weight"), (32, None), (63, "weight")):
            value, logpof, mean, var = c["dev"][m, p, mode]
            idx, bv, blp, bm, bvar = eng.best_ehvi(c["leaves"][_rows(m)], c["member"], c["fronts"][p], c["ref"], True, mode, c["gate"], so)
            assert bm.shape == (2, 3) and bvar.shape == (2, 3)
            for s, (a, b) in enumerate(zip(so[:-1], so[1:])):
                if a == b:
                    assert idx[s] == -1 and np.isnan(bv[s]) and np.isnan(blp[s]) and np.all(np.isnan(bm[:, s])) and np.all(np.isnan(bvar[:, s]))
                    continue
                w = int(np.argmax(value[a:b]))
                assert idx[s] == w, (m, p, mode, s)
                at = a + w
                assert _bits(bv[s]) == _bits(value[at]) and _bits(blp[s]) == _bits(logpof[at]), (m, p, mode, s)
                assert np.array_equal(_bits(bm[:, s]), _bits(mean[:, at])) and np.array_equal(_bits(bvar[:, s]), _bits(var[:, at]))
    # one segment (seg_off None)
    value = c["dev"][162, 31, None][0]
    idx, bv, _, _, _ = eng.best_ehvi(c["leaves"], c["member"], c["fronts"][31], c["ref"])
    assert idx[0] == int(np.argmax(value)) and _bits(bv[0]) == _bits(value.max())
    # a NaN leaf (a NaN coordinate: NaN columns, a NaN EHVI) wins its segment, and only its own
    bad = np.array(c["leaves"])
    bad[40, 1] = np.nan
    for mode in (None, "weight", "gate"):
        idx, bv, blp, bm, bvar = eng.best_ehvi(bad, c["member"], c["fronts"][31], c["ref"], True, mode, c["gate"], np.array([0, 30, 162]))
        assert int(idx[1]) == 10 and np.isnan(bv[1]) and np.all(np.isnan(bm[:, 1])) and np.all(np.isnan(bvar[:, 1])), mode
        assert int(idx[0]) == int(np.argmax(c["dev"][162, 31, mode][0][:30])) and not np.isnan(bv[0]), mode
        assert np.isnan(blp[1]) == bool(c["others"] or c["suc"]), mode  # (no other term: logpof is +0.0 whatever the leaf)


@pytest.mark.parametrize("cfg,st", CASES)
def test_values_against_the_numpy_oracle(cfg, st):
    c = built(cfg, st)
    o_m1, o_m2 = c["o_obj"][0], c["o_mean"][c["member"]]
    o_s1, o_s2 = c["o_s"]
    tol_m = (1e-9 * max(1.0, float(np.max(np.abs(c["y"])))), 1e-9 * max(1.0, float(np.max(np.abs(c["cY"][c["member"]])))))
    tol_v = (1e-9 * c["th_obj"].variance, 1e-9 * c["thetas"][c["member"]].variance)
    for p in PS:
        f, ref = c["fronts"][p], c["ref"]
        value, logpof, mean, var = c["dev"][162, p, None]
        # on the device's own columns: the fold alone
        s1, s2 = eo.sigmas(var[0], c["th_obj"].noise, var[1], c["noise"][c["member"]])
        mod = moderate(c, p, mean[0], s1, mean[1], s2)
        want = eo.ehvi_numpy(f, ref, mean[0], s1, mean[1], s2)
        scale = eo.scale_numpy(f, ref, mean[0], s1, mean[1], s2)
        err = np.abs(value - want) / (eo.ULP * scale)
        print(f"EHVI_ORACLE_GPU {cfg} {st} P={p}: {int(mod.sum())} moderate leaves, worst c on the device's columns {err[mod].max():.2f} "
              f"(allowed {C_VS_ORACLE:.1f}); all leaves {err.max():.2f}")
        assert mod.mean() >= 0.2 and np.all(err[mod] <= C_VS_ORACLE), (p, err[mod].max())
        # on the oracle's columns: plus what the columns' tolerance can move the value
        # (the allowance below divides by s: a leaf with s = 0 on either objective has an infinite z and is no moderate leaf, and
        # the mask says so in its own words as well)
        mod_o = moderate(c, p, o_m1, o_s1, o_m2, o_s2) & (o_s1 > 0.0) & (o_s2 > 0.0)
        want_o = eo.ehvi_numpy(f, ref, o_m1, o_s1, o_m2, o_s2)
        scale_o = eo.scale_numpy(f, ref, o_m1, o_s1, o_m2, o_s2)
        e_p, g_0 = eo._excess(o_m2, o_s2, ref[1]), eo._excess(o_m1, o_s1, ref[0])
        moved = (tol_m[0] + 0.4 * tol_v[0] / (2.0 * o_s1)) * e_p + (tol_m[1] + 0.4 * tol_v[1] / (2.0 * o_s2)) * g_0
        assert np.all(np.abs(value - want_o)[mod_o] <= (C_VS_ORACLE * eo.ULP * scale_o + 2.0 * moved)[mod_o]), p
    # logpof and the weighted value against the oracle's (another libm: relative 1e-9 of the columns' tolerance's reach)
    value, logpof, _, _ = c["dev"][162, 31, "weight"]
    if c["others"] or c["suc"]:
        assert np.allclose(logpof, c["o_logpof"], rtol=1e-6, atol=1e-7)
        keep = logpof >= c["gate"]
        assert keep.any() and (~keep).any() and np.all(np.isneginf(value[~keep]))


@pytest.mark.parametrize("cfg,st", CASES)
def test_posterior_set_and_constrained_calls_are_untouched(cfg, st):
    from pygpso_amd import acquisition as A

    c = built(cfg, st)
    eng = c["eng"]
    eng.ehvi_values(c["leaves"], c["member"], c["fronts"][63], c["ref"], True, "weight", c["gate"])
    eng.best_ehvi(c["leaves"], c["member"], c["fronts"][63], c["ref"], True, "gate", c["gate"], _segments(162))
    assert eng.posterior_hash() == c["hash"]
    k, theta, thr, sense = eng.constraint_info()
    assert k == c["info"][0] and all(np.array_equal(a, b) for a, b in zip((theta, thr, sense), c["info"][1:]))
    assert eng.success_info()[0] == c["suc"]
    again = eng.constrained_best_acq(c["leaves"], A.EI(xi=0.0), "weight", c["gate"], _segments(162), incumbent=0.0)
    for a, b in zip(again, c["con_best"]):
        assert np.array_equal(a, b, equal_nan=True) and (a.dtype != np.float64 or np.array_equal(_bits(a), _bits(b)))
    cols = eng.constrained_acq_values(c["leaves"], A.EI(xi=0.0), "gate", -np.inf, incumbent=0.0, want_members=True)
    for a, b in zip(cols, c["con"][162]):
        assert np.array_equal(_bits(a), _bits(b))
    assert eng.last_ms(1) > 0.0 and eng.last_count(0) == 162 and eng.last_count(1) == 162


def test_engine_side_refusals_return_their_code_and_allocate_nothing():
    """Every refusal of the two calls: its code, a message in the call's own words, and ``gpso_last_count(ctx, 4)`` -- the bytes
    the contexts of this process hold -- read through the context that was called, unchanged across the refused call."""
    import ctypes as C

    from pygpso_amd import HipGPEngine, _lib
    from pygpso_amd import acquisition as A

    c = problem("m52_f64", "middle")
    leaves, front, ref = c["leaves"][:9], c["fronts"][31], c["ref"]
    eng, src, e32 = HipGPEngine("float64"), HipGPEngine("float64"), HipGPEngine("float32")

    def refused(on, fn, code, word):
        held = on.last_count(4)
        with pytest.raises(ValueError if code == _lib.E_ARG else _lib.GpsoHipError) as err:  # (the engine raises GPSO_E_ARG as ValueError)
            fn()
        assert (code == _lib.E_ARG or err.value.code == code) and word in str(err.value), (code, word, str(err.value))
        assert on.last_count(4) == held, word  # nothing was allocated on the way to the refusal

    def push_set():
        for i, th in enumerate(c["thetas"]):
            src.set_data(c["X"], c["cY"][i])
            _fit(src, th)
            eng.constraint_push(src, c["thr"][i], int(c["sense"][i]))

    calls = {"gpso_ehvi_values": lambda e, *a, **k: e.ehvi_values(leaves, *a, **k), "gpso_best_ehvi": lambda e, *a, **k: e.best_ehvi(leaves, *a, **k)}
    for name, call in calls.items():
        refused(eng, lambda: call(eng, 0, front, ref), _lib.E_STATE, name)  # nothing fitted on ctx
    eng.set_data(c["X"], c["y"])
    _fit(eng, c["th_obj"])
    for name, call in calls.items():
        refused(eng, lambda: call(eng, 0, front, ref), _lib.E_STATE, "no constraint set")  # neither a set nor a success member
    # a success member alone is no objective: the one state refusal that is the EHVI calls' own
    Xc, yc, uu, n_ls, mu, S = _classifier_posterior()
    cls = HipGPEngine("float64")
    cls.set_data(Xc, yc)
    cls.vgp_set_likelihood("Bernoulli", 0.0, B.N_GH)
    cls.vgp_set_q(mu, S)
    cls.vgp_posterior(CLS_KERNEL, uu, n_ls, True, 0.0)
    eng.success_push(cls)
    assert eng.success_info()[0] and eng.constraint_info()[0] == 0
    for name, call in calls.items():
        refused(eng, lambda: call(eng, 0, front, ref), _lib.E_STATE, "a success member alone is no objective")
        refused(eng, lambda: call(eng, 0, front, ref), _lib.E_STATE, name)
    # ... and a stale one (the objective's D is no longer the member's) is refused in the constrained calls' words
    X3, y3 = synthetic_problem(N, 3, seed=3)
    eng.set_data(X3, y3)
    eng.fit_eval("Matern52", 0.4, 1.0, 1e-2, 0.0, want_grad=False)
    leaves3 = synthetic_leaves(9, 3, seed=4)
    refused(eng, lambda: eng.ehvi_values(leaves3, 0, front, ref), _lib.E_STATE, "the success member D=2")
    refused(eng, lambda: eng.best_ehvi(leaves3, 0, front, ref), _lib.E_STATE, "the success member D=2")
    eng.success_clear()
    # N = 129 on ctx
    X129, y129 = synthetic_problem(129, D, seed=16)
    eng.set_data(X129, y129)
    eng.fit_eval("Matern52", 0.4, 1.0, 1e-2, 0.0, want_grad=False)
    for name, call in calls.items():
        refused(eng, lambda: call(eng, 0, front, ref), _lib.E_ARG, "N=129")
    eng.set_data(c["X"], c["y"])
    _fit(eng, c["th_obj"])
    push_set()
    e32.set_data(c["X"], c["y"])
    _fit(e32, c["th_obj"])
    for name, call in calls.items():
        refused(e32, lambda: call(e32, 0, front, ref), _lib.E_ARG, name)  # a float32 context
        for member in (-1, 3):
            refused(eng, lambda: call(eng, member, front, ref), _lib.E_ARG, "member")
        refused(eng, lambda: call(eng, 1, eo.make_front(64) + ref, ref), _lib.E_ARG, "63")
        refused(eng, lambda: call(eng, 1, front[::-1], ref), _lib.E_ARG, "ascending")
        refused(eng, lambda: call(eng, 1, np.column_stack([front[:, 0], front[::-1, 1]]), ref), _lib.E_ARG, "descending")
        refused(eng, lambda: call(eng, 1, front, (ref[0], float(front[-1, 1]))), _lib.E_ARG, "strictly above")
        refused(eng, lambda: call(eng, 1, front, (np.nan, ref[1])), _lib.E_ARG, "finite")
        bad = front.copy()
        bad[4, 1] = np.inf
        refused(eng, lambda: call(eng, 1, bad, ref), _lib.E_ARG, "finite")
        refused(eng, lambda: call(eng, 1, front, ref, True, "feasibility"), _lib.E_ARG, "GPSO_CON_FEASIBILITY")
        refused(eng, lambda: call(eng, 1, front, ref, True, 7), _lib.E_ARG, "cspec.mode")
        refused(eng, lambda: call(eng, 1, front, ref, True, "gate", 0.5), _lib.E_ARG, "log_pof_min")
        refused(eng, lambda: call(eng, 1, front, ref, True, "weight", np.nan), _lib.E_ARG, "log_pof_min")
    refused(eng, lambda: eng.best_ehvi(leaves, 1, front, ref, seg_off=np.array([0, 4, 8])), _lib.E_ARG, "seg_off")
    refused(eng, lambda: eng.ehvi_values(np.zeros((0, D)), 1, front, ref), _lib.E_ARG, "gpso_ehvi_values")  # m = 0
    # (J + 1) m above 2^28 with J = 3: the refusal comes before a byte of the leaves is read (the array is never touched: its
    # pages are not even mapped)
    many = np.zeros(((1 << 26) + 1, D))
    refused(eng, lambda: eng.ehvi_values(many, 1, front, ref), _lib.E_ARG, "2^28")
    refused(eng, lambda: eng.best_ehvi(many, 1, front, ref), _lib.E_ARG, "2^28")
    del many
    # what the Python layer never sends, through the C-ABI itself: a NULL idx, every output NULL, nseg outside [1, 1024]
    ptr, dt, mem, m, keep = eng._leaf_args(leaves)
    rec, keep_front = eng._ehvi_rec(1, front, ref, True)
    idx, out = np.zeros(3, dtype=np.int64), np.zeros(6)

    def raw(fn, word):
        held = eng.last_count(4)
        assert fn() == _lib.E_ARG
        msg = eng._lib.gpso_last_error(eng._h).decode()
        assert word in msg and eng.last_count(4) == held, msg

    lib = eng._lib
    raw(lambda: lib.gpso_ehvi_values(eng._h, ptr, dt, mem, m, C.byref(rec), None, None, None, None, None, _lib.MEM_HOST), "every output is NULL")
    raw(lambda: lib.gpso_ehvi_values(eng._h, ptr, dt, mem, m, C.byref(rec), None, C.c_void_p(out.ctypes.data), None, None, None, 7), "out_mem")
    raw(lambda: lib.gpso_best_ehvi(eng._h, ptr, dt, mem, m, None, 1, C.byref(rec), None, None, _lib.dptr(out), None, None, None), "idx must not be NULL")
    for nseg in (0, 1025):
        raw(lambda: lib.gpso_best_ehvi(eng._h, ptr, dt, mem, m, None, nseg, C.byref(rec), None, _lib.i64ptr(idx), None, None, None, None), "nseg")
    raw(lambda: lib.gpso_best_ehvi(eng._h, ptr, dt, mem, m, None, 1, None, None, _lib.i64ptr(idx), None, None, None, None), "ehvi must not be NULL")
    raw(lambda: lib.gpso_ehvi_values(eng._h, None, dt, mem, m, C.byref(rec), None, C.c_void_p(out.ctypes.data), None, None, None, _lib.MEM_HOST), "xs must not be NULL")
    # an asynchronous call open, an ensemble resident, a stale set
    ticket = eng.best_acq_begin(leaves, A.UCBVar(2.0))
    refused(eng, lambda: eng.ehvi_values(leaves, 1, front, ref), _lib.E_STATE, "gpso_ehvi_values")
    eng.best_ucb_end(ticket)
    eng.ensemble_push()
    refused(eng, lambda: eng.best_ehvi(leaves, 1, front, ref), _lib.E_STATE, "ensemble")
    eng.ensemble_clear()
    eng.set_data(c["X"][:-1], c["y"][:-1])
    _fit(eng, c["th_obj"])
    refused(eng, lambda: eng.ehvi_values(leaves, 1, front, ref), _lib.E_STATE, "stale")
    eng.set_data(c["X"], c["y"])
    _fit(eng, c["th_obj"])
    # ... and after all of it the calls are served, and only then is anything allocated for them
    held = eng.last_count(4)
    v, lp, mean, var = eng.ehvi_values(leaves, 1, front, ref)
    assert np.all(v > 0.0) and np.all(lp <= 0.0) and eng.last_count(4) > held
    for e in (eng, src, e32, cls):
        e.close()


def test_ehvi_select_grows_the_hypervolume_of_a_two_output_toy():
    """One surrogate update on a two-output toy, then ``ehvi_select``: the chosen leaf, once evaluated and appended, does not
    reduce the hypervolume of the observed front -- and the selection is the device's arg-max of its own values."""
    from pygpso_amd import GPRSurrogate, pareto
    from pygpso_amd import kernels as K
    from pygpso_amd.constraints import Constraint

    def toy(x):
        x = np.atleast_2d(x)
        return -np.sum((x - 0.25) ** 2, axis=1), -np.sum((x - 0.75) ** 2, axis=1)

    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy(),
                        constraints=[Constraint("f2", lower=-0.7)])
    rng = np.random.default_rng(12)
    x = rng.uniform(0.0, 1.0, (16, 2))
    f1, f2 = toy(x)
    surr.append(x, f1, constraint_values=f2[:, None])
    surr.gp_update()
    leaves = rng.uniform(0.0, 1.0, (162, 2))
    coords, front = surr.pareto_front("f2")
    ref = surr._ehvi_reference(0, f1, None)
    assert front.shape[0] >= 2 and np.all(front > ref)
    before = pareto.hypervolume_2d(front, ref)
    n_points = len(surr.points)
    idx, value, logpof, mean, var = surr.ehvi_select(leaves, "f2")
    assert len(surr.points) == n_points  # stores nothing
    vals = surr.gpflow_model.ehvi_values(leaves, 0, front, ref)[0]
    assert int(idx[0]) == int(np.argmax(vals)) and _bits(value[0]) == _bits(vals.max()) and value[0] > 0.0 and logpof[0] == 0.0
    pick = leaves[int(idx[0])]
    y1, y2 = toy(pick)
    surr.append(pick[None], y1, constraint_values=y2[:, None])
    after = pareto.hypervolume_2d(surr.pareto_front("f2", ref)[1], ref)
    print(f"EHVI_SELECT: hypervolume {before:.6f} -> {after:.6f} (EHVI of the pick {value[0]:.3e})")
    assert after >= before
    surr.close_constraint_models()
