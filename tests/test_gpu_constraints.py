"""
Outcome constraints on the device: a context's constraint set -- J exact-GP posteriors of other
targets, copied in from the contexts they were fitted on -- and the constrained acquisition over them, against the float64
oracle and against the library's own calls.

Shapes: N in {5, 64, 65, 128} (the 64-row boundary of the factor's blocks and the limit), D in {1, 2, 12, 33}, M in {1, 63,
64, 65, 1000} (one leaf, the 64-leaf tile's edges, many tiles), J in {1, 2, 7, 16} (the set's limit), every kernel kind,
"float64" and "mixed" contexts, one case with a noise vector on the objective, one whose members are pushed from the
context itself, one ("block") whose members are fitted on and pushed from a "mixed" source (the other mixed case pushes
from a float64 one).  Every case is built once and shared, never written to.

Thresholds sit at the median of the oracle's constraint mean over the leaves and the gate at the median of the oracle's
logpof, so that both sides of every gate are populated; the tests assert that from the oracle (M > 1).

Tolerances: the columns are held to DESIGN.md 2.1's float64 row -- 1e-9 of max(1, max|targets|) on the mean and of the kernel
variance on the variance (Matern-1/2: 1e-5) -- against the oracle posterior of each member's own (X, c_i, theta_i) and
against gpso_predict on the source context where that context predicts in double (a "mixed" source fits in double -- what a
push copies -- and predicts in float: its members are held to the oracle alone).  The device fold is the host fold of the device's own columns: logpof, the gate
decision, the UCB kinds' values and weight-mode log-EI given l0 bit for bit; EI / PI / log-EI values to tests/acq_oracle.py's
per-value tolerance (another libm).
"""
import numpy as np
import pytest

from oracle import gpr
from tests import acq_oracle, constraints_oracle as co, hetero_oracle
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

VS = gpr.VARSIGMA_DEFAULT
# name: (N, D, M, J, kernel, dtype, noise vector on the objective, ARD, pushed from the context itself)
CASES = {
    "tiny": (5, 1, 1, 1, "Matern52", "float64", False, False, False),
    "block": (64, 2, 63, 2, "Matern32", "mixed", True, False, False),
    "block+1": (65, 12, 64, 7, "Matern12", "float64", False, True, False),
    "limit_wide": (128, 33, 65, 16, "SquaredExponential", "mixed", False, True, False),
    "limit_many": (128, 2, 1000, 7, "Matern52", "float64", False, False, False),
    "self": (52, 2, 162, 2, "SquaredExponential", "float64", False, False, True),
}
KINDS = ("ucb_var", "ucb_std", "ei", "logei", "pi")
_BUILT = {}


def _spec(kind, latent=False):
    from pygpso_amd import acquisition as A

    return {"ucb_var": lambda: A.UCBVar(VS), "ucb_std": lambda: A.UCBStd(VS, latent=latent), "ei": lambda: A.EI(xi=0.01, latent=latent),
            "logei": lambda: A.LogEI(xi=0.01, latent=latent), "pi": lambda: A.PI(xi=0.01, latent=latent)}[kind]()


def _theta(kernel, d, ard, mean_c, rng):
    base = 0.3 * np.sqrt(d)
    ls = base * np.exp(0.3 * rng.standard_normal(d)) if ard else float(base * np.exp(0.3 * rng.standard_normal()))
    return gpr.Theta(kernel, ls, float(1.2 * np.exp(0.3 * rng.standard_normal())), float(2e-3 * np.exp(0.5 * rng.standard_normal())),
                     float(mean_c + 0.1 * rng.standard_normal()))


def constraint_targets(X, j, seed):
    """Synthetic constrained outputs: smooth functions of the same rows, [J, N]."""
    rng = np.random.default_rng([seed, j])
    w = rng.normal(size=(j, X.shape[1]))
    ph = rng.uniform(0.0, 2.0 * np.pi, j)
    return np.array([np.sin(2.0 * X @ w[i] + ph[i]) + 0.25 * np.cos(3.0 * X[:, 0] + i) for i in range(j)])


def problem(name):
    """The inputs of a case and what the oracle says of them: no GPU."""
    n, d, m, j, kernel, dtype, with_s, ard, from_self = CASES[name]
    X, y = synthetic_problem(n, d, seed=3)
    leaves = synthetic_leaves(m, d, seed=4)
    s = np.random.default_rng(5).uniform(0.0, 5e-3, n) if with_s else None
    rng = np.random.default_rng([6, j, d])
    th_obj = _theta(kernel, d, ard, float(y.mean()), rng)
    cY = constraint_targets(X, j, seed=7)
    thetas = [_theta(kernel, d, ard, float(cY[i].mean()), rng) for i in range(j)]
    om, ov = np.empty((j, m)), np.empty((j, m))
    for i, th in enumerate(thetas):
        om[i], ov[i] = gpr.predict_y(gpr.posterior(th, X, cY[i]), leaves)
    thr = np.median(om, axis=1)
    sense = np.array([1 if i % 2 == 0 else -1 for i in range(j)], dtype=np.int64)
    noise = np.array([th.noise for th in thetas])
    o_logpof = co.log_pof_numpy(om, ov, noise, thr, sense)
    gate = float(np.median(o_logpof))
    if s is None:
        obj = gpr.predict_y(gpr.posterior(th_obj, X, y), leaves)
    else:
        obj = hetero_oracle.predict_y(hetero_oracle.posterior(th_obj, X, y, s), leaves)
    return dict(n=n, d=d, m=m, j=j, kernel=kernel, dtype=dtype, s=s, from_self=from_self, X=X, y=y, leaves=leaves, th_obj=th_obj, cY=cY,
                thetas=thetas, o_mean=om, o_var=ov, thr=thr, sense=sense, noise=noise, o_logpof=o_logpof, gate=gate, o_obj=obj,
                inc=float(np.max(y)))


def _fit(eng, th):
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)


def built(name):
    """The case's engine with its constraint set installed and the device's outputs: made once, shared, read-only."""
    if name in _BUILT:
        return _BUILT[name]
    from pygpso_amd import HipGPEngine

    c = problem(name)
    eng = HipGPEngine(c["dtype"])
    src_dtype = "mixed" if name == "block" else "float64"
    src = eng if c["from_self"] else HipGPEngine(src_dtype)
    src_pred = []
    for i, th in enumerate(c["thetas"]):
        src.set_data(c["X"], c["cY"][i])
        _fit(src, th)
        src_pred.append(src.predict(c["leaves"]))
        assert eng.constraint_push(src, c["thr"][i], int(c["sense"][i])) == i
    eng.set_data(c["X"], c["y"])  # (from_self: the objective's targets arrive after the members left; the set stays)
    if c["s"] is not None:
        eng.set_noise_diag(c["s"])
    _fit(eng, c["th_obj"])
    assert eng.constraint_max() == 16 and eng.constraint_info()[0] == c["j"]
    c.update(eng=eng, src=src, src_pred=src_pred, src_dtype=src_dtype, hash=eng.posterior_hash())
    c["plain"] = {kind: eng.acq_values(c["leaves"], _spec(kind), incumbent=c["inc"]) for kind in KINDS}
    c["dev"] = {}
    for kind in KINDS:
        for mode in ("gate", "feasibility") + (() if kind.startswith("ucb") else ("weight",)):
            c["dev"][kind, mode] = eng.constrained_acq_values(c["leaves"], _spec(kind), mode, c["gate"], incumbent=c["inc"], want_members=True)
        c["dev"][kind, "open"] = eng.constrained_acq_values(c["leaves"], _spec(kind), "gate", -np.inf, incumbent=c["inc"])
    for a in (c["X"], c["y"], c["leaves"]):
        a.setflags(write=False)
    _BUILT[name] = c
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _col_bounds(c, targets):
    tol = 1e-5 if c["kernel"] == "Matern12" else 1e-9
    return tol * max(1.0, float(np.max(np.abs(targets)))), tol


@pytest.mark.parametrize("name", list(CASES))
def test_thresholds_populate_both_sides_of_every_gate(name):
    """From the oracle alone (no GPU needed for the claim; the seeds were checked on the CPU)."""
    c = problem(name)
    if c["m"] == 1:
        return
    for i in range(c["j"]):
        assert np.any(c["o_mean"][i] < c["thr"][i]) and np.any(c["o_mean"][i] > c["thr"][i]), (name, i)
    assert np.any(c["o_logpof"] < c["gate"]) and np.any(c["o_logpof"] > c["gate"]), name


@pytest.mark.parametrize("name", list(CASES))
def test_member_columns_against_the_oracle_and_the_source_context(name):
    c = built(name)
    mean, var, _, _, mm, mv = c["dev"]["ucb_var", "gate"]
    assert mm.shape == (c["j"], c["m"]) and mv.shape == (c["j"], c["m"])
    k, theta, thr, sense = c["eng"].constraint_info()
    assert k == c["j"] and theta.shape == (k, 51) and np.array_equal(thr, c["thr"]) and np.array_equal(sense, c["sense"])
    for i, th in enumerate(c["thetas"]):
        ls = np.broadcast_to(np.atleast_1d(th.lengthscales), (c["d"],))
        assert np.array_equal(theta[i, :c["d"]], ls) and tuple(theta[i, 48:]) == (th.variance, th.noise, th.mean_c)
        tol_m, tol_v = _col_bounds(c, c["cY"][i])
        refs = [("oracle", (c["o_mean"][i], c["o_var"][i]))]
        if c["src_dtype"] == "float64":  # (a mixed source predicts in float)
            refs.append(("gpso_predict on src", c["src_pred"][i]))
        for tag, (rm, rv) in refs:
            em, ev = float(np.max(np.abs(mm[i] - rm))), float(np.max(np.abs(mv[i] - rv))) / th.variance
            print(f"CONSTRAINT_PARITY {name} member {i} vs {tag}: mean {em:.2e} (bound {tol_m:.1e}), var {ev:.2e} (bound {tol_v:.1e})")
            assert em <= tol_m and ev <= tol_v, (name, i, tag, em, ev)
    # the objective's columns: the oracle's, and gpso_predict's on the context itself
    tol_m, tol_v = _col_bounds(c, c["y"])
    refs = [c["o_obj"]] + ([c["eng"].predict(c["leaves"])] if c["dtype"] == "float64" else [])  # (a mixed context predicts in float)
    for rm, rv in refs:
        assert float(np.max(np.abs(mean - rm))) <= tol_m and float(np.max(np.abs(var - rv))) / c["th_obj"].variance <= tol_v, name


@pytest.mark.parametrize("name", list(CASES))
def test_device_fold_is_the_host_fold_of_the_devices_own_columns(name):
    from pygpso_amd import HipGPEngine

    c = built(name)
    onoise = c["th_obj"].noise
    for (kind, mode), out in c["dev"].items():
        if mode == "open":
            continue
        mean, var, value, logpof, mm, mv = out
        h_val, h_lp = HipGPEngine.constrained_fold_host(_spec(kind), mean, var, onoise, mm, mv, c["noise"], c["thr"], c["sense"], mode,
                                                        c["gate"], incumbent=c["inc"])
        assert np.array_equal(_bits(logpof), _bits(h_lp)), (name, kind, mode)
        assert np.array_equal(np.isneginf(value), np.isneginf(h_val)), (name, kind, mode)  # the gate's decision
        if mode == "gate":
            assert np.array_equal(np.isneginf(value), ~(logpof >= c["gate"])), (name, kind)
        if mode == "feasibility":
            assert np.array_equal(_bits(value), _bits(logpof)) and np.array_equal(_bits(value), _bits(h_val))
        elif kind.startswith("ucb"):
            assert np.array_equal(_bits(value), _bits(h_val)), (name, kind, mode)
        else:
            tol = acq_oracle.tolerance(acq_oracle.KINDS[kind])[0]
            live = np.isfinite(h_val)
            assert np.array_equal(_bits(value[~live]), _bits(h_val[~live]))
            scale = np.maximum(1.0, np.abs(h_val[live])) if kind == "logei" else np.maximum(np.abs(h_val[live]), 2.0 ** -1022)
            err = float(np.max(np.abs(value[live] - h_val[live]) / scale)) if live.any() else 0.0
            print(f"CONSTRAINT_FOLD {name} {kind} {mode}: device against host {err:.2e} (tolerance {tol:.2e})")
            assert err <= tol, (name, kind, mode, err)
    # an open gate returns the unconstrained numbers of the same stage 1; a surviving leaf keeps those bits; weight-mode
    # log-EI is l0 + logpof to the bit, given the device's l0
    for kind in KINDS:
        o_mean, o_var, o_val, o_lp = c["dev"][kind, "open"]
        mean, var, value, logpof = c["dev"][kind, "gate"][:4]
        assert np.array_equal(_bits(o_mean), _bits(mean)) and np.array_equal(_bits(o_var), _bits(var)) and np.array_equal(_bits(o_lp), _bits(logpof))
        assert not np.any(np.isneginf(o_val)) or kind == "logei"
        keep = logpof >= c["gate"]
        assert np.array_equal(_bits(value[keep]), _bits(o_val[keep])) and np.all(np.isneginf(value[~keep])), (name, kind)
        h_open = HipGPEngine.acq_eval_host(_spec(kind), mean, var, onoise, incumbent=c["inc"])
        if kind.startswith("ucb"):
            assert np.array_equal(_bits(o_val), _bits(h_open))
    l0 = c["dev"]["logei", "open"][2]
    _, _, w_val, w_lp = c["dev"]["logei", "weight"][:4]
    keep = w_lp >= c["gate"]
    assert np.array_equal(_bits(w_val[keep]), _bits((l0 + w_lp)[keep])) and np.all(np.isneginf(w_val[~keep]))
    # a latent kind reads the objective's own noise
    for kind in ("ucb_std", "ei"):
        mean, var, value, logpof, mm, mv = c["eng"].constrained_acq_values(c["leaves"], _spec(kind, latent=True), "gate", c["gate"],
                                                                          incumbent=c["inc"], want_members=True)
        h_val = HipGPEngine.constrained_fold_host(_spec(kind, latent=True), mean, var, onoise, mm, mv, c["noise"], c["thr"], c["sense"], "gate",
                                                  c["gate"], incumbent=c["inc"])[0]
        live = np.isfinite(h_val)
        assert np.array_equal(np.isneginf(value), np.isneginf(h_val))
        if kind == "ucb_std":
            assert np.array_equal(_bits(value), _bits(h_val))
        elif live.any():
            assert float(np.max(np.abs(value[live] - h_val[live]) / np.maximum(np.abs(h_val[live]), 2.0 ** -1022))) <= acq_oracle.tolerance(acq_oracle.EI)[0]


@pytest.mark.parametrize("name", list(CASES))
def test_logpof_against_the_oracle_on_the_devices_columns(name):
    """The device's logpof against mpmath on the device's own member columns: constraints_oracle's measured bound."""
    from tests import mes_oracle

    c = built(name)
    _, _, _, logpof, mm, mv = c["dev"]["ucb_var", "gate"]
    pick = np.unique(np.linspace(0, c["m"] - 1, 40).astype(int))
    want = co.truth_logpof(mm[:, pick], mv[:, pick], c["noise"], c["thr"], c["sense"])
    err, tol = mes_oracle.error(logpof[pick], want), co.tolerance(c["j"])[0]
    print(f"CONSTRAINT_LOGPOF {name}: {err:.2e} (bound {tol:.2e})")
    assert err <= tol, (name, err, tol)


def _segments(m, nseg):
    if nseg == 1:
        return None
    cuts = np.unique(np.round(np.linspace(0, m, nseg + 1)).astype(np.int64))
    return np.concatenate([cuts, np.full(nseg + 1 - cuts.shape[0], m, dtype=np.int64)])  # (M < nseg: empty segments at the end)


@pytest.mark.parametrize("nseg", (1, 5))
@pytest.mark.parametrize("name", list(CASES))
def test_best_acq_is_the_first_row_arg_max_of_acq_values(name, nseg):
    c = built(name)
    so = _segments(c["m"], nseg)
    if so is not None and c["m"] >= 10:
        so = np.concatenate([so[:2], so[1:]])  # an empty segment in the middle
    bounds = np.array([0, c["m"]]) if so is None else so

    def check(kind, mode, gate, cols):
        idx, mean, var, value, logpof = c["eng"].constrained_best_acq(c["leaves"], _spec(kind), mode, gate, so, incumbent=c["inc"])
        gated_segments = 0
        for sgm, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            if a == b:
                assert idx[sgm] == -1 and np.isnan(value[sgm]) and np.isnan(logpof[sgm])
                continue
            j = int(np.argmax(cols[2][a:b]))
            assert int(idx[sgm]) == j, (name, kind, mode, sgm)
            gated_segments += bool(np.all(np.isneginf(cols[2][a:b])))
            for got, col in zip((mean, var, value, logpof), cols):
                assert _bits([got[sgm]])[0] == _bits([col[a + j]])[0], (name, kind, mode, sgm)
        return gated_segments

    for (kind, mode), cols in c["dev"].items():
        check(kind, "gate" if mode == "open" else mode, -np.inf if mode == "open" else c["gate"], cols)
    # a segment in which every leaf is gated: the gate just above the lowest of the segments' best logpof
    lp = c["dev"]["ucb_var", "gate"][3]
    tops = [float(np.max(lp[a:b])) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
    gate = min(float(np.nextafter(min(tops), np.inf)), 0.0)
    cols = c["eng"].constrained_acq_values(c["leaves"], _spec("ucb_var"), "gate", gate)
    assert check("ucb_var", "gate", gate, cols) >= 1


def test_ties_go_to_the_first_leaf_and_a_nan_leaf_wins_its_segment():
    c = built("block")
    eng, leaves = c["eng"], np.array(c["leaves"])
    best = int(eng.constrained_best_acq(leaves, _spec("ucb_var"), "gate", c["gate"])[0][0])
    dup = np.vstack([leaves, leaves[best:best + 1], leaves[best:best + 1]])
    idx = eng.constrained_best_acq(dup, _spec("ucb_var"), "gate", c["gate"])[0]
    vals = eng.constrained_acq_values(dup, _spec("ucb_var"), "gate", c["gate"])[2]
    assert vals[best] == vals[-1] == vals[-2] and int(idx[0]) == best
    # a leaf's numbers depend neither on its slot nor on the rest of the batch
    solo = eng.constrained_acq_values(leaves[best:best + 1], _spec("ucb_var"), "gate", c["gate"])
    full = c["dev"]["ucb_var", "gate"]
    for a, b in zip(solo, full[:4]):
        assert _bits(a)[0] == _bits(b)[best]
    bad = leaves.copy()
    bad[40, 1] = np.nan
    for kind in KINDS:
        idx, mean, var, value, logpof = eng.constrained_best_acq(bad, _spec(kind), "gate", c["gate"], np.array([0, 30, bad.shape[0]]),
                                                                 incumbent=c["inc"])
        assert int(idx[1]) == 10 and np.isnan(value[1]) and np.isnan(logpof[1]) and not np.isnan(value[0]), kind
    # the same call gives the same bits
    again = eng.constrained_acq_values(c["leaves"], _spec("ei"), "weight", c["gate"], incumbent=c["inc"], want_members=True)
    for a, b in zip(again, c["dev"]["ei", "weight"]):
        assert np.array_equal(_bits(a), _bits(b))


def test_push_clear_and_the_calls_leave_the_posterior_and_a_refit_keeps_the_set():
    from pygpso_amd import _lib

    c = built("block+1")
    eng, src = c["eng"], c["src"]
    assert eng.posterior_hash() == c["hash"]  # after every call of built() and of the tests above
    plain = eng.best_acq(c["leaves"], _spec("ei"), incumbent=c["inc"])
    for a, b in zip(eng.acq_values(c["leaves"], _spec("ei"), incumbent=c["inc"]), c["plain"]["ei"]):
        assert np.array_equal(_bits(a), _bits(b))
    eng.constrained_best_acq(c["leaves"], _spec("ei"), "weight", c["gate"], incumbent=c["inc"])
    again = eng.best_acq(c["leaves"], _spec("ei"), incumbent=c["inc"])
    for a, b in zip(plain, again):
        assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))
    # a refit of the objective at another theta keeps the set and the members' bits
    before = c["dev"]["ei", "gate"]
    th = gpr.Theta(c["kernel"], 0.9, 0.7, 5e-3, 0.0)
    _fit(eng, th)
    h = eng.posterior_hash()
    after = eng.constrained_acq_values(c["leaves"], _spec("ei"), "gate", c["gate"], incumbent=c["inc"], want_members=True)
    assert eng.constraint_info()[0] == c["j"] and eng.posterior_hash() == h
    for i in (3, 4, 5):  # logpof and the members' columns
        assert np.array_equal(_bits(before[i]), _bits(after[i]))
    pm, pv = eng.predict(c["leaves"])
    assert np.max(np.abs(after[0] - pm)) <= 1e-5 and np.max(np.abs(after[1] - pv)) <= 1e-5  # (the new objective; Matern-1/2's row)
    # a push onto another context and a clear there leave THIS posterior, and src's, alone
    hs = src.posterior_hash()
    assert src.constraint_push(eng, 0.0, 1) == 0 and src.constraint_info()[0] == 1
    src.constraint_clear()
    assert src.constraint_info()[0] == 0 and src.posterior_hash() == hs and eng.posterior_hash() == h
    _fit(eng, c["th_obj"])
    assert eng.posterior_hash() == c["hash"]
    for a, b in zip(eng.constrained_acq_values(c["leaves"], _spec("ei"), "gate", c["gate"], incumbent=c["inc"], want_members=True), before):
        assert np.array_equal(_bits(a), _bits(b))
    # new data with another N: the set is stale, the call says so, and the set is still what it was
    eng.set_data(c["X"][:40], c["y"][:40])
    _fit(eng, c["th_obj"])
    for fn in (lambda: eng.constrained_acq_values(c["leaves"], _spec("ei"), "gate", c["gate"], incumbent=c["inc"]),
               lambda: eng.constrained_best_acq(c["leaves"], _spec("ei"), "gate", c["gate"], incumbent=c["inc"])):
        with pytest.raises(_lib.GpsoHipError) as err:
            fn()
        assert err.value.code == _lib.E_STATE and "gpso_constrained_" in str(err.value) and "stale" in str(err.value)
    assert eng.constraint_info()[0] == c["j"]
    eng.set_data(c["X"], c["y"])
    _fit(eng, c["th_obj"])
    assert eng.posterior_hash() == c["hash"]
    for a, b in zip(eng.constrained_acq_values(c["leaves"], _spec("ei"), "gate", c["gate"], incumbent=c["inc"], want_members=True), before):
        assert np.array_equal(_bits(a), _bits(b))
    # gpso_alloc_posterior ends the set
    eng.alloc_posterior(c["n"], c["d"])
    assert eng.constraint_info()[0] == 0
    _BUILT.pop("block+1")
    eng.close()
    src.close()


def test_refusals_name_the_call_and_leave_the_set():
    """Every refusal of the push and of the constrained calls, its code, and the set as it was afterwards.  The refusal of a
    source on ANOTHER device needs a second GPU: it is made only where there is one, and never on a one-GPU machine."""
    from pygpso_amd import HipGPEngine, _lib, acquisition as A

    X, y = synthetic_problem(129, 2, seed=16)
    leaves = synthetic_leaves(10, 2, seed=17)
    th = gpr.Theta("Matern52", 0.4, 1.0, 1e-2, 0.0)

    def fit(eng, n, kernel="Matern52", d=2):
        eng.set_data(X[:n, :d], y[:n])
        eng.fit_eval(kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)

    def refused(fn, code, word="gpso_constraint_push"):
        with pytest.raises(ValueError if code == _lib.E_ARG else _lib.GpsoHipError) as err:  # (the engine raises GPSO_E_ARG as ValueError)
            fn()
        assert (code == _lib.E_ARG or err.value.code == code) and word in str(err.value), str(err.value)

    eng, src, e32 = HipGPEngine("float64"), HipGPEngine("mixed"), HipGPEngine("float32")
    fit(eng, 20)
    fit(e32, 20)
    assert e32.constraint_max() == 0 and eng.constraint_max() == 16
    assert src.constraint_max() == 16  # (no data yet: a set may be pushed before the objective's data arrive)
    refused(lambda: eng.constraint_push(e32, 0.0, 1), _lib.E_ARG)  # a float32 source
    refused(lambda: e32.constraint_push(eng, 0.0, 1), _lib.E_ARG)  # a float32 owner
    refused(lambda: eng.constraint_push(src, 0.0, 1), _lib.E_STATE)  # nothing fitted on src
    fit(src, 129)
    assert src.constraint_max() == 0  # (129 rows cannot be the objective of a constrained call)
    refused(lambda: eng.constraint_push(src, 0.0, 1), _lib.E_ARG)  # N = 129
    fit(src, 20)
    refused(lambda: eng.constraint_push(src, 0.0, 0), _lib.E_ARG)  # no sense
    refused(lambda: eng.constraint_push(src, np.nan, 1), _lib.E_ARG)
    refused(lambda: eng.constrained_acq_values(leaves, A.EI(), "gate", -1.0, incumbent=0.0), _lib.E_STATE, "gpso_constrained_acq_values")  # no set
    assert eng.constraint_push(src, 0.1, 1) == 0
    fit(src, 21)
    refused(lambda: eng.constraint_push(src, 0.0, 1), _lib.E_STATE)  # another N
    fit(src, 20, d=1)
    refused(lambda: eng.constraint_push(src, 0.0, 1), _lib.E_STATE)  # another D
    fit(src, 20, "Matern32")
    refused(lambda: eng.constraint_push(src, 0.0, 1), _lib.E_STATE)  # another kernel kind
    fit(src, 20)
    u = th.pack()  # a VGP posterior is no member
    src.vgp_set_q()
    src.vgp_natgrad("Matern52", u, 1, True, 0.0, 1.0)
    src.vgp_posterior("Matern52", u, 1, True, 0.0)
    refused(lambda: eng.constraint_push(src, 0.0, 1), _lib.E_STATE)
    fit(src, 20)
    for i in range(1, 16):
        assert eng.constraint_push(src, 0.1 * i, -1) == i
    refused(lambda: eng.constraint_push(src, 0.0, 1), _lib.E_STATE)  # the 17th
    assert eng.constraint_info()[0] == 16
    for name, call in (("gpso_constrained_acq_values", lambda acq, mode, g: eng.constrained_acq_values(leaves, acq, mode, g, incumbent=0.0)),
                       ("gpso_constrained_best_acq", lambda acq, mode, g: eng.constrained_best_acq(leaves, acq, mode, g, incumbent=0.0))):
        refused(lambda: call(A.MES(), "gate", -1.0), _lib.E_ARG, name)
        refused(lambda: call(A.UCBVar(VS), "weight", -1.0), _lib.E_ARG, name)
        refused(lambda: call(A.UCBStd(VS), "weight", -1.0), _lib.E_ARG, name)
        refused(lambda: call(A.EI(), 7, -1.0), _lib.E_ARG, name)
        refused(lambda: call(A.EI(), "gate", 0.5), _lib.E_ARG, name)
        refused(lambda: call(A.EI(), "gate", np.nan), _lib.E_ARG, name)
    refused(lambda: eng.constrained_best_acq(leaves, A.EI(), "gate", -1.0, np.array([0, 4, 9]), incumbent=0.0), _lib.E_ARG, "seg_off")
    ticket = eng.best_ucb_begin(leaves, VS)  # an open ticket, on the owner and on the source
    refused(lambda: eng.constraint_push(src, 0.0, 1), _lib.E_STATE)
    refused(eng.constraint_clear, _lib.E_STATE, "gpso_constraint_clear")
    refused(lambda: eng.constrained_best_acq(leaves, A.EI(), "gate", -1.0, incumbent=0.0), _lib.E_STATE, "gpso_constrained_best_acq")
    refused(lambda: src.constraint_push(eng, 0.0, 1), _lib.E_STATE)
    eng.best_ucb_end(ticket)
    eng.ensemble_push()  # an ensemble on the same context
    refused(lambda: eng.constrained_acq_values(leaves, A.EI(), "gate", -1.0, incumbent=0.0), _lib.E_STATE, "ensemble")
    eng.ensemble_clear()
    k, _, thr, sense = eng.constraint_info()  # after every refusal the set is what it was
    assert k == 16 and thr[0] == 0.1 and sense[0] == 1 and np.all(sense[1:] == -1)
    assert eng.constrained_best_acq(leaves, A.EI(), "gate", -np.inf, incumbent=0.0)[0].shape == (1,)
    import torch

    if torch.cuda.device_count() > 1:
        other = HipGPEngine("float64", device=1)
        fit(other, 20)
        refused(lambda: eng.constraint_push(other, 0.0, 1), _lib.E_ARG)  # different devices
        other.close()
    for e in (eng, src, e32):
        e.close()


# ---- the host layers on the device --------------------------------------------------------------------------------------
def test_surrogate_ranks_by_the_constrained_call_after_one_update():
    from pygpso_amd import GPRSurrogate, acquisition as A
    from pygpso_amd.constraints import ConstrainedAcq, Constraint
    from pygpso_amd.kernels import Constant, Matern52, Scipy

    X, y = synthetic_problem(30, 2, seed=21)
    cY = constraint_targets(X, 2, seed=22)
    leaves = synthetic_leaves(200, 2, seed=23)
    cons = [Constraint("a", upper=float(np.median(cY[0]))), Constraint("b", lower=float(np.median(cY[1])))]
    surr = GPRSurrogate(gp_kernel=Matern52(lengthscales=0.25, variance=1.0), gp_meanf=Constant(0.0), optimiser=Scipy(), constraints=cons,
                        pof_min=0.5)
    surr.append(X, y, constraint_values=cY.T)
    surr.gp_update()
    model = surr.gpflow_model
    assert surr._constraints_live and model.constraint_count() == 2
    k, theta, thr, sense = model.engine.constraint_info()
    assert list(thr) == [c.threshold for c in cons] and list(sense) == [1, -1]
    for i, cm in enumerate(surr._constraint_models):  # each model: its own context, its own optimum, the objective's rows
        assert cm.engine is not model.engine and np.array_equal(cm.data[0], model.data[0]) and np.array_equal(cm.data[1][:, 0], cY[i])
        assert theta[i, 48] == cm.kernel.variance and theta[i, 49] == cm.likelihood.variance
    cols = model.constrained_acq_values(leaves, ConstrainedAcq(A.UCBVar(surr.gp_varsigma), "gate", 0.5), want_members=True)
    gated = np.isneginf(cols[2])
    assert gated.any() and (~gated).any()
    j = int(np.argmax(cols[2]))
    assert surr.gp_eval_best_ucb(leaves) == (cols[0][j], cols[1][j], cols[2][j])
    # the members' columns are the constraint models' own predictions
    for i, cm in enumerate(surr._constraint_models):
        pm, pv = cm.predict_y(leaves)
        assert np.max(np.abs(cols[4][i] - np.asarray(pm)[:, 0])) <= 1e-9 * max(1.0, float(np.max(np.abs(cY[i]))))
        assert np.max(np.abs(cols[5][i] - np.asarray(pv)[:, 0])) <= 1e-9 * cm.kernel.variance
    # grown leaves: the centres of gpso_grow, one segment per box
    bounds = np.array([[[0.0, 1.0 / 3.0], [0.0, 1.0]], [[2.0 / 3.0, 1.0], [0.0, 1.0]]])
    got = surr.gp_eval_best_ucb_grow(bounds, 3)
    for b, g in zip(bounds, got):
        centres = model.engine.grow(b[None], 3)[0]
        c2 = model.constrained_acq_values(centres, ConstrainedAcq(A.UCBVar(surr.gp_varsigma), "gate", 0.5))
        jj = int(np.argmax(c2[2]))
        assert g == (c2[0][jj], c2[1][jj], c2[2][jj])
    best = surr.highest_feasible_score
    ok = (cY[0] <= cons[0].threshold) & (cY[1] >= cons[1].threshold)
    assert ok.any() and best.score_mu == float(np.max(y[ok])) and best.score_mu < float(np.max(y))
    idx, mean, var, value = surr.gp_eval_best_acq(leaves, "logei")  # improves on the best FEASIBLE score
    w = model.constrained_acq_values(leaves, ConstrainedAcq(A.LogEI(), "gate", 0.5), incumbent=best.score_mu)
    assert int(idx[0]) == int(np.argmax(w[2])) and value[0] == w[2].max()
    with pytest.raises(ValueError, match="constraints"):
        surr.select_batch(leaves, 2)
    surr.close_constraint_models()
    assert surr._constraint_models is None and surr.gp_eval_best_ucb(leaves) == (cols[0][j], cols[1][j], cols[2][j])  # the set stays
    model.engine.close()
