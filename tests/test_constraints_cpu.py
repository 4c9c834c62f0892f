"""CPU-only checks of the outcome constraints: the fold of csrc/constraints.hpp through
``gpso_constrained_fold_host`` against the 60-digit truth of tests/constraints_oracle.py, its mode rules to the bit, and the
host layers (``Constraint``, the side store of constraint values, ``highest_feasible_score``, the optimiser's loop) over the
CPU stand-in engine."""
import logging

import numpy as np
import pytest

from pygpso_amd import GPRSurrogate, GPSOptimiser, HipGPEngine, ParameterSpace, PointLabels
from pygpso_amd import _lib as L
from pygpso_amd import acquisition as A
from pygpso_amd import kernels as K
from pygpso_amd.constraints import ConstrainedAcq, Constraint, feasible_rows
from tests import acq_oracle as AO, constraints_oracle as co, mes_oracle

VS = 2.326347874040841


@pytest.fixture(autouse=True)
def stand_in(monkeypatch):
    monkeypatch.setattr(GPRSurrogate, "engine_factory", co.ConstraintOracleEngine)


# ---- the fold against truth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nj", (1, 2, 16))
def test_host_logpof_against_truth_on_the_grid(nj):
    got, want = co.host_logpof(nj), co.grid_truth(nj)
    tol, own = co.tolerance(nj)
    err = mes_oracle.error(got, want)
    print(f"J = {nj}: logpof {err / co.ULP:.2f} ulp, log Phi measured {own / co.ULP:.2f} ulp, bound {tol / co.ULP:.2f} ulp")
    assert np.isfinite(own) and err <= tol, (nj, err, tol)
    # the grid holds what it says: z = 40 .. -1e6, s2 = 0 on both sides and on the threshold, both senses, NaN members
    cm, cv, cn, th, sn = co.grid(1)
    with np.errstate(all="ignore"):
        z = sn[0] * (th[0] - cm[0]) / np.sqrt(np.maximum(cv[0] - cn[0], 0.0))
    assert np.nanmax(z[np.isfinite(z)]) == 40.0 and np.nanmin(z[np.isfinite(z)]) == -1e6 and set(sn[0]) == {1, -1}
    zero = (cv[0] - cn[0] <= 0.0)
    for s in (1, -1):
        d = (s * (th[0] - cm[0]))[zero & (sn[0] == s)]
        assert np.any(d > 0) and np.any(d == 0) and np.any(d < 0)
    assert np.isnan(got[-1]) and np.isnan(got[-2]) and np.any(np.isneginf(got)) and np.all(got[~np.isnan(got)] <= 0.0)
    with np.errstate(invalid="ignore"):
        far = z == -1e6
    assert far.any() and np.all(np.isfinite(got[far])) and np.all(got[far] < -1e11)  # ten sigma and far more: finite, so still ordered


def test_s2_zero_rule_and_nan_members():
    one = np.ones(1)
    for sense, mean, want in ((1, -0.5, 0.0), (1, 0.0, 0.0), (1, 0.5, -np.inf), (-1, 0.5, 0.0), (-1, 0.0, 0.0), (-1, -0.5, -np.inf)):
        lp = HipGPEngine.constrained_fold_host(A.UCBVar(VS), one, one, 0.0, [[mean]], [[1e-3]], [1e-3], [0.0], [sense], "feasibility")[1]
        assert lp[0] == want, (sense, mean)
    # the ordered sum starts at its first term; a NaN anywhere is NaN, also beside a -inf
    cm, cv = np.array([[0.0], [0.5], [np.nan]]), np.array([[1.0], [0.0], [1.0]])
    val, lp = HipGPEngine.constrained_fold_host(A.UCBVar(VS), one, one, 0.0, cm, cv, [0.0] * 3, [0.0] * 3, [1, 1, 1], "gate", -1.0)
    assert np.isnan(lp[0]) and np.isnan(val[0])
    val, lp = HipGPEngine.constrained_fold_host(A.UCBVar(VS), one, one, 0.0, cm[:2], cv[:2], [0.0] * 2, [0.0] * 2, [1, 1], "gate", -1.0)
    assert lp[0] == -np.inf and val[0] == -np.inf
    # far in the tail the order of two leaves survives
    lp = HipGPEngine.constrained_fold_host(A.UCBVar(VS), np.ones(2), np.ones(2), 0.0, [[10.0, 10.5]], [[1.0, 1.0]], [0.0], [0.0], [1],
                                           "feasibility")[1]
    assert np.all(np.isfinite(lp)) and lp[0] > lp[1] and lp[0] < -50.0


# ---- the mode rules, exactly -------------------------------------------------------------------------------------------
def _columns(seed=0, m=400, nj=3):
    rng = np.random.default_rng(seed)
    mean, var = rng.standard_normal(m), rng.random(m) * 10.0 ** rng.integers(-6, 2, m) + 1e-3
    cm, cv = rng.standard_normal((nj, m)) * 2.0, rng.random((nj, m)) * 10.0 ** rng.integers(-4, 1, (nj, m)) + 2e-3
    cn = np.array([1e-3, 2e-3, 0.0])[:nj]
    thr, sense = rng.standard_normal(nj), np.array([1, -1, 1])[:nj]
    return mean, var, 1e-3, cm, cv, cn, thr, sense


SPECS = {"ucb_var": lambda lat: A.UCBVar(VS), "ucb_std": lambda lat: A.UCBStd(VS, latent=lat), "ei": lambda lat: A.EI(xi=0.01, latent=lat),
         "logei": lambda lat: A.LogEI(xi=0.01, latent=lat), "pi": lambda lat: A.PI(xi=0.01, latent=lat)}


@pytest.mark.parametrize("latent", (False, True))
def test_mode_rules(latent):
    mean, var, noise, cm, cv, cn, thr, sense = _columns()
    lp_ref = HipGPEngine.constrained_fold_host(A.UCBVar(VS), mean, var, noise, cm, cv, cn, thr, sense, "feasibility")[1]
    want = co.truth_logpof(cm, cv, cn, thr, sense)
    assert mes_oracle.error(lp_ref, want) <= co.tolerance(3)[0]
    gate = float(np.median(lp_ref))
    keep = lp_ref >= gate
    assert keep.any() and (~keep).any()
    for kind, make in SPECS.items():
        acq = make(latent)
        a0 = HipGPEngine.acq_eval_host(acq, mean, var, noise, incumbent=0.3)
        # an open gate: gpso_acq_eval_host's bits; a gate: those bits or -inf; feasibility: logpof
        val, lp = HipGPEngine.constrained_fold_host(acq, mean, var, noise, cm, cv, cn, thr, sense, "gate", -np.inf, incumbent=0.3)
        assert np.array_equal(val.view(np.uint64), a0.view(np.uint64)) and np.array_equal(lp.view(np.uint64), lp_ref.view(np.uint64)), kind
        val, lp = HipGPEngine.constrained_fold_host(acq, mean, var, noise, cm, cv, cn, thr, sense, "gate", gate, incumbent=0.3)
        assert np.array_equal(val[keep].view(np.uint64), a0[keep].view(np.uint64)) and np.all(np.isneginf(val[~keep])), kind
        val, lp = HipGPEngine.constrained_fold_host(acq, mean, var, noise, cm, cv, cn, thr, sense, "feasibility", gate, incumbent=0.3)
        assert np.array_equal(val.view(np.uint64), lp_ref.view(np.uint64)), kind
        if kind.startswith("ucb"):
            with pytest.raises(L.GpsoHipError) as err:
                HipGPEngine.constrained_fold_host(acq, mean, var, noise, cm, cv, cn, thr, sense, "weight", gate)
            assert err.value.code == L.E_ARG
            continue
        val, lp = HipGPEngine.constrained_fold_host(acq, mean, var, noise, cm, cv, cn, thr, sense, "weight", gate, incumbent=0.3)
        assert np.all(np.isneginf(val[~keep]))
        if kind == "logei":
            assert np.array_equal(val[keep].view(np.uint64), (a0 + lp_ref)[keep].view(np.uint64))
            continue
        # EI, PI: a0 P(feasible) against the 60-digit product, held to acq_oracle's per-value tolerance and nothing more
        k = AO.KINDS[kind]
        truth = AO.truth(k, mean, var, incumbent=0.3, xi=0.01, s2_add=(-noise,) if latent else ())
        import mpmath as mp

        prod = [t * mp.exp(w) for t, w in zip(truth, want)]
        tol = AO.tolerance(k)[0]
        worst = 0.0
        for j in np.flatnonzero(keep):
            scale = max(abs(prod[j]), mp.mpf(2) ** -1022)
            e = float(abs(mp.mpf(float(val[j])) - prod[j]) / scale)
            worst = max(worst, e / tol)
        print(f"{kind} latent={latent}: weight mode worst error / tolerance = {worst:.3f}")
        assert worst <= 1.0, (kind, worst)
    with pytest.raises(L.GpsoHipError) as err:  # MES
        HipGPEngine.constrained_fold_host(A.MES(), mean, var, noise, cm, cv, cn, thr, sense, "gate", gate)
    assert err.value.code == L.E_ARG
    for bad in (dict(mode=7), dict(log_pof_min=0.5), dict(log_pof_min=np.nan)):
        with pytest.raises(L.GpsoHipError):
            HipGPEngine.constrained_fold_host(A.EI(), mean, var, noise, cm, cv, cn, thr, sense, **{"mode": "gate", "incumbent": 0.0, **bad})
    with pytest.raises(L.GpsoHipError):
        HipGPEngine.constrained_fold_host(A.EI(), mean, var, noise, cm, cv, cn, thr, [1, 0, 1], "gate", incumbent=0.0)


# ---- the Python layer -----------------------------------------------------------------------------------------------
def test_constraint_validates_its_bounds():
    assert (Constraint("rate", upper=40.0).sense, Constraint("rate", upper=40.0).threshold) == (1, 40.0)
    assert (Constraint("margin", lower=0.1).sense, Constraint("margin", lower=0.1).lower, Constraint("margin", lower=0.1).upper) == (-1, 0.1, None)
    for kw in (dict(), dict(upper=1.0, lower=0.0), dict(upper=np.inf), dict(lower=np.nan)):
        with pytest.raises(ValueError):
            Constraint("c", **kw)
    assert list(Constraint("c", upper=1.0).satisfied([0.5, 1.0, 1.5])) == [True, True, False]
    assert list(Constraint("c", lower=1.0).satisfied([0.5, 1.0, 1.5])) == [False, True, True]
    assert list(feasible_rows([Constraint("a", upper=1.0), Constraint("b", lower=0.0)], [[0.5, 0.5], [0.5, -1.0], [2.0, 1.0]])) == [True, False, False]
    for kw in (dict(mode="soft"), dict(pof_min=1.5), dict(pof_min=-0.1)):
        with pytest.raises(ValueError):
            ConstrainedAcq(A.EI(), **kw)
    assert ConstrainedAcq(A.EI(), pof_min=0.0).log_pof_min == -np.inf and ConstrainedAcq(A.EI(), pof_min=0.5).log_pof_min == np.log(0.5)


def _surrogate(cons, **kw):
    return GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy(),
                        constraints=cons, **kw)


def test_side_store_survives_deduplication_and_highest_feasible_score():
    cons = [Constraint("a", upper=1.0), Constraint("b", lower=0.0)]
    surr = _surrogate(cons)
    x = np.array([[0.1, 0.2], [0.5, 0.5], [0.9, 0.3]])
    with pytest.raises(ValueError, match="constraint_values"):
        surr.append(x, np.array([1.0, 3.0, 2.0]))
    with pytest.raises(ValueError, match="shape"):
        surr.append(x, np.array([1.0, 3.0, 2.0]), constraint_values=np.zeros((3, 1)))
    # a gp-based point is replaced by its evaluation in place: the values ride with the coordinates
    from pygpso_amd import GPPoint

    surr.points.append(GPPoint(np.array([0.5, 0.5]), 0.0, 1.0, 2.0, PointLabels.gp_based))
    surr.points.append(GPPoint(np.array([0.7, 0.7]), 0.0, 1.0, 2.0, PointLabels.gp_based))
    surr.append(x, np.array([1.0, 3.0, 2.0]), constraint_values=np.array([[0.5, 0.5], [2.0, 0.5], [0.5, 0.1]]))
    assert surr.num_evaluated == 3 and surr.num_gp_based == 1 and surr.points[0].label == PointLabels.evaluated
    xt, yt = surr.current_training_data
    assert np.array_equal(xt, x[[1, 0, 2]]) and np.array_equal(yt, [3.0, 1.0, 2.0])
    assert np.array_equal(surr.current_training_constraints, [[2.0, 0.5], [0.5, 0.5], [0.5, 0.1]])
    # an evaluated duplicate keeps its score and its values; a near-duplicate within the tolerance too
    surr.append(x[:1] + 1e-14, np.array([9.0]), constraint_values=np.array([[9.0, 9.0]]))
    assert surr.num_evaluated == 3 and np.array_equal(surr.current_training_constraints, [[2.0, 0.5], [0.5, 0.5], [0.5, 0.1]])
    assert surr.highest_score.score_mu == 3.0  # infeasible: a = 2 > 1
    assert surr.highest_feasible_score.score_mu == 2.0
    copy = type(surr.points)(surr.points)
    assert np.array_equal(copy.constraint_matrix(PointLabels.evaluated), surr.current_training_constraints)
    none = _surrogate([Constraint("a", upper=-5.0)])
    none.append(x, np.array([1.0, 3.0, 2.0]), constraint_values=np.zeros((3, 1)))
    assert none.highest_feasible_score is None
    plain = _surrogate(None)
    plain.append(x, np.array([1.0, 3.0, 2.0]))
    assert plain.highest_feasible_score.score_mu == 3.0 and plain.current_training_constraints is None
    with pytest.raises(ValueError):
        plain.append(x, np.array([1.0, 3.0, 2.0]), constraint_values=np.zeros((3, 1)))
    for kw in (dict(dtype="float32"), dict(devices=[0, 1]), dict(refit_every=3), dict(hyper="marginal"), dict(constraint_mode="weight"),
               dict(pof_min=2.0)):
        with pytest.raises(ValueError):
            _surrogate(cons, **kw)
    with pytest.raises(ValueError, match="not saved"):
        surr.save("/nonexistent")


# ---- the loop ---------------------------------------------------------------------------------------------------------
BOUNDS = [[-3.0, 5.0], [-3.0, 3.0]]


EDGE = 1.5


def _c_of(x):
    """The constrained output: smooth and monotone in x alone, zero on the line x = EDGE -- with ``upper=0`` the half-plane
    x > EDGE is infeasible (bounded and curved: an exactly linear output has no finite best lengthscale)."""
    return float(2.0 * np.tanh(x - EDGE))


def _objective(point):
    """The rotated peaks of the loop tests with one constrained output."""
    from tests.helpers import rotated_peaks

    return rotated_peaks(point), _c_of(point[0])


def _run(pof_min, budget=12, upper=0.0, depth=1):
    """exploration_depth = 1: a leaf is scored at its centre alone, so the gate a leaf passed is the gate of the point the
    loop evaluates (with a deeper sub-tree a leaf carries the value of its best sub-leaf, as in the unconstrained loop, and
    is evaluated at its centre).  The objective records, for every point it is asked about once models exist, the ORACLE's
    probability of feasibility under the constraint model the leaf was ranked by."""
    from oracle import gpr

    cons = [Constraint("x", upper=upper)]
    surr = _surrogate(cons, pof_min=pof_min)
    seen = []

    def objective(point):
        if surr._constraint_models is not None:
            post = surr._constraint_models[0].engine.post
            xn = (np.asarray(point, dtype=np.float64) - np.array(BOUNDS)[:, 0]) / (np.array(BOUNDS)[:, 1] - np.array(BOUNDS)[:, 0])
            cm, cv = gpr.predict_y(post, xn[None])
            seen.append((float(point[0]), float(np.exp(co.log_pof_numpy([cm], [cv], [post.theta.noise], [upper], [1])[0]))))
        return _objective(point)

    space = ParameterSpace(parameter_names=["x", "y"], parameter_bounds=BOUNDS)
    opt = GPSOptimiser(parameter_space=space, gp_surrogate=surr, exploration_method="tree", exploration_depth=depth, budget=budget,
                       stopping_condition="iterations", update_cycle=1, n_workers=1)
    best = opt.run(objective, constraints=cons)
    return opt, surr, best, seen


def test_loop_never_evaluates_a_gated_leaf():
    pof_min = 0.5
    opt, surr, best, seen = _run(pof_min)
    assert opt.iterations == 12 and surr._constraints_live and surr.gpflow_model.constraint_count() == 1
    ev = [p for p in surr.points if p.label == PointLabels.evaluated]
    n_init = 2 * 2 + 1
    assert len(seen) == len(ev) - n_init and len(seen) >= 8
    x = np.array([p.normed_coord for p in ev])
    orig = np.array([BOUNDS[0][0] + x[:, 0] * (BOUNDS[0][1] - BOUNDS[0][0])]).T
    assert np.allclose(surr.current_training_constraints[:, 0], [_c_of(v) for v in orig[:, 0]])  # the objective's second output
    # no evaluated point beyond the initial samples lies where the oracle's PoF is below pof_min
    print("evaluated beyond the initial design: (x, oracle PoF) =", [(round(a, 3), round(b, 4)) for a, b in seen])
    assert all(pof >= pof_min for _, pof in seen)
    assert any(px > 0.0 for px, _ in seen)  # (the search did go towards the edge, not only away from it)
    assert best is surr.highest_feasible_score and best is not None and best.score_mu <= surr.highest_score.score_mu
    assert BOUNDS[0][0] + best.normed_coord[0] * 8.0 <= EDGE
    # gated gp-based points carry -inf and were never turned into evaluations
    gated = [p for p in surr.points if p.label == PointLabels.gp_based and p.score_ucb == -np.inf]
    assert gated, "the infeasible half-plane must hold gated leaves"
    # the surrogate's calls go through the constrained ones
    leaves = np.random.default_rng(1).random((50, 2))
    cols = surr.gpflow_model.constrained_acq_values(leaves, ConstrainedAcq(A.UCBVar(surr.gp_varsigma), "gate", pof_min))
    mean, var, ucb = surr.gp_eval_best_ucb(leaves)
    j = int(np.argmax(cols[2]))
    assert (mean, var, ucb) == (cols[0][j], cols[1][j], cols[2][j])
    assert np.array_equal(surr.gp_acq_values(leaves, "ucb_var")[2], cols[2])
    # EI improves on the best score observed feasible, not on the largest one
    inc = surr.highest_feasible_score.score_mu
    idx, _, _, value, logpof = surr.constrained_select(leaves, "ei", "weight")
    w = surr.gpflow_model.constrained_acq_values(leaves, ConstrainedAcq(A.EI(), "weight", pof_min), incumbent=inc)
    assert np.array_equal(surr.gp_acq_values(leaves, "ei")[2], surr.gpflow_model.constrained_acq_values(
        leaves, ConstrainedAcq(A.EI(), "gate", pof_min), incumbent=inc)[2])
    assert np.array_equal(surr.gp_acq_values(leaves, "ei", incumbent=0.25)[2], surr.gpflow_model.constrained_acq_values(
        leaves, ConstrainedAcq(A.EI(), "gate", pof_min), incumbent=0.25)[2])
    assert int(idx[0]) == int(np.argmax(w[2])) and value[0] == w[2].max() and logpof[0] == w[3][int(idx[0])]
    for fn in (lambda: surr.select_batch(leaves, 2), lambda: surr.gp_eval_best_acq(leaves, "mes"), lambda: surr.mes_select(leaves)):
        with pytest.raises(ValueError, match="constraints"):
            fn()
    with pytest.raises(ValueError, match="not saved"):
        opt.save_state("/nonexistent")
    # a deeper sub-tree: the grown leaves go through one constrained call, one segment per box
    opt3, surr3, best3, _ = _run(pof_min, budget=4, depth=3)
    assert opt3.iterations == 4 and best3 is not None


def test_all_gated_run_ends_with_the_warning(caplog):
    # feasible nowhere (c >= -2 everywhere, the bound is -2.5): every leaf is gated at the first selection
    with caplog.at_level(logging.WARNING):
        opt, surr, best, seen = _run(0.999, budget=50, upper=-2.5)
    assert opt.iterations < 50 and not seen
    assert any("pof_min=0.999" in r.getMessage() for r in caplog.records)
    assert best is None


def test_run_refuses_what_does_not_go_with_constraints():
    cons = [Constraint("x", upper=1.0)]
    space = ParameterSpace(parameter_names=["x", "y"], parameter_bounds=BOUNDS)

    class Saver:
        def save_runs(self, *a):
            pass

    for surr, okw, rkw in ((_surrogate(cons), dict(saver=Saver()), {}), (_surrogate(cons), {}, dict(eval_repeats=2, eval_repeats_noise=True)),
                           (_surrogate(None), {}, {}), (_surrogate(None, refit_every=3), {}, {}), (_surrogate(None, hyper="marginal"), {}, {}),
                           (_surrogate([Constraint("x", upper=2.0)]), {}, {})):
        opt = GPSOptimiser(parameter_space=space, gp_surrogate=surr, budget=3, stopping_condition="iterations", **okw)
        with pytest.raises(ValueError):
            opt.run(_objective, constraints=cons, **rkw)
    opt = GPSOptimiser(parameter_space=space, gp_surrogate=_surrogate(cons), budget=3, stopping_condition="iterations")
    with pytest.raises(ValueError, match="constraints"):
        opt.run(_objective)  # the surrogate has them, run was not told
    with pytest.raises(ValueError, match="must return"):
        opt.run(lambda p: 1.0, constraints=cons)
