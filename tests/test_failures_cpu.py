"""CPU-only checks of ``failures="classify"`` over the CPU stand-in engine of tests/failures_oracle.py:
the surrogate's store of failed points, the classifier's training set, the gate by the probability of success in the
optimiser's loop, and the refusals."""
import logging

import numpy as np
import pytest

from pygpso_amd import GPRSurrogate, GPSOptimiser, ParameterSpace, PointLabels, VGPSurrogate
from pygpso_amd import acquisition as A
from pygpso_amd import kernels as K
from pygpso_amd.constraints import ConstrainedAcq, Constraint
from tests.failures_oracle import FailuresOracleEngine
from tests.helpers import rotated_peaks

BOUNDS = [[-3.0, 5.0], [-3.0, 3.0]]
EDGE = 1.5  # the objective returns NaN on the half-plane x > EDGE


@pytest.fixture(autouse=True)
def stand_in(monkeypatch):
    monkeypatch.setattr(GPRSurrogate, "engine_factory", FailuresOracleEngine)


def _surrogate(**kw):
    return GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy(), **kw)


def _optimiser(surr, budget=12, depth=1, **kw):
    space = ParameterSpace(parameter_names=["x", "y"], parameter_bounds=BOUNDS)
    return GPSOptimiser(parameter_space=space, gp_surrogate=surr, exploration_method="tree", exploration_depth=depth, budget=budget,
                        stopping_condition="iterations", update_cycle=1, n_workers=1, **kw)


def _failing(point):
    return float("nan") if point[0] > EDGE else rotated_peaks(point)


# ---- the store ---------------------------------------------------------------------------------------------------------
def test_append_keeps_failed_points_out_of_the_training_set():
    surr = _surrogate(failures="classify")
    x = np.array([[0.1, 0.2], [0.5, 0.5], [0.9, 0.3], [0.8, 0.8]])
    with pytest.raises(ValueError, match="no finite score"):
        surr.append(x[:2], np.array([np.nan, np.inf]))
    assert surr.num_evaluated == 0
    surr.append(x, np.array([1.0, np.nan, 2.0, -np.inf]))
    assert surr.num_evaluated == 4 and surr.num_failed == 2
    xt, yt = surr.current_training_data
    assert np.array_equal(xt, x[[0, 2]]) and np.array_equal(yt, [1.0, 2.0])
    xa, lab = surr.current_attempts
    assert np.array_equal(xa, x) and np.array_equal(lab, [1.0, 0.0, 1.0, 0.0])
    assert surr.highest_score.score_mu == 2.0
    # with a finite score held, a call that brings failures only is served; an evaluated duplicate keeps what it has
    surr.append(np.array([[0.3, 0.3], [0.1, 0.2]]), np.array([np.nan, np.nan]))
    assert surr.num_evaluated == 5 and surr.num_failed == 3 and np.array_equal(surr.current_training_data[1], [1.0, 2.0])
    # a gp-based point is replaced in place by its failed evaluation
    from pygpso_amd import GPPoint

    surr.points.append(GPPoint(np.array([0.6, 0.6]), 0.0, 1.0, 2.0, PointLabels.gp_based))
    surr.append(np.array([[0.6, 0.6]]), np.array([np.nan]))
    assert surr.num_gp_based == 0 and surr.num_failed == 4
    copy = type(surr.points)(surr.points)
    assert np.array_equal(copy.failed_mask(PointLabels.evaluated), surr.points.failed_mask(PointLabels.evaluated))
    with pytest.raises(ValueError, match="not saved"):
        surr.save("/nonexistent")
    # the default surrogate is as it was: a non-finite score is stored as a score
    plain = _surrogate()
    plain.append(x[:2], np.array([1.0, np.nan]))
    assert plain.num_failed == 0 and plain.current_training_data[0].shape[0] == 2
    for kw in (dict(failures="penalise"), dict(failures="classify", dtype="float32"), dict(failures="classify", devices=[0, 1]),
               dict(failures="classify", refit_every=3), dict(failures="classify", hyper="marginal"), dict(failures="classify", pof_min=2.0),
               dict(failures="classify", classifier_schedule={"steps": 3}), dict(failures="classify", classifier_schedule={"natgrad_gamma": 0.0})):
        with pytest.raises(ValueError):
            _surrogate(**kw)


def test_update_trains_the_classifier_on_all_attempts_and_gates_by_it():
    surr = _surrogate(failures="classify", pof_min=0.5)
    rng = np.random.default_rng(0)
    x = rng.random((12, 2))
    y = np.array([rotated_peaks(np.array([-3.0 + 8.0 * a, -3.0 + 6.0 * b])) for a, b in x])
    # before the first failure: no classifier, no member, every call is the default's
    surr.append(x[:6], y[:6])
    surr.gp_update()
    assert surr._classifier is None and not surr._success_live and not surr._gate_live
    ref = _surrogate()
    ref.append(x[:6], y[:6])
    ref.gp_update()
    leaves = rng.random((40, 2))
    assert surr.gp_eval_best_ucb(leaves) == ref.gp_eval_best_ucb(leaves)
    # two failures among twelve
    y2 = y.copy()
    y2[[7, 10]] = np.nan
    surr.append(x[6:], y2[6:])
    surr.gp_update()
    assert surr._success_live and surr.gpflow_model.engine.success_info()[:2] == (True, 12)
    assert surr.gpflow_model.data[0].shape[0] == 10 and np.all(np.isfinite(surr.gpflow_model.data[1]))
    cx, cy = surr._classifier.data
    assert np.array_equal(cx, surr.current_attempts[0]) and np.array_equal(cy[:, 0], surr.current_attempts[1]) and cy.sum() == 10.0
    # the classifier has its own engine and its own copies of the specs
    assert surr._classifier.engine is not surr.gpflow_model.engine and surr._classifier.kernel is not surr.gp_kernel
    # the routes go through the constrained calls, in gate mode on the probability of success
    cols = surr.gpflow_model.constrained_acq_values(leaves, ConstrainedAcq(A.UCBVar(surr.gp_varsigma), "gate", 0.5))
    prob = np.asarray(surr._classifier.predict_prob(leaves)[0])[:, 0]
    np.testing.assert_allclose(np.exp(cols[3]), prob, rtol=1e-12)
    assert np.array_equal(np.isneginf(cols[2]), cols[3] < np.log(0.5))
    med = float(np.median(np.exp(cols[3])))  # (two failures among twelve gate little at 0.5: a gate at the median shows both sides)
    gated = surr.gpflow_model.constrained_acq_values(leaves, ConstrainedAcq(A.UCBVar(surr.gp_varsigma), "gate", med))[2]
    assert np.array_equal(np.isneginf(gated), cols[3] < np.log(med)) and np.isneginf(gated).any() and np.isfinite(gated).any()
    mean, var, ucb = surr.gp_eval_best_ucb(leaves)
    j = int(np.argmax(cols[2]))
    assert (mean, var, ucb) == (cols[0][j], cols[1][j], cols[2][j])
    assert np.array_equal(surr.gp_acq_values(leaves, "ucb_var")[2], cols[2])
    for fn in (lambda: surr.select_batch(leaves, 2), lambda: surr.gp_eval_best_acq(leaves, "mes"), lambda: surr.mes_select(leaves)):
        with pytest.raises(ValueError, match="failures"):
            fn()
    # a further update keeps q of the held rows (the model's rows stay in their order of arrival)
    surr.append(np.array([[0.33, 0.77]]), np.array([np.nan]))
    surr.gp_update()
    assert surr._classifier.q_carried and surr.gpflow_model.engine.success_info()[1] == 13
    surr.close_constraint_models()  # (an engine that came from ``engine_factory`` is the factory's to close, as the constraint models')
    assert surr._classifier is None


# ---- the loop ----------------------------------------------------------------------------------------------------------
def _run(pof_min=0.5, budget=12, objective=_failing, **kw):
    """exploration_depth = 1: a leaf is scored at its centre alone, so the gate a leaf passed is the gate of the point the loop
    evaluates.  The objective records, for every point it is asked about once a classifier is installed, the classifier's
    probability of success there (the posterior the leaf was ranked by)."""
    surr = _surrogate(failures="classify", pof_min=pof_min, **kw)
    seen = []
    lo, hi = np.array(BOUNDS)[:, 0], np.array(BOUNDS)[:, 1]

    def wrapped(point):
        if surr._success_live:
            xn = (np.asarray(point, dtype=np.float64) - lo) / (hi - lo)
            seen.append((float(point[0]), float(surr._classifier.engine.bpost.predict_prob(xn[None])[0][0])))
        return objective(point)

    opt = _optimiser(surr, budget=budget)
    best = opt.run(wrapped, failures="classify")
    return opt, surr, best, seen


def test_loop_with_an_objective_that_fails_on_a_half_plane():
    pof_min = 0.5
    opt, surr, best, seen = _run(pof_min)
    assert opt.iterations == 12  # the run finishes
    ev = [p for p in surr.points if p.label == PointLabels.evaluated]
    failed = surr.points.failed_mask(PointLabels.evaluated)
    orig_x = np.array([BOUNDS[0][0] + p.normed_coord[0] * 8.0 for p in ev])
    assert failed.any() and np.array_equal(failed, orig_x > EDGE)  # the initial design's x = 3 among them
    # no failed point is in the objective's training set; every attempted point is in the classifier's
    xt, yt = surr.gpflow_model.data
    assert xt.shape[0] == int((~failed).sum()) and np.all(np.isfinite(yt))
    assert not any(np.any(np.all(xt == p.normed_coord, axis=1)) for p, bad in zip(ev, failed) if bad)
    cx, cy = surr._classifier.data
    assert cx.shape[0] == len(ev) and all(np.any(np.all(cx == p.normed_coord, axis=1)) for p in ev)
    assert np.array_equal(np.sort(cy[:, 0]), np.sort((~failed).astype(float)))
    # a gated leaf is never evaluated: every evaluation made under a classifier passed its gate
    print("evaluated under the classifier: (x, P(success)) =", [(round(a, 3), round(b, 4)) for a, b in seen])
    assert len(seen) >= 6 and all(p >= pof_min for _, p in seen)
    gated = [p for p in surr.points if p.label == PointLabels.gp_based and p.score_ucb == -np.inf]
    assert gated, "the failing half-plane must hold gated leaves"
    # failed leaves are evaluated, worth -inf and never split
    nodes = [n for n in opt.param_space.iter_preorder() if n.label == PointLabels.evaluated and n.score == -np.inf]
    assert nodes and not any(n.sampled for n in nodes if not n.children)
    # run returns the best finite score
    assert best is surr.highest_score and np.isfinite(best.score_mu) and best.score_mu == max(p.score_mu for p, b in zip(ev, failed) if not b)
    with pytest.raises(ValueError, match="not saved"):
        opt.save_state("/nonexistent")


def test_never_failing_objective_reproduces_the_default_run():
    opt, surr, best, seen = _run(objective=rotated_peaks, budget=8)
    assert not seen and surr._classifier is None and surr.num_failed == 0
    ref = _surrogate()
    ropt = _optimiser(ref, budget=8)
    rbest = ropt.run(rotated_peaks)
    a = [p for p in surr.points if p.label == PointLabels.evaluated]
    b = [p for p in ref.points if p.label == PointLabels.evaluated]
    assert len(a) == len(b) and len(a) > 8
    for p, q in zip(a, b):
        assert np.array_equal(p.normed_coord, q.normed_coord) and float(p.score_mu).hex() == float(q.score_mu).hex()
    assert best.score_mu == rbest.score_mu


def test_repeats_with_one_failure_fail_the_evaluation():
    count = [0]

    def flaky(point):
        count[0] += 1
        return float("inf") if (point[0] > EDGE and count[0] % 2 == 0) else rotated_peaks(point)

    surr = _surrogate(failures="classify")
    opt = _optimiser(surr, budget=2)
    opt.run(flaky, failures="classify", eval_repeats=2, eval_repeats_function=np.max)
    ev = [p for p in surr.points if p.label == PointLabels.evaluated]
    failed = surr.points.failed_mask(PointLabels.evaluated)
    assert failed.any() and all((BOUNDS[0][0] + p.normed_coord[0] * 8.0 > EDGE) == bad for p, bad in zip(ev, failed))


def test_failures_together_with_constraints():
    cons = [Constraint("x", upper=0.0)]  # 2 tanh(x - EDGE) <= 0: the half-plane x > EDGE is infeasible; y > 1 fails

    def objective(point):
        if point[1] > 1.0:
            return float("nan"), float("nan")
        return rotated_peaks(point), float(2.0 * np.tanh(point[0] - EDGE))

    surr = _surrogate(failures="classify", constraints=cons, pof_min=0.5)
    opt = _optimiser(surr, budget=8)
    best = opt.run(objective, constraints=cons, failures="classify")
    assert opt.iterations == 8 and surr._constraints_live and surr._success_live
    failed = surr.points.failed_mask(PointLabels.evaluated)
    assert failed.any() and surr.current_training_constraints.shape == (int((~failed).sum()), 1)
    assert surr._constraint_models[0].data[0].shape[0] == int((~failed).sum())
    assert best is surr.highest_feasible_score and best is not None and np.isfinite(best.score_mu)
    assert -3.0 + 6.0 * best.normed_coord[1] <= 1.0 and BOUNDS[0][0] + 8.0 * best.normed_coord[0] <= EDGE
    # logpof is the constraints' term plus the success term
    leaves = np.random.default_rng(2).random((30, 2))
    cols = surr.gpflow_model.constrained_acq_values(leaves, ConstrainedAcq(A.UCBVar(surr.gp_varsigma), "feasibility", 0.5), want_members=True)
    assert cols[4].shape == (2, 30)  # one constraint model, then the success member's latent columns
    from pygpso_amd import HipGPEngine

    term = HipGPEngine.success_prob_host(cols[4][1], cols[5][1])[1]
    base = HipGPEngine.constrained_fold_host(A.UCBVar(surr.gp_varsigma), cols[0], cols[1], 0.0, cols[4][:1], cols[5][:1],
                                             [surr._constraint_models[0].engine.post.theta.noise], [0.0], [1], "feasibility")[1]
    assert np.array_equal(cols[3], base + term)


def test_all_gated_run_ends_with_the_warning(caplog):
    # everything but the centre fails: the classifier gates every leaf once it has seen the initial design
    def objective(point):
        return rotated_peaks(point) if (abs(point[0] - 1.0) < 1e-9 and abs(point[1]) < 1e-9) else float("nan")

    with caplog.at_level(logging.WARNING):
        opt, surr, best, seen = _run(0.9, budget=50, objective=objective)
    assert opt.iterations < 50
    assert any("pof_min=0.9" in r.getMessage() for r in caplog.records)
    assert best is surr.highest_score and np.isfinite(best.score_mu)


# ---- the refusals ------------------------------------------------------------------------------------------------------
def test_run_refuses_what_does_not_go_with_failures():
    class Saver:
        def save_runs(self, *a):
            pass

    vgp = VGPSurrogate(gp_kernel=K.Matern52(lengthscales=0.25, variance=1.0), gp_meanf=K.Constant(0.0))
    cases = ((_surrogate(failures="classify"), dict(saver=Saver()), {}, "saver"),
             (_surrogate(failures="classify"), {}, dict(eval_repeats=2, eval_repeats_noise=True), "eval_repeats_noise"),
             (_surrogate(refit_every=3), {}, {}, "refit_every"),
             (_surrogate(hyper="marginal"), {}, {}, "hyper"),
             (vgp, {}, {}, "GPRSurrogate"),
             (_surrogate(), {}, {}, "GPRSurrogate\\(failures='classify'\\)"))
    for surr, okw, rkw, words in cases:
        opt = _optimiser(surr, budget=3, **okw)
        with pytest.raises(ValueError, match=words):
            opt.run(_failing, failures="classify", **rkw)
    space = ParameterSpace(parameter_names=["x", "y"], parameter_bounds=BOUNDS)
    sampler = GPSOptimiser(parameter_space=space, gp_surrogate=_surrogate(failures="classify"), exploration_method="sample", budget=3,
                           stopping_condition="iterations")
    with pytest.raises(ValueError, match="tree exploration"):  # (as constraints: only the tree's loop gates its leaves)
        sampler.run(_failing, failures="classify")
    opt = _optimiser(_surrogate(failures="classify"), budget=3)
    with pytest.raises(ValueError, match="failures='classify'"):
        opt.run(_failing)  # the surrogate has it, run was not told
    with pytest.raises(ValueError, match="None or 'classify'"):
        opt.run(_failing, failures="penalise")
