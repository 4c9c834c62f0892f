"""
Multi-start hyper-parameter search (``Scipy(restarts=R)``), host side: the resumable L-BFGS-B state, the lockstep driver,
the winner rule, failures, fallbacks and persistence -- on a stand-in model over the float64 oracle (no GPU).
"""
import json
import os

import numpy as np
import pytest

from oracle import gpr
from pygpso_amd.kernels import Constant, Matern52, Scipy
from tests.multistart_problem import KERNEL, OracleModel, oracle_multistart, problem


def _alone(u):
    X, y, _, _ = problem()
    return Scipy._lbfgsb_direct(lambda v: gpr.loss_and_grad_unconstrained(KERNEL, v, X, y), u)


def test_every_search_of_a_lockstep_run_is_the_search_run_alone_bit_for_bit():
    X, y, u0, starts = problem()
    all_starts = np.vstack([u0[None], starts])
    model = OracleModel(X, y, u0)
    searches = Scipy._lockstep(model._loss_and_grad_batch, all_starts)
    assert searches is not None and len(searches) == 4
    assert model.single_calls == 0 and model.batch_calls >= max(s.nfev for s in searches)
    for s, u in zip(searches, all_starts):
        ref = _alone(u)
        got = s.result()
        assert got.x.tobytes() == ref.x.tobytes()
        assert np.float64(got.fun).tobytes() == np.float64(ref.fun).tobytes()
        assert (got.nfev, got.nit, got.status) == (ref.nfev, ref.nit, ref.status)
        assert got.jac.tobytes() == ref.jac.tobytes()


def test_restarts_1_is_the_default_object_and_never_calls_the_batch():
    X, y, u0, _ = problem()
    a, b = OracleModel(X, y, u0), OracleModel(X, y, u0)
    ra = Scipy().minimize(a.training_loss)
    rb = Scipy(restarts=1).minimize(b.training_loss)
    assert a.batch_calls == 0 and b.batch_calls == 0
    assert ra.x.tobytes() == rb.x.tobytes() == _alone(u0).x.tobytes()
    assert (ra.nfev, ra.nit) == (rb.nfev, rb.nit) and a.single_calls == b.single_calls == ra.nfev
    assert "restarts" not in ra and "restarts" not in rb
    assert a.u.tobytes() == b.u.tobytes() == ra.x.tobytes()


def test_the_restart_that_reaches_the_lower_optimum_wins():
    """Start 0 (the surrogate's default theta) ends at NLML 10.2897, start 1 at 10.1524: more than 1e-3 apart, and the
    multi-start returns the lower one."""
    X, y, u0, starts = problem()
    res = oracle_multistart()
    f0, f1 = _alone(u0).fun, _alone(starts[0]).fun
    assert f0 - f1 >= 1e-3
    assert [r["nfev"] for r in res.restarts] == [_alone(u).nfev for u in np.vstack([u0[None], starts])]
    assert res.winner == int(np.argmin([r["fun"] for r in res.restarts])) != 0
    assert res.fun == res.restarts[res.winner]["fun"] == min(r["fun"] for r in res.restarts) <= f1
    model = OracleModel(X, y, u0)
    again = Scipy(restarts=4, starts=starts).minimize(model.training_loss)
    assert model.u.tobytes() == again.x.tobytes() == res.x.tobytes()  # assigned, and reproducible
    assert model.single_calls == 0


def test_ties_go_to_the_lowest_index():
    X, y, u0, starts = problem()
    model = OracleModel(X, y, u0)
    res = Scipy(restarts=4, starts=np.stack([starts[1], starts[0], starts[0]])).minimize(model.training_loss)
    funs = [r["fun"] for r in res.restarts]
    assert funs[2] == funs[3] == min(funs)  # the same search twice: an exact tie at the lowest loss
    assert res.winner == 2


def test_seeded_starts_are_reproducible_and_move_with_the_call_count():
    X, y, u0, _ = problem()
    opt_a, opt_b = Scipy(restarts=3, seed=5), Scipy(restarts=3, seed=5)
    s1 = opt_a._start_points(u0)
    assert s1.shape == (3, 4) and s1[0].tobytes() == u0.tobytes()
    assert s1.tobytes() == opt_b._start_points(u0).tobytes()
    assert np.allclose(s1[1:], u0 + np.random.default_rng([5, 0]).standard_normal((2, 4)))
    opt_a.minimize(OracleModel(X, y, u0).training_loss)
    assert opt_a.minimize_calls == 1 and opt_a._start_points(u0).tobytes() != s1.tobytes()
    assert Scipy(restarts=3, seed=5, restart_scale=0.0)._start_points(u0)[2].tobytes() == u0.tobytes()


def test_a_restart_whose_evaluation_fails_is_dropped_and_the_rest_finish():
    X, y, u0, starts = problem()
    bad = starts[1]
    model = OracleModel(X, y, u0, fail=lambda u: np.array_equal(u, bad))
    res = Scipy(restarts=4, starts=starts).minimize(model.training_loss)
    ref = oracle_multistart()
    assert res.restarts[2]["status"] == "not positive definite" and np.isnan(res.restarts[2]["fun"])
    for i in (0, 1, 3):
        assert res.restarts[i] == ref.restarts[i]
    assert res.winner == ref.winner and res.x.tobytes() == ref.x.tobytes()


def test_start_0_failing_raises_linalgerror():
    X, y, u0, starts = problem()
    model = OracleModel(X, y, u0, fail=lambda u: np.array_equal(u, u0))
    with pytest.raises(np.linalg.LinAlgError):
        Scipy(restarts=4, starts=starts).minimize(model.training_loss)
    assert model.u.tobytes() == u0.tobytes()  # nothing assigned


def test_start_0_failing_escalates_and_the_whole_multistart_begins_again():
    X, y, u0, starts = problem()
    state = {"broken": True}
    model = OracleModel(X, y, u0, fail=lambda u: state["broken"] and np.array_equal(u, u0))

    def escalate(err, fit=False):
        state["broken"] = False
        return True

    model._escalate = escalate
    res = Scipy(restarts=4, starts=starts).minimize(model.training_loss)
    assert model.fit_escalations == 1
    assert res.restarts == oracle_multistart().restarts


def test_a_model_without_a_batched_loss_is_refused_for_two_restarts():
    X, y, u0, _ = problem()
    model = OracleModel(X, y, u0, with_batch=False)
    with pytest.raises(NotImplementedError, match="restarts"):
        Scipy(restarts=2).minimize(model.training_loss)
    assert Scipy(restarts=1).minimize(model.training_loss).nfev == _alone(u0).nfev
    from pygpso_amd.sgpr import HipSGPR
    from pygpso_amd.vgp import HipVGP

    assert HipVGP._loss_and_grad_batch is None and HipSGPR._loss_and_grad_batch is None


def test_another_scipy_runs_the_starts_one_after_another(monkeypatch):
    """A private routine with another signature: every start goes through scipy.optimize.minimize, same optima."""
    X, y, u0, starts = problem()
    monkeypatch.setattr(Scipy, "_SETULB_DOC", "setulb(something else)")
    model = OracleModel(X, y, u0)
    res = Scipy(restarts=4, starts=starts).minimize(model.training_loss)
    ref = oracle_multistart()
    assert model.batch_calls == 0 and model.single_calls == sum(r["nfev"] for r in res.restarts)
    assert res.winner == ref.winner
    assert [r["nfev"] for r in res.restarts] == [r["nfev"] for r in ref.restarts]
    assert np.allclose([r["fun"] for r in res.restarts], [r["fun"] for r in ref.restarts], rtol=1e-12, atol=0)


def test_bad_arguments():
    with pytest.raises(ValueError):
        Scipy(restarts=0)
    with pytest.raises(ValueError):
        Scipy(restarts=3, starts=np.zeros((1, 4)))
    X, y, u0, _ = problem()
    with pytest.raises(ValueError):
        Scipy(restarts=2, starts=np.zeros((1, 7))).minimize(OracleModel(X, y, u0).training_loss)


def test_save_and_from_saved_round_trip_the_multistart_settings(tmp_path, monkeypatch):
    from pygpso_amd.gp_surrogate import GPRSurrogate
    from tests.oracle_engine import OracleEngine

    monkeypatch.setattr(GPRSurrogate, "engine_factory", OracleEngine)
    X, y, _, _ = problem()

    def surrogate(opt):
        s = GPRSurrogate(gp_kernel=Matern52(lengthscales=0.25, variance=1.0), gp_meanf=Constant(0.0), optimiser=opt)
        s.append(X, y)
        s._gp_train(X, y[:, None])
        return s

    multi = surrogate(Scipy(restarts=3, restart_scale=0.5, seed=11))
    assert multi.optimiser.last_result.winner in (0, 1, 2) and len(multi.optimiser.last_result.restarts) == 3
    folder = str(tmp_path / "multi")
    multi.save(folder)
    back = GPRSurrogate.from_saved(folder)
    assert (back.optimiser.restarts, back.optimiser.restart_scale, back.optimiser.seed) == (3, 0.5, 11)

    plain = surrogate(Scipy())
    folder = str(tmp_path / "plain")
    plain.save(folder)
    with open(os.path.join(folder, GPRSurrogate.GPR_INFO)) as fh:
        assert json.load(fh)["optimiser"] == ["Scipy"]  # the record of before: a file without the settings
    back = GPRSurrogate.from_saved(folder)
    assert (back.optimiser.restarts, back.optimiser.restart_scale, back.optimiser.seed) == (1, 1.0, 0)
