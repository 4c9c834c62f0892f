"""CPU-only checks of the acquisition functions: the maps of csrc/acq.hpp through ``gpso_acq_eval_host`` against the
60-digit truth of tests/acq_oracle.py, and the host layers (surrogate keyword, point scores, save / load, polish) over the
CPU stand-in engine."""
import json
import os
from shutil import rmtree

import numpy as np
import pytest

from pygpso_amd import GPRSurrogate, GPSOptimiser, HipGPEngine, ParameterSpace, PointLabels
from pygpso_amd import acquisition as A
from pygpso_amd import kernels as K
from tests import acq_oracle as AO
from tests.acq_oracle import AcqOracleEngine
from tests.helpers import kat_fixture, rotated_peaks

TMP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_tmp_acq")
SPECS = {AO.EI: A.EI, AO.LOGEI: A.LogEI, AO.PI: A.PI}


@pytest.fixture(autouse=True)
def stand_in(monkeypatch):
    monkeypatch.setattr(GPRSurrogate, "engine_factory", AcqOracleEngine)
    yield
    if os.path.isdir(TMP):
        rmtree(TMP)


# ---- the maps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [AO.EI, AO.LOGEI, AO.PI])
def test_host_maps_against_truth_on_the_grid(kind):
    mean, s2, inc = AO.grid()
    got = HipGPEngine.acq_eval_host(SPECS[kind](incumbent=inc), mean, s2)
    tol, yard = AO.tolerance(kind)
    err = AO.error(kind, got, AO.grid_truth(kind))
    print(f"kind {kind}: library {err:.3e}, yardstick {yard:.3e}, tolerance {tol:.3e}")
    assert np.isfinite(yard)
    assert err <= tol, (kind, err, tol)


def test_s_zero_and_nan_rules():
    mean, s2 = np.array([0.75, 0.0, -0.75, np.nan, 1.0]), np.array([0.0, 0.0, 0.0, 1.0, np.nan])
    ei = HipGPEngine.acq_eval_host(A.EI(incumbent=0.0), mean, s2)
    le = HipGPEngine.acq_eval_host(A.LogEI(incumbent=0.0), mean, s2)
    pi = HipGPEngine.acq_eval_host(A.PI(incumbent=0.0), mean, s2)
    assert list(ei[:3]) == [0.75, 0.0, 0.0] and list(pi[:3]) == [1.0, 0.5, 0.0]
    assert le[0] == np.log(0.75) and le[1] == -np.inf and le[2] == -np.inf
    for v in (ei, le, pi, HipGPEngine.acq_eval_host(A.UCBStd(2.0), mean, s2)):
        assert np.isnan(v[3]) and np.isnan(v[4])
    # a negative variance is clamped; the latent kinds read var - noise
    assert HipGPEngine.acq_eval_host(A.UCBStd(2.0), [1.0], [-1e-9])[0] == 1.0
    lat = HipGPEngine.acq_eval_host(A.UCBStd(2.0, latent=True), [1.0], [0.26], noise=0.01)
    assert lat[0] == 1.0 + 2.0 * np.sqrt(0.26 - 0.01)


def test_ucb_kinds_are_numpys_bits():
    rng = np.random.default_rng(5)
    m = rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 6, 4096)
    v = rng.random(4096) * 10.0 ** rng.integers(-12, 4, 4096)
    for vs in (2.326347874040841, 0.1, 7.0):
        assert np.array_equal(HipGPEngine.acq_eval_host(A.UCBVar(vs), m, v), m + vs * v)
        assert np.array_equal(HipGPEngine.acq_eval_host(A.UCBStd(vs), m, v), m + vs * np.sqrt(v))


def test_bad_records_are_refused():
    from pygpso_amd import _lib as L

    for rec in (L.GpsoAcq(9, 0, 1.0, 0.0, 0.0), L.GpsoAcq(-1, 0, 1.0, 0.0, 0.0), L.GpsoAcq(L.ACQ_EI, 0, 0.0, np.inf, 0.0),
                L.GpsoAcq(L.ACQ_PI, 0, 0.0, 0.0, np.nan), L.GpsoAcq(L.ACQ_UCB_STD, 0, np.nan, 0.0, 0.0)):
        class Spec(A.Acquisition):
            def c_struct(self, incumbent=None, rec=rec):
                return rec
        with pytest.raises(L.GpsoHipError) as err:
            HipGPEngine.acq_eval_host(Spec(), [0.0], [1.0])
        assert err.value.code == L.E_ARG
    one = np.zeros(1)
    assert L.load().gpso_acq_eval_host(None, L.dptr(one), L.dptr(one), 0.0, 1, L.dptr(one)) == L.E_ARG
    # (a UCB kind does not read the incumbent: garbage there is not an error)
    assert HipGPEngine.acq_eval_host(A.UCBStd(1.0), [1.0], [4.0], incumbent=np.nan)[0] == 3.0


def test_logei_ranks_where_float64_ei_is_zero():
    """Late in a run: small variances, every leaf far below the incumbent.  Float64 EI is 0.0 on every row (asserted on the
    yardstick), so its arg-max is row 0 by default; log-EI stays finite and picks truth's row."""
    rng = np.random.default_rng(11)
    n = 500
    s2 = (1e-3 * (1.0 + rng.random(n))) ** 2
    mean = -(40.0 + 20.0 * rng.random(n)) * np.sqrt(s2)  # z in [-60, -40]
    assert np.all(AO.yardstick(AO.EI, mean, s2) == 0.0)
    assert np.all(HipGPEngine.acq_eval_host(A.EI(incumbent=0.0), mean, s2) == 0.0)
    got = HipGPEngine.acq_eval_host(A.LogEI(incumbent=0.0), mean, s2)
    want = AO.truth(AO.LOGEI, mean, s2)
    assert np.all(np.isfinite(got))
    best = max(range(n), key=lambda i: want[i])
    assert int(np.argmax(got)) == best and best != 0
    assert AO.error(AO.LOGEI, got, want) <= AO.tolerance(AO.LOGEI)[0]


# ---- the host layers over the stand-in --------------------------------------------------------------------------------
def _space():
    return ParameterSpace(parameter_names=["x", "y"], parameter_bounds=[[-3, 5], [-3, 3]])


def _surrogate(**kw):
    return GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.3, variance=1.0), gp_meanf=K.Constant(0.0), **kw)


def test_optimiser_run_on_ucb_std_stores_the_gp_ucb_bound():
    surr = _surrogate(gp_acquisition="ucb_std")
    opt = GPSOptimiser(parameter_space=_space(), gp_surrogate=surr, exploration_method="tree", exploration_depth=3,
                       budget=20, stopping_condition="evaluations", update_cycle=1, n_workers=1)
    best = opt.run(rotated_peaks)
    assert best.label == PointLabels.evaluated and opt.n_eval_counter >= 20
    based = [p for p in surr.points if p.label == PointLabels.gp_based]
    assert len(based) > 10
    vs = surr.gp_varsigma
    for p in based:
        assert p.score_ucb == p.score_mu + vs * np.sqrt(p.score_sigma)
    # ... and it is not the default rule's run
    ref = GPSOptimiser(parameter_space=_space(), gp_surrogate=_surrogate(), exploration_method="tree", exploration_depth=3,
                       budget=20, stopping_condition="evaluations", update_cycle=1, n_workers=1)
    ref.run(rotated_peaks)
    assert [p.score_ucb for p in ref.gp_surr.points] != [p.score_ucb for p in surr.points]


@pytest.mark.parametrize("name", ["ei", "logei", "pi", A.EI()])
def test_only_score_unit_kinds_drive_the_loop(name):
    with pytest.raises(ValueError, match="score units"):
        _surrogate(gp_acquisition=name)


def test_unknown_acquisition_name():
    with pytest.raises(ValueError, match="unknown acquisition"):
        _surrogate(gp_acquisition="thompson")


def _trained(**kw):
    pts_x = np.array([p[0] for p in kat_fixture() if p[4] == 1])
    pts_y = np.array([p[1] for p in kat_fixture() if p[4] == 1])
    s = _surrogate(**kw)
    s.append(pts_x, pts_y)
    s.gp_update()
    return s


def test_saved_record_carries_the_key_only_when_not_default():
    s = _trained()
    s.save(TMP)
    with open(os.path.join(TMP, _info_file(TMP))) as fh:
        assert "gp_acquisition" not in json.load(fh)
    assert GPRSurrogate.from_saved(TMP).gp_acquisition == "ucb_var"
    rmtree(TMP)
    s = _trained(gp_acquisition="ucb_std")
    s.save(TMP)
    with open(os.path.join(TMP, _info_file(TMP))) as fh:
        assert json.load(fh)["gp_acquisition"] == "ucb_std"
    assert GPRSurrogate.from_saved(TMP).gp_acquisition == "ucb_std"


def _info_file(folder):
    """The surrogate's record: the JSON file of the folder that holds ``gp_varsigma``."""
    for f in sorted(os.listdir(folder)):
        if f.endswith(".json"):
            with open(os.path.join(folder, f)) as fh:
                data = json.load(fh)
            if isinstance(data, dict) and "gp_varsigma" in data:
                return f
    raise AssertionError("no surrogate record in the saved folder")


def test_gp_eval_best_acq_and_values_on_the_stand_in():
    s = _trained()
    xs = np.random.default_rng(2).random((200, 2))
    inc = float(np.max(s.current_training_data[1]))
    for name in ("ucb_var", "ucb_std", "ei", "logei", "pi"):
        mean, var, val = s.gp_acq_values(xs, name)
        idx, mu, vv, best = s.gp_eval_best_acq(xs, name, seg_off=[0, 120, 200])
        assert idx[0] == np.argmax(val[:120]) and idx[1] == np.argmax(val[120:])
        assert best[0] == val[idx[0]] and mu[1] == mean[120 + idx[1]] and vv[1] == var[120 + idx[1]]
    # the default incumbent is the largest training target
    _, _, a = s.gp_acq_values(xs, "ei")
    _, _, b = s.gp_acq_values(xs, "ei", incumbent=inc)
    assert np.array_equal(a, b)
    _, _, u = s.gp_acq_values(xs, "ucb_var")
    m, v = s.gpflow_model.predict_y(xs)
    assert np.array_equal(u, np.asarray(m)[:, 0] + s.gp_varsigma * np.asarray(v)[:, 0])


def _smooth_trained():
    """The polish tests' problem (tests/predict_grad_oracle.py): 30 points of the toy objective; the fitted lengthscale is
    0.15, so a central difference at h = 1e-5 truncates below 1e-6 of the gradient."""
    from tests.predict_grad_oracle import polish_problem

    coords, scores, _, _ = polish_problem()
    s = _surrogate()
    s.append(coords, scores)
    s.gp_update()
    return s, float(np.max(scores))


@pytest.mark.parametrize("objective,above", [("logei", 0.0), ("logei", 30.0), ("ei", 0.0), ("ucb_std", 0.0)])
def test_chain_rule_gradient_against_central_differences(objective, above):
    """Relative 1e-6: the difference quotient's own truncation error at h = 1e-5.  ``above`` lifts the incumbent over the
    best score: at +30 every z is below -25 (down to -245), where Phi, phi and h underflow and only the tail-stable
    quotients give a gradient at all.  EI itself is checked on the rows with z > -4: further out its VALUE is below 1e-5
    of its scale and a difference quotient of it is rounding noise."""
    s, top = _smooth_trained()
    xs = np.random.default_rng(3).random((12, 2)) * 0.8 + 0.1
    inc = top + above
    mean, var, value, grad = s.acq_value_and_grad(xs, objective, incumbent=inc)
    z = (mean - inc) / np.sqrt(var)
    if above:
        assert z.max() < -25.0 and np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
    h = 1e-5
    num = np.empty_like(grad)
    for k in range(xs.shape[1]):
        e = np.zeros(xs.shape[1])
        e[k] = h
        num[:, k] = (s.acq_value_and_grad(xs + e, objective, incumbent=inc)[2]
                     - s.acq_value_and_grad(xs - e, objective, incumbent=inc)[2]) / (2 * h)
    rows = z > -4.0 if objective == "ei" else np.ones(len(z), dtype=bool)
    assert rows.sum() >= 2
    rel = np.abs(grad - num)[rows] / np.max(np.abs(num), axis=1, keepdims=True)[rows]
    print(objective, above, "worst relative difference", float(rel.max()))
    assert rel.max() <= 1e-6, float(rel.max())


def test_polish_on_logei_climbs():
    s = _trained()
    starts = np.array([[0.3, 0.3], [0.7, 0.6]])
    before = s.acq_value_and_grad(starts, "logei")[2]
    coords, mean, var, value, results = s.polish(starts, objective="logei", options={"maxiter": 15})
    assert np.all(value >= before) and np.all((coords >= 0) & (coords <= 1))
    with pytest.raises(ValueError):
        s.polish(starts, objective="pi")
