"""
Failed evaluations on the device: the success member -- ONE Bernoulli-installed classifier posterior
copied onto the objective's context --, the constrained calls that take it in, and one surrogate update with failed points,
against the float64 oracles (oracle/gpr.py, tests/vgp_bernoulli_oracle.py) and against the library's own host fold.

Shapes: the objective has N = 40 rows under Matern-5/2, the classifier N = 60 under the squared exponential with ARD (the
member's N and kernel are its own), D = 2; M = 300 leaves (five 64-leaf tiles, the last one partial) in 1 and 5 segments;
J = 0 and J = 2 constraint models.  Thresholds sit at the median of the oracle's constraint means and the gate at the median of
the oracle's logpof, so that at least a quarter of the leaves pass and a quarter fail (asserted from the oracle).  Everything is
built once and shared, never written to.
"""
import numpy as np
import pytest

from oracle import gpr
from tests import acq_oracle, constraints_oracle as co
from tests import vgp_bernoulli_oracle as B
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

VS = gpr.VARSIGMA_DEFAULT
N_OBJ, N_CLS, D, M = 40, 60, 2, 300
CLS_KERNEL = "SquaredExponential"
_BUILT = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _spec(kind):
    from pygpso_amd import acquisition as A

    return {"ucb_var": lambda: A.UCBVar(VS), "ucb_std": lambda: A.UCBStd(VS), "ei": lambda: A.EI(xi=0.01), "logei": lambda: A.LogEI(xi=0.01)}[kind]()


def _fit(eng, th):
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)


def _classifier_engine(dtype="float64"):
    """(engine with the Bernoulli install resident, the oracle's posterior of it)."""
    from pygpso_amd import HipGPEngine

    X, y, u, n_ls = B.case_problem(N_CLS, D, CLS_KERNEL, True)
    mu, S = np.zeros(N_CLS), np.eye(N_CLS)
    for gamma, shift in B.STEPS:
        mu, S = B.natgrad(CLS_KERNEL, u + shift, n_ls, True, 0.0, X, y, mu, S, gamma)
    uu = u + B.STEPS[-1][1]
    eng = HipGPEngine(dtype, device=0)
    eng.set_data(X, y)
    eng.vgp_set_likelihood("Bernoulli", 0.0, B.N_GH)
    eng.vgp_set_q(mu, S)
    eng.vgp_posterior(CLS_KERNEL, uu, n_ls, True, 0.0)
    return eng, B.Posterior(CLS_KERNEL, uu, n_ls, True, 0.0, X, mu, S)


def problem():
    """The inputs and what the oracles say of them: no GPU."""
    X, y = synthetic_problem(N_OBJ, D, seed=3)
    leaves = synthetic_leaves(M, D, seed=4)
    th_obj = gpr.Theta("Matern52", 0.4, 1.1, 2e-3, float(y.mean()))
    rng = np.random.default_rng(7)
    w, ph = rng.normal(size=(2, D)), rng.uniform(0.0, 2.0 * np.pi, 2)
    cY = np.array([np.sin(2.0 * X @ w[i] + ph[i]) + 0.25 * np.cos(3.0 * X[:, 0] + i) for i in range(2)])
    thetas = [gpr.Theta("Matern52", 0.35 + 0.1 * i, 1.0 + 0.2 * i, 1e-3 * (i + 1), float(cY[i].mean())) for i in range(2)]
    cols = [gpr.predict_y(gpr.posterior(th, X, cY[i]), leaves) for i, th in enumerate(thetas)]
    om, ov = np.array([c[0] for c in cols]), np.array([c[1] for c in cols])
    thr, sense = np.median(om, axis=1), np.array([1, -1], dtype=np.int64)
    noise = np.array([th.noise for th in thetas])
    return dict(X=X, y=y, leaves=leaves, th_obj=th_obj, cY=cY, thetas=thetas, thr=thr, sense=sense, noise=noise,
                o_con=co.log_pof_numpy(om, ov, noise, thr, sense), o_obj=gpr.predict_y(gpr.posterior(th_obj, X, y), leaves), inc=float(np.max(y)))


def _segments(nseg):
    return None if nseg == 1 else np.round(np.linspace(0, M, nseg + 1)).astype(np.int64)


def built():
    if _BUILT:
        return _BUILT
    from pygpso_amd import HipGPEngine

    c = problem()
    cls, cpost = _classifier_engine()
    o_suc = B.success_log_prob(*cpost.predict_f(c["leaves"]))
    eng = HipGPEngine("float64", device=0)
    eng.set_data(c["X"], c["y"])
    _fit(eng, c["th_obj"])
    h_obj, h_cls = eng.posterior_hash(), cls.posterior_hash()
    p_obj, p_cls = eng.predict(c["leaves"]), cls.predict(c["leaves"])
    eng.success_push(cls)
    c.update(eng=eng, cls=cls, cpost=cpost, o_suc=o_suc, h_obj=h_obj, h_cls=h_cls, p_obj=p_obj, p_cls=p_cls)
    # J = 0: the success member alone; the gate at the median of the oracle's logpof
    c["gate"] = {0: float(np.median(o_suc)), 2: float(np.median(c["o_con"] + o_suc))}
    c["o_logpof"] = {0: o_suc, 2: c["o_con"] + o_suc}
    c["dev"], c["best"] = {}, {}
    for j in (0, 2):
        if j == 2:
            src = HipGPEngine("float64", device=0)
            for i, th in enumerate(c["thetas"]):
                src.set_data(c["X"], c["cY"][i])
                _fit(src, th)
                assert eng.constraint_push(src, c["thr"][i], int(c["sense"][i])) == i
            src.close()
        for kind, mode in (("ucb_var", "gate"), ("ucb_std", "feasibility"), ("ei", "weight"), ("logei", "weight"), ("ei", "gate")):
            c["dev"][j, kind, mode] = eng.constrained_acq_values(c["leaves"], _spec(kind), mode, c["gate"][j], incumbent=c["inc"], want_members=True)
            for nseg in (1, 5):  # (gpso_constrained_best_acq while this J is what the context holds: J = 0 is the member alone)
                c["best"][j, kind, mode, nseg] = eng.constrained_best_acq(c["leaves"], _spec(kind), mode, c["gate"][j], _segments(nseg),
                                                                          incumbent=c["inc"])
    for a in (c["X"], c["y"], c["leaves"]):
        a.setflags(write=False)
    _BUILT.update(c)
    return _BUILT


@pytest.mark.parametrize("j", (0, 2))
def test_gates_are_not_vacuous_under_the_oracle(j):
    """From the oracles alone: at least a quarter of the leaves pass the gate and at least a quarter fail it."""
    c = problem()
    X, y, u, n_ls = B.case_problem(N_CLS, D, CLS_KERNEL, True)
    mu, S = np.zeros(N_CLS), np.eye(N_CLS)
    for gamma, shift in B.STEPS:
        mu, S = B.natgrad(CLS_KERNEL, u + shift, n_ls, True, 0.0, X, y, mu, S, gamma)
    o_suc = B.success_log_prob(*B.Posterior(CLS_KERNEL, u + B.STEPS[-1][1], n_ls, True, 0.0, X, mu, S).predict_f(c["leaves"]))
    lp = o_suc if j == 0 else c["o_con"] + o_suc
    gate = float(np.median(lp))
    assert np.mean(lp >= gate) >= 0.25 and np.mean(lp < gate) >= 0.25
    assert np.exp(o_suc).min() < 0.35 and np.exp(o_suc).max() > 0.65  # the classifier does separate the leaves


@pytest.mark.parametrize("j", (0, 2))
def test_device_fold_is_the_host_fold_of_the_devices_own_columns(j):
    from pygpso_amd import HipGPEngine

    c = built()
    for (jj, kind, mode), out in c["dev"].items():
        if jj != j:
            continue
        mean, var, value, logpof, mm, mv = out
        assert mm.shape == (j + 1, M)  # the J constraint models' columns, then the success member's latent ones
        h_val, h_lp = HipGPEngine.constrained_success_fold_host(_spec(kind), mean, var, c["th_obj"].noise, mm[:j], mv[:j], c["noise"][:j],
                                                                c["thr"][:j], c["sense"][:j], mm[j], mv[j], mode, c["gate"][j], incumbent=c["inc"])
        assert np.array_equal(_bits(logpof), _bits(h_lp)), (j, kind, mode)
        assert np.array_equal(np.isneginf(value), np.isneginf(h_val)), (j, kind, mode)  # the gate's decision
        keep = logpof >= c["gate"][j]
        assert np.mean(keep) >= 0.25 and np.mean(~keep) >= 0.25, (j, np.mean(keep))  # ... is not vacuous on the device either
        if mode == "feasibility" or kind.startswith("ucb"):
            assert np.array_equal(_bits(value), _bits(h_val)), (j, kind, mode)
        else:  # EI / log-EI: the objective's map runs on another libm (section 7r's rule: tests/acq_oracle.py's tolerance)
            tol = acq_oracle.tolerance(acq_oracle.KINDS[kind])[0]
            live = np.isfinite(h_val)
            scale = np.maximum(1.0, np.abs(h_val[live])) if kind == "logei" else np.maximum(np.abs(h_val[live]), 2.0 ** -1022)
            err = float(np.max(np.abs(value[live] - h_val[live]) / scale))
            print(f"SUCCESS_FOLD J={j} {kind} {mode}: device against host {err:.2e} (tolerance {tol:.2e})")
            assert err <= tol
        # the success term is the host map of the member's columns, last in the sum
        term = HipGPEngine.success_prob_host(mm[j], mv[j])[1]
        if j == 0:
            assert np.array_equal(_bits(logpof), _bits(term))
        else:
            base = HipGPEngine.constrained_fold_host(_spec(kind), mean, var, c["th_obj"].noise, mm[:j], mv[:j], c["noise"], c["thr"], c["sense"],
                                                     "feasibility", incumbent=c["inc"])[1]
            assert np.array_equal(_bits(logpof), _bits(base + term))
    # the columns: the objective's and the member's against the oracles and against gpso_predict on their own contexts
    mean, var, _, logpof, mm, mv = c["dev"][j, "ucb_var", "gate"]
    tol_m = 1e-9 * max(1.0, float(np.max(np.abs(c["y"]))))
    assert np.max(np.abs(mean - c["o_obj"][0])) <= tol_m and np.max(np.abs(var - c["o_obj"][1])) <= 1e-9 * c["th_obj"].variance
    assert np.max(np.abs(mean - c["p_obj"][0])) <= tol_m and np.max(np.abs(var - c["p_obj"][1])) <= 1e-9 * c["th_obj"].variance
    sm, sv = c["cpost"].predict_f(c["leaves"])
    assert np.max(np.abs(mm[j] - sm)) <= 2e-9 * max(1.0, float(np.max(np.abs(sm)))) and np.max(np.abs(mv[j] - sv)) <= 2e-9 * c["cpost"].var
    assert np.max(np.abs(mm[j] - c["p_cls"][0])) <= 1e-9 and np.max(np.abs(mv[j] - c["p_cls"][1])) <= 1e-9 * c["cpost"].var
    assert np.max(np.abs(logpof - c["o_logpof"][j])) <= 1e-7 * max(1.0, float(np.max(np.abs(c["o_logpof"][j]))))


@pytest.mark.parametrize("nseg", (1, 5))
@pytest.mark.parametrize("j", (0, 2))
def test_best_acq_is_the_first_row_arg_max_of_acq_values(j, nseg):
    """built() made every best_acq call while the context held that J: with the member alone (J = 0), then with the two
    constraint models beside it."""
    c = built()
    assert c["eng"].constraint_info()[0] == 2  # (the set built() left: J = 2 with the member)
    so = _segments(nseg)
    bounds = np.array([0, M]) if so is None else so
    seen = 0
    for (jj, kind, mode), cols in c["dev"].items():
        if jj != j:
            continue
        seen += 1
        idx, mean, var, value, logpof = c["best"][j, kind, mode, nseg]
        assert idx.shape == (nseg,)
        for sgm, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            w = int(np.argmax(cols[2][a:b]))
            assert int(idx[sgm]) == w, (kind, mode, sgm)
            for got, col in zip((mean, var, value, logpof), cols):
                assert _bits([got[sgm]])[0] == _bits([col[a + w]])[0], (j, kind, mode, sgm)  # the winners' logpof among them
    assert seen == 5
    # the same call gives the same bits (J = 2: what the context holds now)
    if j == 2:
        again = c["eng"].constrained_best_acq(c["leaves"], _spec("ei"), "weight", c["gate"][2], so, incumbent=c["inc"])
        for a, b in zip(again, c["best"][2, "ei", "weight", nseg]):
            assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))
    # a leaf's numbers depend neither on its slot nor on the batch
    full = c["dev"][2, "ucb_var", "gate"]
    solo = c["eng"].constrained_acq_values(c["leaves"][137:138], _spec("ucb_var"), "gate", c["gate"][2], incumbent=c["inc"])
    for a, b in zip(solo, full[:4]):
        assert _bits(a)[0] == _bits(b)[137]


def test_push_clear_and_the_calls_leave_both_posteriors_and_the_member_outlives_the_objectives_data():
    from pygpso_amd import _lib, acquisition as A

    c = built()
    eng, cls = c["eng"], c["cls"]
    # after the push and every call above: hash and predictions of both contexts are what they were
    assert eng.posterior_hash() == c["h_obj"] and cls.posterior_hash() == c["h_cls"]
    for got, want in ((eng.predict(c["leaves"]), c["p_obj"]), (cls.predict(c["leaves"]), c["p_cls"])):
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    present, n_m, theta = eng.success_info()
    assert present and n_m == N_CLS and theta[49] == 0.0 and np.allclose(theta[:D], c["cpost"].ls, rtol=1e-14, atol=0.0)
    assert eng.constraint_info()[0] == 2  # the member is no part of the set's count
    before = c["dev"][2, "ucb_var", "gate"]
    # a refit of the objective keeps the member; its columns keep their bits
    _fit(eng, gpr.Theta("Matern52", 0.9, 0.7, 5e-3, 0.0))
    after = eng.constrained_acq_values(c["leaves"], _spec("ucb_var"), "gate", c["gate"][2], incumbent=c["inc"], want_members=True)
    assert eng.success_info()[0] and np.array_equal(_bits(after[4]), _bits(before[4])) and np.array_equal(_bits(after[5]), _bits(before[5]))
    assert np.array_equal(_bits(after[3]), _bits(before[3]))
    # gpso_set_data of the objective keeps it too (another N: the constraint set goes stale, the member does not)
    eng.set_data(c["X"][:30], c["y"][:30])
    assert eng.success_info()[:2] == (True, N_CLS)
    _fit(eng, c["th_obj"])
    with pytest.raises(_lib.GpsoHipError) as err:
        eng.constrained_acq_values(c["leaves"], _spec("ucb_var"), "gate", -1.0)
    assert err.value.code == _lib.E_STATE and "stale" in str(err.value)
    eng.constraint_clear()
    alone = eng.constrained_acq_values(c["leaves"], _spec("ucb_var"), "feasibility", -1.0, want_members=True)
    assert alone[4].shape == (1, M) and np.array_equal(_bits(alone[4][0]), _bits(before[4][2])) and np.array_equal(_bits(alone[3]), _bits(c["dev"][0, "ucb_std", "feasibility"][3]))
    # clear: J = 0 without the member is refused in the words it always was; both posteriors are untouched
    h = eng.posterior_hash()
    eng.success_clear()
    assert eng.success_info()[0] is False and eng.posterior_hash() == h and cls.posterior_hash() == c["h_cls"]
    with pytest.raises(_lib.GpsoHipError) as err:
        eng.constrained_best_acq(c["leaves"], A.EI(), "gate", -1.0, incumbent=0.0)
    assert err.value.code == _lib.E_STATE and "no constraint set on this context: gpso_constraint_push first" in str(err.value)
    # gpso_alloc_posterior ends a member
    eng.success_push(cls)
    assert eng.success_info()[0]
    eng.alloc_posterior(N_OBJ, D)
    assert eng.success_info()[0] is False
    _BUILT.clear()
    eng.close()
    cls.close()


def test_success_push_refusals():
    from pygpso_amd import HipGPEngine, _lib

    def refused(fn, code, word="gpso_success_push"):
        with pytest.raises(ValueError if code == _lib.E_ARG else _lib.GpsoHipError) as err:  # (the engine raises GPSO_E_ARG as ValueError)
            fn()
        assert (code == _lib.E_ARG or err.value.code == code) and word in str(err.value), str(err.value)

    X, y = synthetic_problem(N_OBJ, D, seed=3)
    leaves = synthetic_leaves(10, D, seed=1)
    cls, _ = _classifier_engine()
    eng, e32 = HipGPEngine("float64", device=0), HipGPEngine("float32", device=0)
    eng.set_data(X, y)
    eng.fit_eval("Matern52", 0.4, 1.0, 1e-2, 0.0, want_grad=False)
    e32.set_data(X, y)
    e32.fit_eval("Matern52", 0.4, 1.0, 1e-2, 0.0, want_grad=False)
    refused(lambda: e32.success_push(cls), _lib.E_ARG)  # a float32 owner
    refused(lambda: eng.success_push(e32), _lib.E_ARG)  # a float32 source
    refused(lambda: cls.success_push(eng), _lib.E_STATE)  # a fitted GPR is no Bernoulli install
    other = HipGPEngine("float64", device=0)
    refused(lambda: eng.success_push(other), _lib.E_STATE)  # nothing on src
    other.set_data(X, y)  # a Gaussian VGP install is none either
    u = gpr.Theta("Matern52", 0.4, 1.0, 1e-2, 0.0).pack()
    other.vgp_set_q()
    other.vgp_natgrad("Matern52", u, 1, True, 0.0, 1.0)
    other.vgp_posterior("Matern52", u, 1, True, 0.0)
    refused(lambda: eng.success_push(other), _lib.E_STATE)
    # D mismatch; N > 128
    X3, y3, u3, n3 = B.case_problem(30, 3, "Matern52", False)
    other.set_data(X3, y3)
    other.vgp_set_likelihood("Bernoulli", 0.0, B.N_GH)
    other.vgp_set_q()
    other.vgp_natgrad("Matern52", u3, n3, True, 0.0, 1.0)
    other.vgp_posterior("Matern52", u3, n3, True, 0.0)
    refused(lambda: eng.success_push(other), _lib.E_ARG)
    X9, y9, u9, n9 = B.case_problem(129, 2, "Matern52", False)
    other.set_data(X9, y9)
    other.vgp_set_q()
    other.vgp_natgrad("Matern52", u9, n9, True, 0.0, 1.0)
    other.vgp_posterior("Matern52", u9, n9, True, 0.0)
    refused(lambda: eng.success_push(other), _lib.E_ARG)
    # open tickets on either side
    ticket = eng.best_ucb_begin(leaves, VS)
    refused(lambda: eng.success_push(cls), _lib.E_STATE)
    refused(eng.success_clear, _lib.E_STATE, "gpso_success_clear")
    eng.best_ucb_end(ticket)
    ticket = cls.best_ucb_begin(leaves, VS)
    refused(lambda: eng.success_push(cls), _lib.E_STATE)
    cls.best_ucb_end(ticket)
    assert eng.success_info()[0] is False  # after every refusal: no member
    eng.success_push(cls)
    # a member of another D than the objective's new data: the call says so
    eng.set_data(X3, y3)
    eng.fit_eval("Matern52", 0.4, 1.0, 1e-2, 0.0, want_grad=False)
    from pygpso_amd import acquisition as A

    with pytest.raises(_lib.GpsoHipError) as err:
        eng.constrained_acq_values(synthetic_leaves(10, 3, seed=1), A.UCBVar(VS), "gate", -1.0)
    assert err.value.code == _lib.E_STATE and "success member" in str(err.value)
    import torch

    if torch.cuda.device_count() > 1:  # (a source on ANOTHER device needs a second GPU: made only where there is one)
        far = HipGPEngine("float64", device=1)
        refused(lambda: far.success_push(cls), _lib.E_ARG)
        far.close()
    for e in (eng, e32, other, cls):
        e.close()


# ---- the host layers on the device ----------------------------------------------------------------------------------------
def test_surrogate_update_with_two_failed_points_among_twelve():
    from pygpso_amd import GPRSurrogate, acquisition as A
    from pygpso_amd.constraints import ConstrainedAcq
    from pygpso_amd.kernels import Constant, Matern52, Scipy
    from tests import vgp_oracle as V

    POF = 0.75  # (the oracle's replay gates 30 % of the leaves there, none at 0.5: checked on the CPU)
    rng = np.random.default_rng(11)
    X = rng.random((12, 2))
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + 0.5 * X[:, 1]
    failed = X[:, 0] > np.sort(X[:, 0])[-3]  # the two points furthest along x
    assert failed.sum() == 2
    scores = np.where(failed, np.nan, y)
    leaves = synthetic_leaves(200, 2, seed=23)
    surr = GPRSurrogate(gp_kernel=Matern52(lengthscales=0.25, variance=1.0), gp_meanf=Constant(0.0), optimiser=Scipy(), failures="classify",
                        pof_min=POF)
    surr.append(X, scores)
    surr.gp_update()
    model, cls = surr.gpflow_model, surr._classifier
    assert surr._success_live and model.engine.success_info()[:2] == (True, 12) and model.constraint_count() == 0
    assert model.data[0].shape[0] == 10 and cls.data[0].shape[0] == 12 and cls.engine is not model.engine
    # it ranks by the constrained call
    cols = model.constrained_acq_values(leaves, ConstrainedAcq(A.UCBVar(surr.gp_varsigma), "gate", POF), want_members=True)
    gated = np.isneginf(cols[2])
    assert gated.any() and (~gated).any()
    j = int(np.argmax(cols[2]))
    assert surr.gp_eval_best_ucb(leaves) == (cols[0][j], cols[1][j], cols[2][j])
    # the member's columns are the classifier's own latent predictions
    pm, pv = cls.predict_f(leaves)
    assert np.max(np.abs(cols[4][0] - np.asarray(pm)[:, 0])) <= 1e-9 * max(1.0, float(np.max(np.abs(pm))))
    assert np.max(np.abs(cols[5][0] - np.asarray(pv)[:, 0])) <= 1e-9 * cls.kernel.variance
    # the oracle's replay: the classifier's schedule (10 iterations: natgrad 0.5, Adam(0.05)) from the surrogate's specs; the
    # objective's posterior at the hyper-parameters the device's search found
    xa, lab = surr.current_attempts
    u0 = B.initial_u(0.25, 1.0, 0.0)
    u_c, mu, S, _ = B.train("Matern52", u0, 1, True, 0.0, xa, lab, np.zeros(12), np.eye(12), 10, 0.5, V.Adam(0.05))
    np.testing.assert_allclose(cls._device_u(), u_c, rtol=1e-7, atol=1e-9)
    cpost = B.Posterior("Matern52", u_c, 1, True, 0.0, xa, mu, S)
    o_lp = B.success_log_prob(*cpost.predict_f(leaves))
    name, ls, var, noise, cc = model._theta()
    om, ov = gpr.predict_y(gpr.posterior(gpr.Theta(name, ls, var, noise, cc), model.data[0], model.data[1][:, 0]), leaves)
    o_val = np.where(o_lp >= np.log(POF), om + surr.gp_varsigma * ov, -np.inf)
    print(f"FAILURES update: {int(gated.sum())} of 200 leaves gated; oracle {int(np.isneginf(o_val).sum())}")
    assert int(np.argmax(o_val)) == j  # the selected leaf is the oracle replay's
    assert np.max(np.abs(cols[3] - o_lp)) <= 1e-6 * max(1.0, float(np.max(np.abs(o_lp))))
    assert surr.highest_score.score_mu == float(np.max(y[~failed]))
    surr.close_constraint_models()
    assert surr._classifier is None and surr.gp_eval_best_ucb(leaves) == (cols[0][j], cols[1][j], cols[2][j])  # the member stays
    model.engine.close()
