"""
The hyper-parameter ensemble on the device: K posteriors of the same data resident on one context
and the integrated acquisition over them, against the float64 oracle (tests/ensemble_oracle.py) and against the library's
own calls at every member's theta.

Shapes: N in {5, 64, 65, 128} (the 64-row boundary of the factor's blocks and the limit), D in {1, 2, 12, 33}, M in {1, 63,
64, 65, 1000} (one leaf, the 64-leaf tile's edges, many tiles), K in {1, 2, 7, 32}, every kernel kind, "float64" and "mixed"
contexts, with and without a per-point noise vector.  Every case is built once and shared, never written to.

Tolerances: a member's columns are held to DESIGN.md 2.1's float64 row -- 1e-9 of max(1, max|y|) on the mean and of the
kernel variance on the variance (Matern-1/2: 1e-5) -- against the oracle and against gpso_predict on a context fitted at the
member's theta; bit equality is not promised (other kernels).  The device fold is the host fold of the device's own columns:
bitwise for the UCB kinds and the moments, tests/acq_oracle.py's per-value tolerance for EI / PI / log-EI (another libm).
"""
import numpy as np
import pytest

from oracle import gpr
from tests import acq_oracle, context_stages as CS, ensemble_oracle as eo
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

VS = gpr.VARSIGMA_DEFAULT
# (name, N, D, M, K, kernel, dtype, noise vector, ARD)
CASES = {
    "tiny": (5, 1, 1, 1, "Matern52", "float64", False, False),
    "block": (64, 2, 63, 2, "Matern32", "mixed", True, False),
    "block+1": (65, 12, 64, 7, "Matern12", "float64", False, True),
    "limit_wide": (128, 33, 65, 32, "SquaredExponential", "mixed", False, True),
    "limit_many": (128, 2, 1000, 7, "Matern52", "float64", True, False),
    "loop": (52, 2, 162, 32, "SquaredExponential", "float64", False, False),
}
KINDS = ("ucb_var", "ucb_std", "ei", "logei", "pi")
_BUILT = {}


def _spec(kind, latent=False):
    from pygpso_amd import acquisition as A

    return {"ucb_var": lambda: A.UCBVar(VS), "ucb_std": lambda: A.UCBStd(VS, latent=latent), "ei": lambda: A.EI(xi=0.01, latent=latent),
            "logei": lambda: A.LogEI(xi=0.01, latent=latent), "pi": lambda: A.PI(xi=0.01, latent=latent)}[kind]()


def _thetas(kernel, d, k, ard, y, seed):
    rng = np.random.default_rng([seed, k, d])
    out = []
    for _ in range(k):
        base = 0.3 * np.sqrt(d)
        ls = base * np.exp(0.3 * rng.standard_normal(d)) if ard else float(base * np.exp(0.3 * rng.standard_normal()))
        out.append(gpr.Theta(kernel, ls, float(1.2 * np.exp(0.3 * rng.standard_normal())), float(2e-3 * np.exp(0.5 * rng.standard_normal())),
                             float(y.mean() + 0.1 * rng.standard_normal())))
    return out


def _push_all(eng, thetas):
    for i, th in enumerate(thetas):
        eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
        assert eng.ensemble_push() == i


def built(name):
    """The case's engine with its ensemble installed, inputs and the device's outputs: made once, shared, read-only."""
    if name in _BUILT:
        return _BUILT[name]
    from pygpso_amd import HipGPEngine

    n, d, m, k, kernel, dtype, with_s, ard = CASES[name]
    X, y = synthetic_problem(n, d, seed=3)
    leaves = synthetic_leaves(m, d, seed=4)
    s = np.random.default_rng(5).uniform(0.0, 5e-3, n) if with_s else None
    thetas = _thetas(kernel, d, k, ard, y, seed=6)
    eng = HipGPEngine(dtype)
    eng.set_data(X, y)
    if with_s:
        eng.set_noise_diag(s)
    assert eng.ensemble_max() == 32
    _push_all(eng, thetas)
    case = dict(eng=eng, X=X, y=y, s=s, leaves=leaves, thetas=thetas, k=k, kernel=kernel, dtype=dtype, n=n, d=d, m=m)
    case["inc"] = float(np.max(y))
    case["dev"] = {kind: eng.ensemble_acq_values(leaves, _spec(kind), incumbent=case["inc"], want_members=True) for kind in KINDS}
    case["oracle_members"] = eo.members(thetas, X, y, leaves, s)
    for a in (X, y, leaves):
        a.setflags(write=False)
    _BUILT[name] = case
    return case


def _member_bounds(case):
    tol = 1e-5 if case["kernel"] == "Matern12" else 1e-9
    return tol * max(1.0, float(np.max(np.abs(case["y"])))), tol


@pytest.mark.parametrize("name", list(CASES))
def test_member_columns_against_the_oracle_posterior_at_every_theta(name):
    c = built(name)
    _, _, _, mm, mv = c["dev"]["ucb_var"]
    om, ov = c["oracle_members"]
    assert mm.shape == (c["k"], c["m"]) and mv.shape == (c["k"], c["m"])
    k_info, theta = c["eng"].ensemble_info()
    assert k_info == c["k"] and theta.shape == (c["k"], 51)
    tol_m, tol_v = _member_bounds(c)
    for i, th in enumerate(c["thetas"]):
        ls = np.broadcast_to(np.atleast_1d(th.lengthscales), (c["d"],))
        assert np.array_equal(theta[i, :c["d"]], ls) and tuple(theta[i, 48:]) == (th.variance, th.noise, th.mean_c)
        em, ev = float(np.max(np.abs(mm[i] - om[i]))), float(np.max(np.abs(mv[i] - ov[i]))) / th.variance
        print(f"ENSEMBLE_PARITY {name} member {i}: mean {em:.2e} (bound {tol_m:.1e}), var {ev:.2e} (bound {tol_v:.1e})")
        assert em <= tol_m and ev <= tol_v, (name, i, em, ev)


@pytest.mark.parametrize("name", list(CASES))
def test_member_columns_against_gpso_predict_on_a_context_fitted_at_theta(name):
    from pygpso_amd import HipGPEngine

    c = built(name)
    _, _, _, mm, mv = c["dev"]["ucb_var"]
    tol_m, tol_v = _member_bounds(c)
    other = HipGPEngine("float64")
    other.set_data(c["X"], c["y"])
    if c["s"] is not None:
        other.set_noise_diag(c["s"])
    for i, th in enumerate(c["thetas"]):
        other.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
        pm, pv = other.predict(c["leaves"])
        assert float(np.max(np.abs(mm[i] - pm))) <= tol_m and float(np.max(np.abs(mv[i] - pv))) / th.variance <= tol_v, (name, i)
    other.close()


@pytest.mark.parametrize("name", list(CASES))
def test_device_fold_is_the_host_fold_of_the_devices_own_columns(name):
    from pygpso_amd import HipGPEngine

    c = built(name)
    noise = np.array([th.noise for th in c["thetas"]])
    for kind in KINDS:
        mean_mix, var_mix, value, mm, mv = c["dev"][kind]
        h_mean, h_var, h_val = HipGPEngine.ensemble_fold_host(_spec(kind), mm, mv, noise, incumbent=c["inc"])
        assert np.array_equal(mean_mix, h_mean) and np.array_equal(var_mix, h_var), (name, kind)
        if kind in ("ucb_var", "ucb_std"):
            assert np.array_equal(value, h_val), (name, kind)
            assert np.array_equal(value, eo.fold_numpy(eo.UCB_VAR if kind == "ucb_var" else eo.UCB_STD, mm, mv, VS)[2])
        else:
            tol = acq_oracle.tolerance(acq_oracle.KINDS[kind])[0]
            scale = np.maximum(1.0, np.abs(h_val)) if kind == "logei" else np.maximum(np.abs(h_val), 2.0 ** -1022)
            err = float(np.max(np.abs(value - h_val) / scale))
            print(f"ENSEMBLE_FOLD {name} {kind}: device against host {err:.2e} (tolerance {tol:.2e})")
            assert err <= tol, (name, kind, err)
    # a latent kind reads every member's own noise
    for kind in ("ucb_std", "ei"):
        _, _, value, mm, mv = c["eng"].ensemble_acq_values(c["leaves"], _spec(kind, latent=True), incumbent=c["inc"], want_members=True)
        h_val = HipGPEngine.ensemble_fold_host(_spec(kind, latent=True), mm, mv, noise, incumbent=c["inc"])[2]
        if kind == "ucb_std":
            assert np.array_equal(value, h_val)
        else:
            assert float(np.max(np.abs(value - h_val) / np.maximum(np.abs(h_val), 2.0 ** -1022))) <= acq_oracle.tolerance(acq_oracle.EI)[0]


def _segments(m, nseg):
    if nseg == 1:
        return None
    cuts = np.unique(np.round(np.linspace(0, m, nseg + 1)).astype(np.int64))
    so = np.concatenate([cuts, np.full(nseg + 1 - cuts.shape[0], m, dtype=np.int64)])  # (M < nseg: empty segments at the end)
    return so


@pytest.mark.parametrize("nseg", (1, 5))
@pytest.mark.parametrize("name", list(CASES))
def test_best_acq_is_the_row_arg_max_of_acq_values_and_the_oracles_winner(name, nseg):
    c = built(name)
    so = _segments(c["m"], nseg)
    bounds = np.array([0, c["m"]]) if so is None else so
    for kind in KINDS:
        idx, mean_mix, var_mix, value = c["eng"].ensemble_best_acq(c["leaves"], _spec(kind), so, incumbent=c["inc"])
        col_mean, col_var, col_val, _, _ = c["dev"][kind]
        for sgm, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            if a == b:
                assert idx[sgm] == -1 and np.isnan(value[sgm])
                continue
            j = int(np.argmax(col_val[a:b]))
            assert int(idx[sgm]) == j, (name, kind, sgm)
            for got, col in ((mean_mix, col_mean), (var_mix, col_var), (value, col_val)):
                assert np.array([got[sgm]]).view(np.uint64)[0] == np.array([col[a + j]]).view(np.uint64)[0], (name, kind, sgm)
    # the oracle's winner under the reference's rule, where its top two are further apart than the members' tolerance
    om, ov = c["oracle_members"]
    ref = eo.fold_numpy(eo.UCB_VAR, om, ov, VS)[2]
    idx = c["eng"].ensemble_best_acq(c["leaves"], _spec("ucb_var"), so)[0]
    gap_needed = 4.0 * (_member_bounds(c)[0] + VS * _member_bounds(c)[1] * max(th.variance for th in c["thetas"]))
    for sgm, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        if b - a == 0:
            continue
        top = np.sort(ref[a:b])[::-1]
        if b - a > 1:
            assert top[0] - top[1] > gap_needed, (name, sgm, top[0] - top[1], gap_needed)  # (checked on the CPU when the seeds were chosen)
        assert int(idx[sgm]) == int(np.argmax(ref[a:b])), (name, sgm)


def test_ties_go_to_the_first_leaf_and_a_nan_leaf_wins_its_segment():
    c = built("block")
    eng, leaves = c["eng"], np.array(c["leaves"])
    best = int(eng.ensemble_best_acq(leaves, _spec("ucb_var"))[0][0])
    dup = np.vstack([leaves, leaves[best:best + 1], leaves[best:best + 1]])  # the winner three times: the first one wins
    so = np.array([0, 10, dup.shape[0]], dtype=np.int64)
    idx, _, _, value = eng.ensemble_best_acq(dup, _spec("ucb_var"), so)
    vals = eng.ensemble_acq_values(dup, _spec("ucb_var"))[2]
    assert vals[best] == vals[-1] == vals[-2]
    assert int(idx[1]) + 10 == best if best >= 10 else int(idx[0]) == best
    two = np.vstack([leaves[best:best + 1]] * 3)
    assert int(eng.ensemble_best_acq(two, _spec("ei"), incumbent=c["inc"])[0][0]) == 0
    bad = leaves.copy()
    bad[40, 1] = np.nan
    for kind in KINDS:
        idx, mean_mix, var_mix, value = eng.ensemble_best_acq(bad, _spec(kind), np.array([0, 30, bad.shape[0]]), incumbent=c["inc"])
        assert int(idx[1]) == 10 and np.isnan(value[1]) and np.isnan(mean_mix[1]) and not np.isnan(value[0]), kind
    mm = eng.ensemble_acq_values(bad, _spec("ucb_var"), want_members=True)[3]
    assert np.all(np.isnan(mm[:, 40])) and not np.any(np.isnan(np.delete(mm, 40, axis=1)))
    # float32 leaves take the same path (scaled in double by each member's lengthscales)
    v32 = eng.ensemble_acq_values(leaves.astype(np.float32), _spec("ucb_var"))[2]
    v64 = eng.ensemble_acq_values(leaves.astype(np.float32).astype(np.float64), _spec("ucb_var"))[2]
    assert np.array_equal(v32, v64)


def _observe(eng, leaves, inc):
    out = {}
    for kind in ("ucb_var", "logei"):
        a = eng.ensemble_acq_values(leaves, _spec(kind), incumbent=inc, want_members=True)
        b = eng.ensemble_best_acq(leaves, _spec(kind), np.array([0, 7, leaves.shape[0]]), incumbent=inc)
        for tag, arr in zip(("mean_mix", "var_mix", "value", "member_mean", "member_var"), a):
            out[f"{kind}.{tag}"] = arr
        for tag, arr in zip(("idx", "w_mean", "w_var", "w_value"), b):
            out[f"{kind}.{tag}"] = arr
    return out


@pytest.mark.parametrize("dtype", ("float64", "mixed"))
def test_same_call_twice_and_after_a_history_of_other_calls_same_bits(dtype):
    """The pattern of tests/test_gpu_context_reuse.py: a fresh context against one that ran other stages first."""
    from pygpso_amd import HipGPEngine

    X, y = synthetic_problem(40, 3, seed=8)
    leaves = synthetic_leaves(150, 3, seed=9)
    thetas = _thetas("Matern52", 3, 5, True, y, seed=10)

    def run(history):
        eng = HipGPEngine(dtype)
        for h in history:
            CS.STAGES[h](eng)
        eng.set_data(X, y)
        _push_all(eng, thetas)
        first = _observe(eng, leaves, float(y.max()))
        again = _observe(eng, leaves, float(y.max()))
        eng.close()
        return first, again

    fresh, again = run(())
    assert not CS.compare("ensemble", again, fresh), CS.report(CS.compare("ensemble", again, fresh))
    history = ("gpr_general", "append_in_place", "set_posterior", "vgp_gauss", "sgpr", "gpr_wide") + CS.CALL_STAGES[dtype]
    after, _ = run(history)
    assert not CS.compare("ensemble", after, fresh), CS.report(CS.compare("ensemble", after, fresh))


def test_install_ensemble_leaves_the_resident_posterior_and_its_hash():
    from pygpso_amd import priors as P
    from pygpso_amd.kernels import Constant, Matern52
    from pygpso_amd.model import HipGPR

    X, y = synthetic_problem(30, 2, seed=11)
    leaves = synthetic_leaves(100, 2, seed=12)
    m = HipGPR((X, y), Matern52(variance=1.1, lengthscales=0.4), Constant(float(y.mean())), noise_variance=3e-3)
    mean0, var0 = m.predict_y(leaves)
    hash0 = m.engine.posterior_hash()
    theta0 = m._device_theta
    P.attach(m, P.default_priors())
    U, info = m.sample_hyper(6, rng=0, chains=4, burn=8, leapfrog=4)
    assert U.shape == (6, 4) and info["batch_calls"] > 0
    assert m.engine.posterior_hash() == hash0  # (the batched evaluations leave the posterior alone)
    installed, skipped = m.install_ensemble(U)
    assert (installed, skipped) == (6, 0) and m.ensemble_size() == 6
    mean1, var1 = m.predict_y(leaves)
    assert m.engine.posterior_hash() == hash0 and m._device_theta == theta0
    assert np.array_equal(np.asarray(mean0), np.asarray(mean1)) and np.array_equal(np.asarray(var0), np.asarray(var1))
    from pygpso_amd import acquisition as A

    idx, mean_mix, var_mix, value = m.ensemble_best_acq(leaves, A.EI())
    cols = m.ensemble_acq_values(leaves, A.EI())
    assert int(idx[0]) == int(np.argmax(cols[2])) and value[0] == cols[2].max()
    # a row that is not positive definite is skipped and counted
    U_bad = np.vstack([U[:2], [[60.0, 5.0, -60.0, 0.0]]])  # a lengthscale of 60 and a noise at its floor: singular in float64
    installed, skipped = m.install_ensemble(U_bad)
    assert installed + skipped == 3 and m.ensemble_size() == installed
    m.engine.close()


CLEARING = ("set_data", "append", "append_noise", "set_noise_diag", "set_posterior", "vgp", "sgpr", "svgp", "alloc_posterior", "adopt_posterior")


@pytest.mark.parametrize("call", CLEARING)
def test_whatever_changes_the_data_ends_the_ensemble(call):
    """(gpso_adopt_posterior is legal on a context that fitted its own posterior -- it needs a shape, nothing more -- and re-reads
    the context's own hyper block: the sequence fit, push, adopt is the one place where Resident::adopted() alone ends the ensemble.)"""
    from pygpso_amd import HipGPEngine, _lib

    X, y = synthetic_problem(24, 2, seed=13)
    leaves = synthetic_leaves(20, 2, seed=14)
    thetas = _thetas("Matern52", 2, 3, False, y, seed=15)
    eng = HipGPEngine("float64")
    eng.set_data(X[:20], y[:20])
    _push_all(eng, thetas)
    assert eng.ensemble_info()[0] == 3
    th = thetas[0]
    u = th.pack()
    {"set_data": lambda: eng.set_data(X, y),
     "append": lambda: eng.append(X[20:], y[20:]),
     "append_noise": lambda: eng.append(X[20:], y[20:], np.full(4, 1e-3)),
     "set_noise_diag": lambda: eng.set_noise_diag(np.full(20, 1e-3)),
     "set_posterior": lambda: CS.STAGES["set_posterior"](eng),
     "vgp": lambda: (eng.vgp_set_q(), eng.vgp_natgrad("Matern52", u, 1, True, 0.0, 1.0), eng.vgp_posterior("Matern52", u, 1, True, 0.0)),
     "sgpr": lambda: CS.STAGES["sgpr"](eng),
     "svgp": lambda: CS.STAGES["svgp"](eng),
     "alloc_posterior": lambda: eng.alloc_posterior(20, 2),
     "adopt_posterior": lambda: eng.adopt_posterior()}[call]()
    assert eng.ensemble_info()[0] == 0, call
    leaves = synthetic_leaves(20, eng.d, seed=14)  # (a stage may have left rows of another dimension)
    for fn in (lambda: eng.ensemble_acq_values(leaves, _spec("ucb_var")), lambda: eng.ensemble_best_acq(leaves, _spec("ucb_var"))):
        with pytest.raises(_lib.GpsoHipError) as err:
            fn()
        assert err.value.code == _lib.E_STATE and "gpso_ensemble_" in str(err.value), call
    eng.close()


def test_a_push_after_an_append_holds_the_extended_posterior():
    """Fit at N = 60, gpso_append 5 rows (with and without their noise), push: the member's columns are the oracle's at N = 65."""
    from pygpso_amd import HipGPEngine

    X, y = synthetic_problem(65, 3, seed=18)
    leaves = synthetic_leaves(70, 3, seed=19)
    th = _thetas("Matern52", 3, 1, True, y, seed=20)[0]
    for s_new in (None, np.full(5, 2e-3)):
        eng = HipGPEngine("float64")
        eng.set_data(X[:60], y[:60])
        eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
        if s_new is None:
            eng.append(X[60:], y[60:])
        else:
            eng.append(X[60:], y[60:], s_new)
        assert eng.ensemble_info()[0] == 0 and eng.ensemble_push() == 0
        _, _, _, mm, mv = eng.ensemble_acq_values(leaves, _spec("ucb_var"), want_members=True)
        s_all = None if s_new is None else np.concatenate([np.zeros(60), s_new])
        om, ov = eo.members([th], X, y, leaves, s_all)
        pm, pv = eng.predict(leaves)
        for ref_m, ref_v in ((om[0], ov[0]), (pm, pv)):
            assert np.max(np.abs(mm[0] - ref_m)) <= 1e-9 * max(1.0, float(np.max(np.abs(y)))) and np.max(np.abs(mv[0] - ref_v)) <= 1e-9 * th.variance
        eng.close()


def test_a_refit_at_another_theta_keeps_the_members_and_their_bits():
    c = built("block+1")
    eng = c["eng"]
    before = eng.ensemble_acq_values(c["leaves"], _spec("ei"), incumbent=c["inc"], want_members=True)
    hash_before = None
    th = gpr.Theta(c["kernel"], 0.9, 0.7, 5e-3, 0.0)
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=True)
    hash_before = eng.posterior_hash()
    after = eng.ensemble_acq_values(c["leaves"], _spec("ei"), incumbent=c["inc"], want_members=True)
    assert eng.ensemble_info()[0] == c["k"]
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert eng.posterior_hash() == hash_before  # the integrated call writes nothing of the posterior's
    pm, pv = eng.predict(c["leaves"])
    ref_m, ref_v = gpr.predict_y(gpr.posterior(th, c["X"], c["y"]), c["leaves"])
    assert np.max(np.abs(pm - ref_m)) <= 1e-5 and np.max(np.abs(pv - ref_v)) <= 1e-5  # (Matern-1/2's row)


def test_refusals_name_the_call():
    from pygpso_amd import HipGPEngine, _lib, acquisition as A

    X, y = synthetic_problem(129, 2, seed=16)
    leaves = synthetic_leaves(10, 2, seed=17)
    th = gpr.Theta("Matern52", 0.4, 1.0, 1e-2, 0.0)

    def fit(eng, n, kernel="Matern52"):
        eng.set_data(X[:n], y[:n])
        eng.fit_eval(kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)

    def state_error(fn, word):
        with pytest.raises(_lib.GpsoHipError) as err:
            fn()
        assert err.value.code == _lib.E_STATE and word in str(err.value), str(err.value)

    e32 = HipGPEngine("float32")  # float32: GPSO_E_ARG
    fit(e32, 20)
    assert e32.ensemble_max() == 0
    with pytest.raises(ValueError, match="gpso_ensemble_push"):
        e32.ensemble_push()
    with pytest.raises(ValueError, match="gpso_ensemble_acq_values"):
        e32.ensemble_acq_values(leaves, A.UCBVar(VS))
    e32.close()
    eng = HipGPEngine("float64")
    fit(eng, 129)  # N = 129
    assert eng.ensemble_max() == 0
    with pytest.raises(ValueError, match="gpso_ensemble_push"):
        eng.ensemble_push()
    fit(eng, 128)
    assert eng.ensemble_max() == 32 and eng.ensemble_push() == 0
    fit(eng, 20)
    assert eng.ensemble_push() == 0  # (new data ended the ensemble: member 0 again)
    eng.fit_eval("Matern32", th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    state_error(eng.ensemble_push, "gpso_ensemble_push")  # another kernel kind
    eng.fit_eval("Matern52", th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    for i in range(1, 32):
        assert eng.ensemble_push() == i
    state_error(eng.ensemble_push, "gpso_ensemble_push")  # the 33rd
    assert eng.ensemble_info()[0] == 32
    for fn, word in ((lambda: eng.ensemble_acq_values(leaves, A.MES()), "gpso_ensemble_acq_values"),
                     (lambda: eng.ensemble_best_acq(leaves, A.MES()), "gpso_ensemble_best_acq")):
        with pytest.raises(ValueError, match=word):  # MES: GPSO_E_ARG
            fn()
    ticket = eng.best_ucb_begin(leaves, VS)  # an open ticket
    state_error(eng.ensemble_push, "gpso_ensemble_push")
    state_error(eng.ensemble_clear, "gpso_ensemble_clear")
    state_error(lambda: eng.ensemble_best_acq(leaves, A.UCBVar(VS)), "gpso_ensemble_best_acq")
    eng.best_ucb_end(ticket)
    assert eng.ensemble_best_acq(leaves, A.UCBVar(VS))[0].shape == (1,)
    eng.ensemble_clear()
    assert eng.ensemble_info()[0] == 0
    u = th.pack()  # a VGP posterior is no member
    eng.vgp_set_q()
    eng.vgp_natgrad("Matern52", u, 1, True, 0.0, 1.0)
    eng.vgp_posterior("Matern52", u, 1, True, 0.0)
    state_error(eng.ensemble_push, "gpso_ensemble_push")
    eng.close()


# ---- end to end: GPRSurrogate(hyper="marginal") in the optimiser's loop ---------------------------------------------------
def _marginal_run(seed):
    from pygpso_amd import GPRSurrogate, GPSOptimiser, ParameterSpace
    from pygpso_amd.kernels import Constant, Matern52, Scipy
    from tests.helpers import load_goldens, rotated_peaks

    bounds = load_goldens()["G4"]["bounds"]  # the 2-D toy problem of the loop tests (tests/test_gpu_goldens.py)
    surr = GPRSurrogate(gp_kernel=Matern52(lengthscales=0.25, variance=1.0), gp_meanf=Constant(0.0), optimiser=Scipy(),
                        hyper="marginal", n_theta=8, hyper_seed=seed, hyper_options=dict(burn=20, leapfrog=6))
    space = ParameterSpace(parameter_names=["x", "y"], parameter_bounds=bounds)
    opt = GPSOptimiser(parameter_space=space, gp_surrogate=surr, exploration_method="tree", exploration_depth=3, budget=20,
                       stopping_condition="iterations", update_cycle=1, n_workers=1)
    best = opt.run(rotated_peaks)
    return opt, surr, best


def test_marginal_surrogate_runs_the_loop_and_the_same_seed_gives_the_same_run():
    opt, surr, best = _marginal_run(3)
    assert opt.iterations == 20 and surr._ensemble_live and surr.gpflow_model.ensemble_size() == surr.last_hyper_info["installed"] >= 1
    rows = np.array([[*p.normed_coord, p.score_mu, p.score_sigma, p.score_ucb] for p in surr.points])
    assert np.all(np.isfinite(rows))
    evaluated = np.array([p.normed_coord for p in surr.points if p.label.name == "evaluated"])
    assert evaluated.shape[0] == surr.num_evaluated and np.unique(evaluated, axis=0).shape[0] == evaluated.shape[0]  # no duplicates
    assert np.all(np.isfinite(np.array(opt.trace, dtype=np.float64)))
    assert np.all(surr.last_hyper_info["accept_rate"] > 0.0)
    opt2, surr2, best2 = _marginal_run(3)
    rows2 = np.array([[*p.normed_coord, p.score_mu, p.score_sigma, p.score_ucb] for p in surr2.points])
    assert np.array_equal(rows, rows2) and opt.trace == opt2.trace and best == best2
    # MES, select_batch and what reads one theta are refused in words
    coords = synthetic_leaves(8, 2, seed=1)
    for fn in (lambda: surr.select_batch(coords, 2), lambda: surr.gp_eval_best_acq(coords, "mes"), lambda: surr.mes_select(coords)):
        with pytest.raises(ValueError, match="marginal"):
            fn()
    idx, mean, var, val = surr.gp_eval_best_acq(coords, "logei")
    cols = surr.gp_acq_values(coords, "logei")
    assert int(idx[0]) == int(np.argmax(cols[2])) and val[0] == cols[2].max()


def test_marginal_is_refused_where_it_does_not_apply():
    from pygpso_amd import GPRSurrogate
    from pygpso_amd.kernels import Matern52

    k = Matern52(lengthscales=0.25, variance=1.0)
    for kw in (dict(dtype="float32"), dict(devices=[0, 1]), dict(n_theta=33), dict(refit_every=3), dict(objective="loo")):
        with pytest.raises(ValueError):
            GPRSurrogate(gp_kernel=k, hyper="marginal", **kw)
    with pytest.raises(ValueError):
        GPRSurrogate(gp_kernel=k, hyper="bayes")
    assert GPRSurrogate(gp_kernel=k).hyper == "point"
    # the priors go to the surrogate's own copies: the caller's kernel stays as it was given
    surr = GPRSurrogate(gp_kernel=k, hyper="marginal")
    assert surr.gp_kernel is not k and surr.gp_kernel.lengthscales == k.lengthscales
    x = np.random.default_rng(0).random((6, 2))
    surr._gp_train(x, np.sin(3.0 * x[:, :1]))
    assert surr.gp_kernel.lengthscales_prior is not None and surr._ensemble_live
    assert k.lengthscales_prior is None and k.variance_prior is None
