"""
A context's history never changes a call's result bits.

One ``gpso_ctx`` serves a whole optimiser run and any C-ABI caller's mix of calls; its device buffers only grow and
keep their old bytes, and one host-side record (pygpso_amd/csrc/resident.hpp) says what is resident. The stages of
tests/context_stages.py are run here (a) on a fresh context, where they are held to the float64 oracle at the
tolerances the family's own test file states (imported from there, not restated), (b) on a second fresh context
(determinism), and (c) after every other stage, after failed calls, along seeded walks and along the optimiser's
growth path -- where every observable must equal the fresh run's bit for bit: fits and predictions are deterministic
(test_deterministic_bitwise, test_repeated_calls_give_identical_bits), so any difference is an effect of what the
context held before. No tolerance applies to (b) and (c).

Run on the GPU box with ``pytest -m gpu``.  test_fresh_results_are_the_oracles prints each stage's errors against the
oracle as a ``CONTEXT_REUSE_PARITY`` line (``-s`` shows them): the material for a profiles/ record.
"""
import numpy as np
import pytest

from oracle import gpr, tree
from tests import context_stages as CS
from tests import inducing_oracle as I
from tests import sgpr_oracle as S
from tests import svgp_oracle as O
from tests import vgp_oracle as V
from tests import vgp_studentt_oracle as T
from tests.helpers import synthetic_leaves, synthetic_problem, winner_is_the_oracles
from tests.test_gpu_parity import SMALL_FLOAT_BOUNDS, WINNER_GAP
from tests.test_gpu_sgpr import TOL

pytestmark = pytest.mark.gpu

DTYPES = ("float64", "mixed", "float32")
VS = gpr.VARSIGMA_DEFAULT
CASES = [(dt, name) for dt in DTYPES for name in CS.stages_for(dt)]


def _maker(dtype):
    def make():
        from pygpso_amd import HipGPEngine

        return HipGPEngine(dtype)

    return make


_FRESH, _SECOND = {}, {}


def fresh(dtype, name):
    """The stage on a context of its own: made once per (dtype, stage), shared by every test, never written to."""
    key = (dtype, name)
    if key not in _FRESH:
        _FRESH[key] = CS.run_stage(_maker(dtype), name)
    return _FRESH[key]


def nondeterminism(dtype, name):
    """Mismatches between two fresh contexts ([]: the stage is deterministic and its history tests mean something)."""
    key = (dtype, name)
    if key not in _SECOND:
        _SECOND[key] = CS.compare(name, CS.run_stage(_maker(dtype), name), fresh(dtype, name))
    return _SECOND[key]


def settled(dtype, names):
    """(the stages of ``names`` that are deterministic with their fresh results, the others)."""
    good = [n for n in names if not nondeterminism(dtype, n)]
    return {n: fresh(dtype, n) for n in good}, [n for n in names if n not in good]


# ---- fresh results are the oracle's ---------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _arr(obs, key):
    assert key in obs and not isinstance(obs[key], str), (key, obs.get(key))
    return np.asarray(obs[key])


def _check_predict(errs, dtype, obs, m_ref, v_ref, y, variance):
    """float64: 1e-9 of max(1, max|y|) and of sigma^2 (tests/test_gpu_parity.py::test_predict_fp64); float predict
    arithmetic: SMALL_FLOAT_BOUNDS of tests/test_gpu_parity.py."""
    mean, var = _arr(obs, "predict.mean"), _arr(obs, "predict.var")
    errs["var"] = float(np.max(np.abs(var - v_ref)) / variance)
    if dtype == "float64":
        errs["mean"] = float(np.max(np.abs(mean - m_ref)) / max(1.0, float(np.max(np.abs(y)))))
        assert errs["mean"] <= 1e-9 and errs["var"] <= 1e-9, errs
    else:
        errs["mean"] = float(np.max(np.abs(mean - m_ref)) / np.max(np.abs(y)))
        assert errs["mean"] <= SMALL_FLOAT_BOUNDS[0] and errs["var"] <= SMALL_FLOAT_BOUNDS[1], errs


def _check_winners(dtype, obs, key, ucb_segments, scale):
    idx, ucb = _arr(obs, key + ".idx"), _arr(obs, key + ".ucb")
    assert len(idx) == len(ucb_segments)
    for s, ref in enumerate(ucb_segments):
        if ref.size == 0:
            assert idx[s] == -1 and np.isnan(ucb[s]), (key, s)
        elif dtype == "float64":
            assert int(idx[s]) == int(np.argmax(ref)), (key, s)
            assert abs(ucb[s] - ref.max()) <= 1e-9 * scale, (key, s)
        else:
            winner_is_the_oracles(idx[s], ref, WINNER_GAP, f"context reuse {key}")


def _grown_segments(predict, p):
    out = []
    for bb in p.bounds:
        m, v = predict(tree.grow([tuple(r) for r in bb], p.depth))
        out.append(m + VS * v)
    return out


def _check_gpr(dtype, name, obs, errs):
    p = CS.inputs(name)
    double_fit = dtype != "float32"
    if name == "batch":  # tests/test_gpu_multistart.py: 1e-9 on the loss, 1e-7 of max(1, |g|) on the gradient; every dtype
        for tm, tag in ((True, "trained"), (False, "fixed")):
            loss, grad, ok = (_arr(obs, f"batch.mean_{tag}.{k}") for k in ("loss", "grad", "ok"))
            assert np.all(ok)
            for b, u in enumerate(p.U[tm]):
                f_ref, g_ref = gpr.loss_and_grad_unconstrained(CS.KERNEL, u if tm else np.append(u, p.c_fixed), p.X, p.y)
                g_ref = g_ref if tm else g_ref[:-1]
                errs[f"loss_{tag}"] = max(errs.get(f"loss_{tag}", 0.0), abs(loss[b] - f_ref) / abs(f_ref))
                errs[f"grad_{tag}"] = max(errs.get(f"grad_{tag}", 0.0), float(np.max(np.abs(grad[b] - g_ref) / np.maximum(1.0, np.abs(g_ref)))))
            assert errs[f"loss_{tag}"] <= 1e-9 and errs[f"grad_{tag}"] <= 1e-7, errs
        return
    if name == "failed_fit":
        assert obs["fit"].startswith("LinAlgError") and "pivot" in obs["fit"], obs
        return
    th = p.th
    post = p.post if name == "set_posterior" else gpr.posterior(th, p.X, p.y)
    m_ref, v_ref = gpr.predict_y(post, p.leaves)
    _check_predict(errs, dtype, obs, m_ref, v_ref, p.y, th.variance)
    if name == "set_posterior":
        return
    f_ref, g_ref = gpr.nlml_and_grad(th, p.X, p.y)
    tol_f, tol_g = (1e-9, 1e-8) if double_fit else (2e-5, 5e-3)  # test_fit_stages_fp64 / test_fit_and_predict_fp32
    if name.startswith("append"):
        assert bool(obs["append.in_place"]) == (name == "append_in_place")
        errs["nlml"] = abs(float(obs["append.nlml"]) - f_ref) / abs(f_ref)
    else:
        errs["nlml"] = abs(float(obs["fit.nlml"]) - f_ref) / abs(f_ref)
        if p.grad:
            errs["grad"] = float(np.max(np.abs(_arr(obs, "fit.grad") - g_ref) / np.maximum(1.0, np.abs(g_ref))))
            assert errs["grad"] < tol_g, errs
    assert errs["nlml"] <= tol_f, errs
    if double_fit:  # (a float32 context's factor has no stated bound of its own: its NLML, gradient and predictions do)
        Linv = np.linalg.inv(post.L)
        errs["chol"], errs["linv"] = _rel(_arr(obs, "chol"), post.L), _rel(_arr(obs, "linv"), Linv)
        errs["alpha"] = _rel(_arr(obs, "alpha"), post.alpha)
        assert errs["chol"] < 1e-9 and errs["linv"] < 1e-8 and errs["alpha"] < 1e-8, errs
        if "kinv" in obs:
            errs["kinv"] = _rel(_arr(obs, "kinv"), Linv.T @ Linv)
            assert errs["kinv"] < 1e-8, errs
    scale = max(1.0, float(np.max(np.abs(p.y))))
    if "grow.idx" in obs:
        _check_winners(dtype, obs, "grow", _grown_segments(lambda xs: gpr.predict_y(post, xs), p), scale)
    if "best_ucb.idx" in obs:
        ucb = m_ref + VS * v_ref
        _check_winners(dtype, obs, "best_ucb", [ucb[a:b] for a, b in zip(CS.SEG_RAGGED[:-1], CS.SEG_RAGGED[1:])], scale)


def _check_predict_var(errs, dtype, obs, m_ref, v_ref, y, variance):
    """The variational and sparse families: 1e-9 relative in float64 (test_predict_and_best_ucb_against_oracle of each
    file); mixed: 2e-5 sigma^2 and 1e-4 max(1, max|y|), the bounds of their mixed tests."""
    mean, var = _arr(obs, "predict.mean"), _arr(obs, "predict.var")
    if dtype == "float64":
        errs["mean"], errs["var"] = _rel(mean, m_ref), _rel(var, v_ref)
        assert errs["mean"] <= 1e-9 and errs["var"] <= 1e-9, errs
    else:
        errs["mean"] = float(np.max(np.abs(mean - m_ref)) / max(1.0, float(np.max(np.abs(y)))))
        errs["var"] = float(np.max(np.abs(var - v_ref)) / variance)
        assert errs["mean"] <= 1e-4 and errs["var"] <= 2e-5, errs


def _check_vgp(dtype, name, obs, errs):
    """tests/test_gpu_vgp.py / test_gpu_vgp_studentt.py: 2e-9 on q, the loss and the gradient, each step from the q the
    device held before it."""
    p = CS.inputs(name)
    n = p.X.shape[0]
    st = p.lik[0] == "StudentT"
    mu, Sq = np.zeros(n), np.eye(n)
    uu = p.u
    for k, (gamma, shift) in enumerate(p.steps):
        uu = p.u + shift
        assert f"natgrad{k}" not in obs, obs.get(f"natgrad{k}")
        if st:
            mu, Sq = T.natgrad(CS.KERNEL, uu, 1, True, 0.0, p.X, p.y, mu, Sq, p.lik, gamma)
        else:
            mu, Sq = V.natgrad(CS.KERNEL, uu, 1, True, 0.0, p.X, p.y, mu, Sq, gamma)
        dmu, dS = _arr(obs, f"q{k}.mu"), _arr(obs, f"q{k}.S")
        errs[f"q{k}"] = max(_rel(dmu, mu), _rel(dS @ dS.T, Sq @ Sq.T))
        assert errs[f"q{k}"] <= TOL, errs
        mu, Sq = dmu, dS
    if st:
        f_ref, g_ref, th_ref = T.neg_elbo_and_grad_u(CS.KERNEL, uu, 1, True, 0.0, p.X, p.y, mu, Sq, p.lik)
        post = T.Posterior(CS.KERNEL, uu, 1, True, 0.0, p.X, mu, Sq, p.lik, installed=True)
    else:
        f_ref, g_ref, th_ref = V.neg_elbo_and_grad_u(CS.KERNEL, uu, 1, True, 0.0, p.X, p.y, mu, Sq)
        post = V.Posterior(CS.KERNEL, uu, 1, True, 0.0, p.X, mu, Sq)
    errs["elbo"], errs["grad"] = abs(float(obs["elbo.loss"]) - f_ref) / abs(f_ref), _rel(_arr(obs, "elbo.grad"), g_ref)
    assert errs["elbo"] <= TOL and errs["grad"] <= TOL, errs
    np.testing.assert_allclose(_arr(obs, "elbo.theta"), th_ref, rtol=1e-15)
    assert "posterior" not in obs, obs.get("posterior")
    m_ref, v_ref = post.predict_y(p.leaves)
    _check_predict_var(errs, dtype, obs, m_ref, v_ref, p.y, post.var)
    _check_winners(dtype, obs, "grow", _grown_segments(post.predict_y, p), max(1.0, float(np.max(np.abs(p.y)))))


def _check_sgpr(dtype, name, obs, errs):
    """tests/test_gpu_sgpr.py / test_gpu_inducing.py: TOL = 2e-9 on the factors, the bound, its gradients, C and beta."""
    p = CS.inputs(name)
    if name == "sgpr_moved":
        Z = p.Z1
        f_ref, g_ref, gz_ref = I.sgpr_loss_and_grads(CS.KERNEL, p.u, p.n_ls, True, 0.0, p.X, p.y, Z)
        errs["grad_z"] = _rel(_arr(obs, "bound.grad_z"), gz_ref)
        assert errs["grad_z"] <= TOL, errs
    else:
        ls, var, _, _ = S.unpack(p.u, p.n_ls, True)
        picks = S.greedy_select(CS.KERNEL, p.X, ls, var, p.m)
        np.testing.assert_array_equal(_arr(obs, "picks"), picks)
        Z = p.X[picks]
        f_ref, g_ref, _ = S.neg_bound_and_grad_u(CS.KERNEL, p.u, p.n_ls, True, 0.0, p.X, p.y, Z)
    np.testing.assert_array_equal(_arr(obs, "inducing.Z"), Z)
    assert int(obs["inducing.n_data"]) == p.X.shape[0]
    fac = S.factors(CS.KERNEL, p.u, p.n_ls, True, 0.0, p.X, p.y, Z)
    for which, ref in (("Kuf", fac.Kuf), ("Lu", fac.Lu), ("LB", fac.LB), ("cv", fac.cv)):
        errs[which] = _rel(_arr(obs, which), ref)
    errs["bound"], errs["grad"] = abs(float(obs["bound.loss"]) - f_ref) / abs(f_ref), _rel(_arr(obs, "bound.grad_u"), g_ref)
    post = S.Posterior(CS.KERNEL, p.u, p.n_ls, True, 0.0, p.X, p.y, Z)
    C_ref, beta_ref, _, d_ref = post.installed()
    errs["C"], errs["beta"] = _rel(_arr(obs, "linv"), C_ref), _rel(_arr(obs, "alpha"), beta_ref)
    assert all(errs[k] <= TOL for k in ("Kuf", "Lu", "LB", "cv", "bound", "grad", "C", "beta")), errs
    assert float(obs["delta"]) == d_ref == 0.0
    m_ref, v_ref = post.predict_y(p.leaves)
    _check_predict_var(errs, dtype, obs, m_ref, v_ref, p.y, post.f.var)


def _check_svgp(dtype, name, obs, errs):
    """tests/test_gpu_svgp.py / test_gpu_inducing.py: TOL = 2e-9, each step from the q the device held before it; the
    predictive is the installed form."""
    p = CS.inputs(name)
    assert "init_q" not in obs, obs.get("init_q")
    mu, Sq = O.conjugate_start(CS.KERNEL, p.u, 1, True, 0.0, p.X, p.y, p.Z0, p.lik, p.s2)
    dmu, dS = _arr(obs, "q0.mu"), _arr(obs, "q0.S")
    errs["q0"] = max(_rel(dmu, mu), _rel(dS, Sq))
    mu, Sq, Z = dmu, dS, p.Z0
    if name == "svgp":
        for k in (1, 2):
            try:
                mu_r, S_r = O.natgrad(CS.KERNEL, p.u, 1, True, 0.0, p.X, p.y, Z, mu, Sq, p.lik, 0.5)
            except np.linalg.LinAlgError:  # (an indefinite step: the device must say so and keep q)
                assert obs.get(f"natgrad{k}", "").startswith("LinAlgError"), (k, obs.get(f"natgrad{k}"))
                np.testing.assert_array_equal(_arr(obs, f"q{k}.mu"), mu)
                continue
            assert f"natgrad{k}" not in obs, obs.get(f"natgrad{k}")
            dmu, dS = _arr(obs, f"q{k}.mu"), _arr(obs, f"q{k}.S")
            errs[f"q{k}"] = max(_rel(dmu, mu_r), _rel(dS, S_r))
            mu, Sq = dmu, dS
        f_ref, g_ref, th_ref = O.neg_elbo_and_grad_u(CS.KERNEL, p.u, 1, True, 0.0, p.X, p.y, Z, mu, Sq, p.lik)
    else:
        Z = p.Z1
        f_ref, g_ref, gz_ref = I.svgp_loss_and_grads(CS.KERNEL, p.u, 1, True, 0.0, p.X, p.y, Z, mu, Sq, p.lik)
        errs["grad_z"] = _rel(_arr(obs, "elbo.grad_z"), gz_ref)
        np.testing.assert_array_equal(_arr(obs, "q1.mu"), mu)  # q is kept while Z moves
        np.testing.assert_array_equal(_arr(obs, "q1.S"), Sq)
    errs["elbo"], errs["grad"] = abs(float(obs["elbo.loss"]) - f_ref) / abs(f_ref), _rel(_arr(obs, "elbo.grad_u"), g_ref)
    post = O.Posterior(CS.KERNEL, p.u, 1, True, 0.0, p.X, Z, mu, Sq, p.lik)
    C_ref, beta_ref, _, d_ref = post.installed()
    errs["C"], errs["beta"] = _rel(_arr(obs, "linv"), C_ref), _rel(_arr(obs, "alpha"), beta_ref)
    assert all(v <= TOL for v in errs.values()), errs
    assert float(obs["delta"]) == d_ref
    m_ref, v_ref = post.predict_y_installed(p.leaves)
    _check_predict_var(errs, dtype, obs, m_ref, v_ref, p.y, post.f.var)


@pytest.mark.parametrize("dtype,name", CASES)
def test_fresh_results_are_the_oracles(dtype, name):
    obs, errs = fresh(dtype, name), {}
    check = (_check_vgp if name.startswith("vgp") else _check_sgpr if name.startswith("sgpr") else
             _check_svgp if name.startswith("svgp") else _check_gpr)
    try:
        check(dtype, name, obs, errs)
    finally:
        print(f"CONTEXT_REUSE_PARITY dtype={dtype} stage={name} " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))


# ---- determinism first ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,name", CASES)
def test_a_second_fresh_context_gives_the_same_bits(dtype, name):
    bad = nondeterminism(dtype, name)
    assert not bad, "non-determinism (two fresh contexts differ; no history involved):\n  " + "\n  ".join(map(str, bad))


def _require_deterministic(dtype, name):
    if nondeterminism(dtype, name):
        pytest.skip(f"{name} is not deterministic in {dtype} contexts (test_a_second_fresh_context_gives_the_same_bits reports it): "
                    "a history effect cannot be told from it")


# ---- all ordered pairs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,first", CASES)
def test_all_ordered_pairs(dtype, first):
    """A context runs ``first``, then B, for every stage B (B = first included): B's observables are the fresh B's."""
    _require_deterministic(dtype, first)
    want, _ = settled(dtype, CS.stages_for(dtype))
    bad = CS.pair_mismatches(_maker(dtype), first, list(want), want)
    assert not bad, CS.report(bad)


# ---- the batch leaves the resident posterior alone ----------------------------------------------------------------------
def _resident(eng, leaves):
    obs = {}
    CS.posterior_observables(eng, obs, leaves)
    return obs


@pytest.mark.parametrize("dtype,name", [c for c in CASES if c[1] not in CS.NO_POSTERIOR])
def test_the_batch_leaves_the_resident_posterior_alone(dtype, name):
    """tests/test_gpu_multistart.py::test_the_batch_leaves_the_context_alone for every family: predictions, hash, the
    matrices and vectors the getters return are the same bits before and after a ``gpso_fit_eval_u_batch`` on the rows the
    context holds -- whether the batch runs (the one-launch fit applies to what is resident) or is refused (N > 128)."""
    import ctypes as C

    from pygpso_amd import _lib as L

    eng = _maker(dtype)()
    CS.STAGES[name](eng)
    d = eng.d
    leaves = synthetic_leaves(257, d, seed=7)
    before = _resident(eng, leaves)
    assert "predict.mean" in before and not isinstance(before.get("hash"), str), before.keys()
    U = CS.u_rows(5, d, 1, True, seed=5)
    f, g = np.full(5, np.nan), np.full(U.shape, np.nan)
    st = np.full(5, 99, dtype=np.intc)
    cap = eng.fit_batch_max()
    rc = eng._lib.gpso_fit_eval_u_batch(eng._h, L.MATERN32, L.dptr(U), 5, 1, 1, 0.0, L.dptr(f), L.dptr(g),
                                        st.ctypes.data_as(C.POINTER(C.c_int)), None)
    if cap > 0:
        assert rc == L.OK, eng.last_message()
    else:
        assert rc in (L.E_ARG, L.E_STATE), (rc, eng.last_message())
    bad = CS.compare(name, _resident(eng, leaves), before)
    eng.close()
    assert not bad, f"batch (fit_batch_max {cap}, rc {rc}) changed the resident posterior:\n" + CS.report(bad)


# ---- a failed call changes nothing it should not -------------------------------------------------------------------------
def _failed_append(eng):  # tests/test_gpu_append.py::test_a_block_that_is_not_positive_definite_leaves_the_posterior_alone
    n, d = 300, 3
    X, y = synthetic_problem(n, d, seed=11)
    eng.set_data(X, y)
    eng.fit_eval("Matern52", 0.25 * np.sqrt(d) * np.ones(1), 1.3, 1e-6, float(y.mean()))
    with pytest.raises(np.linalg.LinAlgError, match="pivot"):
        eng.append(np.vstack([X[:2], np.full((1, d), np.nan)]), np.zeros(3))


def _failed_vgp_step(eng):  # tests/test_gpu_vgp_studentt.py::test_indefinite_step_raises_and_keeps_q
    X, y = synthetic_problem(40, 2, seed=8)
    y = y.copy()
    y[7] += 30.0
    rng = np.random.default_rng(9)
    mu0 = 0.2 * rng.normal(size=40)
    S0 = np.tril(0.05 * rng.normal(size=(40, 40)), -1) + np.diag(0.6 + 0.3 * rng.random(40))
    eng.set_data(X, y)
    eng.vgp_set_likelihood("StudentT", 3.0, T.N_GH)
    eng.vgp_set_q(mu0, S0)
    with pytest.raises(np.linalg.LinAlgError):
        eng.vgp_natgrad("Matern52", T.initial_u(0.3, 1.0, 0.05, 0.0), 1, True, 0.0, 1.0)


def _failed_svgp_step(eng):  # tests/test_gpu_svgp.py::test_indefinite_step_keeps_q
    from tests.test_gpu_svgp import OUT_LIK, _outlier_problem

    X, y, _, _ = _outlier_problem()
    u = O.initial_u(0.3, 1.0, 0.2, OUT_LIK, c=0.0)
    eng.set_data(X, y)
    eng.vgp_set_likelihood("StudentT", 3.0, T.N_GH)
    eng.sgpr_select_inducing("Matern52", u, 1, 64)
    eng.svgp_set_q()
    with pytest.raises(np.linalg.LinAlgError):
        for _ in range(2):
            eng.svgp_natgrad("Matern52", u, 1, False, 0.0, 0.1)


FAILURES = {"append": (_failed_append, DTYPES), "vgp_step": (_failed_vgp_step, DTYPES[:2]), "svgp_step": (_failed_svgp_step, DTYPES[:2])}


@pytest.mark.parametrize("dtype,failure", [(dt, k) for k, (_, dts) in FAILURES.items() for dt in dts])
def test_a_stage_after_a_failed_call_equals_fresh(dtype, failure):
    """(The failed fit is a stage of its own: test_all_ordered_pairs[*-failed_fit] is ``failed_fit``, B for every B.)"""
    want, _ = settled(dtype, CS.stages_for(dtype))
    bad = []
    for b in want:
        eng = _maker(dtype)()
        FAILURES[failure][0](eng)
        bad += CS.compare(b, CS.STAGES[b](eng), want[b])
        eng.close()
    assert not bad, f"after a failed {failure}: " + CS.report(bad)


# ---- seeded walks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("dtype", DTYPES)
def test_seeded_walks(dtype, seed):
    want, _ = settled(dtype, CS.stages_for(dtype))
    sequence = CS.walk_sequence(list(want), seed, steps=12)
    bad = CS.walk_mismatches(_maker(dtype), sequence, want)
    assert not bad, f"walk {sequence}: " + CS.report(bad)


# ---- the optimiser's growth path ------------------------------------------------------------------------------------------
GROWTH_N = (100, 127, 128, 129, 200, 255, 256, 257, 300)
GROWTH_D, GROWTH_M = 4, 32


@pytest.fixture(scope="module")
def growth_data():
    X, y = synthetic_problem(GROWTH_N[-1], GROWTH_D, seed=7)
    return X, y, synthetic_leaves(300, GROWTH_D, seed=8), CS.grow_bounds(GROWTH_D)


def _growth_step(eng, family, n, data, q=None, extend=False, q_out=None):
    """One step of the path at N = n -> observables.  ``q``: the variational state to install first (the fresh side of the
    VGP chain); ``extend``: ``vgp_extend_q`` after ``set_data`` (the chain side); ``q_out``: receives the q the step started from."""
    X, y, leaves, bounds = data
    obs = {}
    eng.set_data(X[:n], y[:n])
    c = float(y.mean())
    if family == "gpr":
        CS._try(obs, "fit", lambda: eng.fit_eval("Matern52", 0.25 * np.sqrt(GROWTH_D) * np.ones(1), 1.3, 1e-3, c), ("nlml", "grad"))
    elif family == "vgp":
        u = V.initial_u(0.3 * np.sqrt(GROWTH_D), 1.1, 0.01, 0.05)
        eng.vgp_set_likelihood("Gaussian")
        if extend:
            eng.vgp_extend_q()
        elif q is not None:
            eng.vgp_set_q(*q)
        else:
            eng.vgp_set_q()
        if q_out is not None:
            q_out.append(eng.vgp_get_q())
        eng.vgp_natgrad("Matern52", u, 1, True, 0.0, 0.5)
        CS._try(obs, "q", lambda: eng.vgp_get_q(), ("mu", "S"))
        CS._try(obs, "elbo", lambda: eng.vgp_elbo_u("Matern52", u, 1, True, 0.0), ("loss", "grad", "theta"))
        eng.vgp_posterior("Matern52", u, 1, True, 0.0)
    else:
        lik = CS.LIK_SVGP_T if family == "svgp" else CS.GAUSS
        u = O.initial_u(0.3 * np.sqrt(GROWTH_D), 1.1, 1.0 if family == "svgp" else 0.01, lik, c=0.05)
        CS._set_likelihood(eng, obs, lik)
        CS._try(obs, "picks", lambda: eng.sgpr_select_inducing("Matern52", u, 1, GROWTH_M))
        if family == "sgpr":
            CS._try(obs, "bound", lambda: eng.sgpr_bound_u("Matern52", u, 1, True, 0.0), ("loss", "grad", "theta"))
            CS._try(obs, "delta", lambda: eng.sgpr_posterior("Matern52", u, 1, True, 0.0))
        else:
            eng.svgp_init_q("Matern52", u, 1, True, 0.0, O.predictive_noise(lik, O.unpack(u, 1, True, 0.0, lik)[2]))
            CS._try(obs, "natgrad", lambda: eng.svgp_natgrad("Matern52", u, 1, True, 0.0, 0.5))
            CS._try(obs, "q", lambda: eng.svgp_get_q(), ("mu", "S"))
            CS._try(obs, "elbo", lambda: eng.svgp_elbo_u("Matern52", u, 1, True, 0.0), ("loss", "grad", "theta"))
            CS._try(obs, "delta", lambda: eng.svgp_posterior("Matern52", u, 1, True, 0.0))
    CS._try(obs, "predict", lambda: eng.predict(leaves), ("mean", "var"))
    CS._try(obs, "grow", lambda: eng.best_ucb_grow(bounds, 5, VS), CS.WIN)
    CS._try(obs, "hash", lambda: eng.posterior_hash())
    CS._try(obs, "padded_n", lambda: eng.padded_n)
    info = CS._try(obs, "precision_info", lambda: eng.precision_info())  # (slots 10 and 11: the arithmetic the auto ladder settled on)
    if info is not None:
        del obs["precision_info"]
        obs["generation"], obs["predict_math"] = info["generation"], info["predict_math"]
    return obs


@pytest.mark.parametrize("direction", ["up", "down"])
@pytest.mark.parametrize("family,dtype", [("gpr", dt) for dt in DTYPES] + [(f, dt) for f in ("sgpr", "svgp", "vgp") for dt in DTYPES[:2]])
def test_the_growth_path_equals_fresh_contexts(family, dtype, direction, growth_data):
    """One context walks N = 100 .. 300 (or back) across the one-launch limit and the padded sizes, predict math on its
    default; each step equals a context that was given that N alone.  The VGP's q travels with ``vgp_extend_q`` on the
    way up; the fresh side is handed the q the chain's step started from."""
    make = _maker(dtype)
    chain = make()
    bad = []
    ns = GROWTH_N if direction == "up" else GROWTH_N[::-1]
    for k, n in enumerate(ns):
        q_seen = []
        extend = family == "vgp" and direction == "up" and k > 0
        got = _growth_step(chain, family, n, growth_data, extend=extend, q_out=q_seen if family == "vgp" else None)
        one = make()
        want = _growth_step(one, family, n, growth_data, q=q_seen[0] if extend else None)
        one.close()
        assert "predict.mean" in want and not isinstance(want.get("hash"), str), (n, want.keys())
        for m in CS.compare(f"{family} N={n}", got, want):
            m.note = f"step {k} of {list(ns)}"
            bad.append(m)
    chain.close()
    assert not bad, CS.report(bad)


def test_a_change_of_d_on_the_same_context():
    """d = 12 -> 3 -> 33 -> 1 at n = 130 on one context per dtype: fit and predict equal a fresh context's."""
    bad = []
    for dtype in DTYPES:
        chain = _maker(dtype)()
        for d in (12, 3, 33, 1):
            X, y, th = CS._problem(130, d, ard=d > 1)
            leaves = synthetic_leaves(257, d)
            res = []
            for eng in (chain, _maker(dtype)()):
                obs = {}
                CS._fit(eng, obs, X, y, th, True)
                CS.posterior_observables(eng, obs, leaves)
                res.append(obs)
                if eng is not chain:
                    eng.close()
            assert "predict.mean" in res[1], res[1].keys()
            bad += CS.compare(f"{dtype} d={d}", res[0], res[1])
        chain.close()
    assert not bad, CS.report(bad)
