"""
GPU tests of ``gpso_paths_draw_q`` (pathwise draws of the VGP, SGPR and SVGP posteriors) through the
C-ABI, with ``gpso_paths_eval`` / ``gpso_paths_info`` serving its set, and of the surrogates' ``thompson_select_leaves`` on
top, against the float64 oracle of tests/paths_q_oracle.py.  The cases, their shapes and their bar are tests/paths_q_cases.py's:
  values ..... 1e-8 of max(max|y|, sqrt(variance) max|w|) per case, section 7j's float64 stage tolerance; 1e-4 for the
               Matern-1/2.  On float64 AND mixed engines: the draw reads the double factors
  best_val ... the same bar
  best_idx ... the oracle's for every (draw, segment) pair whose two highest oracle values differ by ten times the bar or
               more; at most 5 % of the pairs may fall under that (tests/test_paths_q_cpu.py: none of these cases' does)
The achieved maxima are recorded in profiles/paths_q_parity.json by tools/paths_q_errors.py.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import gpr
from tests import paths_oracle as po
from tests import paths_q_cases as qc
from tests import vgp_studentt_oracle as T

pytestmark = pytest.mark.gpu
N_LS, TM = qc.N_LS, qc.TRAIN_MEAN


def _engine(dtype="float64", **kw):
    from pygpso_amd import HipGPEngine

    return HipGPEngine(dtype, **kw)


def install(eng, r):
    """The family's install of case ``r`` on ``eng`` (data, likelihood, Z and q already there or put there)."""
    a = (r["kernel"], r["u"], N_LS, TM, 0.0)
    if r["family"] == "vgp":
        eng.vgp_posterior(*a)
    elif r["family"] == "sgpr":
        eng.sgpr_posterior(*a)
    else:
        eng.svgp_posterior(*a)


def installed(r, dtype="float64"):
    eng = _engine(dtype)
    eng.set_data(r["X"], r["y"])
    if r["lik"][0] == "StudentT":
        eng.vgp_set_likelihood("StudentT", r["lik"][1], T.N_GH)
    if r["family"] == "vgp":
        eng.vgp_set_q(r["mu"], r["S"])
    else:
        eng.sgpr_set_inducing(r["Z"])
        if r["family"] == "svgp":
            eng.svgp_set_q(r["mu"], r["S"])
    install(eng, r)
    return eng


def drawn(r, dtype="float64"):
    eng = installed(r, dtype)
    eng.paths_draw_q(r["omega"], r["phase"], r["w"], r["eps"])
    return eng


def measure(got, r, seg_off=None):
    """(largest value error, largest best_val error, indices that differ among the decided pairs, undecided pairs, pairs)."""
    values, idx, val = got
    want_i, want_v = po.seg_argmax(r["values"], seg_off)
    decided = ~qc.undecided(r, seg_off)
    return (float(np.max(np.abs(values - r["values"]))), float(np.max(np.abs(val - want_v))),
            int(np.sum(idx[decided] != want_i[decided])), int(np.sum(~decided)), int(decided.size))


def _hold(got, r, what, seg_off=None):
    assert got[0].shape == r["values"].shape
    e_val, e_best, wrong, undecided, pairs = measure(got, r, seg_off)
    print(f"{what}: values {e_val:.2e}, best_val {e_best:.2e} (bar {r['tol']:.2e}), {undecided} of {pairs} pairs undecided, {wrong} indices differ")
    assert e_val <= r["tol"] and e_best <= r["tol"]
    assert 20 * undecided <= pairs and wrong == 0


# ---- 1. parity with the oracle on float64 and mixed engines ----------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(qc.CASES)))
def test_parity_with_the_oracle(index):
    r = qc.reference(index)
    for dtype in ("float64", "mixed"):
        eng = drawn(r, dtype)
        assert eng.paths_info() == r["w"].shape
        _hold(eng.paths_eval(r["Xs"]), r, f"paths_q {qc.name(index)} {dtype}")
        if r["Xs"].shape[0] == 130:
            _hold(eng.paths_eval(r["Xs"], seg_off=qc.SEGMENTS), r, f"paths_q {qc.name(index)} {dtype}, three segments", qc.SEGMENTS)
        eng.close()


@pytest.mark.parametrize("index", (2, 6, 10, 11))  # a Student-t VGP, an SGPR, a Student-t SVGP, an SVGP at 129 rows
def test_zero_weights_give_the_mean_of_predict_grad(index):
    """w = 0, eps = 0 (and eps NULL): every path equals ``gpso_predict_grad``'s mean on the same context to 1e-8 max|y|."""
    r = qc.reference(index)
    eng = installed(r)
    mean = eng.predict_grad(r["Xs"])[0]
    for eps in (np.zeros_like(r["eps"]), None):
        eng.paths_draw_q(r["omega"], r["phase"], np.zeros_like(r["w"]), eps)
        values = eng.paths_eval(r["Xs"])[0]
        err = float(np.max(np.abs(values - mean[None, :])) / np.max(np.abs(r["y"])))
        print(f"{qc.name(index)}: zero-weight paths against gpso_predict_grad's mean {err:.2e}")
        assert err <= 1e-8
    eng.close()


# ---- 2. bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", (3, 6))  # S = 129 on a VGP (lower Q) and on an SGPR (transposed Q)
def test_a_draws_bits_do_not_depend_on_s_and_null_eps_is_zeros(index):
    r = qc.reference(index)
    eng = drawn(r)
    Xs = r["Xs"]
    a = eng.paths_eval(Xs)[0]
    eng.paths_draw_q(r["omega"], r["phase"], r["w"], r["eps"])  # the same call again: the same set
    assert np.array_equal(eng.paths_eval(Xs)[0], a)
    for s in (0, 70, 128):  # a draw alone: the bits it has inside the 129
        eng.paths_draw_q(r["omega"], r["phase"], r["w"][s:s + 1], r["eps"][s:s + 1])
        assert eng.paths_info() == (1, r["w"].shape[1])
        assert np.array_equal(eng.paths_eval(Xs)[0][0], a[s])
    eng.paths_draw_q(r["omega"], r["phase"], r["w"][:17], np.zeros((17, r["eps"].shape[1])))
    zeros = eng.paths_eval(Xs)[0]
    eng.paths_draw_q(r["omega"], r["phase"], r["w"][:17], None)
    assert np.array_equal(eng.paths_eval(Xs)[0], zeros) and not np.array_equal(zeros, a[:17])
    eng.close()


@pytest.mark.parametrize("index", (1, 5, 10))  # one per family
def test_predict_type_calls_between_install_and_draw_change_no_bit_and_the_draw_changes_nothing_else(index):
    """``gpso_predict``, ``gpso_predict_grad`` and ``gpso_predict_joint`` touch none of Lf, beta, q's root or the SGPR's LB^-1
    (DESIGN.md section 3.1): a draw after them has the bits of a draw right after the install.  The draw and the evaluation
    leave ``gpso_posterior_hash`` and ``gpso_predict``'s bits alone."""
    r = qc.reference(index)
    Xs = r["Xs"][:40]
    eng = installed(r)
    h0, p0 = eng.posterior_hash(), eng.predict(Xs)
    eng.paths_draw_q(r["omega"], r["phase"], r["w"], r["eps"])
    want = eng.paths_eval(r["Xs"])[0]
    p1 = eng.predict(Xs)
    assert eng.posterior_hash() == h0 and np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])
    eng.close()
    eng = installed(r)
    eng.predict(Xs)
    eng.predict_grad(Xs)
    eng.predict_joint(Xs, 0.0)
    eng.paths_draw_q(r["omega"], r["phase"], r["w"], r["eps"])
    assert np.array_equal(eng.paths_eval(r["Xs"])[0], want)
    eng.set_timing(True)
    eng.paths_draw_q(r["omega"], r["phase"], r["w"], r["eps"])
    assert eng.last_ms(1) > 0.0 and np.array_equal(eng.paths_eval(r["Xs"])[0], want)
    eng.close()


def test_a_smaller_posterior_after_a_larger_one_gives_a_fresh_contexts_bits():
    """An SVGP context installed over 129 inducing rows, then over 33 (another D too): the larger problem's rows sit in the
    padding of Lf, q's root, beta and the scratch the draw rebuilds Lu^-1 in; nothing may read them."""
    big, r = qc.reference(11), qc.reference(10)
    used = installed(big)
    used.paths_draw_q(big["omega"], big["phase"], big["w"], big["eps"])
    used.set_data(r["X"], r["y"])
    used.vgp_set_likelihood("StudentT", r["lik"][1], T.N_GH)
    used.sgpr_set_inducing(r["Z"])
    used.svgp_set_q(r["mu"], r["S"])
    install(used, r)
    used.paths_draw_q(r["omega"], r["phase"], r["w"], r["eps"])
    fresh = drawn(r)
    for a, b in zip(used.paths_eval(r["Xs"]), fresh.paths_eval(r["Xs"])):
        assert np.array_equal(a, b)
    used.close()
    fresh.close()


# ---- 3. refusals and invalidation ------------------------------------------------------------------------------------------------
def _eval_code(eng, Xs):
    from pygpso_amd import _lib as L

    xs = np.ascontiguousarray(Xs, dtype=np.float64)
    m = xs.shape[0]
    values, idx, val = np.empty((256, m)), np.empty(256, dtype=np.int64), np.empty(256)
    return eng._lib.gpso_paths_eval(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, m, None, 1,
                                    C.c_void_p(values.ctypes.data), L.MEM_HOST, L.i64ptr(idx), L.dptr(val))


def _draw_code(eng, omega, phase, w, eps, s=None, f=None):
    from pygpso_amd import _lib as L

    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (omega, phase, w, eps)]
    return eng._lib.gpso_paths_draw_q(eng._h, L.dptr(arrs[0]), L.dptr(arrs[1]), w.shape[1] if f is None else f, L.dptr(arrs[2]),
                                      L.dptr(arrs[3]), w.shape[0] if s is None else s)


def test_every_status_and_a_refused_draw_leaves_the_old_set_serving():
    from pygpso_amd import _lib as L

    r = qc.reference(5)  # an SGPR over 17 inducing rows, D = 3, F = 5, S = 17
    Xs, args = r["Xs"], (r["omega"], r["phase"], r["w"], r["eps"])
    eng = _engine()
    assert _draw_code(eng, *args) == L.E_STATE                      # no posterior
    eng.set_data(r["X"], r["y"])
    eng.sgpr_set_inducing(r["Z"])
    assert _draw_code(eng, *args) == L.E_STATE                      # data and Z, nothing installed
    eng.sgpr_bound_u(r["kernel"], r["u"], N_LS, TM, 0.0)
    assert _draw_code(eng, *args) == L.E_STATE                      # an evaluation is no install
    install(eng, r)
    assert eng.paths_info() == (0, 0) and _eval_code(eng, Xs) == L.E_STATE
    eng.paths_draw_q(*args)
    want = eng.paths_eval(Xs)[0]
    # refused draws leave the set serving the same bits: s = 257, f = 0, a NaN in eps, a NULL, an open ticket
    bad_eps = r["eps"].copy()
    bad_eps[3, 1] = np.nan
    assert _draw_code(eng, r["omega"], r["phase"], np.zeros((257, 5)), np.zeros((257, 17))) == L.E_ARG
    assert _draw_code(eng, *args, f=0) == L.E_ARG
    assert _draw_code(eng, r["omega"], r["phase"], r["w"], bad_eps) == L.E_ARG
    assert eng._lib.gpso_paths_draw_q(eng._h, L.dptr(r["omega"]), None, 5, L.dptr(r["w"]), None, 17) == L.E_ARG
    ticket = eng.best_ucb_begin(Xs, gpr.VARSIGMA_DEFAULT)
    assert _draw_code(eng, *args) == L.E_STATE and _eval_code(eng, Xs) == L.E_STATE
    eng.best_ucb_end(ticket)
    assert eng.paths_info() == (17, 5) and np.array_equal(eng.paths_eval(Xs)[0], want)
    # gpso_paths_draw keeps its own answer on a variational posterior
    a = [np.ascontiguousarray(v) for v in args]
    assert eng._lib.gpso_paths_draw(eng._h, L.dptr(a[0]), L.dptr(a[1]), 5, L.dptr(a[2]), L.dptr(a[3]), 17) == L.E_STATE
    assert np.array_equal(eng.paths_eval(Xs)[0], want)
    # every invalidating transition ends the set; after each the draw needs a new install
    for change in (lambda: eng.sgpr_bound_u(r["kernel"], r["u"], N_LS, TM, 0.0), lambda: eng.sgpr_move_inducing(r["Z"] + 1e-3),
                   lambda: eng.sgpr_set_inducing(r["Z"]), lambda: eng.set_data(r["X"], r["y"])):
        if eng.paths_info() == (0, 0):
            eng.sgpr_set_inducing(r["Z"])
            install(eng, r)
            eng.paths_draw_q(*args)
        assert eng.paths_info() == (17, 5)
        change()
        assert eng.paths_info() == (0, 0) and _eval_code(eng, Xs) == L.E_STATE and _draw_code(eng, *args) == L.E_STATE
    eng.close()
    # a fitted exact GP, an installed posterior: gpso_paths_draw_q answers GPSO_E_STATE; a float32 context GPSO_E_ARG
    ex = _engine()
    ex.set_data(r["X"][:17], r["y"][:17])
    ex.fit_eval("Matern32", [0.4], 1.3, 1e-2, 0.0, want_grad=False)
    assert _draw_code(ex, *args) == L.E_STATE and "takes gpso_paths_draw" in ex.last_message()
    post = gpr.posterior(gpr.Theta("Matern32", [0.4], 1.3, 1e-2, 0.0), r["X"][:17], r["y"][:17])
    ex.set_posterior(r["X"][:17], post.L, post.alpha, "Matern32", [0.4], 1.3, 1e-2, 0.0)
    assert _draw_code(ex, *args) == L.E_STATE
    ex.close()
    e32 = _engine("float32")
    e32.set_data(r["X"][:17], r["y"][:17])
    e32.fit_eval("Matern32", [0.4], 1.3, 1e-2, 0.0, want_grad=False)
    assert _draw_code(e32, *args) == L.E_ARG
    e32.close()


def test_a_new_natural_gradient_step_and_install_end_the_set_and_the_next_one_is_the_new_qs():
    """SVGP: a set drawn from q, a natural-gradient step on the device (the set ends, the draw is refused until the
    install), the install, a new set: it matches the oracle's for the q the device now holds."""
    from pygpso_amd import _lib as L
    from tests import paths_q_oracle as pq

    r = qc.reference(9)
    Xs = r["Xs"][:65]
    args = (r["omega"], r["phase"], r["w"], r["eps"])
    eng = drawn(r)
    before = eng.paths_eval(Xs)[0]
    eng.svgp_natgrad(r["kernel"], r["u"], N_LS, TM, 0.0, 0.5)
    assert eng.paths_info() == (0, 0) and _eval_code(eng, Xs) == L.E_STATE and _draw_code(eng, *args) == L.E_STATE
    install(eng, r)
    assert eng.paths_info() == (0, 0)
    eng.paths_draw_q(*args)
    mu, S = eng.svgp_get_q()
    post = pq.svgp_posterior(r["kernel"], r["u"], N_LS, TM, 0.0, r["X"], r["Z"], mu, S, r["lik"])
    want = pq.path_values(post, *args, Xs)
    got = eng.paths_eval(Xs)[0]
    assert np.max(np.abs(got - want)) <= r["tol"] and not np.array_equal(got, before)
    eng.close()
    # a VGP the same way
    v = qc.reference(1)
    vargs = (v["omega"], v["phase"], v["w"], v["eps"])
    vg = drawn(v)
    vg.vgp_natgrad(v["kernel"], v["u"], N_LS, TM, 0.0, 0.5)
    assert vg.paths_info() == (0, 0) and _draw_code(vg, *vargs) == L.E_STATE
    install(vg, v)
    vg.paths_draw_q(*vargs)
    mu, S = vg.vgp_get_q()
    post = pq.vgp_posterior(v["kernel"], v["u"], N_LS, TM, 0.0, v["X"], mu, S, v["lik"])
    assert np.max(np.abs(vg.paths_eval(v["Xs"])[0] - pq.path_values(post, *vargs, v["Xs"]))) <= v["tol"]
    vg.close()


@pytest.mark.parametrize("sender", ["variational", "fitted"])
def test_an_adopted_posterior_ends_the_set_and_is_refused(sender):
    """The receiving context holds an installed SGPR posterior and a drawn set -- its own Lu, beta and LB^-1 stay in Lf,
    alpha_f and sgM2 --; a posterior is handed off onto it (the hand-off replayed with plain copies on one card, as
    tests/test_gpu_joint.py does): the set ends, ``gpso_paths_draw_q`` and ``gpso_paths_eval`` answer GPSO_E_STATE, and the
    adopted posterior serves the sender's predictions."""
    from pygpso_amd import _lib as L
    from tests.test_gpu_distributed import _handoff

    r = qc.reference(5)  # an SGPR over 17 inducing rows, D = 3
    Xs, args = r["Xs"], (r["omega"], r["phase"], r["w"], r["eps"])
    dst = drawn(r)
    assert dst.paths_info() == (17, 5)
    if sender == "variational":
        src = installed(r)
    else:
        src = _engine()
        src.set_data(r["X"][:17], r["y"][:17])
        src.fit_eval("Matern32", [0.4], 1.3, 1e-2, 0.0, want_grad=False)
    _handoff(src, dst)
    assert dst.paths_info() == (0, 0)
    assert _draw_code(dst, *args) == L.E_STATE and "gpso_vgp_posterior" in dst.last_message()
    assert _eval_code(dst, Xs) == L.E_STATE
    m0, v0 = src.predict(Xs)
    m1, v1 = dst.predict(Xs)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    assert _draw_code(dst, *args) == L.E_STATE and dst.paths_info() == (0, 0)
    # the sender is untouched: it still draws (a variational one) or is pointed at gpso_paths_draw (a fitted one)
    if sender == "variational":
        src.paths_draw_q(*args)
        _hold(src.paths_eval(Xs), r, "the sender after the hand-off")
    else:
        assert _draw_code(src, *args) == L.E_STATE and "takes gpso_paths_draw" in src.last_message()
    src.close()
    dst.close()


# ---- 4. the surrogates end to end ----------------------------------------------------------------------------------------------
def test_svgp_surrogate_thompson_select_leaves_over_2187_leaves_in_3_segments():
    from pygpso_amd import SVGPSurrogate
    from pygpso_amd import kernels as K

    rng = np.random.default_rng(5)
    coords = rng.random((60, 3))
    scores = np.sin(3.0 * coords[:, 0]) + coords[:, 1] ** 2 - coords[:, 2]
    surr = SVGPSurrogate(gp_kernel=K.Matern52(lengthscales=0.3, variance=1.0), gp_meanf=K.Constant(0.0), num_inducing=16,
                         train_iterations=3)
    surr.append(coords, scores)
    surr.gp_update()
    stored = list(surr.points)
    leaves = rng.random((2187, 3))
    seg = [0, 729, 1458, 2187]
    surr.gp_sample_paths(8, n_features=256, rng=7)
    f = surr.gp_eval_paths(leaves)
    idx, val = surr.thompson_select_leaves(leaves, seg_off=seg)
    want_i, want_v = po.seg_argmax(f, seg)
    assert f.shape == (8, 2187) and idx.shape == (8, 3) and np.array_equal(idx, want_i) and np.array_equal(val, want_v)
    assert not np.array_equal(f[0], f[1])  # (eight functions, not one eight times)
    surr.gp_sample_paths(8, n_features=256, rng=7)
    assert np.array_equal(surr.gp_eval_paths(leaves), f)
    assert list(surr.points) == stored


@pytest.mark.parametrize("which", ["VGP", "SGPR"])
def test_the_other_surrogates_sample_and_select(which):
    from pygpso_amd import SGPRSurrogate, VGPSurrogate
    from pygpso_amd import kernels as K

    rng = np.random.default_rng(6)
    coords = rng.random((40, 2))
    scores = np.sin(3.0 * coords[:, 0]) + coords[:, 1] ** 2
    kw = dict(gp_kernel=K.Matern52(lengthscales=0.3, variance=1.0), gp_meanf=K.Constant(0.0))
    surr = VGPSurrogate(train_iterations=3, **kw) if which == "VGP" else SGPRSurrogate(num_inducing=12, **kw)
    surr.append(coords, scores)
    surr.gp_update()
    leaves = rng.random((500, 2))
    surr.gp_sample_paths(4, n_features=128, rng=3)
    f = surr.gp_eval_paths(leaves)
    idx, val = surr.thompson_select_leaves(leaves)
    assert f.shape == (4, 500) and np.array_equal(idx[:, 0], np.argmax(f, axis=1)) and np.array_equal(val[:, 0], np.max(f, axis=1))
    assert not np.array_equal(f[0], f[1])
    surr.gp_sample_paths(4, n_features=128, rng=3)
    assert np.array_equal(surr.gp_eval_paths(leaves), f)
