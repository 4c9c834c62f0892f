"""
GPU tests of ``gpso_paths_draw`` / ``gpso_paths_eval`` / ``gpso_paths_info`` (pathwise posterior draws)
through the C-ABI, and of ``GPSurrogate.thompson_select_leaves`` on top of them, against the float64 oracle of
tests/paths_oracle.py.  The parity cases, their shapes and their tolerance are tests/paths_cases.py's:
  values ..... 1e-8 of max(max|y|, sqrt(variance) max|w|) per case, the project's float64 stage tolerance; 1e-4 for the
               Matern-1/2 (section 7h's reason).  They hold on float64 AND mixed engines: both calls read the dense double factor
  best_val ... the same tolerance, always
  best_idx ... the oracle's, wherever the oracle's two highest values of that (draw, segment) differ by more than twice the
               tolerance (tests/test_paths_cpu.py: no pair of these cases is excluded by that rule)
The achieved maxima are recorded in profiles/paths_parity.json by tools/paths_errors.py.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import gpr
from tests import paths_cases as pc
from tests import paths_oracle as po
from tests.helpers import synthetic_problem

pytestmark = pytest.mark.gpu


def _engine(dtype="float64", **kw):
    from pygpso_amd import HipGPEngine

    return HipGPEngine(dtype, **kw)


def fitted(r, dtype="float64"):
    eng = _engine(dtype)
    eng.set_data(r["X"], r["y"])
    if r["s"] is not None:
        eng.set_noise_diag(r["s"])
    th = r["th"]
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    return eng


def drawn(r, dtype="float64"):
    eng = fitted(r, dtype)
    eng.paths_draw(r["omega"], r["phase"], r["w"], r["eps"])
    return eng


def _hold(got, r, what, seg_off=None):
    values, idx, val = got
    want_i, want_v = po.seg_argmax(r["values"], seg_off)
    e_val = float(np.max(np.abs(values - r["values"])))
    e_best = float(np.max(np.abs(val - want_v)))
    decided = po.top_two_gap(r["values"], seg_off) > 2.0 * r["tol"]
    print(f"{what}: values {e_val:.2e}, best_val {e_best:.2e} (tolerance {r['tol']:.2e}), {int(np.sum(~decided))} pairs undecided")
    assert values.shape == r["values"].shape and idx.shape == want_i.shape
    assert e_val <= r["tol"] and e_best <= r["tol"]
    assert np.array_equal(idx[decided], want_i[decided])


# ---- 1. parity with the oracle on float64 and mixed engines ----------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(pc.CASES)))
def test_parity_with_the_oracle(index):
    r = pc.reference(index)
    for dtype in ("float64", "mixed"):
        eng = drawn(r, dtype)
        assert eng.paths_info() == (r["w"].shape[0], r["w"].shape[1])
        _hold(eng.paths_eval(r["Xs"]), r, f"paths {pc.name(index)} {dtype}")
        if r["Xs"].shape[0] == 130:
            _hold(eng.paths_eval(r["Xs"], seg_off=pc.SEGMENTS), r, f"paths {pc.name(index)} {dtype}, three segments", pc.SEGMENTS)
        eng.close()


def test_zero_weights_give_the_posterior_mean_of_predict_grad():
    """w = 0, eps = 0 (and eps NULL): every path equals ``gpso_predict_grad``'s mean on the same context to 1e-8 max|y|."""
    for index in (4, 7):
        r = pc.reference(index)
        for dtype in ("float64", "mixed"):
            eng = fitted(r, dtype)
            mean = eng.predict_grad(r["Xs"])[0]
            for eps in (np.zeros_like(r["eps"]), None):
                eng.paths_draw(r["omega"], r["phase"], np.zeros_like(r["w"]), eps)
                values = eng.paths_eval(r["Xs"])[0]
                err = float(np.max(np.abs(values - mean[None, :])) / np.max(np.abs(r["y"])))
                print(f"{pc.name(index)} {dtype}: zero-weight paths against gpso_predict_grad's mean {err:.2e}")
                assert err <= 1e-8
            eng.close()


# ---- 2. segments -------------------------------------------------------------------------------------------------------------
def test_segments_empty_ones_and_ties():
    r = pc.reference(5)
    eng = drawn(r)
    values, idx, val = eng.paths_eval(r["Xs"])
    # an empty segment in front, between and behind: -1 and a NaN, the others as without them
    seg = np.array([0, 0, 1, 70, 70, 130, 130])
    _, i6, v6 = eng.paths_eval(r["Xs"], seg_off=seg)
    _, i3, v3 = eng.paths_eval(r["Xs"], seg_off=pc.SEGMENTS)
    assert np.all(i6[:, [0, 3, 5]] == -1) and np.all(np.isnan(v6[:, [0, 3, 5]]))
    assert np.array_equal(i6[:, [1, 2, 4]], i3) and np.array_equal(v6[:, [1, 2, 4]], v3)
    want_i, want_v = po.seg_argmax(values, pc.SEGMENTS)  # (the device's own values: exact)
    assert np.array_equal(i3, want_i) and np.array_equal(v3, want_v)
    # ties: bit-identical copies of draw 0's winning row behind the batch, in another tile -- the original index wins
    win = int(idx[0, 0])
    more = np.vstack([r["Xs"], np.repeat(r["Xs"][win:win + 1], 70, axis=0)])
    v2, i2, b2 = eng.paths_eval(more)
    assert np.array_equal(v2[:, 130:], np.repeat(v2[:, win:win + 1], 70, axis=1))
    assert int(i2[0, 0]) == win and b2[0, 0] == val[0, 0]
    # ... and across chunks: the copies behind a full chunk
    far = np.vstack([r["Xs"], np.tile(r["Xs"][:1], (pc.CHUNK, 1)), r["Xs"][win:win + 1]])
    _, i4, b4 = eng.paths_eval(far, want_values=False)
    assert int(i4[0, 0]) == win and b4[0, 0] == val[0, 0]


# ---- 3. bits -----------------------------------------------------------------------------------------------------------------
def test_same_bits_again_alone_permuted_and_whatever_s():
    r = pc.reference(7)
    eng = drawn(r)
    Xs = r["Xs"]
    a, ia, va = eng.paths_eval(Xs)
    b, ib, vb = eng.paths_eval(Xs)
    assert np.array_equal(a, b) and np.array_equal(ia, ib) and np.array_equal(va, vb)
    # the same draw call again: the same set
    eng.paths_draw(r["omega"], r["phase"], r["w"], r["eps"])
    assert np.array_equal(eng.paths_eval(Xs)[0], a)
    # a point alone, in a batch and in a permuted batch
    assert np.array_equal(eng.paths_eval(Xs[77:78])[0][:, 0], a[:, 77])
    perm = np.random.default_rng(1).permutation(Xs.shape[0])
    assert np.array_equal(eng.paths_eval(Xs[perm])[0], a[:, perm])
    # draw 0 of the S = 16 set against an S = 1 set and an S = 17 set of the same randoms
    extra_w = np.random.default_rng(2).standard_normal((1, r["w"].shape[1]))
    extra_e = np.random.default_rng(3).standard_normal((1, r["eps"].shape[1]))
    eng.paths_draw(r["omega"], r["phase"], r["w"][:1], r["eps"][:1])
    assert np.array_equal(eng.paths_eval(Xs)[0][0], a[0])
    eng.paths_draw(r["omega"], r["phase"], np.vstack([r["w"], extra_w]), np.vstack([r["eps"], extra_e]))
    assert np.array_equal(eng.paths_eval(Xs)[0][:16], a)


def test_chunking_does_not_change_a_points_bits():
    """The points of the case that crosses the chunk: the three behind it again as a call of their own."""
    r = pc.reference(10)
    eng = drawn(r)
    values = eng.paths_eval(r["Xs"])[0]
    assert np.array_equal(eng.paths_eval(r["Xs"][pc.CHUNK:])[0], values[:, pc.CHUNK:])
    assert np.array_equal(eng.paths_eval(r["Xs"][pc.CHUNK - 30:pc.CHUNK + 1])[0], values[:, pc.CHUNK - 30:pc.CHUNK + 1])


def test_device_points_and_device_values_equal_the_host_path():
    import torch

    r = pc.reference(7)
    eng = drawn(r)
    host = eng.paths_eval(r["Xs"])
    dev = torch.device("cuda", eng.device)
    xt = torch.from_numpy(r["Xs"]).to(dev)
    out = torch.empty(16, 130, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    values, idx, val = eng.paths_eval(xt, out=out)
    assert np.array_equal(host[0], out.cpu().numpy()) and np.array_equal(host[1], idx) and np.array_equal(host[2], val)
    _, idx, val = eng.paths_eval(xt, want_values=False)
    assert np.array_equal(host[1], idx) and np.array_equal(host[2], val)
    eng.set_timing(True)
    eng.paths_eval(xt, want_values=False)
    assert eng.last_ms(1) > 0.0 and eng.last_count(0) == 130 and eng.last_count(1) == 130
    eng.paths_draw(r["omega"], r["phase"], r["w"], r["eps"])
    assert eng.last_ms(1) > 0.0


# ---- 4. the posterior moves on -------------------------------------------------------------------------------------------------
def test_after_an_append_the_old_set_is_refused_and_a_new_one_matches():
    """k = 3 points appended in place to N = 300: the set drawn before is refused; a new one against the oracle's
    from-scratch posterior of the 303."""
    from pygpso_amd import _lib as L

    r = pc.append_case()
    X, y, th, Xs = r["X"], r["y"], r["th"], r["Xs"]
    eng = _engine()
    eng.set_data(X[:300], y[:300])
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    eng.paths_draw(r["omega"], r["phase"], r["w"], r["eps"][:, :300])
    eng.paths_eval(Xs)
    _, in_place = eng.append(X[300:], y[300:])
    assert in_place and eng.paths_info() == (0, 0) and _eval_code(eng, Xs) == L.E_STATE
    eng.paths_draw(r["omega"], r["phase"], r["w"], r["eps"])
    _hold(eng.paths_eval(Xs), r, "paths after gpso_append")


def test_a_smaller_problem_after_a_larger_one_gives_a_fresh_contexts_bits():
    """A mixed context fitted at N = 500, then at N = 300 (N_pad = 512 both times): the larger problem's rows sit in the
    padding of the factor, the targets and the scaled inputs; nothing may read them."""
    X, y = synthetic_problem(500, 5, seed=3)
    th = ("Matern52", [0.6], 1.3, 1.0e-3, float(y.mean()))
    Xs = pc.points_at(70, 5)
    omega, phase, w, eps = pc.inputs("Matern52", 3, 20, 300, 5, seed=4)
    used = _engine("mixed")
    for n in (500, 300):
        used.set_data(X[:n], y[:n])
        used.fit_eval(*th, want_grad=False)
    used.paths_draw(omega, phase, w, eps)
    fresh = _engine("mixed")
    fresh.set_data(X[:300], y[:300])
    fresh.fit_eval(*th, want_grad=False)
    fresh.paths_draw(omega, phase, w, eps)
    for a, b in zip(used.paths_eval(Xs), fresh.paths_eval(Xs)):
        assert np.array_equal(a, b)


# ---- 5. refusals and invalidation ------------------------------------------------------------------------------------------------
def _eval_code(eng, Xs):
    """The status gpso_paths_eval itself returns for host points and host outputs."""
    from pygpso_amd import _lib as L

    xs = np.ascontiguousarray(Xs, dtype=np.float64)
    m = xs.shape[0]
    values, idx, val = np.empty((256, m)), np.empty(256, dtype=np.int64), np.empty(256)
    return eng._lib.gpso_paths_eval(eng._h, C.c_void_p(xs.ctypes.data), L.F64, L.MEM_HOST, m, None, 1,
                                    C.c_void_p(values.ctypes.data), L.MEM_HOST, L.i64ptr(idx), L.dptr(val))


def _draw_code(eng, omega, phase, w, eps, s=None, f=None):
    from pygpso_amd import _lib as L

    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (omega, phase, w, eps)]
    return eng._lib.gpso_paths_draw(eng._h, L.dptr(arrs[0]), L.dptr(arrs[1]), w.shape[1] if f is None else f, L.dptr(arrs[2]),
                                    L.dptr(arrs[3]), w.shape[0] if s is None else s)


def test_refusals_invalidation_and_nothing_else_moves():
    from pygpso_amd import _lib as L
    from tests import vgp_oracle as V

    r = pc.reference(3)  # N = 17, D = 3, Matern32, with a noise vector
    th, Xs = r["th"], r["Xs"]
    fit = lambda e: e.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    args = (r["omega"], r["phase"], r["w"], r["eps"])
    eng = fitted(r)
    # before a draw
    assert eng.paths_info() == (0, 0) and _eval_code(eng, Xs) == L.E_STATE
    # a draw and an eval change nothing else
    h0, p0 = eng.posterior_hash(), eng.predict(Xs)
    eng.paths_draw(*args)
    want = eng.paths_eval(Xs)[0]
    assert eng.paths_info() == (16, 4)
    p1 = eng.predict(Xs)
    assert eng.posterior_hash() == h0 and np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])
    # refused draws leave the set serving the same bits: s = 257, f = 0, a NaN in w, a NULL, an open ticket
    bad_w = r["w"].copy()
    bad_w[3, 1] = np.nan
    assert _draw_code(eng, r["omega"], r["phase"], np.zeros((257, 4)), np.zeros((257, 17))) == L.E_ARG
    assert _draw_code(eng, *args, f=0) == L.E_ARG
    assert _draw_code(eng, r["omega"], r["phase"], bad_w, r["eps"]) == L.E_ARG
    assert eng._lib.gpso_paths_draw(eng._h, None, L.dptr(r["phase"]), 4, L.dptr(r["w"]), None, 16) == L.E_ARG
    ticket = eng.best_ucb_begin(Xs, gpr.VARSIGMA_DEFAULT)
    assert _draw_code(eng, *args) == L.E_STATE and _eval_code(eng, Xs) == L.E_STATE
    eng.best_ucb_end(ticket)
    assert eng.paths_info() == (16, 4) and np.array_equal(eng.paths_eval(Xs)[0], want)
    # eval's own argument checks
    xs = np.ascontiguousarray(Xs)
    ptr = C.c_void_p(xs.ctypes.data)
    assert eng._lib.gpso_paths_eval(eng._h, ptr, L.F64, L.MEM_HOST, 64, None, 1, None, L.MEM_HOST, None, None) == L.E_ARG
    assert eng._lib.gpso_paths_eval(eng._h, ptr, L.F64, L.MEM_HOST, 0, None, 1, ptr, L.MEM_HOST, None, None) == L.E_ARG
    bad_seg = np.array([0, 70, 60], dtype=np.int64)
    out = np.empty((16, 64))
    assert eng._lib.gpso_paths_eval(eng._h, ptr, L.F64, L.MEM_HOST, 64, L.i64ptr(bad_seg), 2, C.c_void_p(out.ctypes.data),
                                    L.MEM_HOST, None, None) == L.E_ARG
    assert np.array_equal(eng.paths_eval(Xs)[0], want)
    # every change of the posterior ends the set
    fit(eng)
    assert eng.paths_info() == (0, 0) and _eval_code(eng, Xs) == L.E_STATE
    for change in (lambda: eng.set_data(r["X"], r["y"]), lambda: eng.set_noise_diag(r["s"]),
                   lambda: eng.set_posterior(r["X"], r["post"].L, r["post"].alpha, th.kernel, th.lengthscales, th.variance,
                                             th.noise, th.mean_c)):
        if eng.paths_info() == (0, 0):
            eng.set_data(r["X"], r["y"])
            fit(eng)
            eng.paths_draw(r["omega"], r["phase"], r["w"], None)
        assert eng.paths_info() == (16, 4)
        change()
        assert eng.paths_info() == (0, 0) and _eval_code(eng, Xs) == L.E_STATE
    # an installed posterior has no targets: no draw; neither has a variational one; a float32 context has no double factor
    assert _draw_code(eng, *args) == L.E_STATE
    vg = _engine()
    vg.set_data(r["X"], r["y"])
    u = V.initial_u(0.3 * np.sqrt(3), 1.1, 0.01, 0.05)
    vg.vgp_set_q()
    vg.vgp_natgrad("Matern52", u, 1, True, 0.0, 0.5)
    vg.vgp_posterior("Matern52", u, 1, True, 0.0)
    assert _draw_code(vg, *args) == L.E_STATE
    e32 = _engine("float32")
    e32.set_data(r["X"], r["y"])
    fit(e32)
    assert _draw_code(e32, *args) == L.E_ARG and _eval_code(e32, Xs) == L.E_ARG
    e32.predict(Xs)


# ---- 6. the surrogate end to end -----------------------------------------------------------------------------------------------
def test_thompson_select_leaves_over_more_rows_than_the_joint_calls_take():
    from pygpso_amd import GPRSurrogate
    from pygpso_amd import kernels as K

    rng = np.random.default_rng(5)
    coords = rng.random((30, 3))
    scores = np.sin(3.0 * coords[:, 0]) + coords[:, 1] ** 2 - coords[:, 2]
    surr = GPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.3, variance=1.0), gp_meanf=K.Constant(0.0), optimiser=K.Scipy())
    surr.append(coords, scores)
    surr.gp_update()
    stored = list(surr.points)
    leaves = rng.random((5000, 3))
    seg = [0, 1200, 5000]
    surr.gp_sample_paths(8, n_features=256, rng=7)
    f = surr.gp_eval_paths(leaves)
    idx, val = surr.thompson_select_leaves(leaves, seg_off=seg)
    want_i, want_v = po.seg_argmax(f, seg)
    assert f.shape == (8, 5000) and np.array_equal(idx, want_i) and np.array_equal(val, want_v)
    assert not np.array_equal(f[0], f[1]) and not np.array_equal(val[0], val[1])  # (eight functions, not one eight times)
    surr.gp_sample_paths(8, n_features=256, rng=7)
    assert np.array_equal(surr.gp_eval_paths(leaves), f)
    assert list(surr.points) == stored
