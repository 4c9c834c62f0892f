"""
GPSO_OPT_PARK_BYTES: the default split predict kernel (fp16 split, fused step, one chunk of the fp16 contraction) parks the
lowest even k-steps' cross-Gram pieces in a workgroup's first row block and reloads them in its later row blocks instead of
generating them again (leaf_split.hpp, PARK).  The reloaded pieces are the bits generation produces and the k order is
unchanged, so every result must be EQUAL, bit for bit, to the same context's result with the option off -- and the off arm is
held to the float64 oracle within the bounds of tests/test_gpu_parity.py, so that "equal" is not "equally wrong".

Shapes: the smallest that reach each branch.  N = 768 is three row blocks (the middle one reloads steps 0, 2, 4, 6 -- the only
reload there is); N = 700 pads to the same with q_max inside the last block; N = 1280 is five (reloads in three blocks, chains of
up to twelve DMAs).  D = 12 is one chunk of the fp16 contraction with the packed last chunk; D = 40 is two chunks, whose LDS
has no room for the reload windows: the option must then behave as off.  512 leaves are two full leaf tiles, 300 a ragged one.
Batches this small get one row block per workgroup from the launcher's model, so the tests force ONE workgroup per leaf tile
(GPSO_OPT_ROW_LOOP = -1) -- what C3's 65 536 leaves get -- and, at N = 1280, two.
"""
import numpy as np
import pytest

from oracle import gpr, tree
from tests.helpers import synthetic_leaves, synthetic_problem
from tests.test_gpu_parity import FLOAT_BOUNDS

pytestmark = pytest.mark.gpu

VS = gpr.VARSIGMA_DEFAULT
STEP_BYTES = 8 * 4096  # one parked k-step of one workgroup: 4 KB per wave
BIG = 1 << 28

_cache = {}


def _case(n, d):
    """Problem, fitted float32 engine and leaves of a shape; the float64 oracle's predictions of the leaves -- computed once."""
    if (n, d) not in _cache:
        from pygpso_amd import HipGPEngine

        X, y = synthetic_problem(n, d, seed=0)
        th = gpr.Theta("Matern52", 0.25 * np.sqrt(d) * np.ones(1), 1.0, 1e-3, float(y.mean()))
        eng = HipGPEngine("float32", predict_math="f16x3", generation="float32", precision_check=False)
        eng.set_data(X, y)
        eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
        Xs = synthetic_leaves(512, d, seed=3).astype(np.float32)
        mean_ref, var_ref = gpr.predict_y(gpr.posterior(th, X, y), Xs.astype(np.float64))
        _cache[(n, d)] = dict(eng=eng, th=th, y=y, Xs=Xs, mean_ref=mean_ref, var_ref=var_ref)
    return _cache[(n, d)]


def _expected(n, d, splits, park_steps_paid):
    """(parked, reloaded) k-steps per leaf tile as the launcher counts them (leaf_split.hpp): workgroup `split` of `splits` takes
    the row blocks of rank j S + (j even ? split : S - 1 - split), heaviest first; it parks the even steps below 2 P that lie
    below its first row block's diagonal steps and reloads those below each later row block's."""
    nbi = (n + 255) // 256
    if d > 28 or nbi - 1 - splits < 1:  # two chunks of the fp16 contraction: no room in LDS | nothing any workgroup could reload
        return 0, 0
    p = min(park_steps_paid, 4 * (nbi - 1 - splits))
    parked = reloaded = 0
    for split in range(splits if p > 0 else 0):
        j = 0
        while True:
            rank = j * splits + ((splits - 1 - split) if j & 1 else split)
            if rank >= nbi:
                break
            lim = min(2 * p, 8 * (nbi - 1 - rank))
            if j == 0:
                parked += (lim + 1) // 2
            else:
                reloaded += (lim + 1) // 2
            j += 1
    return parked, reloaded


def _run(eng, Xs):
    seg = np.array([0, len(Xs) // 3, len(Xs) // 3, len(Xs) - 5, len(Xs)], dtype=np.int64)
    mean, var = eng.predict(Xs)
    counts = (eng.last_count(5), eng.last_count(6))
    best = eng.best_ucb(Xs, VS, seg)
    assert (eng.last_count(5), eng.last_count(6)) == counts
    return mean, var, best, counts


@pytest.mark.parametrize("n,d,m,row_loop", [(768, 12, 512, -1), (700, 12, 300, -1), (1280, 12, 512, -1), (1280, 12, 300, 2),
                                            (768, 40, 512, -1), (1280, 40, 300, -1)])
def test_parked_steps_reload_to_the_bits_of_generation(n, d, m, row_loop):
    """predict (mean, var) and best_ucb (index, mean, var, ucb) with the option on -- every step the shape allows parked, ONE step
    parked, a budget one byte short of one step -- are the bits of the option off; the counters say that steps were reloaded
    exactly where they can be; the off arm is inside the float64 oracle's bounds."""
    c = _case(n, d)
    eng, Xs = c["eng"], c["Xs"][:m]
    splits = 1 if row_loop < 0 else row_loop
    wgs = (m + 255) // 256 * splits
    eng.set_row_loop(row_loop)
    eng.set_park_bytes(0)
    mean0, var0, best0, counts0 = _run(eng, Xs)
    assert eng.last_count(3) == splits and counts0 == (0, 0)
    bm, bv = FLOAT_BOUNDS["C3" if d == 12 else "C5"]
    em = np.max(np.abs(mean0 - c["mean_ref"][:m])) / np.max(np.abs(c["y"]))
    ev = np.max(np.abs(var0 - c["var_ref"][:m])) / c["th"].variance
    print(f"N {n} D {d} m {m}: off arm |d mean| {em:.2e} (bound {bm:.1e}), |d var| {ev:.2e} (bound {bv:.1e})")
    assert em <= bm and ev <= bv
    for budget, paid in ((BIG, BIG // (STEP_BYTES * wgs)), (STEP_BYTES * wgs, 1), (STEP_BYTES * wgs - 1, 0)):
        eng.set_park_bytes(budget)
        mean1, var1, best1, counts1 = _run(eng, Xs)
        want = _expected(n, d, splits, paid)
        print(f"  budget {budget}: parked {counts1[0]}, reloaded {counts1[1]} k-steps per leaf tile (expected {want})")
        assert counts1 == want
        if d == 12 and paid > 0:
            assert counts1[1] > 0
        else:
            assert counts1 == (0, 0)  # (too small a budget, or no room for the windows: it behaves as off)
        assert mean1.tobytes() == mean0.tobytes() and var1.tobytes() == var0.tobytes()
        for a, b in zip(best1, best0):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    eng.set_park_bytes(0)
    mean2, var2, _, counts2 = _run(eng, Xs)  # (and off again: the kernel without it, the same bits)
    assert counts2 == (0, 0) and mean2.tobytes() == mean0.tobytes() and var2.tobytes() == var0.tobytes()
    eng.set_row_loop(1)


def test_a_grown_batch_with_device_counted_rows_reloads_to_the_same_bits():
    """best_ucb_grow: the live row count is known to the device only (a workgroup beyond it leaves at once, the others park in
    their own first row block).  General sequence, one workgroup per leaf tile: same winners and values, and steps were reloaded."""
    n, d, depth = 1280, 12, 7
    c = _case(n, d)
    eng = c["eng"]
    kids = tree.split_bounds([(0.0, 1.0)] * d)
    boxes = np.array([kids[0], kids[2]])
    eng.set_small_calls(0)
    eng.set_row_loop(-1)
    try:
        eng.set_park_bytes(0)
        off = eng.best_ucb_grow(boxes, depth, VS)
        assert (eng.last_count(5), eng.last_count(6)) == (0, 0)
        eng.set_park_bytes(BIG)
        on = eng.best_ucb_grow(boxes, depth, VS)
        print(f"grown batch: {eng.last_count(0)} rows scored, parked {eng.last_count(5)}, reloaded {eng.last_count(6)} k-steps per leaf tile")
        assert eng.last_count(6) > 0
        for a, b in zip(on, off):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    finally:
        eng.set_park_bytes(0)
        eng.set_row_loop(1)
        eng.set_small_calls(1)
