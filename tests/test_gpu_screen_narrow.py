"""
GPSO_OPT_SURVIVOR_TILE: the survivors' launch of a screened best-UCB call runs the NARROW tile of the split predict kernel -- a
workgroup of 4 waves, one column tile of 16 leaves per wave, 64 leaves -- in place of the batch kernel's 8 waves x 2 column tiles
(csrc/leaf_split.hpp, predict_split_f32_narrow.hip).  A leaf's arithmetic depends neither on its lane nor on
its wave nor on its workgroup, so every (mean, var) must be EQUAL, byte for byte, whichever tile computed it, and a screened
record equal to the unscreened one.

(a) every leaf: ``predict`` with the option at 2 (narrow wherever the default family runs) against 1 (wide everywhere), at the
    smallest shapes at which each path of the kernel exists --
      N = 256 one row block, diagonal steps only | 600 a last block of 88 rows: the RTL = 8 copies | 700 a ragged last block
      with q_max inside it | 768 three full blocks;
      D = 12 one chunk of the fp16 contraction, packed last chunk | 20 one chunk, unpacked | 40 two chunks;
      m = 16 one column tile | 17 a ragged narrow tile | 64 one full narrow workgroup | 65 one leaf into the next | 300 a ragged
      wide tile | 1000 several tiles;
    each with GPSO_OPT_ROW_LOOP at its default and at -1 (one workgroup walks every row block).
(b) exact survivor counts at the tile edges: with varsigma = 0 a leaf survives iff its mean equals the largest one, so a batch
    that holds the winner's row c times has exactly c survivors.
(c) the screened suite's landscapes (tests/test_gpu_screen.py) once more, with the tile asserted.
"""
import numpy as np
import pytest
from scipy.special import erfcinv

from oracle import gpr
from pygpso_amd import _lib as L
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu

VS = float(erfcinv(0.01))
BIG_M = 24000
NARROW, WIDE = 64, 256  # gpso_last_count(ctx, 9)
MS = (16, 17, 64, 65, 300, 1000)

_engines = {}


def _theta(kernel, d, y, noise=1e-3):
    return gpr.Theta(kernel, 0.25 * np.sqrt(d) * np.ones(1), 1.0, noise, float(y.mean()))


def _fit(eng, th):
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)


def _engine(n, d, seed=0, noise=1e-3, flat=False, kernel="Matern52"):
    """A float32 engine on the default float kernels (tests/test_gpu_screen.py's), fitted; one per key."""
    key = (n, d, seed, noise, flat, kernel)
    if key not in _engines:
        from pygpso_amd import HipGPEngine

        X, y = synthetic_problem(n, d, seed=seed)
        if flat:
            y = np.full_like(y, 0.3)
        eng = HipGPEngine("float32", predict_math="f16x3", generation="float32", precision_check=False)
        eng.set_data(X, y)
        th = _theta(kernel, d, y, noise)
        if flat:
            th.mean_c = 0.3
        _fit(eng, th)
        _engines[key] = (eng, th)
    return _engines[key]


def _leaves(m, d, seed=1):
    import torch

    return torch.from_numpy(synthetic_leaves(m, d, seed=seed).astype(np.float32)).cuda()


def _bytes(rec):
    return b"".join(np.asarray(a).tobytes() for a in rec)


def _default_family_applies(eng, Xs):
    """Does the engine run the default family (fp16 split, fp16 contraction, fused step, float generation) on this batch?  The
    screen's probe is the engine's own answer: it refuses (GPSO_E_STATE) where a screened call does not exist."""
    try:
        eng.screen_probe(Xs, VS)
    except (L.GpsoHipError, ValueError):
        return False
    return True


def _narrow_against_wide(eng, d, ms):
    all_leaves = _leaves(max(ms), d)
    for m in ms:
        Xs = all_leaves[:m].contiguous()
        assert _default_family_applies(eng, Xs), f"the default family does not apply at m = {m}"
        for row_loop in (1, -1):
            eng.set_row_loop(row_loop)
            try:
                eng.set_survivor_tile(1)
                wide = eng.predict(Xs)
                assert eng.last_count(9) == WIDE
                eng.set_survivor_tile(2)
                narrow = eng.predict(Xs)
                assert eng.last_count(9) == NARROW
            finally:
                eng.set_survivor_tile(0)
                eng.set_row_loop(1)
            assert np.all(np.isfinite(wide[0])) and np.all(wide[1] > 0.0)
            assert narrow[0].tobytes() == wide[0].tobytes(), f"mean, m = {m}, row loop {row_loop}"
            assert narrow[1].tobytes() == wide[1].tobytes(), f"var, m = {m}, row loop {row_loop}"


@pytest.mark.parametrize("d", [12, 20, 40])
@pytest.mark.parametrize("n", [256, 600, 700, 768])
def test_every_leaf_has_the_wide_kernels_bits(n, d):
    eng, _ = _engine(n, d)
    _narrow_against_wide(eng, d, MS)


@pytest.mark.parametrize("kernel", ["Matern32", "Matern12", "SquaredExponential"])
def test_every_leaf_has_the_wide_kernels_bits_under_the_other_kernels(kernel):
    eng, _ = _engine(700, 12, kernel=kernel)
    _narrow_against_wide(eng, 12, (300,))


def test_the_option_is_validated_and_per_context():
    from pygpso_amd import HipGPEngine

    eng, _ = _engine(256, 12)
    other = HipGPEngine("float32", predict_math="f16x3", generation="float32", precision_check=False)
    try:
        for bad in (-1, 3):
            with pytest.raises(ValueError, match="survivor tile"):  # (GPSO_E_ARG)
                other.set_survivor_tile(bad)
        other.set_survivor_tile(2)  # (another context's setting: this one keeps its default)
        Xs = _leaves(300, 12)
        eng.predict(Xs)
        assert eng.last_count(9) == WIDE
    finally:
        other.close()


def _screened(eng, th, Xs, vs, tile):
    """The record of a screened call under survivor tile `tile` on a posterior made new again, and (survivors, verdict, tile)."""
    _fit(eng, th)
    eng.set_screen(2)
    eng.set_survivor_tile(tile)
    try:
        rec = eng.best_ucb(Xs, vs)
        return rec, (eng.last_count(7), eng.last_count(8), eng.last_count(9))
    finally:
        eng.set_screen(0)
        eng.set_survivor_tile(0)


def _unscreened(eng, Xs, vs):
    eng.set_screen(0)
    rec = eng.best_ucb(Xs, vs)
    assert eng.last_count(8) == L.SCREEN_NONE and eng.last_count(7) == 0
    return rec


@pytest.mark.parametrize("c", [1, 16, 17, 64, 65, 129])
def test_exact_survivor_counts_at_the_tile_edges(c):
    n, d, m = 700, 12, 1000
    eng, th = _engine(n, d)
    Xs = _leaves(m, d)
    w = int(_unscreened(eng, Xs, 0.0)[0][0])
    for k in range(c):  # (37 and 1000 are coprime: c distinct positions, the winner's own among them)
        Xs[(w + 37 * k) % m] = Xs[w]
    off = _unscreened(eng, Xs, 0.0)
    on, (count, verdict, tile) = _screened(eng, th, Xs, 0.0, 0)
    print(f"c {c}: {count} survivors, verdict {verdict}, {tile} leaves per workgroup")
    assert count == c
    assert verdict == L.SCREEN_ACCEPTED
    assert tile == NARROW
    assert _bytes(on) == _bytes(off)
    wide, (count_w, verdict_w, tile_w) = _screened(eng, th, Xs, 0.0, 1)
    assert (count_w, verdict_w, tile_w) == (c, L.SCREEN_ACCEPTED, WIDE)
    assert _bytes(wide) == _bytes(off)


@pytest.mark.parametrize("noise", [1e-2, 1e-6])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_a_screened_call_on_narrow_tiles_gives_the_unscreened_bits(seed, noise):
    n, d, m = 768, 12, 1000
    eng, th = _engine(n, d, seed, noise)
    Xs = _leaves(m, d, seed + 1)
    for vs in (0.0, VS, 50.0):
        off = _unscreened(eng, Xs, vs)
        on, (count, verdict, tile) = _screened(eng, th, Xs, vs, 0)
        print(f"seed {seed} noise {noise:g} varsigma {vs:.3g}: {count} survivors, verdict {verdict}")
        assert _bytes(on) == _bytes(off)
        assert verdict == L.SCREEN_ACCEPTED and 1 <= count <= m and tile == NARROW


def test_the_refused_large_batch_keeps_its_bits_and_its_verdict():
    n, d = 768, 12
    eng, th = _engine(n, d)
    Xs = _leaves(BIG_M, d, 7)
    cap = eng.screen_probe(Xs, 50.0)[3]["cap"]
    off = _unscreened(eng, Xs, 50.0)
    on, (count, verdict, _) = _screened(eng, th, Xs, 50.0, 0)
    assert _bytes(on) == _bytes(off)
    # (everything within 50 of the largest mean survives: all of them, more than the launch has room for)
    assert count == BIG_M and verdict == (L.SCREEN_ACCEPTED if count <= cap else L.SCREEN_REFUSED)
    assert cap >= BIG_M or verdict == L.SCREEN_REFUSED


def test_both_sides_of_the_threshold_in_one_room():
    """24 000 leaves at N = 768 have room for 21 760 survivors and the model gives the narrow tile 15 744 of them: both launches
    are enqueued, one leaves at once.  A varsigma found on the probe for either side: same bytes, accepted, the tile as modelled."""
    from pygpso_amd import _lib

    n, d = 768, 12
    eng, th = _engine(n, d)
    Xs = _leaves(BIG_M, d, 7)
    cap = eng.screen_probe(Xs, VS)[3]["cap"]
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    top = _lib.load().gpso_survivor_narrow_max_host(3, cus, cap)
    assert 0 < top < cap

    def varsigma_with(lo_count, hi_count):
        lo, hi = 0.0, 50.0
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            s = eng.screen_probe(Xs, mid)[3]["survivors"]
            if lo_count < s <= hi_count:
                return mid, s
            lo, hi = (mid, hi) if s <= lo_count else (lo, mid)
        raise AssertionError(f"no varsigma with a count in ({lo_count}, {hi_count}]")

    for (lo_c, hi_c), tile in (((256, top), NARROW), ((top, cap), WIDE)):
        vs, s = varsigma_with(lo_c, hi_c)
        off = _unscreened(eng, Xs, vs)
        on, (count, verdict, ran) = _screened(eng, th, Xs, vs, 0)
        print(f"varsigma {vs:.4g}: {count} survivors (narrow up to {top}, room {cap}), verdict {verdict}, tile {ran}")
        assert count == s and verdict == L.SCREEN_ACCEPTED and ran == tile
        assert _bytes(on) == _bytes(off)


def test_a_flat_mean_is_refused_with_the_same_bits():
    n, d = 768, 12
    eng, th = _engine(n, d, flat=True)
    Xs = _leaves(BIG_M, d, 3)
    info = eng.screen_probe(Xs, VS)[3]
    assert info["cap"] < BIG_M and info["survivors"] == BIG_M
    off = _unscreened(eng, Xs, VS)
    on, (count, verdict, _) = _screened(eng, th, Xs, VS, 0)
    assert _bytes(on) == _bytes(off) and count == BIG_M and verdict == L.SCREEN_REFUSED


def test_two_calls_in_flight_on_narrow_tiles_give_the_same_bits():
    n, d = 768, 12
    eng, th = _engine(n, d)
    small_a, small_b = _leaves(1000, d, 11), _leaves(512, d, 12)
    ref = [_unscreened(eng, small_a, VS), _unscreened(eng, small_b, VS)]
    _fit(eng, th)
    eng.set_screen(2)
    try:
        t0, t1 = eng.best_ucb_begin(small_a, VS), eng.best_ucb_begin(small_b, VS)
        got = [eng.best_ucb_end(t0)]
        assert eng.last_count(8) == L.SCREEN_ACCEPTED and eng.last_count(9) == NARROW
        got.append(eng.best_ucb_end(t1))
        assert eng.last_count(8) == L.SCREEN_ACCEPTED
    finally:
        eng.set_screen(0)
    for g, r in zip(got, ref):
        assert _bytes(g) == _bytes(r)
