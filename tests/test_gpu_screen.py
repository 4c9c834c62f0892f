"""
GPSO_OPT_SCREEN: a best-UCB call computes every leaf's mean alone, drops the leaves whose ucb at zero variance share lies below
that of the largest mean, and runs the tile kernel on the survivors only (csrc/screen.hpp, screen.hip).  The
record of a call must be EQUAL, bit for bit, whether it was screened or not -- whatever the screen kept, and whether the
call's last kernel accepted the record or sent the call back to the general sequence.

Shapes: N = 768 is three row blocks, N = 700 pads to the same with a ragged last one (q_max inside it); D = 12 is one chunk of
the fp16 contraction (its packed last chunk), D = 40 two.  300 leaves are a ragged leaf tile, 512 two full ones, 1 000 four with
a ragged one.  The tests set the option to 2 (any batch size).  A call has room for CUs / 3 leaf tiles of survivors at these N
(21 760 rows on 256 CUs), so a REFUSAL needs a batch above that in which nearly everything survives: 24 000 leaves with
varsigma = 50, or under a flat mean (constant targets) -- tools/screen_mean_census.py says which landscape does what.
"""
import math

import numpy as np
import pytest
from scipy.special import erfcinv

from oracle import gpr
from pygpso_amd import _lib as L
from pygpso_amd import acquisition as A
from tests.helpers import synthetic_leaves, synthetic_problem
from tools.screen_mean_census import census

pytestmark = pytest.mark.gpu

VS = float(erfcinv(0.01))
BIG_M = 24000

_engines = {}


def _theta(d, y, noise=1e-3):
    return gpr.Theta("Matern52", 0.25 * np.sqrt(d) * np.ones(1), 1.0, noise, float(y.mean()))


def _fit(eng, th):
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)


def _engine(n, d, seed=0, noise=1e-3, flat=False):
    """A float32 engine on the default float kernels, fitted; one per (shape, seed, noise, flat), refitted by the caller to make
    a posterior new again."""
    key = (n, d, seed, noise, flat)
    if key not in _engines:
        from pygpso_amd import HipGPEngine

        X, y = synthetic_problem(n, d, seed=seed)
        if flat:
            y = np.full_like(y, 0.3)
        eng = HipGPEngine("float32", predict_math="f16x3", generation="float32", precision_check=False)
        eng.set_data(X, y)
        th = _theta(d, y, noise)
        if flat:
            th.mean_c = 0.3  # (y - c is then exactly zero: alpha = 0)
        _fit(eng, th)
        _engines[key] = (eng, th)
    return _engines[key]


def _leaves(m, d, seed=1):
    import torch

    return torch.from_numpy(synthetic_leaves(m, d, seed=seed).astype(np.float32)).cuda()


def _bytes(rec):
    return b"".join(np.asarray(a).tobytes() for a in rec)


def _both(eng, th, Xs, vs):
    """The record with the option off and with every call screened (on a posterior made new again), and the screened call's
    counters."""
    eng.set_screen(0)
    off = eng.best_ucb(Xs, vs)
    assert eng.last_count(8) == L.SCREEN_NONE and eng.last_count(7) == 0
    _fit(eng, th)
    eng.set_screen(2)
    on = eng.best_ucb(Xs, vs)
    counters = (eng.last_count(7), eng.last_count(8))
    eng.set_screen(0)
    return off, on, counters


@pytest.mark.parametrize("n,d,m", [(768, 12, 512), (700, 12, 300), (768, 40, 1000), (700, 12, 1000)])
def test_the_mean_pass_gives_predicts_means_and_the_bound_holds(n, d, m):
    eng, th = _engine(n, d)
    Xs = _leaves(m, d)
    eng.set_screen(0)
    mean, var = eng.predict(Xs)
    _, _, ucb = eng.acq_values(Xs, A.UCBVar(VS))
    idx0 = int(eng.best_ucb(Xs, VS)[0][0])
    my, ub, keep, info = eng.screen_probe(Xs, VS)
    print(f"N {n} D {d} m {m}: {info['survivors']} survivors (room {info['cap']}), max (ucb - ub) {np.max(ucb - ub):.3e}")
    assert my.tobytes() == mean.tobytes()
    assert np.all(ub >= ucb)
    assert keep[idx0] and info["survivors"] == int(keep.sum())
    t_ref = np.max(my) + VS * th.noise
    assert info["threshold"] == t_ref
    assert np.array_equal(keep, ~(ub < t_ref))


@pytest.mark.parametrize("noise", [1e-2, 1e-6])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_a_screened_call_gives_the_bits_of_an_unscreened_one(seed, noise):
    n, d, m = 768, 12, 1000
    eng, th = _engine(n, d, seed, noise)
    Xs = _leaves(m, d, seed + 1)
    for vs in (0.0, VS, 50.0):
        survivors = eng.screen_probe(Xs, vs)[3]["survivors"]
        off, on, (count, verdict) = _both(eng, th, Xs, vs)
        c = census(d, n, m, seed, noise, vs)
        print(f"seed {seed} noise {noise:g} varsigma {vs:.3g}: {count} survivors (oracle: {c['survivors']}), verdict {verdict}")
        assert _bytes(on) == _bytes(off)
        # (1 000 leaves fit the survivors' launch whatever survives: the census says "accepted" for all of these)
        assert c["fits"] and c["accepted"] and verdict == L.SCREEN_ACCEPTED
        assert 1 <= count <= m and count == survivors


@pytest.mark.parametrize("vs", [0.0, VS, 50.0])
def test_a_large_batch_is_accepted_or_refused_as_the_census_says_with_the_same_bits(vs):
    n, d = 768, 12
    eng, th = _engine(n, d)
    Xs = _leaves(BIG_M, d, 7)
    cap = eng.screen_probe(Xs, vs)[3]["cap"]
    c = census(d, n, BIG_M, 0, th.noise, vs, leaf_seed=7)
    off, on, (count, verdict) = _both(eng, th, Xs, vs)
    print(f"varsigma {vs:.3g}: {count} survivors (oracle: {c['survivors']}), room {cap}, verdict {verdict}")
    assert _bytes(on) == _bytes(off)
    assert verdict == (L.SCREEN_ACCEPTED if count <= cap else L.SCREEN_REFUSED)
    if vs == 50.0:  # everything within 50 of the largest mean survives: all of them, more than the launch has room for
        assert c["survivors"] == BIG_M and count == BIG_M and (cap >= BIG_M or verdict == L.SCREEN_REFUSED)
    elif abs(c["survivors"] - cap) > BIG_M // 20:  # (clear of the room's edge, the oracle's count decides as the device's does)
        assert verdict == (L.SCREEN_ACCEPTED if c["survivors"] <= cap else L.SCREEN_REFUSED)


def test_ties_go_to_the_lower_index_either_way():
    n, d, m = 768, 12, 1000
    eng, th = _engine(n, d)
    Xs = _leaves(m, d)
    eng.set_screen(0)
    w = int(eng.best_ucb(Xs, VS)[0][0])
    a, b = (w + 300) % m, (w + 700) % m
    Xs[a] = Xs[w]
    Xs[b] = Xs[w]
    off, on, (count, verdict) = _both(eng, th, Xs, VS)
    assert int(off[0][0]) == min(w, a, b) and _bytes(on) == _bytes(off) and verdict == L.SCREEN_ACCEPTED and count >= 3


def test_a_nan_coordinate_gives_the_record_of_the_unscreened_call():
    n, d, m = 700, 12, 1000
    eng, th = _engine(n, d)
    Xs = _leaves(m, d)
    Xs[613, 5] = float("nan")
    off, on, (count, verdict) = _both(eng, th, Xs, VS)
    assert int(off[0][0]) == 613 and math.isnan(off[3][0])
    assert _bytes(on) == _bytes(off) and verdict == L.SCREEN_ACCEPTED


def test_a_flat_mean_refuses_once_per_posterior():
    n, d = 768, 12
    eng, th = _engine(n, d, flat=True)
    Xs = _leaves(BIG_M, d, 3)
    my, ub, keep, info = eng.screen_probe(Xs, VS)
    assert np.all(my == th.mean_c) and keep.all()  # (alpha = 0: every mean is the constant, nothing can be pruned)
    assert info["cap"] < BIG_M  # (256 CUs / 3 row blocks: 85 leaf tiles)
    off, on, (count, verdict) = _both(eng, th, Xs, VS)
    assert _bytes(on) == _bytes(off) and count == BIG_M and verdict == L.SCREEN_REFUSED
    eng.set_screen(2)
    again = eng.best_ucb(Xs, VS)  # the same posterior: not screened again
    assert eng.last_count(8) == L.SCREEN_NONE and _bytes(again) == _bytes(off)
    _fit(eng, th)  # a new posterior: screened (and refused) again
    third = eng.best_ucb(Xs, VS)
    assert eng.last_count(8) == L.SCREEN_REFUSED and _bytes(third) == _bytes(off)
    eng.set_screen(0)


def test_two_calls_in_flight_give_the_same_bits():
    n, d = 768, 12
    eng, th = _engine(n, d)
    small_a, small_b = _leaves(1000, d, 11), _leaves(512, d, 12)
    big = _leaves(BIG_M, d, 13)
    eng.set_screen(0)
    ref = [eng.best_ucb(small_a, VS), eng.best_ucb(small_b, VS), eng.best_ucb(big, 50.0), eng.best_ucb(big, VS)]
    _fit(eng, th)
    eng.set_screen(2)
    t0, t1 = eng.best_ucb_begin(small_a, VS), eng.best_ucb_begin(small_b, VS)
    got = [eng.best_ucb_end(t0)]
    assert eng.last_count(8) == L.SCREEN_ACCEPTED
    got.append(eng.best_ucb_end(t1))
    # (both enqueued screened; the first to end is refused where the launch lacks the room, and runs again behind the second)
    t2, t3 = eng.best_ucb_begin(big, 50.0), eng.best_ucb_begin(big, VS)
    got.append(eng.best_ucb_end(t2))
    verdict2 = eng.last_count(8)
    got.append(eng.best_ucb_end(t3))
    eng.set_screen(0)
    print(f"in flight: verdict of the varsigma = 50 call {verdict2}")
    assert verdict2 in (L.SCREEN_ACCEPTED, L.SCREEN_REFUSED)
    for g, r in zip(got, ref):
        assert _bytes(g) == _bytes(r)


def test_the_default_screens_large_single_segment_calls_only():
    n, d = 768, 12
    eng, th = _engine(n, d)
    _fit(eng, th)
    eng.set_screen(1)
    try:
        eng.best_ucb(_leaves(300, d), VS)
        assert eng.last_count(8) == L.SCREEN_NONE
        big = _leaves(BIG_M, d, 5)
        eng.best_ucb(big, VS, np.array([0, 9000, BIG_M], dtype=np.int64))
        assert eng.last_count(8) == L.SCREEN_NONE
        rec = eng.best_ucb(big, VS)
        assert eng.last_count(8) == L.SCREEN_ACCEPTED and 0 < eng.last_count(7) < BIG_M
        assert eng.last_count(0) == BIG_M and eng.last_count(1) == BIG_M
        eng.best_ucb(big.cpu().numpy(), VS)  # host leaves: as today
        assert eng.last_count(8) == L.SCREEN_NONE
        eng.set_screen(0)
        assert _bytes(eng.best_ucb(big, VS)) == _bytes(rec)
    finally:
        eng.set_screen(0)
