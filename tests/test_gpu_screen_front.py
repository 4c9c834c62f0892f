"""
The stages of a screened best-UCB call in front of the survivors' launch (csrc/screen.hip): the mean pass --
128 leaves per workgroup, every row block in ascending order, the f64 sum of the shares kept in registers -- and the compaction
over a grid of workgroups that count, then scatter.  What tests/test_gpu_screen.py cannot see: the compact list itself
(gpso_screen_list), the largest mean behind a ragged leaf tile, the batch size at which the mean pass splits the row blocks.

Shapes: N = 768 is three row blocks, N = 700 pads to the same with a ragged last one (q_max inside it); D = 12 is one chunk of
the fp16 contraction (its packed last chunk), D = 40 two.  300 and 1 000 leaves end in a ragged 128-leaf tile (and a ragged
256-leaf one); 24 000 leaves are 94 parts of the compaction and more than a call has room for when everything survives;
16 640 leaves (130 tiles) are fewer than two tiles per CU: the mean pass splits the row blocks there -- as it does for every
batch below 512 tiles on 256 CUs.  So the small shapes run twice: under the default rule (the split route) and with
GPSO_OPT_ROW_LOOP = -1 (one workgroup per tile whatever the batch: the folded sum, the route of C3's 65 536 leaves), and one
batch of 65 300 leaves takes the folded route by the default rule itself.
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

_engines = {}
_leaf_cache = {}


def _engine(n, d):
    """A float32 engine on the default float kernels, fitted; one per shape."""
    if (n, d) not in _engines:
        from pygpso_amd import HipGPEngine

        X, y = synthetic_problem(n, d, seed=0)
        eng = HipGPEngine("float32", predict_math="f16x3", generation="float32", precision_check=False)
        eng.set_data(X, y)
        th = gpr.Theta("Matern52", 0.25 * np.sqrt(d) * np.ones(1), 1.0, 1e-3, float(y.mean()))
        _engines[(n, d)] = (eng, th)
        _fit(eng, th)
    return _engines[(n, d)]


def _fit(eng, th):
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)


def _leaves(m, d, seed=1):
    """(host float32 rows, the same on the device); shared, never written: a test that edits leaves clones them."""
    import torch

    if (m, d, seed) not in _leaf_cache:
        host = synthetic_leaves(m, d, seed=seed).astype(np.float32)
        _leaf_cache[(m, d, seed)] = (host, torch.from_numpy(host).cuda())
    return _leaf_cache[(m, d, seed)]


def _bytes(rec):
    return b"".join(np.asarray(a).tobytes() for a in rec)


def _both(eng, th, Xs, vs):
    """The record with the option off and with every call screened (on a posterior made new again), and the screened call's
    counters."""
    eng.set_screen(0)
    off = eng.best_ucb(Xs, vs)
    _fit(eng, th)
    eng.set_screen(2)
    on = eng.best_ucb(Xs, vs)
    counters = (eng.last_count(7), eng.last_count(8))
    eng.set_screen(0)
    return off, on, counters


@pytest.fixture(params=[-1, 1], ids=["folded", "default"])
def row_loop(request):
    """GPSO_OPT_ROW_LOOP for a test to set on its engine; every engine of this file is back at the default behind it."""
    yield request.param
    for eng, _ in _engines.values():
        eng.set_row_loop(1)


@pytest.mark.parametrize("n,d,m", [(768, 12, 300), (700, 12, 1000), (768, 40, 1000), (700, 40, 300), (768, 12, 65300)])
def test_the_mean_pass_gives_predicts_mean_and_padding_stays_out_of_the_maximum(n, d, m, row_loop):
    eng, th = _engine(n, d)
    _, Xs = _leaves(m, d)
    eng.set_screen(0)
    eng.set_row_loop(1)
    mean, _ = eng.predict(Xs)
    eng.set_row_loop(row_loop)
    my, ub, keep, info = eng.screen_probe(Xs, VS)
    print(f"N {n} D {d} m {m}: max my {np.max(my):.17g}, threshold {info['threshold']:.17g}, {info['survivors']} survivors")
    assert my.tobytes() == mean.tobytes()
    # (the zero rows that pad the last leaf tile have a finite mean of their own: it must not reach T')
    assert info["threshold"] == np.max(my) + VS * th.noise


@pytest.mark.parametrize("vs", [0.0, VS, 50.0])
@pytest.mark.parametrize("m", [300, 1000, BIG_M])
def test_the_compact_list_holds_the_survivors_in_order_with_their_rows(m, vs, row_loop):
    n, d = 768, 12
    eng, th = _engine(n, d)
    eng.set_row_loop(row_loop)
    host, Xs = _leaves(m, d, 7)
    my, ub, keep, info = eng.screen_probe(Xs, vs)
    key, rows = eng.screen_list()
    cap = info["cap"]
    want = np.flatnonzero(keep)[:cap]
    print(f"m {m} varsigma {vs:.3g}: {info['survivors']} survivors, room {cap}, list of {len(key)}")
    assert info["survivors"] == int(keep.sum())
    assert np.array_equal(key, want)
    assert rows.shape == (len(want), d) and rows.tobytes() == host[want].tobytes()
    if vs == 50.0 and m == BIG_M:  # everything survives: more than the launch has room for, the list is the batch's head
        assert info["survivors"] == m and (m <= cap or (len(key) == cap and key[-1] == cap - 1))


def test_nan_leaves_survive_and_stay_out_of_the_maximum(row_loop):
    n, d, m = 700, 12, 300
    eng, th = _engine(n, d)
    eng.set_row_loop(row_loop)
    _, Xs0 = _leaves(m, d)
    Xs = Xs0.clone()
    Xs[m - 1, 3] = float("nan")  # the last live row of the ragged tile
    Xs[0, 7] = float("nan")
    my, ub, keep, info = eng.screen_probe(Xs, VS)
    key, rows = eng.screen_list()
    assert np.isnan(my[0]) and np.isnan(my[m - 1]) and np.isfinite(my[1:m - 1]).all()
    assert keep[0] and keep[m - 1] and key[0] == 0 and key[-1] == m - 1
    assert info["threshold"] == np.max(my[1:m - 1]) + VS * th.noise
    off, on, (count, verdict) = _both(eng, th, Xs, VS)
    assert _bytes(on) == _bytes(off) and verdict == L.SCREEN_ACCEPTED and count == int(keep.sum())
    Xs = Xs0.clone()
    Xs[:, 2] = float("nan")  # no finite mean at all: T' = -inf, nothing is pruned
    my, ub, keep, info = eng.screen_probe(Xs, VS)
    key, rows = eng.screen_list()
    assert np.isnan(my).all() and keep.all() and info["threshold"] == -np.inf and info["survivors"] == m
    assert np.array_equal(key, np.arange(m))


def test_a_mid_size_batch_gives_the_bits_of_an_unscreened_call():
    n, d, m = 768, 12, 16640
    eng, th = _engine(n, d)
    _, Xs = _leaves(m, d, 5)
    eng.set_screen(0)
    mean, _ = eng.predict(Xs)
    my = eng.screen_probe(Xs, VS)[0]
    assert my.tobytes() == mean.tobytes()
    off, on, (count, verdict) = _both(eng, th, Xs, VS)
    print(f"m {m}: {count} survivors, verdict {verdict}")
    assert _bytes(on) == _bytes(off) and verdict == L.SCREEN_ACCEPTED and 1 <= count < m


def test_a_screened_call_reports_the_split_count_of_the_host_rule():
    import torch

    from tests.test_gpu_parity import _leaf_row_splits

    n, d = 768, 12
    eng, th = _engine(n, d)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    _fit(eng, th)
    eng.set_screen(2)
    try:
        for m in (1000, 16640, BIG_M):
            eng.best_ucb(_leaves(m, d, 5)[1], VS)
            assert eng.last_count(8) == L.SCREEN_ACCEPTED
            assert eng.last_count(3) == _leaf_row_splits(1, (m + 255) // 256, n // 256, ncu), (m, eng.last_count(3))
    finally:
        eng.set_screen(0)
