"""
GPU tests of what a fit call records and how it ends (csrc/fit_call.hpp, the stages of ``fit_eval_impl``): the
timed span of every fit-side entry point, the same bits whether the call waits for its events, a completion token or the
stream, and the LOO read-back on a context whose pinned scratch has to grow for it.  float64, N = 52 (the one-launch fit)
and N = 300 (the dense sequence).  No tolerance: everything is equality, or > 0 / == 0.
"""
import numpy as np
import pytest

from tests.helpers import synthetic_problem

pytestmark = pytest.mark.gpu

KERNEL = "Matern52"
SHAPES = [(52, 2), (300, 3)]


def _problem(n, d):
    X, y = synthetic_problem(n, d, seed=17 + n)
    return X, y, (KERNEL, 0.25 * np.sqrt(d) * np.ones(1), 1.3, 1.0e-3, float(y.mean()))


def _engine(X=None, y=None):
    from pygpso_amd import HipGPEngine

    eng = HipGPEngine("float64")
    if X is not None:
        eng.set_data(X, y)
    return eng


def _posterior(eng):
    from pygpso_amd import _lib as L

    return [eng.get_matrix(L.MAT_LINV), eng.get_vector(L.VEC_ALPHA)]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a, b))


def test_every_fit_side_entry_point_times_its_span_and_only_when_asked():
    X52, y52, th52 = _problem(52, 2)
    X300, y300, th300 = _problem(300, 3)
    U = np.array([[0.3, 0.5, -6.0, 0.1], [0.1, 0.2, -5.0, 0.0]])
    small, dense = _engine(X52, y52), _engine()

    def calls():
        yield "fit_eval N=52", small, lambda: small.fit_eval(*th52)
        yield "fit_eval_loo N=52", small, lambda: small.fit_eval_loo(*th52)
        yield "fit_eval_u_batch N=52", small, lambda: small.fit_eval_u_batch(KERNEL, U, 1, True)
        dense.set_data(X300[:297], y300[:297])
        yield "fit_eval N=297", dense, lambda: dense.fit_eval(*th300, want_grad=False)
        yield "append 297+3", dense, lambda: dense.append(X300[297:], y300[297:])
        yield "fit_eval_loo N=300", dense, lambda: dense.fit_eval_loo(*th300)

    for name, eng, call in calls():
        out = call()
        if name.startswith("append"):
            assert out[1], "the append ran in place"
        assert eng.last_ms(2) > 0.0, name
    small.set_timing(False)
    dense.set_timing(False)
    assert small.last_ms(2) == 0.0 and dense.last_ms(2) == 0.0
    for name, eng, call in calls():
        out = call()
        if name.startswith("append"):
            assert out[1], "the append ran in place"
        assert eng.last_ms(2) == 0.0, name
    small.close()
    dense.close()


@pytest.mark.parametrize("n,d", SHAPES)
def test_a_fit_returns_the_same_bits_timed_and_untimed(n, d):
    X, y, th = _problem(n, d)
    got = {}
    for timed in (True, False):
        eng = _engine(X, y)
        eng.set_timing(timed)
        f, g = eng.fit_eval(*th)
        got["fit_eval", timed] = [f, g] + _posterior(eng)
        loss, gl, nlml = eng.fit_eval_loo(*th)
        got["fit_eval_loo", timed] = [loss, gl, nlml] + _posterior(eng)
        assert (eng.last_ms(2) > 0.0) == timed
        eng.close()
    for entry in ("fit_eval", "fit_eval_loo"):
        assert _same(got[entry, True], got[entry, False]), entry
        assert all(np.all(np.isfinite(p)) for p in got[entry, True]), entry


@pytest.mark.parametrize("timed", [True, False])
@pytest.mark.parametrize("n,d", SHAPES)
def test_the_first_loo_call_of_a_context_that_has_fitted_returns_a_fresh_contexts_bits(n, d, timed):
    X, y, th = _problem(n, d)

    def loo(eng):
        loss, g, nlml = eng.fit_eval_loo(*th)
        return [loss, g, nlml] + _posterior(eng)

    fresh = _engine(X, y)
    fresh.set_timing(timed)
    want = loo(fresh)
    # a plain fit first: its scratch holds no LOO region yet, the LOO call has to grow it before anything points into it
    used = _engine(X, y)
    used.set_timing(timed)
    f, g = used.fit_eval(*th)
    assert _same(loo(used), want)
    assert f == want[2]
    # ... and on a context that takes over the pinned buffers of a destroyed one whose scratch a plain fit sized.  The library
    # keeps up to four sets of a destroyed context's host resources and hands out the last one given: four open contexts
    # empty that pool, so `pooled` gets `donor`'s set and nothing that an earlier test's LOO call has grown
    holders = [_engine() for _ in range(4)]
    donor = _engine(X, y)
    donor.fit_eval(*th)
    donor.close()
    pooled = _engine(X, y)
    pooled.set_timing(timed)
    pooled.fit_eval(*th)
    assert _same(loo(pooled), want)
    for eng in [pooled, used, fresh] + holders:
        eng.close()
