"""
Who frees what (csrc/devbuf.hpp) on the MI355X: every byte of device memory a context allocates goes back when the context
is closed.  ``last_count(4)`` is the process-wide count of bytes the contexts' buffers hold now; a probe context that is
never given data reads it before a context of each model family is opened, while that context lives (it holds at least
the buffers the family is known to work in) and after it is closed -- where the count stands exactly where it stood.
The equalities are exact by construction: the count moves by a buffer's size when it is allocated and when it is freed.
"""
import functools
import gc

import numpy as np
import pytest

from tests.helpers import synthetic_leaves, synthetic_problem
from tests.test_gpu_theta import GAUSS, KERNEL, _u

pytestmark = pytest.mark.gpu
N, D, M, LEAVES = 300, 3, 64, 257


@functools.lru_cache(maxsize=None)
def _problem():
    X, y = synthetic_problem(N, D, seed=7)
    leaves = synthetic_leaves(LEAVES, D, seed=11)
    Z = X[::4][:M].copy()
    for a in (X, y, leaves, Z):
        a.setflags(write=False)
    return X, y, Z, leaves


@pytest.fixture(scope="module")
def probe():
    from pygpso_amd import HipGPEngine

    gc.collect()  # (a context an earlier test left to the collector is closed now, not between two readings)
    eng = HipGPEngine("float64", device=0)
    yield eng
    eng.close()


def _gpr(eng, u, Z):
    eng.fit_eval_u(KERNEL, u, D, True)  # (the evaluation leaves its posterior resident)
    return eng.padded_n ** 2 * 8  # K in the fit type is half of that in a float32 context; Lf, linv and work lie beside it


def _vgp(eng, u, Z):
    eng.vgp_set_likelihood(*GAUSS, 20)
    eng.vgp_set_q(np.zeros(N), 0.5 * np.eye(N))
    eng.vgp_elbo_u(KERNEL, u, D, True)
    eng.vgp_posterior(KERNEL, u, D, True)
    return 4 * eng.padded_n ** 2 * 8  # vA, vB, vC, q's S


def _sparse(svgp, moving):
    def run(eng, u, Z):
        n_pad = eng.padded_n
        eng.vgp_set_likelihood(*GAUSS, 20)
        eng.sgpr_set_inducing(Z)
        if svgp:
            eng.svgp_init_q(KERNEL, u, D, True, 0.0, 0.01)
        Z2 = Z + 0.01 if moving else None
        if moving:
            (eng.svgp_elbo_uz if svgp else eng.sgpr_bound_uz)(KERNEL, u, D, True, 0.0, Z=Z2)
        else:
            (eng.svgp_elbo_u if svgp else eng.sgpr_bound_u)(KERNEL, u, D, True)
        (eng.svgp_posterior if svgp else eng.sgpr_posterior)(KERNEL, u, D, True)
        assert (n_pad, eng.padded_n) == (384, 128)
        return 3 * eng.padded_n * n_pad * 8  # sgKuf, sgA and sgW (SGPR) or svB (SVGP)

    return run


CASES = [("gpr-float64", "float64", _gpr), ("gpr-float32", "float32", _gpr), ("gpr-mixed", "mixed", _gpr),
         ("vgp", "float64", _vgp), ("sgpr", "float64", _sparse(False, False)), ("svgp", "float64", _sparse(True, False)),
         ("sgpr-moving-z", "float64", _sparse(False, True)), ("svgp-moving-z", "float64", _sparse(True, True))]


@pytest.mark.parametrize("dtype,run", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_a_closed_context_holds_nothing(probe, dtype, run):
    from pygpso_amd import HipGPEngine

    X, y, Z, leaves = _problem()
    b0 = probe.last_count(4)
    assert b0 >= 0
    eng = HipGPEngine(dtype, device=0)
    eng.set_data(X, y)
    known = run(eng, _u(D, True, "ordinary"), Z)
    mean, var = eng.predict(leaves)
    assert mean.shape == (LEAVES,) and np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    held = probe.last_count(4) - b0
    print(f"held while alive: {held} bytes (known buffers {known})")
    assert held >= known, (held, known)
    eng.close()
    assert probe.last_count(4) == b0, (probe.last_count(4), b0)


def test_q_replaced_across_a_padded_size_goes_back_too(probe):
    """gpso_vgp_extend_q from N = 120 (N_pad 128) to 140 (N_pad 256) makes q's two buffers anew and frees the old pair."""
    from pygpso_amd import HipGPEngine

    X, y, _, _ = _problem()
    b0 = probe.last_count(4)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X[:120], y[:120])
    assert eng.padded_n == 128
    eng.vgp_set_q(np.zeros(120), 0.5 * np.eye(120))
    with_q = probe.last_count(4)
    eng.set_data(X[:140], y[:140])
    assert eng.padded_n == 256
    before = probe.last_count(4)
    eng.vgp_extend_q()
    # S [N_pad^2] and mu [N_pad] at the new padded size in place of those at the old one, and nothing else
    assert probe.last_count(4) - before == (256 * 256 + 256) * 8 - (128 * 128 + 128) * 8
    assert with_q - b0 >= (128 * 128 + 128) * 8
    mu, S = eng.vgp_get_q()
    assert np.array_equal(mu, np.zeros(140)) and np.array_equal(S[:120, :120], 0.5 * np.eye(120)) and np.array_equal(S[120:, 120:], np.eye(20))
    eng.close()
    assert probe.last_count(4) == b0, (probe.last_count(4), b0)
