"""CPU checks of greedy batch selection under hallucinated updates: the library's host entry point
(``gpso_batch_greedy_host``, the arithmetic of csrc/batch.hpp the device kernels share) against the dense-solve oracle of
``tests/batch_oracle.py``, the oracle against a refit with the picks appended, the end rules and the refusals.

Tolerances: picks identical; var, value and var_after within 1e-10 of the kernel variance (1.0 here) -- two float64 routes
to the same conditional covariance, the recursion's q rank-one downdates against one dense solve.  Picks are only asked
where they are decidable: at every round the oracle's relative gap between the best and the runner-up exceeds 100 x 1e-8
(the gaps of these cases lie between 9e-4 and 1e-1) -- asserted, no round excused."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import gpr
from pygpso_amd import HipGPEngine
from pygpso_amd import _lib as L
from pygpso_amd import acquisition as A
from tests import batch_oracle as B
from tests import hetero_oracle as H
from tests.joint_oracle import textbook_joint

VS = gpr.VARSIGMA_DEFAULT
TOL = 1e-10


def _spec(name):
    return A.UCBVar(VS) if name == "ucb_var" else A.UCBStd(VS)


@functools.lru_cache(maxsize=None)
def _case(i):
    X, y, theta, leaves = B.problem(i)
    mean, Sigma = textbook_joint(theta, X, y, leaves)
    return X, y, theta, leaves, mean, Sigma


@pytest.mark.parametrize("name", ["ucb_var", "ucb_std"])
@pytest.mark.parametrize("i", range(len(B.PROBLEMS)))
def test_host_rounds_agree_with_the_dense_solve_oracle(i, name):
    X, y, theta, leaves, mean, Sigma = _case(i)
    s2 = np.diag(Sigma) + theta.noise
    want = B.greedy(mean, Sigma, leaves, theta.noise, theta.noise, name, B.ROUNDS)
    print(f"case {i} {name}: gaps {[f'{g:.1e}' for g in want.gaps]}")
    assert len(want.idx) == B.ROUNDS and np.all(want.gaps > B.GAP_FLOOR), want.gaps
    idx, var, val, after = HipGPEngine.batch_greedy_host(_spec(name), mean, s2, Sigma, theta.noise, theta.noise, B.ROUNDS)
    assert list(idx) == list(want.idx)
    assert len(set(idx.tolist())) == B.ROUNDS
    for got, ref, what in ((var, want.var, "var"), (val, want.value, "value"), (after, want.var_after, "var_after")):
        err = float(np.max(np.abs(got - ref)))
        print(f"  {what}: {err:.2e}")
        assert err <= TOL * theta.variance, (what, err)
    # round 0 is the plain arg-max of the unconditioned column, and every variance only falls
    assert idx[0] == int(np.argmax(B.acq_column(name, mean, s2)))
    assert np.all(after <= s2 + 1e-15)


@pytest.mark.parametrize("obs_factor", [1.0, 3.0])
@pytest.mark.parametrize("i", range(len(B.PROBLEMS)))
def test_oracle_agrees_with_a_refit_on_the_picks(i, obs_factor):
    """Append the picks to (X, y) at y = their means with per-point noise obs_noise - noise (the form of section 7f): the
    refitted predictive has the oracle's variances and the old means."""
    X, y, theta, leaves, mean, Sigma = _case(i)
    obs = obs_factor * theta.noise
    res = B.greedy(mean, Sigma, leaves, theta.noise, obs, "ucb_var", B.ROUNDS)
    P = res.idx
    X2, y2 = np.vstack([X, leaves[P]]), np.concatenate([y, mean[P]])
    if obs_factor == 1.0:
        post = gpr.posterior(theta, X2, y2)
    else:
        post = H.posterior(theta, X2, y2, np.concatenate([np.zeros(len(y)), np.full(len(P), obs - theta.noise)]))
    m2, v2 = gpr.predict_y(post, leaves)
    assert float(np.max(np.abs(v2 - res.var_after))) <= 1e-9
    assert float(np.max(np.abs(m2 - mean))) <= 1e-9


def _toy(m=6):
    rng = np.random.default_rng(7)
    Aq = rng.normal(size=(m, m))
    Sigma = Aq @ Aq.T / m + 0.1 * np.eye(m)
    return rng.normal(size=m), Sigma


def test_q_beyond_the_distinct_rows_ends_with_the_rows():
    mean, Sigma = _toy(5)
    idx, var, val, after = HipGPEngine.batch_greedy_host(A.UCBVar(VS), mean, np.diag(Sigma) + 0.01, Sigma, 0.01, 0.01, 9)
    assert sorted(idx.tolist()) == [0, 1, 2, 3, 4]
    want = B.greedy(mean, Sigma, np.arange(5.0)[:, None], 0.01, 0.01, "ucb_var", 9)
    assert list(idx) == list(want.idx)
    np.testing.assert_allclose(after, want.var_after, rtol=0, atol=TOL)


def test_a_duplicated_row_is_retired_with_its_twin():
    X, y, theta, leaves, _, _ = _case(1)
    leaves = np.vstack([leaves[:20], leaves[:20][::-1]])  # every row twice
    mean, Sigma = B.expanded_joint(theta, X, y, leaves)
    s2 = np.diag(Sigma) + theta.noise
    idx, var, val, after = HipGPEngine.batch_greedy_host(A.UCBVar(VS), mean, s2, Sigma, theta.noise, theta.noise, 30)
    assert len(idx) == 20  # q = 30 > 20 distinct rows
    rows = {tuple(leaves[i]) for i in idx}
    assert len(rows) == 20
    want = B.greedy(mean, Sigma, leaves, theta.noise, theta.noise, "ucb_var", 30)
    assert list(idx[:6]) == list(want.idx[:6])  # (the first of each pair: the lower index)
    # a retired row's variance is still updated: the twin has the pick's var_after
    twin = 39 - idx[0]  # (the pick is the first of its pair)
    assert after[twin] == after[idx[0]] and after[twin] < s2[twin]


def test_a_pick_with_no_variance_left_ends_the_batch_after_it():
    """obs_noise = 0 at a training input of a noise-free model: its latent variance is zero -- written here as the exact
    zeros of that row and column --, so d = 0: the pick is reported, changes nothing, and the batch ends."""
    mean, Sigma = _toy(6)
    p = 3
    Sigma[p, :] = Sigma[:, p] = 0.0
    mean[p] = 10.0
    s2 = np.diag(Sigma) + 0.01
    idx, var, val, after = HipGPEngine.batch_greedy_host(A.UCBVar(VS), mean, s2, Sigma, 0.01, 0.0, 4)
    assert list(idx) == [p] and var[0] == s2[p] and val[0] == mean[p] + VS * s2[p]
    np.testing.assert_array_equal(after, s2)
    want = B.greedy(mean, Sigma, np.arange(6.0)[:, None], 0.01, 0.0, "ucb_var", 4)
    assert list(want.idx) == [p]
    # with any fantasy noise the same pick goes through
    idx, *_ = HipGPEngine.batch_greedy_host(A.UCBVar(VS), mean, s2, Sigma, 0.01, 0.01, 4)
    assert len(idx) == 4 and idx[0] == p


def test_a_nan_row_is_picked_first_and_ends_the_batch():
    mean, Sigma = _toy(6)
    mean[4] = np.nan
    s2 = np.diag(Sigma) + 0.01
    for spec in (A.UCBVar(VS), A.UCBStd(VS), A.EI(incumbent=0.0), A.LogEI(incumbent=0.0), A.PI(incumbent=0.0)):
        idx, var, val, after = HipGPEngine.batch_greedy_host(spec, mean, s2, Sigma, 0.01, 0.01, 3)
        assert list(idx) == [4] and np.isnan(val[0])
        np.testing.assert_array_equal(after, s2)


def test_latent_kinds_read_the_variance_without_the_noise():
    mean, Sigma = _toy(6)
    s2 = np.diag(Sigma) + 0.05
    a = HipGPEngine.batch_greedy_host(A.UCBStd(VS, latent=True), mean, s2, Sigma, 0.05, 0.05, 4)
    want = B.greedy(mean, Sigma, np.arange(6.0)[:, None], 0.05, 0.05, "ucb_std", 4, latent=True)
    assert list(a[0]) == list(want.idx)
    np.testing.assert_allclose(a[2], want.value, rtol=0, atol=TOL)
    b = HipGPEngine.batch_greedy_host(A.UCBStd(VS), mean, s2, Sigma, 0.05, 0.05, 4)
    assert not np.array_equal(a[2], b[2])


def test_refusals_that_need_no_device():
    lib = L.load()
    mean, Sigma = _toy(4)
    s2 = np.diag(Sigma) + 0.01
    idx, var, val, after = np.zeros(64, dtype=np.int64), np.zeros(64), np.zeros(64), np.zeros(4)
    n = C.c_int(-7)

    def call(rec, obs=0.01, m=4, q=2, mean_p=L.dptr(mean), idx_p=L.i64ptr(idx), n_p=C.byref(n)):
        return lib.gpso_batch_greedy_host(rec, mean_p, L.dptr(s2), L.dptr(Sigma), 0.01, obs, m, q, idx_p, L.dptr(var), L.dptr(val), n_p,
                                          L.dptr(after))

    good = A.UCBVar(VS).c_struct(None)
    assert call(C.byref(good)) == L.OK and n.value == 2
    n.value = -7
    assert call(None) == L.E_ARG
    assert call(C.byref(A.UCBStd(np.nan).c_struct(None))) == L.E_ARG
    assert call(C.byref(A.EI(incumbent=np.inf).c_struct(None))) == L.E_ARG
    for kw in (dict(q=0), dict(q=65), dict(m=0), dict(obs=-1e-3), dict(obs=np.nan), dict(obs=np.inf), dict(mean_p=None), dict(idx_p=None),
               dict(n_p=None), dict(m=(1 << 27) // 2 + 1, q=2)):
        assert call(C.byref(good), **kw) == L.E_ARG, kw
    assert n.value == -7  # a refused call writes nothing
