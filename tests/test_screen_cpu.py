"""CPU-only checks of the screened best-UCB call's arithmetic: csrc/screen.hpp through ``gpso_screen_*_host`` (the header the
device code includes), and tools/screen_mean_census.py against the oracle."""
import numpy as np
import pytest

from oracle import gpr
from pygpso_amd import HipGPEngine
from tools.screen_mean_census import census


def test_the_finalise_expression_never_exceeds_the_bound():
    """Random (my, v >= 0, variance, noise, varsigma >= 0) in double: ucb(my, v) <= ub(my) = ucb(my, 0), and the host's
    restatement is numpy's two roundings."""
    rng = np.random.default_rng(0)
    n = 20000
    for _ in range(25):
        variance = float(10.0 ** rng.uniform(-3, 3))
        noise = float(10.0 ** rng.uniform(-9, 0))
        varsigma = float(rng.choice([0.0, 1e-3, gpr.VARSIGMA_DEFAULT, 50.0, 10.0 ** rng.uniform(-6, 6)]))
        my = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, size=n)
        # variance shares from 0 (and denormal) to beyond the prior variance (a negative fv: the kernel's arithmetic allows it)
        v = np.abs(rng.normal(size=n)) * variance * 10.0 ** rng.uniform(-20, 0.5, size=n)
        v[:100] = 0.0
        v[100:200] = 5e-324
        ucb, ub = HipGPEngine.screen_eval_host(my, v, variance, noise, varsigma)
        assert np.all(ucb <= ub)
        assert np.array_equal(ucb, my + varsigma * ((variance - v) + noise))
        assert np.array_equal(ub, my + varsigma * (variance + noise))
        assert np.array_equal(ucb[:100], ub[:100])


def test_threshold_survival_and_acceptance_rules():
    threshold, survives, accepts = HipGPEngine.screen_rules_host()
    nan, inf = float("nan"), float("inf")
    assert threshold(2.5, 1e-3, 1.5) == 2.5 + 1.5 * 1e-3
    assert threshold(-inf, 1e-3, 1.5) == -inf  # (no finite mean: nothing is pruned)
    # a leaf survives unless its bound lies below the threshold; a mean that is not finite always survives
    assert survives(0.0, 1.0, 1.0) and survives(0.0, 2.0, 1.0) and not survives(0.0, 0.999, 1.0)
    assert survives(nan, nan, 1.0) and survives(inf, inf, 1.0) and survives(-inf, -inf, 1.0)
    assert survives(0.0, -1e300, -inf)
    # the survivors' winner: accepted iff its ucb is NaN or reaches the threshold, and the survivors fitted the launch
    assert accepts(1.0, 1.0, 5, 10) and accepts(3.0, 1.0, 10, 10) and accepts(nan, 1.0, 5, 10)
    assert not accepts(0.999, 1.0, 5, 10)  # u* < T': cannot be provoked on a device, so it is checked here
    assert not accepts(3.0, 1.0, 11, 10) and not accepts(nan, 1.0, 11, 10) and not accepts(3.0, 1.0, 0, 10)
    assert accepts(-1e300, -inf, 5, 10)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_the_census_keeps_the_oracles_argmax_at_c3(seed):
    """C3's posterior (N 2048, D 12, theta as bench.py) on 4 096 of its leaves: the survivors contain the oracle's arg-max over
    ALL leaves, the winner among the survivors is that leaf, and the landscape prunes most of the batch."""
    c = census(12, 2048, 4096, seed=seed, check=True)
    assert c["winner_among_survivors"] and c["same_winner"] and c["accepted"] and c["fits"]
    assert c["oracle_argmax"] in set(c["survivor_index"].tolist())
    assert 1 <= c["survivors"] < 4096 // 4


def test_a_flat_mean_prunes_nothing():
    c = census(12, 768, 2000, seed=0, flat=True, check=True)
    assert c["survivors"] == 2000 and c["winner_among_survivors"] and c["same_winner"]
