#!/usr/bin/env python3
"""Census for the SCREENED best-UCB call (GPSO_OPT_SCREEN, csrc/screen.hpp): what a landscape prunes, from the CPU oracle alone.

A leaf survives the screen when its ucb at zero variance share, ub = mean + varsigma (sigma^2 + noise), is not below
T' = max(mean) + varsigma noise.  This tool repeats that in float64 numpy on bench.py's own problems
(tests.helpers.synthetic_problem / synthetic_leaves, theta as in bench.py) and prints, per landscape, how many leaves survive,
how many 256-leaf tiles of the compact list that is against the room the survivors' launch has (CUs / row blocks tiles, at
least one), and whether the oracle's arg-max is among the survivors -- so that a reader sees what a landscape prunes before
running anything on a GPU.  The means cost N D per leaf; the variances (N^2 per leaf) are only formed with --check, which
compares against the oracle's arg-max over ALL leaves, and for the survivors.

    python tools/screen_mean_census.py [c3] [--seeds 0 1 2 3 4] [--noise 1e-3] [--leaves M] [--check] [--flat]

--flat: the landscape that prunes nothing -- constant targets, so the posterior mean is flat and the variance decides.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import gpr  # noqa: E402
from tests.helpers import synthetic_leaves, synthetic_problem  # noqa: E402

# name: (D, N, leaves) -- bench.py's workloads
SHAPES = {"c2": (6, 256, 4096), "c3": (12, 2048, 65536), "c4": (20, 8192, 32768), "c5": (40, 16384, 131072)}
CUS = 256


def census(d, n, m, seed=0, noise=1.0e-3, varsigma=gpr.VARSIGMA_DEFAULT, flat=False, check=False, cus=CUS, chunk=16384,
           leaf_seed=None):
    """One landscape -> dict.  `check`: also the oracle's arg-max over all leaves (the full variance: slow at C3's size).
    leaf_seed: the leaves' own seed (default: seed + 1, as bench.py draws them)."""
    X, y = synthetic_problem(n, d, seed=seed)
    if flat:
        y = np.full_like(y, float(y.mean()))
    Xs = synthetic_leaves(m, d, seed=seed + 1 if leaf_seed is None else leaf_seed)
    th = gpr.Theta("Matern52", 0.25 * math.sqrt(d), 1.0, noise, float(y.mean()))
    post = gpr.posterior(th, X, y)
    mean = np.empty(m)
    for s in range(0, m, chunk):
        e = min(m, s + chunk)
        mean[s:e] = gpr.gram(th.kernel, post.X, Xs[s:e], th.lengthscales, th.variance).T @ post.alpha + th.mean_c
    ub = mean + varsigma * (th.variance + th.noise)
    threshold = float(mean.max() + varsigma * th.noise)
    keep = np.flatnonzero(~(ub < threshold))
    # the survivors' full records: the winner among them is the call's result
    var_s = gpr.predict_y(post, Xs[keep])[1]
    ucb_s = mean[keep] + varsigma * var_s  # (the means the screen saw: one summation order)
    winner = int(keep[int(np.argmax(ucb_s))])
    nbi = (n + 255) // 256
    cap_tiles = max(1, cus // nbi)
    out = {"D": d, "N": n, "leaves": m, "seed": seed, "noise": noise, "varsigma": varsigma, "flat": bool(flat),
           "survivors": int(keep.size), "survivor_fraction": keep.size / m, "survivor_tiles": int((keep.size + 255) // 256),
           "room_tiles": cap_tiles, "fits": bool(keep.size <= cap_tiles * 256), "accepted": bool(ucb_s.max() >= threshold),
           "winner": winner, "threshold": threshold, "mean_spread": [float(mean.min()), float(mean.max())],
           "varsigma_var_max": float(varsigma * var_s.max())}
    if check:
        i_ref = gpr.best_ucb(post, Xs, varsigma)[0]
        out["oracle_argmax"] = int(i_ref)
        out["winner_among_survivors"] = bool(i_ref in set(keep.tolist()))
        out["same_winner"] = bool(i_ref == winner)
    out["survivor_index"] = keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["c3"])
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 1, 2, 3, 4])
    ap.add_argument("--noise", type=float, nargs="*", default=[1.0e-3])
    ap.add_argument("--leaves", type=int, default=0, help="leaves per landscape (default: the workload's own count)")
    ap.add_argument("--varsigma", type=float, default=gpr.VARSIGMA_DEFAULT)
    ap.add_argument("--check", action="store_true", help="compare with the oracle's arg-max over all leaves (slow)")
    ap.add_argument("--flat", action="store_true", help="constant targets: the landscape that prunes nothing")
    a = ap.parse_args()
    for name in a.shapes:
        d, n, m = SHAPES[name]
        for noise in a.noise:
            for seed in a.seeds:
                r = census(d, n, a.leaves or m, seed, noise, a.varsigma, a.flat, a.check)
                r.pop("survivor_index")
                print(json.dumps({"shape": name, **r}), flush=True)


if __name__ == "__main__":
    main()
