#!/usr/bin/env python3
"""
What the constrained acquisition costs on the device, beside the way a user had before it.

One process, one GPU.  For J in {1, 4, 16} constraint models and the shapes (N, D, M) = (52, 2, 162) -- the optimiser's
regime: one exploration level of the 2-D loop -- and (128, 12, 65 536) -- the constraint set's limit in N and a full batch of
leaves --, two candidates are timed in turn (interleaved: whatever else the host does meets both):

  constrained   ONE context holding the objective's posterior and J members; one gpso_constrained_best_acq call (stage 1 for
                the objective and for the members, the fold, the arg-max, the gather, one read-back of a record)
  j_contexts    the way of the parent commit: J + 1 contexts, each fitted on its own targets; J + 1 gpso_acq_values calls (3
                columns of M doubles over PCIe each), the fold (scipy's log_ndtr, the gate) and the arg-max in numpy

Each figure is the median host wall time of CALLS synchronous calls after WARMUP, repeated REPEATS times; the min and max of
the repeated medians are kept beside their median.  Both candidates rank by the reference's mean + varsigma * var in gate mode
at P(feasible) >= 0.5, thresholds at the median of each model's training targets, the leaves are host float64 arrays, and
the winners are compared (the same leaf, values within 1e-9).

Nothing here has a target: the figures are recorded.  Without a GPU the script fails (no fallback).
Writes one JSON document (default profiles/constraints_bench.json).
"""
import argparse
import json
import os
import sys

import numpy as np
from scipy.special import log_ndtr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ensemble_bench import problem, thetas, timed  # noqa: E402

from pygpso_amd import HipGPEngine, acquisition  # noqa: E402

VARSIGMA = 1.82138636771845
SHAPES = ((52, 2, 162), (128, 12, 65536))
JS = (1, 4, 16)
LOG_POF_MIN = float(np.log(0.5))


def constraint_targets(X, j, seed=3):
    rng = np.random.default_rng([seed, j, X.shape[1]])
    w = rng.normal(size=(j, X.shape[1]))
    ph = rng.uniform(0.0, 2.0 * np.pi, j)
    return np.array([np.sin(2.0 * X @ w[i] + ph[i]) for i in range(j)])


def bench_shape(n, d, m, j, calls, warmup, repeats):
    X, y, leaves = problem(n, d, m)
    cY = constraint_targets(X, j)
    th = thetas(j + 1, d, y)
    acq = acquisition.UCBVar(VARSIGMA)
    thr = np.median(cY, axis=1)
    sense = np.array([1 if i % 2 == 0 else -1 for i in range(j)])
    many = []
    for i, (ls, var, noise, c) in enumerate(th):
        e = HipGPEngine("float64")
        e.set_data(X, y if i == 0 else cY[i - 1])
        e.fit_eval("Matern52", [ls], var, noise, c if i == 0 else float(cY[i - 1].mean()), want_grad=False)
        many.append(e)
    one = many[0]  # (the objective's context holds the set: the constrained calls leave its posterior alone)
    for i in range(j):
        one.constraint_push(many[i + 1], thr[i], int(sense[i]))
    noise = np.array([t[2] for t in th[1:]])

    def constrained():
        return one.constrained_best_acq(leaves, acq, "gate", LOG_POF_MIN)

    def j_contexts():
        value = many[0].acq_values(leaves, acq)[2]
        logpof = None
        for i in range(j):
            cm, cv, _ = many[i + 1].acq_values(leaves, acq)
            s = np.sqrt(np.maximum(cv - noise[i], 0.0))
            lp = log_ndtr(sense[i] * (thr[i] - cm) / s)
            logpof = lp if logpof is None else logpof + lp
        value = np.where(logpof >= LOG_POF_MIN, value, -np.inf)
        k = int(np.argmax(value))
        return k, value[k]

    idx, _, _, value, _ = constrained()
    k, v = j_contexts()
    same = bool(int(idx[0]) == k and (value[0] == v or abs(value[0] - v) <= 1e-9 * max(1.0, abs(v))))
    res = timed({"constrained": constrained, "j_contexts": j_contexts}, calls, warmup, repeats)
    res["same_winner"] = same
    one.constrained_best_acq(leaves, acq, "gate", LOG_POF_MIN)
    res["device_ms_constrained"] = one.last_ms(1)
    for e in many:
        e.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constraints_bench.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    doc = {"tool": "tools/constraints_bench.py", "calls": args.calls, "warmup": args.warmup, "repeats": args.repeats,
           "clock": "host wall time around synchronous calls", "acquisition": "ucb_var", "mode": "gate", "pof_min": 0.5,
           "leaves": "host float64", "shapes": []}
    for n, d, m in SHAPES:
        for j in JS:
            r = bench_shape(n, d, m, j, args.calls, args.warmup, args.repeats)
            r.update(n=n, d=d, m=m, j=j)
            doc["shapes"].append(r)
            print(f"N={n} D={d} M={m} J={j}: constrained {r['constrained']['median_us']:.0f} us, J + 1 contexts "
                  f"{r['j_contexts']['median_us']:.0f} us, same winner {r['same_winner']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
