#!/usr/bin/env python3
"""
What the integrated acquisition over a hyper-parameter ensemble costs on the device, beside the way a user had before it.

One process, one GPU.  For K in {4, 16, 32} members and the shapes (N, D, M) = (52, 2, 162) -- the optimiser's regime: one
exploration level of the 2-D loop -- and (128, 12, 65 536) -- the ensemble's limit in N and a full batch of leaves --, two
candidates are timed in turn (interleaved: whatever else the host does meets both):

  integrated   ONE context holding K members; one gpso_ensemble_best_acq call (stage 1, the fold, the arg-max, one read-back
               of a record)
  k_contexts   the way of the parent commit: K contexts, each fitted at its theta; K gpso_acq_values calls (3 columns of M
               doubles over PCIe each) and the fold and arg-max in numpy

Each figure is the median host wall time of CALLS synchronous calls after WARMUP, repeated REPEATS times; the min and max of
the repeated medians are kept beside their median.  Both candidates rank by the reference's mean + varsigma * var, the leaves
are host float64 arrays, and the winners are compared (the same leaf, values within 1e-9).
Then ``HipGPR.sample_hyper`` -- what hyper="marginal" adds to every update -- at the default tuning on the N = 52 problem:
wall time of one call and its number of batched launches.

Nothing here has a target: the figures are recorded.  Without a GPU the script fails (no fallback).
Writes one JSON document (default profiles/ensemble_bench.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pygpso_amd import HipGPEngine, acquisition, priors  # noqa: E402
from pygpso_amd.kernels import Constant, Matern52  # noqa: E402
from pygpso_amd.model import HipGPR  # noqa: E402

VARSIGMA = 1.82138636771845
SHAPES = ((52, 2, 162), (128, 12, 65536))
KS = (4, 16, 32)


def problem(n, d, m, seed=0):
    rng = np.random.default_rng([seed, n, d])
    X = rng.random((n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.05 * rng.standard_normal(n)
    leaves = np.random.default_rng([seed + 1, m, d]).random((m, d))
    return X, y, leaves


def thetas(k, d, y, seed=2):
    rng = np.random.default_rng([seed, k, d])
    return [(float(0.3 * np.sqrt(d) * np.exp(0.3 * rng.standard_normal())), float(np.exp(0.3 * rng.standard_normal())),
             float(2e-3 * np.exp(0.5 * rng.standard_normal())), float(y.mean())) for _ in range(k)]


def timed(fns, calls, warmup, repeats):
    """{name: {"median_us", "min_us", "max_us"}} of the candidates ``fns``, run in turn within every repeat."""
    meds = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            for _ in range(warmup):
                fn()
            ts = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            meds[name].append(statistics.median(ts) * 1e6)
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in meds.items()}


def bench_shape(n, d, m, k, calls, warmup, repeats):
    X, y, leaves = problem(n, d, m)
    th = thetas(k, d, y)
    acq = acquisition.UCBVar(VARSIGMA)
    one = HipGPEngine("float64")
    one.set_data(X, y)
    many = []
    for ls, var, noise, c in th:
        one.fit_eval("Matern52", [ls], var, noise, c, want_grad=False)
        one.ensemble_push()
        e = HipGPEngine("float64")
        e.set_data(X, y)
        e.fit_eval("Matern52", [ls], var, noise, c, want_grad=False)
        many.append(e)

    def integrated():
        return one.ensemble_best_acq(leaves, acq)

    def k_contexts():
        total = None
        for e in many:
            val = e.acq_values(leaves, acq)[2]
            total = val if total is None else total + val
        total = total / float(k)
        j = int(np.argmax(total))
        return j, total[j]

    idx, _, _, value = integrated()
    j, v = k_contexts()
    same = bool(int(idx[0]) == j and abs(value[0] - v) <= 1e-9 * max(1.0, abs(v)))
    res = timed({"integrated": integrated, "k_contexts": k_contexts}, calls, warmup, repeats)
    res["same_winner"] = same
    res["device_ms_integrated"] = one.last_ms(1)
    for e in many:
        e.close()
    one.close()
    return res


def bench_sampler(repeats):
    X, y, _ = problem(52, 2, 1)
    model = HipGPR((X, y), Matern52(variance=1.0, lengthscales=0.25), Constant(0.0), noise_variance=1e-3)
    priors.attach(model, priors.default_priors())
    model.sample_hyper(16, rng=0)  # warm-up: code objects, buffers
    ts, calls = [], 0
    for r in range(repeats):
        t0 = time.perf_counter()
        _, info = model.sample_hyper(16, rng=r + 1)
        ts.append(time.perf_counter() - t0)
        calls = info["batch_calls"]
    t0 = time.perf_counter()
    U, _ = model.sample_hyper(16, rng=0)
    model.install_ensemble(U)
    both = time.perf_counter() - t0
    model.engine.close()
    return {"n": 52, "d": 2, "n_samples": 16, "batch_calls": calls, "median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3,
            "max_ms": max(ts) * 1e3, "sample_and_install_ms": both * 1e3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    doc = {"tool": "tools/ensemble_bench.py", "calls": args.calls, "warmup": args.warmup, "repeats": args.repeats,
           "clock": "host wall time around synchronous calls", "acquisition": "ucb_var", "leaves": "host float64", "shapes": []}
    for n, d, m in SHAPES:
        for k in KS:
            r = bench_shape(n, d, m, k, args.calls, args.warmup, args.repeats)
            r.update(n=n, d=d, m=m, k=k)
            doc["shapes"].append(r)
            print(f"N={n} D={d} M={m} K={k}: integrated {r['integrated']['median_us']:.0f} us, K contexts "
                  f"{r['k_contexts']['median_us']:.0f} us, same winner {r['same_winner']}", flush=True)
    doc["sample_hyper"] = bench_sampler(args.repeats)
    print("sample_hyper:", doc["sample_hyper"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
