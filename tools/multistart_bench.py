#!/usr/bin/env python3
"""
Multi-start hyper-parameter search: what a batched evaluation costs, and what restarts buy.

Part 1 -- one gpso_fit_eval_u_batch of B entries against B sequential gpso_fit_eval_u calls (the path of a search without
restarts, launch for launch) on one float64 context, in one process: (N, D) = (16, 2), (52, 2), (52, 12), (128, 12),
B = 1, 8, 64, 256.  Wall time per call around the C-ABI call (host clock; the calls are synchronous), a warm-up, then
--reps timed calls: median, min, max.
Part 2 -- the rotated-peaks toy run of tests/helpers.py with Scipy(restarts=1) and Scipy(restarts=8), same seeds: per
gp_update the final NLML and the wall time of the update, and how often a restart beat the warm start.

Writes profiles/multistart_bench.json.     python tools/multistart_bench.py [--reps 30] [--part 1|2|all]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(samples_us):
    a = np.sort(np.asarray(samples_us))
    return {"median_us": float(np.median(a)), "min_us": float(a[0]), "max_us": float(a[-1]), "n": int(a.size)}


def part1(reps, warmup=5):
    from oracle import gpr
    from pygpso_amd import HipGPEngine
    from tests.helpers import synthetic_problem

    rows = []
    for n, d in [(16, 2), (52, 2), (52, 12), (128, 12)]:
        X, y = synthetic_problem(n, d, seed=0)
        eng = HipGPEngine("float64")
        eng.set_timing(False)  # (as the surrogate's engine runs: no event pairs around the calls)
        eng.set_data(X, y)
        rng = np.random.default_rng(n + d)
        centre = np.array([gpr.softplus_inv(0.25 * np.sqrt(d)), gpr.softplus_inv(1.3), gpr.softplus_inv(1e-2), float(y.mean())])
        for B in (1, 8, 64, 256):
            U = np.ascontiguousarray(centre + 0.3 * rng.standard_normal((B, 4)))
            tb, ts = [], []
            for it in range(warmup + reps):
                t0 = time.perf_counter()
                loss, _, ok = eng.fit_eval_u_batch("Matern52", U, 1, True)
                t1 = time.perf_counter()
                for u in U:
                    eng.fit_eval_u("Matern52", u, 1, True)
                t2 = time.perf_counter()
                if it >= warmup:
                    tb.append((t1 - t0) * 1e6)
                    ts.append((t2 - t1) * 1e6)
            assert np.all(ok)
            b, s = _stats(tb), _stats(ts)
            rows.append({"n": n, "d": d, "B": B, "batch": b, "sequential": s,
                         "sequential_over_batch": s["median_us"] / b["median_us"]})
            print(f"N={n:4d} D={d:3d} B={B:4d}: batch {b['median_us']:9.1f} us [{b['min_us']:.1f}, {b['max_us']:.1f}]   "
                  f"sequential {s['median_us']:10.1f} us [{s['min_us']:.1f}, {s['max_us']:.1f}]   x{rows[-1]['sequential_over_batch']:.1f}",
                  flush=True)
        eng.close()
    for r in rows:  # B = 256 against B = 1 at the same shape
        one = next(q for q in rows if (q["n"], q["d"], q["B"]) == (r["n"], r["d"], 1))
        r["batch_over_batch_of_1"] = r["batch"]["median_us"] / one["batch"]["median_us"]
    return rows


def part2():
    from pygpso_amd import GPRSurrogate, GPSOptimiser, ParameterSpace
    from pygpso_amd.kernels import Constant, Matern52, Scipy
    from tests.helpers import load_goldens, rotated_peaks

    g4 = load_goldens()["G4"]
    out = {}
    for restarts in (1, 8):
        surr = GPRSurrogate(gp_kernel=Matern52(lengthscales=0.25, variance=1.0), gp_meanf=Constant(0.0),
                            optimiser=Scipy(restarts=restarts, seed=0), gauss_likelihood_sigma=1.0e-3)
        updates = []
        inner = surr.gp_update

        def timed_update():
            t0 = time.perf_counter()
            inner()
            dt = time.perf_counter() - t0
            res = surr.optimiser.last_result
            updates.append({"n": int(surr.num_evaluated), "nlml": float(res.fun), "wall_ms": dt * 1e3,
                            "winner": int(res.get("winner", 0)), "nfev": int(sum(r["nfev"] for r in res["restarts"])) if "restarts" in res else int(res.nfev)})

        surr.gp_update = timed_update
        space = ParameterSpace(parameter_names=["x", "y"], parameter_bounds=g4["bounds"])
        opt = GPSOptimiser(parameter_space=space, gp_surrogate=surr, exploration_method="tree", exploration_depth=g4["depth"],
                           budget=g4["budget"], stopping_condition="evaluations", update_cycle=1, n_workers=1)
        best = opt.run(rotated_peaks)
        out[f"restarts_{restarts}"] = {"best_score": float(best.score_mu), "updates": updates,
                                       "restart_won": int(sum(1 for u in updates if u["winner"] != 0)),
                                       "wall_ms_total": float(sum(u["wall_ms"] for u in updates))}
        print(f"restarts={restarts}: {len(updates)} updates, {out[f'restarts_{restarts}']['wall_ms_total']:.1f} ms in gp_update, "
              f"a restart won {out[f'restarts_{restarts}']['restart_won']} times, best score {best.score_mu:.8f}", flush=True)
        surr.gpflow_model.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--part", default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistart_bench.json"))
    a = ap.parse_args()
    result = {"note": "wall time around synchronous C-ABI calls, one process, one float64 context per shape; "
                      "the two runs of part 2 diverge once a restart wins, so their updates are not at the same data"}
    if a.part in ("1", "all"):
        result["batch_vs_sequential"] = part1(max(20, a.reps))
    if a.part in ("2", "all"):
        result["toy_run"] = part2()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
