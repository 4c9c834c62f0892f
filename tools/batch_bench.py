#!/usr/bin/env python3
"""
What one gpso_best_batch call (q leaves picked greedily under hallucinated updates) costs, beside the only route to the same
picks that existed before it: q rounds of gpso_best_acq followed by gpso_append at y = mean on a scratch context.

Shapes (N, D, M, q) = (2048, 12, 65536, 16), (8192, 20, 32768, 16), (52, 6, 729, 4), Matern-5/2, noise 1e-3, ucb_var, float64
and mixed engines.  Median of --reps calls after 3 warm-up calls: device time (gpso_last_ms(ctx, 1), event timing on) and wall
time (host clock around the synchronous call, timing off).  A split per later round comes from three more timings of the
same context: the call with q = 1 (round 0 alone: the predict path, one arg-max, one finish), the call with q rounds with
and without var_after, and gpso_cross_cov of 64 points against one (the pick vectors plus one column tile):
    later_round = (t(q) - t(1)) / (q - 1),   pick_vectors ~ t(cross_cov, m = 64, b = 1),   column + finish = the rest.

    python tools/batch_bench.py [--reps 7]                      # the new call -> profiles/batch_bench.json
    GPSO_HIP_LIB=<the parent commit's library> GPSO_HIP_LIB_OLDER=1 python tools/batch_bench.py --old-route --out old.json
    python tools/batch_bench.py --merge old.json                # adds the old route's rows to profiles/batch_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/batch_bench.py --calls-only 2048,12,65536,16
                                                                # four mixed calls and nothing else: the per-kernel split
                                                                # (profiles/batch_kernel_stats_n2048.csv, _n8192.csv)

The old route is timed per call as the q rounds alone; the fit that resets the scratch context between calls is not counted
(a caller would copy the posterior instead).  An append that crosses a padding boundary refits from scratch: that is what
the route costs at N = 2048 and 8192, and the row says how many appends ran in place.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((2048, 12, 65536, 16), (8192, 20, 32768, 16), (52, 6, 729, 4))
NOISE = 1.0e-3


def _stats(samples):
    a = np.sort(np.asarray(samples, dtype=np.float64))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "n": int(a.size)}


def _time(eng, call, reps, warmup=3):
    wall, dev = [], []
    eng.set_timing(False)
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        if it >= warmup:
            wall.append((time.perf_counter() - t0) * 1e6)
    eng.set_timing(True)
    for it in range(warmup + reps):
        call()
        if it >= warmup:
            dev.append(eng.last_ms(1) * 1e3)
    return {"wall_us": _stats(wall), "device_us": _stats(dev)}


def _fitted(dtype, X, y, d):
    from pygpso_amd import HipGPEngine

    eng = HipGPEngine(dtype)
    eng.set_data(X, y)
    eng.fit_eval("Matern52", 0.25 * np.sqrt(d), 1.0, NOISE, float(y.mean()), want_grad=False)
    return eng


def new_call(reps):
    from pygpso_amd import acquisition as A
    from tests.helpers import synthetic_leaves, synthetic_problem

    rows = []
    for n, d, m, q in SHAPES:
        X, y = synthetic_problem(n, d, seed=0)
        leaves = synthetic_leaves(m, d, seed=1)
        for dtype in ("float64", "mixed"):
            eng = _fitted(dtype, X, y, d)
            spec = A.UCBVar(2.0)
            row = {"n": n, "d": d, "m": m, "q": q, "dtype": dtype,
                   "best_batch": _time(eng, lambda: eng.best_batch(leaves, spec, q, NOISE), reps),
                   "best_batch_var_after": _time(eng, lambda: eng.best_batch(leaves, spec, q, NOISE, want_var_after=True), reps),
                   "best_batch_q1": _time(eng, lambda: eng.best_batch(leaves, spec, 1, NOISE), reps),
                   "best_acq": _time(eng, lambda: eng.best_acq(leaves, spec), reps),
                   "cross_cov_m64_b1": _time(eng, lambda: eng.cross_cov(leaves[:64], leaves[:1]), reps)}
            split = {}
            for key in ("wall_us", "device_us"):
                tq, t1 = row["best_batch"][key]["median"], row["best_batch_q1"][key]["median"]
                later = (tq - t1) / (q - 1)
                pick = row["cross_cov_m64_b1"][key]["median"]
                split[key] = {"round_0": t1, "later_round": later, "pick_vectors_upper": pick, "column_and_finish": later - pick}
            row["split"] = split
            rows.append(row)
            dv = row["best_batch"]["device_us"]["median"]
            print(f"N={n:5d} D={d:3d} M={m:6d} q={q:2d} {dtype:8s}: best_batch {dv:10.1f} us device / "
                  f"{row['best_batch']['wall_us']['median']:10.1f} us wall;  round 0 {split['device_us']['round_0']:9.1f}, later round "
                  f"{split['device_us']['later_round']:9.1f} (pick vectors <= {split['device_us']['pick_vectors_upper']:8.1f})", flush=True)
            eng.close()
    return rows


def old_route(reps):
    from pygpso_amd import acquisition as A
    from tests.helpers import synthetic_leaves, synthetic_problem

    rows = []
    for n, d, m, q in SHAPES:
        X, y = synthetic_problem(n, d, seed=0)
        leaves = synthetic_leaves(m, d, seed=1)
        for dtype in ("float64", "mixed"):
            eng = _fitted(dtype, X, y, d)
            eng.set_timing(False)
            spec = A.UCBVar(2.0)
            wall, in_place = [], 0
            for it in range(3 + reps):
                eng.set_data(X, y)
                eng.fit_eval("Matern52", 0.25 * np.sqrt(d), 1.0, NOISE, float(y.mean()), want_grad=False)
                eng.synchronize()
                t0 = time.perf_counter()
                for _ in range(q):
                    idx, mean, _, _ = eng.best_acq(leaves, spec)
                    _, ok = eng.append(leaves[idx[0]:idx[0] + 1], mean[:1])
                    in_place += int(ok) if it >= 3 else 0
                eng.synchronize()
                if it >= 3:
                    wall.append((time.perf_counter() - t0) * 1e6)
            rows.append({"n": n, "d": d, "m": m, "q": q, "dtype": dtype, "append_then_best_acq": {"wall_us": _stats(wall)},
                         "appends_in_place": in_place, "appends": q * reps})
            print(f"N={n:5d} D={d:3d} M={m:6d} q={q:2d} {dtype:8s}: old route {np.median(wall):10.1f} us wall "
                  f"({in_place} of {q * reps} appends in place)", flush=True)
            eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--old-route", action="store_true")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--calls-only", default=None, metavar="N,D,M,Q")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.json"))
    a = ap.parse_args()
    if a.calls_only:
        from pygpso_amd import acquisition as A
        from tests.helpers import synthetic_leaves, synthetic_problem

        n, d, m, q = (int(v) for v in a.calls_only.split(","))
        X, y = synthetic_problem(n, d, seed=0)
        eng, leaves = _fitted("mixed", X, y, d), synthetic_leaves(m, d, seed=1)
        for _ in range(4):
            eng.best_batch(leaves, A.UCBVar(2.0), q, NOISE)
        eng.close()
        return
    if a.merge:
        with open(a.out) as fh:
            doc = json.load(fh)
        with open(a.merge) as fh:
            old = json.load(fh)
        doc["old_route_note"] = old["note"]
        for row in doc["rows"]:
            for o in old["rows"]:
                if all(row[k] == o[k] for k in ("n", "d", "m", "q", "dtype")):
                    row["old_route"] = {k: o[k] for k in ("append_then_best_acq", "appends_in_place", "appends")}
                    row["old_over_new_wall"] = o["append_then_best_acq"]["wall_us"]["median"] / row["best_batch"]["wall_us"]["median"]
    elif a.old_route:
        doc = {"note": "q rounds of gpso_best_acq + gpso_append at y = mean on a scratch context, library of the parent commit; wall "
                       "time of the q rounds, median of --reps after 3; the fit that resets the context between calls is not counted",
               "reps": a.reps, "rows": old_route(a.reps)}
    else:
        doc = {"note": "one process, one context per shape and engine, Matern-5/2, noise 1e-3, ucb_var, obs_noise = noise; medians of "
                       "--reps calls after 3 warm-up calls; device: gpso_last_ms(ctx, 1) with event timing on (the host-to-device copy "
                       "of the leaves and the read-back included); wall: host clock around the synchronous call with timing off; "
                       "split: round_0 = the call with q = 1, later_round = (t(q) - t(1)) / (q - 1), pick_vectors_upper = "
                       "gpso_cross_cov of 64 points against 1 (the pick vectors plus one column tile and a copy)",
               "reps": a.reps, "rows": new_call(a.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
