#!/usr/bin/env python3
"""
What one gpso_predict_grad (mean, var and both gradients at M test points) costs on a float64 context beside one
gpso_predict for the same M -- half the matrix work, on the tuned native f64 tile kernel -- and beside the 2 D + 1
gpso_predict calls that central differences would take for the same gradients: (N, D, M) = (52, 6, 8), (128, 6, 1024),
(2048, 12, 8), (2048, 12, 4096), Matern-5/2.  Device time of gpso_last_ms(ctx, 1) with timing on and wall time around the
synchronous call with timing off: a warm-up, then --reps calls each; median, min, max.  The 2 D + 1 calls are timed as the
loop a caller would run (their device times summed).

Writes profiles/predict_grad_bench.json.     python tools/predict_grad_bench.py [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(samples):
    a = np.sort(np.asarray(samples))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "n": int(a.size)}


def _time(eng, call, reps, warmup=3):
    """call() -> device microseconds of what it ran (read from gpso_last_ms while timing is on)."""
    wall, dev = [], []
    eng.set_timing(False)
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        if it >= warmup:
            wall.append((time.perf_counter() - t0) * 1e6)
    eng.set_timing(True)
    for it in range(warmup + reps):
        us = call()
        if it >= warmup:
            dev.append(us)
    return {"wall_us": _stats(wall), "device_us": _stats(dev)}


def main():
    from pygpso_amd import HipGPEngine
    from tests.helpers import synthetic_problem

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_grad_bench.json"))
    a = ap.parse_args()
    rows = []
    for n, d, m in ((52, 6, 8), (128, 6, 1024), (2048, 12, 8), (2048, 12, 4096)):
        X, y = synthetic_problem(n, d, seed=0)
        eng = HipGPEngine("float64")
        eng.set_data(X, y)
        eng.fit_eval("Matern52", 0.25 * np.sqrt(d), 1.3, 1.0e-3, float(y.mean()), want_grad=False)
        xs = np.random.default_rng(1).random((m, d))
        shifted = [xs] + [xs + s * 1e-6 * np.eye(d)[k] for k in range(d) for s in (1.0, -1.0)]

        def grad():
            eng.predict_grad(xs)
            return eng.last_ms(1) * 1e3

        def predict():
            eng.predict(xs)
            return eng.last_ms(1) * 1e3

        def differences():
            us = 0.0
            for z in shifted:
                eng.predict(z)
                us += eng.last_ms(1) * 1e3
            return us

        row = {"n": n, "d": d, "m": m, "predict_grad": _time(eng, grad, a.reps), "predict": _time(eng, predict, a.reps),
               "predict_2d_plus_1": _time(eng, differences, a.reps)}
        for key in ("wall_us", "device_us"):
            row[f"grad_over_predict_{key}"] = row["predict_grad"][key]["median"] / row["predict"][key]["median"]
            row[f"grad_over_differences_{key}"] = row["predict_grad"][key]["median"] / row["predict_2d_plus_1"][key]["median"]
        rows.append(row)
        print(f"N={n:5d} D={d:3d} M={m:5d}: predict_grad {row['predict_grad']['device_us']['median']:9.1f} us device / "
              f"{row['predict_grad']['wall_us']['median']:9.1f} us wall,   predict {row['predict']['device_us']['median']:9.1f} / "
              f"{row['predict']['wall_us']['median']:9.1f},   {2 * d + 1} predicts {row['predict_2d_plus_1']['device_us']['median']:9.1f} / "
              f"{row['predict_2d_plus_1']['wall_us']['median']:9.1f}", flush=True)
        eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"note": "one process, one float64 context per shape, Matern-5/2, noise 1e-3; medians of --reps calls after 3 warm-up "
                           "calls; device: gpso_last_ms(ctx, 1) with event timing on (host-to-device copy of the points and the "
                           "read-back included, as for gpso_predict); wall: host clock around the synchronous call with timing off; "
                           "predict_2d_plus_1: the 2 D + 1 gpso_predict calls of central differences, summed",
                   "reps": a.reps, "rows": rows}, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
