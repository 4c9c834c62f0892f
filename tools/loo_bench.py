#!/usr/bin/env python3
"""
What one LOO-CV evaluation (gpso_fit_eval_loo: loss + gradient) costs beside one NLML + gradient evaluation (gpso_fit_eval)
on the same float64 context: N = 52, 128 (the one-launch fit and the one-workgroup LOO kernel behind it), 512, 2048 (the
general sequence), D = 6, Matern-5/2.  Wall time around the synchronous C-ABI call (host clock, event timing off, as the
surrogate's engine runs) and the device time of gpso_last_ms(ctx, 2) from a second pass with timing on: a warm-up, then
--reps calls each; median, min, max.  At N <= 128 the general LOO sequence (GPSO_OPT_FIT_FUSED_SMALL = 0) is timed as well.

Writes profiles/loo_bench.json.     python tools/loo_bench.py [--reps 5]
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
            dev.append(eng.last_ms(2) * 1e3)
    return {"wall_us": _stats(wall), "device_us": _stats(dev)}


def main():
    from pygpso_amd import HipGPEngine
    from pygpso_amd import _lib as L
    from tests.helpers import synthetic_problem

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_bench.json"))
    a = ap.parse_args()
    d, rows = 6, []
    for n in (52, 128, 512, 2048):
        X, y = synthetic_problem(n, d, seed=0)
        theta = ("Matern52", 0.25 * np.sqrt(d), 1.3, 1.0e-3, float(y.mean()))
        eng = HipGPEngine("float64")
        eng.set_data(X, y)
        row = {"n": n, "d": d, "path": "small" if n <= 128 else "general"}
        row["nlml_grad"] = _time(eng, lambda: eng.fit_eval(*theta), a.reps)
        row["loo_grad"] = _time(eng, lambda: eng.fit_eval_loo(*theta), a.reps)
        if n <= 128:
            eng._check(eng._lib.gpso_set_option(eng._h, L.OPT_FIT_FUSED_SMALL, 0))
            row["nlml_grad_general"] = _time(eng, lambda: eng.fit_eval(*theta), a.reps)
            row["loo_grad_general"] = _time(eng, lambda: eng.fit_eval_loo(*theta), a.reps)
        for key in ("wall_us", "device_us"):
            row[f"loo_over_nlml_{key}"] = row["loo_grad"][key]["median"] / row["nlml_grad"][key]["median"]
        rows.append(row)
        print(f"N={n:5d}: NLML+grad {row['nlml_grad']['wall_us']['median']:9.1f} us wall / {row['nlml_grad']['device_us']['median']:9.1f} us device,"
              f"   LOO+grad {row['loo_grad']['wall_us']['median']:9.1f} / {row['loo_grad']['device_us']['median']:9.1f}"
              f"   x{row['loo_over_nlml_wall_us']:.2f} wall, x{row['loo_over_nlml_device_us']:.2f} device", flush=True)
        eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"note": "one process, one float64 context per N, D = 6, Matern-5/2, noise 1e-3; medians of --reps calls after 3 "
                           "warm-up calls; wall: host clock around the synchronous call with event timing off; device: gpso_last_ms(ctx, 2)",
                   "reps": a.reps, "rows": rows}, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
