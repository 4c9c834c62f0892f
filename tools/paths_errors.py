#!/usr/bin/env python3
"""
Measured errors and cost of gpso_paths_draw / gpso_paths_eval.

Parity: the cases of tests/paths_cases.py (what tests/test_gpu_paths.py asserts) on float64 and mixed engines against the
float64 oracle of tests/paths_oracle.py -- per kernel class (the three smooth ones | Matern-1/2) and engine type the largest
value error over the case's tolerance scale, with the case that set it, and the number of (draw, segment) pairs whose index
disagreed with the oracle's.  Writes profiles/paths_parity.json.

Cost: D = 12, N = 2048, Matern-5/2, float64, F = 1024 and 4096, S = 16 and 64: the device time (the event pair behind
gpso_last_ms(ctx, 1), medians) of one gpso_paths_draw and of one gpso_paths_eval over 65 536 device-resident rows with the
values left on the device, the evaluation's useful FLOP rate 2 S M (N + F) / time as a share of the 78.6 TFLOP/s float64
matrix peak, and its generated values M (N + F) per second.  The time is the whole call's (input scaling, the evaluation
kernel, the arg-max), so the kernel's own share is at least what is stated.  Beside it the wall time of the numpy oracle
for the same evaluation on the host (measured over --oracle-rows of the rows in blocks of 1024 and scaled: the [N, M, D]
difference array of all of them at once is 13 GB), the only other route to these values.  Writes profiles/paths_bench.json.

    python tools/paths_errors.py [--out-dir profiles] [--reps 5] [--skip-parity] [--skip-bench]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MATRIX_PEAK = 78.6e12


def _parity():
    from tests import paths_cases as pc
    from tests import paths_oracle as po
    from tests import test_gpu_paths as T

    worst = {}
    for index in range(len(pc.CASES)):
        r = pc.reference(index)
        kernel = pc.CASES[index][2]
        scale = r["tol"] / (1.0e-4 if kernel == "Matern12" else 1.0e-8)
        for dtype in ("float64", "mixed"):
            eng = T.drawn(r, dtype)
            values, idx, val = eng.paths_eval(r["Xs"])
            eng.close()
            want_i, want_v = po.seg_argmax(r["values"])
            b = worst.setdefault(f"{'Matern12' if kernel == 'Matern12' else 'smooth'} {dtype}",
                                 {"values": {"max": -1.0}, "best_val": {"max": -1.0}, "index_mismatches": 0, "pairs": 0})
            for key, err in (("values", np.max(np.abs(values - r["values"]))), ("best_val", np.max(np.abs(val - want_v)))):
                if err / scale > b[key]["max"]:
                    b[key] = {"max": float(err / scale), "case": pc.name(index)}
            b["index_mismatches"] += int(np.sum(idx != want_i))
            b["pairs"] += int(idx.size)
    return worst


def _bench(reps, oracle_rows):
    import torch

    from oracle import gpr
    from pygpso_amd import HipGPEngine
    from pygpso_amd import paths as P
    from tests import paths_oracle as po
    from tests.helpers import synthetic_leaves, synthetic_problem

    n, d, m = 2048, 12, 65536
    X, y = synthetic_problem(n, d, seed=1)
    th = gpr.Theta("Matern52", [0.25 * np.sqrt(d)], 1.0, 1.0e-2, float(y.mean()))
    leaves = synthetic_leaves(m, d, seed=2)
    eng = HipGPEngine("float64")
    eng.set_timing(True)
    eng.set_data(X, y)
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
    xt = torch.from_numpy(leaves).to(torch.device("cuda", eng.device))
    torch.cuda.synchronize()
    rows = []
    for f in (1024, 4096):
        for s in (16, 64):
            omega, phase, w, eps = P.draw_path_inputs(th.kernel, s, f, n, d, rng=3)
            draw_ms, eval_ms = [], []
            for rep in range(reps + 1):  # (the first pass warms both shapes up and is dropped)
                eng.paths_draw(omega, phase, w, eps)
                draw_ms.append(eng.last_ms(1))
                _, idx, val = eng.paths_eval(xt, want_values=False)
                eval_ms.append(eng.last_ms(1))
            t = float(np.median(eval_ms[1:])) * 1e-3
            row = {"f": f, "s": s, "draw_device_ms": float(np.median(draw_ms[1:])), "eval_device_ms": t * 1e3,
                   "eval_useful_tflops": 2.0 * s * m * (n + f) / t / 1e12,
                   "eval_share_of_f64_matrix_peak": 2.0 * s * m * (n + f) / t / F64_MATRIX_PEAK,
                   "generated_values_per_s": m * (n + f) / t}
            if (f, s) == (1024, 16) and oracle_rows > 0:
                post = gpr.posterior(th, X, y)
                v = po.solve_v(post, po.residual(post, None, omega, phase, w, eps))
                t0 = time.perf_counter()
                parts = [po.evaluate(post, omega, phase, w, v, leaves[o:o + 1024]) for o in range(0, oracle_rows, 1024)]
                wall = time.perf_counter() - t0
                got = eng.paths_eval(leaves[:oracle_rows])[0]
                row["numpy_oracle_wall_s_scaled_to_all_rows"] = wall * m / oracle_rows
                row["numpy_oracle_rows_measured"] = oracle_rows
                row["max_abs_difference_to_the_oracle"] = float(np.max(np.abs(np.hstack(parts) - got)))
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    return {"n": n, "d": d, "m": m, "kernel": "Matern52", "dtype": "float64", "reps": reps, "cases": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-rows", type=int, default=8192)
    ap.add_argument("--skip-parity", action="store_true")
    ap.add_argument("--skip-bench", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if not a.skip_bench:
        import torch  # (before the library opens the device, as under pytest: torch finds no GPU behind it otherwise)

        if torch.cuda.device_count() < 1:
            raise SystemExit("the cost figures need a GPU")
    if not a.skip_parity:
        worst = _parity()
        with open(os.path.join(a.out_dir, "paths_parity.json"), "w") as fh:
            json.dump({"note": "gpso_paths_draw + gpso_paths_eval against tests/paths_oracle.py over the cases of tests/paths_cases.py; "
                               "errors by the case's scale max(max|y|, sqrt(variance) max|w|)",
                       "tolerances": {"smooth": 1.0e-8, "Matern12": 1.0e-4}, "measured": worst}, fh, indent=1)
            fh.write("\n")
        for cls, b in worst.items():
            print(cls, f"values {b['values']['max']:.2e}, best_val {b['best_val']['max']:.2e}, "
                       f"index mismatches {b['index_mismatches']} of {b['pairs']}", flush=True)
    if not a.skip_bench:
        bench = _bench(a.reps, a.oracle_rows)
        with open(os.path.join(a.out_dir, "paths_bench.json"), "w") as fh:
            json.dump({"note": "one MI355X, one process, medians of the device time between the event pair of each call "
                               "(gpso_last_ms(ctx, 1)); the evaluation over 65 536 device-resident float64 rows, values left on "
                               "the device (best_idx / best_val only); rates count the useful work 2 S M (N + F)", **bench},
                      fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
