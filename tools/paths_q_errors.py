#!/usr/bin/env python3
"""
Measured errors and cost of gpso_paths_draw_q, beside tools/paths_errors.py.

Parity: the cases of tests/paths_q_cases.py (what tests/test_gpu_paths_q.py asserts) on float64 and mixed engines against
the float64 oracle of tests/paths_q_oracle.py -- per kernel class (the three smooth ones | Matern-1/2) and engine type the
largest value and best_val error over the case's scale, with the case that set it, the (draw, segment) pairs the gap rule
left out and the indices that differed from the oracle's among the others; every case's own figures too.  Writes
profiles/paths_q_parity.json.

Cost: D = 12, Matern-5/2, float64, F = 1024, S = 16 and 64: the device time (the event pair behind gpso_last_ms(ctx, 1),
medians of --reps after one dropped pass) of one gpso_paths_draw_q and of one gpso_paths_eval over 65 536 device-resident
rows with the values left on the device, for a VGP at N = 2048 (one natural-gradient step from the prior) and an SGPR at
N = 8192 with M = 256 and 1024 inducing rows (the first M training rows).  The exact GP's row at N = 2048 is
profiles/paths_bench.json's (tools/paths_errors.py); the expectation to confirm or refute is that the evaluation's time
follows n + F, n the resident rows.  Writes profiles/paths_q_bench.json.

    python tools/paths_q_errors.py [--out-dir profiles] [--reps 5] [--skip-parity] [--skip-bench]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _parity():
    from tests import paths_q_cases as qc
    from tests import test_gpu_paths_q as G

    worst, cases = {}, []
    for index in range(len(qc.CASES)):
        r = qc.reference(index)
        kernel = r["kernel"]
        scale = r["tol"] / (1.0e-4 if kernel == "Matern12" else 1.0e-8)
        for dtype in ("float64", "mixed"):
            eng = G.drawn(r, dtype)
            got = [(None, eng.paths_eval(r["Xs"]))]
            if r["Xs"].shape[0] == 130:
                got.append((qc.SEGMENTS, eng.paths_eval(r["Xs"], seg_off=qc.SEGMENTS)))
            eng.close()
            b = worst.setdefault(f"{'Matern12' if kernel == 'Matern12' else 'smooth'} {dtype}",
                                 {"values": {"max": -1.0}, "best_val": {"max": -1.0}, "index_mismatches": 0, "pairs_left_out": 0,
                                  "pairs": 0})
            for seg, g in got:
                e_val, e_best, wrong, undecided, pairs = G.measure(g, r, seg)
                for key, err in (("values", e_val), ("best_val", e_best)):
                    if err / scale > b[key]["max"]:
                        b[key] = {"max": float(err / scale), "case": qc.name(index)}
                b["index_mismatches"] += wrong
                b["pairs_left_out"] += undecided
                b["pairs"] += pairs
                if seg is None:
                    cases.append({"case": qc.name(index), "dtype": dtype, "values": e_val / scale, "best_val": e_best / scale})
    return worst, cases


def _bench(reps):
    import torch

    from pygpso_amd import HipGPEngine
    from pygpso_amd import paths as P
    from tests import sgpr_oracle as SG
    from tests.helpers import synthetic_leaves, synthetic_problem

    d, m, f, kernel = 12, 65536, 1024, "Matern52"
    leaves = synthetic_leaves(m, d, seed=2)
    rows = []
    for family, big_n, n in (("vgp", 2048, 2048), ("sgpr", 8192, 256), ("sgpr", 8192, 1024)):
        X, y = synthetic_problem(big_n, d, seed=1)
        u = SG.initial_u(0.25 * np.sqrt(d), 1.0, 1.0e-2, float(y.mean()))
        eng = HipGPEngine("float64")
        eng.set_timing(True)
        eng.set_data(X, y)
        if family == "vgp":
            eng.vgp_set_q()
            eng.vgp_natgrad(kernel, u, 1, True, 0.0, 1.0)
            eng.vgp_posterior(kernel, u, 1, True, 0.0)
        else:
            eng.sgpr_set_inducing(X[:n])
            eng.sgpr_posterior(kernel, u, 1, True, 0.0)
        xt = torch.from_numpy(leaves).to(torch.device("cuda", eng.device))
        torch.cuda.synchronize()
        for s in (16, 64):
            omega, phase, w, eps = P.draw_path_inputs(kernel, s, f, n, d, rng=3)
            draw_ms, eval_ms = [], []
            for rep in range(reps + 1):  # (the first pass warms both shapes up and is dropped)
                eng.paths_draw_q(omega, phase, w, eps)
                draw_ms.append(eng.last_ms(1))
                eng.paths_eval(xt, want_values=False)
                eval_ms.append(eng.last_ms(1))
            t = float(np.median(eval_ms[1:]))
            row = {"family": family, "n_train": big_n, "resident_rows": n, "f": f, "s": s,
                   "draw_device_ms": float(np.median(draw_ms[1:])), "eval_device_ms": t,
                   "eval_ns_per_point_and_index": t * 1e6 / (m * (n + f)), "generated_values_per_s": m * (n + f) / (t * 1e-3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        eng.close()
    return {"d": d, "m": m, "kernel": kernel, "dtype": "float64", "reps": reps, "cases": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-parity", action="store_true")
    ap.add_argument("--skip-bench", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if not a.skip_bench:
        import torch  # (before the library opens the device, as under pytest: torch finds no GPU behind it otherwise)

        if torch.cuda.device_count() < 1:
            raise SystemExit("the cost figures need a GPU")
    if not a.skip_parity:
        worst, cases = _parity()
        with open(os.path.join(a.out_dir, "paths_q_parity.json"), "w") as fh:
            json.dump({"note": "gpso_paths_draw_q + gpso_paths_eval against tests/paths_q_oracle.py over the cases of "
                               "tests/paths_q_cases.py; errors by the case's scale max(max|y|, sqrt(variance) max|w|); an index "
                               "is compared where the oracle's two highest values differ by ten times the bar or more",
                       "tolerances": {"smooth": 1.0e-8, "Matern12": 1.0e-4}, "measured": worst, "cases": cases}, fh, indent=1)
            fh.write("\n")
        for cls, b in worst.items():
            print(cls, f"values {b['values']['max']:.2e}, best_val {b['best_val']['max']:.2e}, index mismatches "
                       f"{b['index_mismatches']}, left out {b['pairs_left_out']} of {b['pairs']}", flush=True)
    if not a.skip_bench:
        bench = _bench(a.reps)
        with open(os.path.join(a.out_dir, "paths_q_bench.json"), "w") as fh:
            json.dump({"note": "one MI355X, one process, medians of the device time between the event pair of each call "
                               "(gpso_last_ms(ctx, 1)); the evaluation over 65 536 device-resident float64 rows, values left on "
                               "the device (best_idx / best_val only); the exact GP's rows are profiles/paths_bench.json's", **bench},
                      fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
