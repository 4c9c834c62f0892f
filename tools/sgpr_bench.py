#!/usr/bin/env python3
"""
Cost of the sparse GP (SGPR) on one MI355X beside the exact float64 GPR of the same N, in ONE process on one GPU:

  * one -bound + gradient evaluation (``gpso_sgpr_bound_u``) against one NLML + gradient evaluation (``gpso_fit_eval_u``);
  * the greedy selection of Z on the device, and the install of the predictive;
  * leaf-UCB (``gpso_best_ucb``) on the installed SGPR posterior (M rows) against the GPR posterior (N rows);
  * the approximation: RMS difference of SGPR and GPR mean / variance on 8192 of the leaves, from the device predictions of
    both and -- for N <= 2048 -- from the float64 oracle of both on 2048 of them (``rms_*_vs_gpr_oracle``), with the
    device's Z.

Every figure is a host clock around a call that ends in a device synchronise: median of ``--reps`` calls after one warm-up
call of the same shape, with min and max.  ``select`` is the selection alone (the data already on the device; it includes
the read-back of the picks, the host gather of Z and its upload).  ``eval_tflops`` is the WHOLE evaluation's matrix-product
arithmetic (three M_pad^2 N_pad rectangular products, five M_pad^3 square ones) over its wall time -- an end-to-end figure,
not a kernel's share of peak.

Per-kernel shares of the float64 matrix peak: run ONE evaluation under the kernel tracer and fold it --
    rocprofv3 --kernel-trace -d DIR -o sgpr -- python tools/sgpr_bench.py --one-eval 16384:40:1024
    python tools/sgpr_bench.py --stages DIR/sgpr_results.db --one-eval 16384:40:1024
(the GEMM row: every gemm128_kernel launch of the traced evaluation -- the three rectangular and five square products, and
the factorisations' own above the single-level size -- against the flop count of the eight products; the cross contraction: its tile kernel
against 3 D_pad + 4 n_ls' + 40 flops per entry of the M x N matrix, n_ls' = D for ARD and 0 otherwise.)

Usage: python tools/sgpr_bench.py [--configs 2048:12,8192:20,16384:40] [--m 256,512,1024] [--reps 5] [--out FILE]
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

from pygpso_amd import HipGPEngine  # noqa: E402
from tests.helpers import synthetic_leaves, synthetic_problem  # noqa: E402

F64_MATRIX_PEAK_TFLOPS = 78.6  # MI355X float64 matrix peak
LEAVES = {2048: 65536, 8192: 65536, 16384: 131072}  # the README's leaf counts


def _softplus_inv(x):
    return np.log(np.expm1(x))


def _u(d):
    return np.array([_softplus_inv(0.25 * np.sqrt(d)), _softplus_inv(1.0), _softplus_inv(1.0e-2 - 1.0e-6), 0.0])


def timed(call, reps):
    call()  # warm-up of this shape: allocations, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": reps}


def bench(n, d, ms, reps, kernel="Matern52"):
    X, y = synthetic_problem(n, d, seed=0)
    leaves = synthetic_leaves(LEAVES.get(n, 65536), d, seed=1)
    u = _u(d)
    varsigma = 1.82138636771845
    out = {"n": n, "d": d, "leaves": int(leaves.shape[0]), "kernel": kernel, "sgpr": []}
    gpr = HipGPEngine("float64", device=0)
    gpr.set_data(X, y)
    out["gpr_eval"] = timed(lambda: gpr.fit_eval_u(kernel, u, 1, True, 0.0), reps)
    out["gpr_leaf_ucb"] = timed(lambda: gpr.best_ucb(leaves, varsigma), reps)
    mean_g, var_g = gpr.predict(leaves[:8192])
    gpr.close()
    for m in ms:
        if m > n:
            continue
        eng = HipGPEngine("float64", device=0)

        eng.set_data(X, y)
        row = {"m": m, "select": timed(lambda: eng.sgpr_select_inducing(kernel, u, 1, m), reps)}
        row["eval"] = timed(lambda: eng.sgpr_bound_u(kernel, u, 1, True, 0.0), reps)
        row["install"] = timed(lambda: eng.sgpr_posterior(kernel, u, 1, True, 0.0), reps)
        row["leaf_ucb"] = timed(lambda: eng.best_ucb(leaves, varsigma), reps)
        mp = eng.padded_n
        flops = 6.0 * mp * mp * ((n + 127) // 128 * 128) + 10.0 * mp ** 3
        row["eval_tflops"] = flops / (row["eval"]["median_ms"] * 1e-3) / 1e12
        row["eval_fraction_of_f64_matrix_peak"] = row["eval_tflops"] / F64_MATRIX_PEAK_TFLOPS
        row["eval_vs_gpr"] = row["eval"]["median_ms"] / out["gpr_eval"]["median_ms"]
        row["leaf_ucb_vs_gpr"] = row["leaf_ucb"]["median_ms"] / out["gpr_leaf_ucb"]["median_ms"]
        row["m_over_n_squared"] = (m / n) ** 2
        mean_s, var_s = eng.predict(leaves[:8192])
        row["rms_mean_vs_gpr"] = float(np.sqrt(np.mean((mean_s - mean_g) ** 2)))
        row["rms_var_vs_gpr"] = float(np.sqrt(np.mean((var_s - var_g) ** 2)))
        if n <= 2048:
            from oracle import gpr as ogpr
            from tests import sgpr_oracle as S

            Z = eng.sgpr_get_inducing()[0]
            th = ogpr.Theta(kernel, 0.25 * np.sqrt(d), 1.0, 1.0e-2, 0.0)
            mo_g, vo_g = ogpr.predict_y(ogpr.posterior(th, X, y), leaves[:2048])
            mo_s, vo_s = S.Posterior(kernel, u, 1, True, 0.0, X, y, Z).predict_y(leaves[:2048])
            row["rms_mean_vs_gpr_oracle"] = float(np.sqrt(np.mean((mo_s - mo_g) ** 2)))
            row["rms_var_vs_gpr_oracle"] = float(np.sqrt(np.mean((vo_s - vo_g) ** 2)))
        eng.close()
        out["sgpr"].append(row)
        print(json.dumps({"n": n, "d": d, **row}), flush=True)
    return out


def one_eval(n, d, m, kernel="Matern52"):
    """ONE -bound + gradient evaluation (after the selection), for a kernel trace"""
    X, y = synthetic_problem(n, d, seed=0)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    eng.sgpr_select_inducing(kernel, _u(d), 1, m)
    eng.sgpr_bound_u(kernel, _u(d), 1, True, 0.0)
    eng.close()


def stages(db_path, n, d, m):
    """fold the kernels of a rocprofv3 database of --one-eval by name; shares of the f64 matrix peak from flop counts"""
    import sqlite3

    out = {}
    for name, ns in sqlite3.connect(db_path).execute("select name, end - start from kernels"):
        key = name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].replace("void ", "").replace("gpso::", "")[:48]
        e = out.setdefault(key, {"ms": 0.0, "launches": 0})
        e["ms"] += ns * 1e-6
        e["launches"] += 1
    mp, npad, dp = (m + 127) // 128 * 128, (n + 127) // 128 * 128, (d + 3) // 4 * 4
    flops = {"gemm128_kernel": 3 * 2.0 * mp * mp * npad + 5 * 2.0 * mp ** 3, "sgpr_cross_grad_kernel": (3.0 * dp + 40.0) * m * n}
    for key, fl in flops.items():
        if key in out:
            out[key]["flops"] = fl
            out[key]["tflops"] = fl / (out[key]["ms"] * 1e-3) / 1e12
            out[key]["fraction_of_f64_matrix_peak"] = out[key]["tflops"] / F64_MATRIX_PEAK_TFLOPS
    return dict(sorted(out.items(), key=lambda kv: -kv[1]["ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2048:12,8192:20,16384:40")
    ap.add_argument("--m", default="256,512,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-eval", default=None, help="N:D:M -- run ONE selection + evaluation (for rocprofv3 --kernel-trace)")
    ap.add_argument("--stages", default=None, help="rocprofv3 database of a --one-eval run (give --one-eval too): ms per kernel")
    a = ap.parse_args()
    if a.one_eval:
        n, d, m = (int(v) for v in a.one_eval.split(":"))
        if a.stages:
            res = {"tool": "tools/sgpr_bench.py --stages", "n": n, "d": d, "m": m, "kernels": stages(a.stages, n, d, m)}
            if a.out:
                with open(a.out, "w") as fh:
                    json.dump(res, fh, indent=1)
            print(json.dumps(res, indent=1))
        else:
            one_eval(n, d, m)
        return
    ms = [int(v) for v in a.m.split(",")]
    res = {"tool": "tools/sgpr_bench.py", "f64_matrix_peak_tflops": F64_MATRIX_PEAK_TFLOPS, "configs": []}
    for cfg in a.configs.split(","):
        n, d = (int(v) for v in cfg.split(":"))
        res["configs"].append(bench(n, d, ms, a.reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"done": True, "configs": len(res["configs"])}))


if __name__ == "__main__":
    main()
