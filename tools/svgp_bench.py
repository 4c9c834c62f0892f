#!/usr/bin/env python3
"""
Cost of the sparse variational GP (SVGP) on one MI355X, in ONE process on one GPU, for the Gaussian and the Student-t
likelihood on a grid of N x M:

  * one natural-gradient step on q (``gpso_svgp_natgrad``), one -ELBO + gradient evaluation (``gpso_svgp_elbo_u``), the
    install of the predictive (``gpso_svgp_posterior``) and leaf-UCB on it (``gpso_best_ucb``);
  * the yardsticks of the same run: the dense VGP with the Student-t likelihood (``gpso_vgp_natgrad`` + ``gpso_vgp_elbo_u``,
    one training iteration) at N = 2048 and 8192, and the SGPR's evaluation (``gpso_sgpr_bound_u``) on the same Z for the
    Gaussian case.

Every figure is a host clock around a call that ends in a device synchronise: median of ``--reps`` calls after one warm-up
call of the same shape, with min and max.  ``iter_ms`` = natgrad + -ELBO/gradient: one ``SVGPSurrogate`` training
iteration.  ``elbo_tflops`` is the whole -ELBO + gradient evaluation's matrix-product arithmetic (four M_pad^2 N_pad
rectangular products, six M_pad^3 square ones) over its wall time -- an end-to-end figure, not a kernel's share of peak.

Per-kernel shares of the float64 matrix peak: run ONE natgrad step and ONE evaluation under the kernel tracer and fold it --
    rocprofv3 --kernel-trace -d DIR -o svgp -- python tools/svgp_bench.py --one-iter 16384:40:1024
    python tools/svgp_bench.py --stages DIR/svgp_results.db --one-iter 16384:40:1024

Usage: python tools/svgp_bench.py [--configs 2048:12,8192:20,16384:40] [--m 256,512,1024] [--reps 5] [--out FILE]
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
DF, SCALE = 3.0, 0.5
VGP_YARDSTICK_N = (2048, 8192)


def _softplus_inv(x):
    return np.log(np.expm1(x))


def _u(d, lik):
    p = _softplus_inv(SCALE) if lik == "StudentT" else _softplus_inv(1.0e-2 - 1.0e-6)
    return np.array([_softplus_inv(0.25 * np.sqrt(d)), _softplus_inv(1.0), p, 0.0])


def timed(call, reps):
    call()  # warm-up of this shape: allocations, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": reps}


def _svgp_engine(X, y, d, m, lik, kernel="Matern52"):
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    eng.vgp_set_likelihood(lik, DF, 20)
    eng.sgpr_select_inducing(kernel, _u(d, lik), 1, m)
    s2 = SCALE ** 2 * DF / (DF - 2.0) if lik == "StudentT" else 1.0e-2
    eng.svgp_init_q(kernel, _u(d, lik), 1, True, 0.0, s2)
    return eng


def bench(n, d, ms, reps, kernel="Matern52"):
    X, y = synthetic_problem(n, d, seed=0)
    leaves = synthetic_leaves(LEAVES.get(n, 65536), d, seed=1)
    varsigma = 1.82138636771845
    out = {"n": n, "d": d, "leaves": int(leaves.shape[0]), "kernel": kernel, "svgp": []}
    if n in VGP_YARDSTICK_N:  # the dense Student-t VGP: one training iteration
        u = _u(d, "StudentT")
        vgp = HipGPEngine("float64", device=0)
        vgp.set_data(X, y)
        vgp.vgp_set_likelihood("StudentT", DF, 20)
        vgp.vgp_set_q()
        out["vgp_studentt_natgrad"] = timed(lambda: vgp.vgp_natgrad(kernel, u, 1, True, 0.0, 0.1), reps)
        out["vgp_studentt_elbo"] = timed(lambda: vgp.vgp_elbo_u(kernel, u, 1, True, 0.0), reps)
        out["vgp_studentt_iter_ms"] = out["vgp_studentt_natgrad"]["median_ms"] + out["vgp_studentt_elbo"]["median_ms"]
        vgp.close()
    for m in ms:
        if m > n:
            continue
        for lik in ("Gaussian", "StudentT"):
            eng = _svgp_engine(X, y, d, m, lik, kernel)
            u = _u(d, lik)
            row = {"m": m, "likelihood": lik}
            row["natgrad"] = timed(lambda: eng.svgp_natgrad(kernel, u, 1, True, 0.0, 0.1), reps)
            row["elbo"] = timed(lambda: eng.svgp_elbo_u(kernel, u, 1, True, 0.0), reps)
            row["install"] = timed(lambda: eng.svgp_posterior(kernel, u, 1, True, 0.0), reps)
            row["leaf_ucb"] = timed(lambda: eng.best_ucb(leaves, varsigma), reps)
            row["iter_ms"] = row["natgrad"]["median_ms"] + row["elbo"]["median_ms"]
            mp, npad = eng.padded_n, (n + 127) // 128 * 128
            flops = 2.0 * (4.0 * mp * mp * npad + 6.0 * mp ** 3)
            row["elbo_tflops"] = flops / (row["elbo"]["median_ms"] * 1e-3) / 1e12
            row["elbo_fraction_of_f64_matrix_peak"] = row["elbo_tflops"] / F64_MATRIX_PEAK_TFLOPS
            if lik == "StudentT" and "vgp_studentt_iter_ms" in out:
                row["iter_vs_vgp_studentt"] = row["iter_ms"] / out["vgp_studentt_iter_ms"]
            if lik == "Gaussian":
                row["sgpr_eval"] = timed(lambda: eng.sgpr_bound_u(kernel, _u(d, lik), 1, True, 0.0), reps)
                row["elbo_vs_sgpr_eval"] = row["elbo"]["median_ms"] / row["sgpr_eval"]["median_ms"]
            eng.close()
            out["svgp"].append(row)
            print(json.dumps({"n": n, "d": d, **row}), flush=True)
    return out


def one_iter(n, d, m, kernel="Matern52"):
    """ONE Student-t natgrad step and ONE -ELBO + gradient evaluation (after the selection and q's start), for a trace"""
    X, y = synthetic_problem(n, d, seed=0)
    eng = _svgp_engine(X, y, d, m, "StudentT", kernel)
    eng.svgp_natgrad(kernel, _u(d, "StudentT"), 1, True, 0.0, 0.1)
    eng.svgp_elbo_u(kernel, _u(d, "StudentT"), 1, True, 0.0)
    eng.close()


def stages(db_path, n, d, m):
    """fold the kernels of a rocprofv3 database of --one-iter by name (the selection and the start included)"""
    import sqlite3

    out = {}
    for name, ns in sqlite3.connect(db_path).execute("select name, end - start from kernels"):
        key = name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].replace("void ", "").replace("gpso::", "")[:48]
        e = out.setdefault(key, {"ms": 0.0, "launches": 0})
        e["ms"] += ns * 1e-6
        e["launches"] += 1
    mp, npad = (m + 127) // 128 * 128, (n + 127) // 128 * 128
    # the rectangular products of the traced calls: the start's natgrad (A, A diag(a) A^T), natgrad (A, S^T A, A diag(a)
    # A^T), elbo (A, S^T A, A diag(a) A^T, g); the square ones are counted at M_pad^3 each (start 3, natgrad 4, elbo 6)
    rect, sq = 2 + 3 + 4, 3 + 4 + 6
    fl = 2.0 * (rect * mp * mp * npad + sq * mp ** 3)
    if "gemm128_kernel" in out:
        g = out["gemm128_kernel"]
        g["flops"] = fl
        g["tflops"] = fl / (g["ms"] * 1e-3) / 1e12
        g["fraction_of_f64_matrix_peak"] = g["tflops"] / F64_MATRIX_PEAK_TFLOPS
    return dict(sorted(out.items(), key=lambda kv: -kv[1]["ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2048:12,8192:20,16384:40")
    ap.add_argument("--m", default="256,512,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-iter", default=None, help="N:D:M -- ONE natgrad + ONE evaluation (for rocprofv3 --kernel-trace)")
    ap.add_argument("--stages", default=None, help="rocprofv3 database of a --one-iter run (give --one-iter too): ms per kernel")
    a = ap.parse_args()
    if a.one_iter:
        n, d, m = (int(v) for v in a.one_iter.split(":"))
        if a.stages:
            res = {"tool": "tools/svgp_bench.py --stages", "n": n, "d": d, "m": m, "likelihood": "StudentT",
                   "kernels": stages(a.stages, n, d, m)}
            if a.out:
                with open(a.out, "w") as fh:
                    json.dump(res, fh, indent=1)
            print(json.dumps(res, indent=1))
        else:
            one_iter(n, d, m)
        return
    ms = [int(v) for v in a.m.split(",")]
    res = {"tool": "tools/svgp_bench.py", "f64_matrix_peak_tflops": F64_MATRIX_PEAK_TFLOPS, "studentt": {"df": DF, "scale": SCALE},
           "configs": []}
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
