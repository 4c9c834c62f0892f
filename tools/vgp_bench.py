#!/usr/bin/env python3
"""
Cost of the variational GP on one MI355X (float64):

  * one ``VGPSurrogate._gp_train`` of 10 iterations (natgrad step + Adam step each) at N = 50, 500, 2048, 8192, D = 12,
    wall clock, plus the predictive install (the first predict after training);
  * leaf-UCB predictions/s on a VGP posterior at C3 (D = 12, N = 2048, 65 536 leaves) beside a GPR posterior of the same
    shape -- the same kernels serve both;
  * a torch.linalg yardstick of the same iteration (natgrad + -ELBO with autograd) on the same GPU.

Usage: python tools/vgp_bench.py [--sizes 50,500,2048,8192] [--likelihood {gaussian,studentt}] [--out FILE]

--likelihood studentt times the same training with ``StudentT(scale=1, df=3)`` and natgrad gamma 0.1 (the quadrature
sequence: one more GEMM and two small passes per natgrad step), beside the Gaussian's numbers of the same run; the torch
yardstick (Gaussian only) is skipped there.

Device time per stage: run ONE training call (10 iterations + the predictive install) under the kernel tracer and fold
its kernels by stage --
    rocprofv3 --kernel-trace -d DIR -o vgp -- python tools/vgp_bench.py --one-train 2048
    python tools/vgp_bench.py --stages DIR/vgp_results.db
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pygpso_amd import HipGPEngine  # noqa: E402
from pygpso_amd import kernels as K  # noqa: E402
from pygpso_amd.gp_surrogate import VGPSurrogate  # noqa: E402
from tests.helpers import synthetic_leaves, synthetic_problem  # noqa: E402


def _surrogate(d, iters, likelihood="gaussian"):
    if likelihood == "studentt":
        return VGPSurrogate(gp_kernel=K.Matern52(lengthscales=0.25 * np.sqrt(d)), gp_meanf=K.Constant(),
                            likelihood=K.StudentT(scale=1.0, df=3.0), natgrad_learning_rate=0.1, train_iterations=iters)
    return VGPSurrogate(gp_kernel=K.Matern52(lengthscales=0.25 * np.sqrt(d)), gp_meanf=K.Constant(), train_iterations=iters)


def time_train(n, d, iters=10, likelihood="gaussian"):
    X, y = synthetic_problem(n, d, seed=0)
    s = _surrogate(d, iters, likelihood)
    s._gp_train(X, y[:, None])  # warm-up: allocations, code objects
    t0 = time.perf_counter()
    s._gp_train(X, y[:, None])
    t1 = time.perf_counter()
    s.gpflow_model.predict_y(X[:1])  # installs the predictive
    t2 = time.perf_counter()
    return {**({"likelihood": likelihood} if likelihood != "gaussian" else {}), "n": n, "d": d, "iterations": iters, "train_ms": (t1 - t0) * 1e3, "per_iteration_ms": (t1 - t0) * 1e3 / iters,
            "install_and_first_predict_ms": (t2 - t1) * 1e3}


def leaf_rate(kind, n=2048, d=12, m=65536, reps=20):
    X, y = synthetic_problem(n, d, seed=0)
    leaves = synthetic_leaves(m, d, seed=1)
    eng = HipGPEngine("float64", device=0)
    eng.set_data(X, y)
    if kind == "vgp":
        u = np.concatenate([[np.log(np.expm1(0.25 * np.sqrt(d)))], [0.5413248546129181], [np.log(np.expm1(1e-3 - 1e-6))], [0.0]])
        eng.vgp_natgrad("Matern52", u, 1, True)
        eng.vgp_posterior("Matern52", u, 1, True)
    else:
        eng.fit_eval("Matern52", 0.25 * np.sqrt(d), 1.0, 1e-3, 0.0, want_grad=False)
    eng.best_ucb(leaves, 1.82)
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.best_ucb(leaves, 1.82)
    dt = (time.perf_counter() - t0) / reps
    eng.close()
    return {"posterior": kind, "n": n, "d": d, "leaves": m, "ms_per_call": dt * 1e3, "predictions_per_s": m / dt}


def torch_yardstick(n, d, iters=10):
    import torch

    dev = torch.device("cuda:0")
    X, y = synthetic_problem(n, d, seed=0)
    Xt = torch.tensor(X, dtype=torch.float64, device=dev)
    yt = torch.tensor(y, dtype=torch.float64, device=dev)
    ls = torch.tensor(0.25 * np.sqrt(d), dtype=torch.float64, device=dev, requires_grad=True)
    var = torch.tensor(1.0, dtype=torch.float64, device=dev, requires_grad=True)
    s2 = torch.tensor(1e-3, dtype=torch.float64, device=dev, requires_grad=True)
    c = torch.tensor(0.0, dtype=torch.float64, device=dev, requires_grad=True)
    eye = torch.eye(n, dtype=torch.float64, device=dev)

    def chol_k():
        r = torch.sqrt(torch.clamp(torch.cdist(Xt / ls, Xt / ls) ** 2, min=1e-36))
        k = var * (1 + 5 ** 0.5 * r + 5.0 / 3.0 * r * r) * torch.exp(-(5 ** 0.5) * r)
        return torch.linalg.cholesky(k + 1e-6 * eye)

    def step():
        with torch.no_grad():
            L = chol_k()
            lam = eye + L.T @ L / s2
            h = L.T @ (yt - c) / s2
            V = torch.linalg.solve_triangular(torch.linalg.cholesky(lam), eye, upper=False)
            Sig = V.T @ V
            mu = Sig @ h
            S = torch.linalg.cholesky(Sig)
        L = chol_k()
        r = yt - (L @ mu + c)
        LS = L @ S
        loss = (0.5 * n * torch.log(2 * np.pi * s2) + (r @ r + (LS * LS).sum()) / (2 * s2)
                + 0.5 * ((S * S).sum() + mu @ mu - n - torch.log(torch.diagonal(S) ** 2).sum()))
        loss.backward()

    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return {"n": n, "d": d, "iterations": iters, "torch_ms": (time.perf_counter() - t0) * 1e3}


# kernel name (substring) -> stage of the VGP iteration
STAGES = (("gram", "Gram k(X, X)"), ("potrf", "Cholesky"), ("inv_lastrow", "Cholesky"), ("kinv_rows", "Cholesky"),
          ("trinv", "triangular inverse"), ("trtri", "triangular inverse"), ("gemm", "GEMM (LDS-DMA tiles)"),
          ("grad_", "gradient contraction"), ("scale_x", "input scaling"), ("vgp_", "VGP element-wise / gemv / sums"),
          ("pack_linv", "install: packing"), ("convert_vec", "install: packing"), ("leaf", "first predict"), ("prep_leaves", "first predict"),
          ("fillBuffer", "memset / copy"), ("copyBuffer", "memset / copy"))


def stages(db_path):
    """fold the kernels of a rocprofv3 database (one training call) by stage: device ms and launches per stage"""
    import sqlite3

    out = {}
    for name, ns in sqlite3.connect(db_path).execute("select name, end - start from kernels"):
        stage = next((st for key, st in STAGES if key in name), "other: " + name.split("(")[0][:60])
        e = out.setdefault(stage, {"ms": 0.0, "launches": 0})
        e["ms"] += ns * 1e-6
        e["launches"] += 1
    return dict(sorted(out.items(), key=lambda kv: -kv[1]["ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50,500,2048,8192")
    ap.add_argument("--out", default=None)
    ap.add_argument("--likelihood", choices=("gaussian", "studentt"), default="gaussian")
    ap.add_argument("--one-train", type=int, default=None, help="run ONE _gp_train of 10 iterations at this N (D = 12)")
    ap.add_argument("--stages", default=None, help="rocprofv3 database of a --one-train run: print device ms per stage")
    a = ap.parse_args()
    if a.stages:
        print(json.dumps(stages(a.stages), indent=1))
        return
    if a.one_train:
        X, y = synthetic_problem(a.one_train, 12, seed=0)
        s = _surrogate(12, 10, a.likelihood)
        s._gp_train(X, y[:, None])
        s.gpflow_model.predict_y(X[:1])
        return
    try:  # (torch opens the device first: initialised after the library's contexts it reports no HIP device)
        import torch

        torch.zeros(1, device="cuda:0")
    except Exception:
        pass
    if a.likelihood == "studentt":
        res = {"train": [], "train_gaussian": [], "ratio_to_gaussian": []}
        for n in [int(v) for v in a.sizes.split(",")]:
            res["train"].append(time_train(n, 12, likelihood="studentt"))
            res["train_gaussian"].append(time_train(n, 12))
            res["ratio_to_gaussian"].append({"n": n, "train_ms": res["train"][-1]["train_ms"] / res["train_gaussian"][-1]["train_ms"]})
            for key in ("train", "train_gaussian", "ratio_to_gaussian"):
                print(json.dumps(res[key][-1]), flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res, indent=1) + "\n")
        return
    res = {"train": [], "leaf_ucb": [], "torch_yardstick": []}
    for n in [int(v) for v in a.sizes.split(",")]:
        res["train"].append(time_train(n, 12))
        print(json.dumps(res["train"][-1]), flush=True)
        try:
            res["torch_yardstick"].append(torch_yardstick(n, 12))
        except Exception as err:  # (a yardstick that cannot run is reported, not fatal)
            res["torch_yardstick"].append({"n": n, "error": str(err)})
        print(json.dumps(res["torch_yardstick"][-1]), flush=True)
    for kind in ("vgp", "gpr"):
        res["leaf_ucb"].append(leaf_rate(kind))
        print(json.dumps(res["leaf_ucb"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
