#!/usr/bin/env python3
"""
What the acquisition maps cost on the device, and that gpso_best_ucb costs what it did.

One process, one GPU.  Per workload and context: wall time of a synchronous gpso_best_ucb / gpso_best_acq call (every kind),
as the median of CALLS calls after WARMUP, repeated REPEATS times with the candidates interleaved; min and max of the
repeated medians are kept beside their median (the run-to-run spread a comparison has to clear).  With --parent-lib the
same gpso_best_ucb figures are taken from an EARLIER build of the library loaded into the same process (its own contexts,
interleaved with the current build's): `gpso_best_ucb` of this build must not exceed the parent's median by more than the
parent's own max - min.

  workload "leaves":  N = 2048, D = 12, 65 536 leaves in one segment      (GPSO_MIXED and GPSO_F64)
  workload "grow":    N = 52,   D = 2,  best_*_grow of 3 boxes at depth 6 (the optimiser's regime)

Writes one JSON document (default profiles/acq_bench.json).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pygpso_amd import _lib as L  # noqa: E402

KINDS = [("ucb_var", L.ACQ_UCB_VAR), ("ucb_std", L.ACQ_UCB_STD), ("ei", L.ACQ_EI), ("logei", L.ACQ_LOGEI), ("pi", L.ACQ_PI)]
VARSIGMA = 1.82138636771845


def open_lib(path):
    lib = C.CDLL(path)
    for name, (restype, argtypes) in L.SIGNATURES.items():
        if hasattr(lib, name):  # (an earlier build lacks the newer entry points)
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


class Ctx:
    """A fitted context of one build of the library, through the C-ABI."""

    def __init__(self, lib, dtype, X, y, lengthscale):
        self.lib = lib
        self.h = C.c_void_p()
        self.ok(lib.gpso_create(C.byref(self.h), 0, dtype))
        n, d = X.shape
        self.ok(lib.gpso_set_data(self.h, L.dptr(X), L.dptr(y), n, d))
        ls = np.array([lengthscale], dtype=np.float64)
        nlml = C.c_double()
        self.ok(lib.gpso_fit_eval(self.h, L.MATERN52, L.dptr(ls), 1, 1.0, 1.0e-3, float(y.mean()), C.byref(nlml), None))
        self.idx = np.empty(8, dtype=np.int64)
        self.out = [np.empty(8, dtype=np.float64) for _ in range(3)]
        self.outs = (L.i64ptr(self.idx),) + tuple(L.dptr(o) for o in self.out)

    def ok(self, rc):
        if rc < 0:
            raise RuntimeError(f"status {rc}: {self.lib.gpso_last_error(self.h).decode()}")

    def best_ucb(self, leaves):
        self.ok(self.lib.gpso_best_ucb(self.h, C.c_void_p(leaves.ctypes.data), L.F64, L.MEM_HOST, leaves.shape[0], None, 1,
                                       VARSIGMA, *self.outs))

    def best_acq(self, leaves, rec):
        self.ok(self.lib.gpso_best_acq(self.h, C.c_void_p(leaves.ctypes.data), L.F64, L.MEM_HOST, leaves.shape[0], None, 1,
                                       C.byref(rec), *self.outs))

    def best_ucb_grow(self, boxes, depth):
        self.ok(self.lib.gpso_best_ucb_grow(self.h, L.dptr(boxes), boxes.shape[0], depth, VARSIGMA, *self.outs))

    def best_acq_grow(self, boxes, depth, rec):
        self.ok(self.lib.gpso_best_acq_grow(self.h, L.dptr(boxes), boxes.shape[0], depth, C.byref(rec), *self.outs))

    def close(self):
        self.lib.gpso_destroy(self.h)


def median_us(fn, calls):
    t = np.empty(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        fn()
        t[i] = time.perf_counter() - t0
    return float(np.median(t) * 1e6)


def measure(cands, calls, warmup, repeats):
    """cands: {name: callable} -> {name: {median_us, min_us, max_us, medians_us}} over `repeats` interleaved rounds."""
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    meds = {k: [] for k in cands}
    for _ in range(repeats):
        for k, fn in cands.items():
            meds[k].append(median_us(fn, calls))
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "medians_us": v} for k, v in meds.items()}


def problem(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return np.ascontiguousarray(X), np.ascontiguousarray((y - y.mean()) / y.std())


def candidates(new, parent, run_ucb, run_acq, incumbent):
    c = {}
    if parent is not None:
        c["parent.best_ucb"] = lambda: run_ucb(parent)
    c["best_ucb"] = lambda: run_ucb(new)
    for name, kind in KINDS:
        rec = L.GpsoAcq(kind, 0, VARSIGMA, incumbent, 0.0)
        c[f"best_acq.{name}"] = (lambda rec=rec: run_acq(new, rec))
    return c


def verdict(res):
    """best_ucb against the parent: slower by no more than the parent's own spread."""
    if "parent.best_ucb" not in res:
        return None
    p, n = res["parent.best_ucb"], res["best_ucb"]
    spread = p["max_us"] - p["min_us"]
    return {"parent_median_us": p["median_us"], "median_us": n["median_us"], "parent_spread_us": spread,
            "within_parent_spread": bool(n["median_us"] - p["median_us"] <= spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libgpso_hip.so of the parent commit (same session, same box)")
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acq_bench.json"))
    args = ap.parse_args()
    assert args.calls >= 20
    new_lib = open_lib(L.LIB_PATH)
    parent_lib = open_lib(args.parent_lib) if args.parent_lib else None
    doc = {"tool": "tools/acq_bench.py", "library": new_lib.gpso_version().decode(), "calls": args.calls, "warmup": args.warmup,
           "repeats": args.repeats, "parent_lib": bool(parent_lib), "unit": "wall microseconds per synchronous call",
           "workloads": {}}
    for dname, dtype in (("mixed", L.MIXED), ("float64", L.F64)):
        X, y = problem(2048, 12, 0)
        leaves = np.ascontiguousarray(np.random.default_rng(1).random((65536, 12)))
        new = Ctx(new_lib, dtype, X, y, 0.25 * np.sqrt(12))
        parent = Ctx(parent_lib, dtype, X, y, 0.25 * np.sqrt(12)) if parent_lib else None
        res = measure(candidates(new, parent, lambda c: c.best_ucb(leaves), lambda c, r: c.best_acq(leaves, r), float(y.max())),
                      args.calls, args.warmup, args.repeats)
        res["best_ucb_vs_parent"] = verdict(res)
        res["logei_over_ucb"] = res["best_acq.logei"]["median_us"] / res["best_ucb"]["median_us"] - 1.0
        doc["workloads"][f"leaves_n2048_d12_m65536_{dname}"] = res
        print(dname, "leaves", json.dumps({k: (round(v["median_us"], 1) if isinstance(v, dict) and "median_us" in v else v)
                                           for k, v in res.items()}), flush=True)
        new.close()
        if parent:
            parent.close()
        X, y = problem(52, 2, 2)
        boxes = np.array([[[0.0, 1 / 3], [0.0, 1.0]], [[1 / 3, 2 / 3], [1 / 3, 2 / 3]], [[2 / 3, 1.0], [0.0, 1 / 3]]])
        new = Ctx(new_lib, dtype, X, y, 0.25 * np.sqrt(2))
        parent = Ctx(parent_lib, dtype, X, y, 0.25 * np.sqrt(2)) if parent_lib else None
        res = measure(candidates(new, parent, lambda c: c.best_ucb_grow(boxes, 6), lambda c, r: c.best_acq_grow(boxes, 6, r),
                                 float(y.max())), max(args.calls, 100), args.warmup, args.repeats)
        res["best_ucb_vs_parent"] = verdict(res)
        res["logei_over_ucb"] = res["best_acq.logei"]["median_us"] / res["best_ucb"]["median_us"] - 1.0
        doc["workloads"][f"grow_n52_d2_3boxes_depth6_{dname}"] = res
        print(dname, "grow", json.dumps({k: (round(v["median_us"], 1) if isinstance(v, dict) and "median_us" in v else v)
                                         for k, v in res.items()}), flush=True)
        new.close()
        if parent:
            parent.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
