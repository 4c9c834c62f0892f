#!/usr/bin/env python3
"""
What max-value entropy search costs on the device, and that the calls beside it cost what they did.

One process, one GPU; the method of tools/acq_bench.py (its workloads, its contexts, its interleaved candidates: the median of
CALLS synchronous calls after WARMUP, repeated REPEATS times, min and max of the repeated medians kept beside their median).

  gpso_best_acq with GPSO_ACQ_MES at K = 1, 16 and 64 maxima, beside GPSO_ACQ_LOGEI and gpso_best_ucb, on
      workload "leaves":  N = 2048, D = 12, 65 536 leaves in one segment      (GPSO_MIXED and GPSO_F64)
      workload "grow":    N = 52,   D = 2,  best_*_grow of 3 boxes at depth 6 (the optimiser's regime)
  gpso_max_logcdf at m = 65 536, g = 64, columns in device memory and in host memory.
  With --parent-lib: gpso_best_ucb and gpso_best_acq(LOGEI) of this build against an EARLIER build of the library loaded
  into the same process (its own contexts, interleaved).  The bar is acq_bench's: this build's median may not exceed the
  parent's by more than the parent's own max - min.  The MES and max-logcdf figures have no target: they are recorded.

Writes one JSON document (default profiles/mes_bench.json).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import acq_bench as AB  # noqa: E402
from acq_bench import L, ROOT  # noqa: E402

KS = (1, 16, 64)


def candidates(new, parent, run_ucb, run_acq, y):
    inc = float(y.max())
    logei = L.GpsoAcq(L.ACQ_LOGEI, 0, AB.VARSIGMA, inc, 0.0)
    mes = L.GpsoAcq(L.ACQ_MES, 1, 0.0, 0.0, 0.0)
    c = {}
    if parent is not None:
        c["parent.best_ucb"] = lambda: run_ucb(parent)
        c["parent.best_acq.logei"] = lambda: run_acq(parent, logei)
    c["best_ucb"] = lambda: run_ucb(new)
    c["best_acq.logei"] = lambda: run_acq(new, logei)

    def run_mes(k):
        # (the maxima are installed per call, as the Python layer does for a spec that carries them: K doubles to the device)
        ys = np.ascontiguousarray(inc + np.linspace(0.0, 1.5, k))
        new.ok(new.lib.gpso_acq_set_maxima(new.h, L.dptr(ys), k))
        run_acq(new, mes)

    ys16 = np.ascontiguousarray(inc + np.linspace(0.0, 1.5, 16))

    def run_mes_resident():  # (a set that is there already: what a loop over one set of samples pays per call)
        if resident_k(new) != 16:
            new.ok(new.lib.gpso_acq_set_maxima(new.h, L.dptr(ys16), 16))
        run_acq(new, mes)

    for k in KS:
        c[f"best_acq.mes_k{k}"] = (lambda k=k: run_mes(k))
    c["best_acq.mes_k16_resident"] = run_mes_resident
    return c


def resident_k(ctx):
    k = C.c_int(0)
    ctx.ok(ctx.lib.gpso_acq_get_maxima(ctx.h, None, C.byref(k)))
    return k.value


def verdicts(res):
    out = {}
    for name in ("best_ucb", "best_acq.logei"):
        if "parent." + name not in res:
            return None
        p, n = res["parent." + name], res[name]
        spread = p["max_us"] - p["min_us"]
        out[name] = {"parent_median_us": p["median_us"], "median_us": n["median_us"], "parent_spread_us": spread,
                     "within_parent_spread": bool(n["median_us"] - p["median_us"] <= spread)}
    return out


def summarise(res):
    res["vs_parent"] = verdicts(res)
    for k in KS:
        res[f"mes_k{k}_over_logei"] = res[f"best_acq.mes_k{k}"]["median_us"] / res["best_acq.logei"]["median_us"] - 1.0
    return res


def short(res):
    return json.dumps({k: (round(v["median_us"], 1) if isinstance(v, dict) and "median_us" in v else v) for k, v in res.items()})


def max_logcdf(lib, ctx, calls, warmup, repeats):
    m, g = 65536, 64
    rng = np.random.default_rng(3)
    mean, var = np.ascontiguousarray(rng.normal(0.0, 1.0, m)), np.ascontiguousarray(rng.uniform(0.01, 2.0, m))
    y = np.ascontiguousarray(np.linspace(mean.max(), (mean + 6.0 * np.sqrt(var)).max(), g))
    out = np.empty(g)
    used = C.c_int64(0)
    hip = C.CDLL("libamdhip64.so")  # (the columns in device memory: two plain allocations of the runtime the library uses)
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    dm, dv = C.c_void_p(), C.c_void_p()
    for dev, host in ((dm, mean), (dv, var)):
        if hip.hipMalloc(C.byref(dev), host.nbytes) != 0 or hip.hipMemcpy(dev, C.c_void_p(host.ctypes.data), host.nbytes, 1) != 0:
            raise RuntimeError("hipMalloc / hipMemcpy of a column failed")

    def run(pm, pv, mem):
        ctx.ok(lib.gpso_max_logcdf(ctx.h, C.c_void_p(pm), C.c_void_p(pv), mem, m, 1.0e-3, L.dptr(y), g, L.dptr(out), C.byref(used)))

    res = AB.measure({"device_columns": lambda: run(dm.value, dv.value, L.MEM_DEVICE),
                      "host_columns": lambda: run(mean.ctypes.data, var.ctypes.data, L.MEM_HOST)}, calls, warmup, repeats)
    host_out = out.copy()
    run(dm.value, dv.value, L.MEM_DEVICE)
    assert np.array_equal(out, host_out), "the two memories give the same bits"
    hip.hipFree(dm)
    hip.hipFree(dv)
    res["m"], res["g"], res["rows_used"] = m, g, int(used.value)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libgpso_hip.so of the parent commit (same session, same box)")
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mes_bench.json"))
    args = ap.parse_args()
    assert args.calls >= 20
    new_lib = AB.open_lib(L.LIB_PATH)
    parent_lib = AB.open_lib(args.parent_lib) if args.parent_lib else None
    doc = {"tool": "tools/mes_bench.py", "library": new_lib.gpso_version().decode(), "calls": args.calls, "warmup": args.warmup,
           "repeats": args.repeats, "parent_lib": bool(parent_lib), "unit": "wall microseconds per synchronous call",
           "workloads": {}}
    for dname, dtype in (("mixed", L.MIXED), ("float64", L.F64)):
        X, y = AB.problem(2048, 12, 0)
        leaves = np.ascontiguousarray(np.random.default_rng(1).random((65536, 12)))
        new = AB.Ctx(new_lib, dtype, X, y, 0.25 * np.sqrt(12))
        parent = AB.Ctx(parent_lib, dtype, X, y, 0.25 * np.sqrt(12)) if parent_lib else None
        res = summarise(AB.measure(candidates(new, parent, lambda c: c.best_ucb(leaves), lambda c, r: c.best_acq(leaves, r), y),
                                   args.calls, args.warmup, args.repeats))
        doc["workloads"][f"leaves_n2048_d12_m65536_{dname}"] = res
        print(dname, "leaves", short(res), flush=True)
        if dname == "float64":
            doc["max_logcdf_m65536_g64"] = max_logcdf(new_lib, new, args.calls, args.warmup, args.repeats)
            print("max_logcdf", short(doc["max_logcdf_m65536_g64"]), flush=True)
        new.close()
        if parent:
            parent.close()
        X, y = AB.problem(52, 2, 2)
        boxes = np.array([[[0.0, 1 / 3], [0.0, 1.0]], [[1 / 3, 2 / 3], [1 / 3, 2 / 3]], [[2 / 3, 1.0], [0.0, 1 / 3]]])
        new = AB.Ctx(new_lib, dtype, X, y, 0.25 * np.sqrt(2))
        parent = AB.Ctx(parent_lib, dtype, X, y, 0.25 * np.sqrt(2)) if parent_lib else None
        res = summarise(AB.measure(candidates(new, parent, lambda c: c.best_ucb_grow(boxes, 6), lambda c, r: c.best_acq_grow(boxes, 6, r), y),
                                   max(args.calls, 100), args.warmup, args.repeats))
        doc["workloads"][f"grow_n52_d2_3boxes_depth6_{dname}"] = res
        print(dname, "grow", short(res), flush=True)
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
