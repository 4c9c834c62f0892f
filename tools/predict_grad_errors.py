#!/usr/bin/env python3
"""
Measured errors of gpso_predict_grad against the float64 oracle of tests/predict_grad_oracle.py, on the parity cases of
tests/test_gpu_predict_grad.py (its shapes, kernels, isotropic and ARD lengthscales, noises, per-point noise vectors, float64
and mixed engines, M = 1, 16, 17, 300): per kernel class (the three smooth ones | Matern-1/2) and engine type the maxima of
the mean, var, dmean and dvar errors in the test's own measures, with the case that set each.

Writes profiles/predict_grad_parity.json.     python tools/predict_grad_errors.py [--out-dir profiles]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import test_gpu_predict_grad as T

    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    worst = {f"{cls} {dtype}": {} for cls in ("smooth", "Matern12") for dtype in ("float64", "mixed")}
    for n, d in T.SHAPES:
        for kernel in T.KERNELS:
            for ard in (False, True):
                for noise in T.NOISES:
                    r = T.reference(n, d, ard, kernel, noise)
                    for dtype in ("float64", "mixed"):
                        eng = T.fitted(r, dtype)
                        for m in T.MS:
                            errs = T.errors(eng.predict_grad(r["Xs"][:m]), tuple(x[:m] for x in r["out"]), r["y"], r["th"].variance)
                            bucket = worst[f"{'Matern12' if kernel == 'Matern12' else 'smooth'} {dtype}"]
                            for k, v in errs.items():
                                if v > bucket.get(k, {"max": -1.0})["max"]:
                                    bucket[k] = {"max": float(v), "case": f"N={n} D={d} {kernel} ard={ard} noise={noise:g} "
                                                                          f"s={'yes' if r['s'] is not None else 'no'} M={m}"}
                        eng.close()
    with open(os.path.join(a.out_dir, "predict_grad_parity.json"), "w") as fh:
        json.dump({"note": "gpso_predict_grad against tests/predict_grad_oracle.py over the parity cases of tests/test_gpu_predict_grad.py; "
                           "mean by max|y|, var by the kernel variance, dmean and dvar by max(1, max|g|) per case",
                   "tolerances": {"smooth": T.tolerances("Matern52"), "Matern12": T.tolerances("Matern12")}, "measured": worst}, fh, indent=1)
    for cls, b in worst.items():
        print(cls, ", ".join(f"{k} {v['max']:.2e}" for k, v in b.items()), flush=True)


if __name__ == "__main__":
    main()
