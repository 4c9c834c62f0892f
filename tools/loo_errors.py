#!/usr/bin/env python3
"""
Measured errors of the leave-one-out entry points against the float64 oracle of tests/loo_oracle.py, on the cases of
tests/test_gpu_loo.py (its shapes, kernels, noises and per-point noise vectors; both paths where N <= 128):

  profiles/loo_parity.json ....... float64: per kernel class (the three smooth ones | Matern-1/2) the maxima of the loss, NLML,
                                   gradient, mean, var and lpd errors in the test's own measures, with the case that set each
  profiles/loo_float_errors.txt .. gpso_loo on float32 and mixed engines at FLOAT_SHAPES: max |d mean| / max|y|,
                                   max |d var| / var, max |d lpd| / max(1, |lpd|) per shape -- what FLOAT32_LOO_BOUNDS is 5 x of

python tools/loo_errors.py [--out-dir profiles]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from pygpso_amd import HipGPEngine
    from pygpso_amd import _lib as L
    from tests import test_gpu_loo as T

    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    worst = {"smooth": {}, "Matern12": {}}
    for n, d, ard, kernel in T.CASES:
        for noise in T.NOISES:
            r = T.reference(n, d, ard, kernel, noise)
            th = r["th"]
            for fused in ((1, 0) if n <= 128 else (1,)):
                eng = HipGPEngine("float64")
                eng._check(eng._lib.gpso_set_option(eng._h, L.OPT_FIT_FUSED_SMALL, fused))
                T._load(eng, r)
                f, g, nlml = eng.fit_eval_loo(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c)
                errs = T.objective_errors(r, f, g, nlml)
                errs.update(T.predictive_errors(r, *eng.loo()[:3]))
                eng.close()
                bucket = worst["Matern12" if kernel == "Matern12" else "smooth"]
                for k, v in errs.items():
                    if v > bucket.get(k, {"max": -1.0})["max"]:
                        bucket[k] = {"max": float(v), "case": f"N={n} D={d} {kernel} noise={noise:g} s={'yes' if r['s'] is not None else 'no'} "
                                                              f"path={'small' if (fused and n <= 128) else 'general'}"}
    with open(os.path.join(a.out_dir, "loo_parity.json"), "w") as fh:
        json.dump({"note": "float64 context against tests/loo_oracle.py over the cases of tests/test_gpu_loo.py; loss and nlml relative, "
                           "grad by max(1, |g|), mean by max|y|, var relative, lpd by max(1, |lpd|)",
                   "tolerances": {"smooth": T._tols("Matern52"), "Matern12": T._tols("Matern12")}, "measured": worst}, fh, indent=1)
    for cls, b in worst.items():
        print(cls, ", ".join(f"{k} {v['max']:.2e}" for k, v in b.items()), flush=True)
    lines = ["gpso_loo on float engines against the float64 oracle (tests/test_gpu_loo.py: FLOAT_SHAPES, Matern-5/2, noise 1e-3)",
             "dtype    N    D   max|d mean|/max|y|   max|d var|/var   max|d lpd|/max(1,|lpd|)"]
    top = [0.0, 0.0]
    for dtype in ("float32", "mixed"):
        for n, d, ard in T.FLOAT_SHAPES:
            r = T.reference(n, d, ard, "Matern52", 1.0e-3)
            th = r["th"]
            eng = HipGPEngine(dtype)
            T._load(eng, r)
            eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)
            e = T.predictive_errors(r, *eng.loo()[:3])
            eng.close()
            if dtype == "float32":
                top = [max(top[0], e["mean"]), max(top[1], e["var"])]
            lines.append(f"{dtype:8s} {n:4d} {d:3d}   {e['mean']:.3e}            {e['var']:.3e}        {e['lpd']:.3e}")
    lines.append(f"float32 maxima: mean {top[0]:.3e}, var {top[1]:.3e}   ->   FLOAT32_LOO_BOUNDS = 5 x = ({5 * top[0]:.1e}, {5 * top[1]:.1e})")
    with open(os.path.join(a.out_dir, "loo_float_errors.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
