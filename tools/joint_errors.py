#!/usr/bin/env python3
"""
Measured errors of gpso_predict_joint and gpso_sample_joint against the float64 oracle of tests/joint_oracle.py, on the cases
of tests/test_gpu_joint.py (its shapes, four kernels, noises, float64 and mixed engines, M = 1 .. 130): per kernel class (the
three smooth ones | Matern-1/2) and engine type the maxima of the mean and covariance errors and of L L^T from the identity
draws, in the test's own measures, with the case that set each; and the largest error of the draws for seeded normals beside
the test's bound.

Also the wall time of one predict_joint at (N, M) = (2048, 1024), D = 12, beside the only route there was before the call
existed: read L^-1 back with gpso_get_matrix and form the covariance in numpy on the host.

Writes profiles/joint_parity.json.     python tools/joint_errors.py [--out-dir profiles] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _worst(bucket, key, value, case):
    if value > bucket.get(key, {"max": -1.0})["max"]:
        bucket[key] = {"max": float(value), "case": case}


def _parity():
    from tests import joint_oracle as jo
    from tests import test_gpu_joint as T
    from tests import test_gpu_predict_grad as PG

    worst = {f"{cls} {dtype}": {} for cls in ("smooth", "Matern12") for dtype in T.DTYPES}
    draws = {dtype: {} for dtype in T.DTYPES}
    for n, d in T.SHAPES:
        for kernel in T.KERNELS:
            for noise in T.NOISES:
                r = T.reference(n, d, kernel, noise)
                for dtype in T.DTYPES:
                    eng = PG.fitted(r, dtype)
                    bucket = worst[f"{'Matern12' if kernel == 'Matern12' else 'smooth'} {dtype}"]
                    for m in T.MS:
                        case = f"N={n} D={d} {kernel} noise={noise:g} s={'yes' if r['s'] is not None else 'no'} M={m}"
                        Xs = r["Xs"][:m]
                        mean, cov = eng.predict_joint(Xs)
                        for k, v in T.joint_errors((mean, cov), r["mean"][:m], r["cov"][:m, :m], r).items():
                            _worst(bucket, k, v, case)
                        f, _, _ = eng.sample_joint(Xs, np.eye(m), T.JITTER)
                        Lf = (f - mean[None, :]).T
                        e = np.max(np.abs(Lf @ Lf.T - T.with_diag(r["cov"][:m, :m], T.JITTER))) / r["th"].variance
                        _worst(bucket, "factor", e, case)
                        if kernel == "Matern52" and noise == 1.0e-1:  # (the draws' cases of the test, its seeds and bound)
                            z = np.random.default_rng(100 + m).standard_normal((7, m))
                            want = jo.draws(r["mean"][:m], T.with_diag(r["cov"][:m, :m], noise), z)
                            bound = T.tolerance(kernel) * np.max(np.abs(r["y"])) + jo.chol_perturbation_bound(
                                T.with_diag(r["cov"][:m, :m], noise), T.tolerance(kernel) * r["th"].variance) * np.linalg.norm(z, axis=1)
                            err = np.max(np.abs(eng.sample_joint(Xs, z, noise)[0] - want), axis=1)
                            _worst(draws[dtype], "error", float(np.max(err)), case)
                            _worst(draws[dtype], "error_over_bound", float(np.max(err / bound)), case)
                    eng.close()
    return worst, draws


def _median_ms(call, reps):
    call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def _timing(reps):
    from oracle import gpr
    from pygpso_amd import HipGPEngine, _lib
    from tests import joint_oracle as jo
    from tests.helpers import synthetic_problem

    n, d, m = 2048, 12, 1024
    X, y = synthetic_problem(n, d, seed=1)
    th = gpr.Theta("Matern52", [0.25 * np.sqrt(d)], 1.0, 1.0e-2, float(y.mean()))
    Xs = np.random.default_rng(2).uniform(-0.2, 1.2, size=(m, d))
    eng = HipGPEngine("float64")
    eng.set_data(X, y)
    eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=False)

    def host_route():
        C_, alpha = eng.get_matrix(_lib.MAT_LINV), eng.get_vector(_lib.VEC_ALPHA)
        return jo.predictive_joint(np.tril(C_), alpha, X, th, Xs, 0.0)

    dev = eng.predict_joint(Xs)
    host = host_route()
    out = {"n": n, "d": d, "m": m, "reps": reps,
           "predict_joint_wall_ms": _median_ms(lambda: eng.predict_joint(Xs), reps),
           "get_matrix_and_numpy_wall_ms": _median_ms(host_route, reps),
           "max_abs_cov_difference": float(np.max(np.abs(dev[1] - host[1])))}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    from tests import test_gpu_joint as T

    worst, draws = _parity()
    timing = _timing(a.reps)
    with open(os.path.join(a.out_dir, "joint_parity.json"), "w") as fh:
        json.dump({"note": "gpso_predict_joint / gpso_sample_joint against tests/joint_oracle.py over the cases of "
                           "tests/test_gpu_joint.py; mean by max|y|, cov and factor (L L^T from identity draws, latent f + "
                           "jitter 1e-6) by the kernel variance",
                   "tolerances": {"smooth": T.tolerance("Matern52"), "Matern12": T.tolerance("Matern12")},
                   "measured": worst,
                   "draws": {"note": "seeded normals, S = 7, Matern52, noise 1e-1 on the diagonal: largest |draw - oracle's| and "
                                     "its largest ratio to the test's first-order bound", "measured": draws},
                   "wall_time": timing}, fh, indent=1)
        fh.write("\n")
    for cls, b in worst.items():
        print(cls, ", ".join(f"{k} {v['max']:.2e}" for k, v in b.items()), flush=True)
    for dtype, b in draws.items():
        print("draws", dtype, ", ".join(f"{k} {v['max']:.2e}" for k, v in b.items()), flush=True)
    print(json.dumps(timing), flush=True)


if __name__ == "__main__":
    main()
