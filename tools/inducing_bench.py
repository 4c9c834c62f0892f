#!/usr/bin/env python3
"""
Cost and effect of training the inducing points on one MI355X, in ONE process on one GPU:

  --eval     one loss + gradient evaluation WITH grad_z (``gpso_sgpr_bound_uz`` / ``gpso_svgp_elbo_uz``, Z passed in) beside
             the fixed-Z evaluation (``gpso_sgpr_bound_u`` / ``gpso_svgp_elbo_u``: the parent commit's code path, launch for
             launch) at the nine (N, D, M) sizes of section 7b's table;
  --update   wall time of the second and third ``gp_update`` of an ``SGPRSurrogate`` at M = 1024 with ``train_inducing``
             True against False, the selection's share and ``num_loss_evals`` (``--maxfun`` caps L-BFGS-B's evaluations per
             update for both; 0: SciPy's default);
  --quality  RMS difference of the SGPR's predictive mean / variance from the exact GPR's at the same hyper-parameters
             (N = 2048, 8192 leaves, device predictions of both), Z the greedy picks against Z trained on the bound from
             them by L-BFGS-B at those hyper-parameters.

Every time is a host clock around calls that end in a device synchronise: median of ``--reps`` after one warm-up call of
the same shape, with min and max.

Usage: python tools/inducing_bench.py [--eval] [--update] [--quality] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.optimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pygpso_amd import HipGPEngine, SGPRSurrogate  # noqa: E402
from pygpso_amd import kernels as K  # noqa: E402
from pygpso_amd.vgp import GH_POINTS  # noqa: E402
from tests.helpers import synthetic_leaves, synthetic_problem  # noqa: E402

CONFIGS = [(2048, 12), (8192, 20), (16384, 40)]
MS = [256, 512, 1024]
KERNEL = "Matern52"


def _softplus_inv(x):
    return np.log(np.expm1(x))


def _u(d, p=1.0e-2 - 1.0e-6):
    return np.array([_softplus_inv(0.25 * np.sqrt(d)), _softplus_inv(1.0), _softplus_inv(p), 0.0])


def timed(call, reps):
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": reps}


def bench_eval(reps):
    rows = []
    for n, d in CONFIGS:
        X, y = synthetic_problem(n, d, seed=0)
        for m in MS:
            eng = HipGPEngine("float64", device=0)
            eng.set_data(X, y)
            u = _u(d)
            eng.sgpr_select_inducing(KERNEL, u, 1, m)
            Z = eng.sgpr_get_inducing()[0] + 0.01  # (moved off the data: the general case of a trained Z)
            row = {"n": n, "d": d, "m": m}
            row["sgpr_fixed"] = timed(lambda: eng.sgpr_bound_u(KERNEL, u, 1, True, 0.0), reps)
            row["sgpr_train_z"] = timed(lambda: eng.sgpr_bound_uz(KERNEL, u, 1, True, 0.0, Z=Z), reps)
            row["sgpr_ratio"] = row["sgpr_train_z"]["median_ms"] / row["sgpr_fixed"]["median_ms"]
            uv = _u(d, 0.3)
            eng.vgp_set_likelihood("StudentT", 4.0, GH_POINTS)
            eng.svgp_init_q(KERNEL, uv, 1, True, 0.0, 0.18)
            row["svgp_fixed"] = timed(lambda: eng.svgp_elbo_u(KERNEL, uv, 1, True, 0.0), reps)
            row["svgp_train_z"] = timed(lambda: eng.svgp_elbo_uz(KERNEL, uv, 1, True, 0.0, Z=Z), reps)
            row["svgp_ratio"] = row["svgp_train_z"]["median_ms"] / row["svgp_fixed"]["median_ms"]
            eng.close()
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def _capped(maxfun):
    """L-BFGS-B with a cap on its evaluations (the surrogates' default ``Scipy()`` has none: SciPy's 15 000)."""
    return K.Scipy(options={"maxfun": maxfun}) if maxfun > 0 else K.Scipy()


def bench_update(maxfun, sizes):
    rows = []
    for n, d in sizes:
        X, y = synthetic_problem(n + 128, d, seed=0)
        for train in (False, True):
            s = SGPRSurrogate(gp_kernel=K.Matern52(lengthscales=0.25 * np.sqrt(d)), gp_meanf=K.Constant(0.0),
                              gauss_likelihood_sigma=1e-2, num_inducing=1024, optimiser=_capped(maxfun), train_inducing=train)
            s.append(X[:n - 128], y[:n - 128])
            row = {"n": n, "d": d, "m": 1024, "train_inducing": train, "maxfun": maxfun, "updates": []}
            for k in range(3):
                if k:
                    s.append(X[n - 128 + 64 * (k - 1): n - 128 + 64 * k], y[n - 128 + 64 * (k - 1): n - 128 + 64 * k])
                sel = []
                eng = s.gpflow_model.engine if s.gpflow_model is not None else None
                if eng is not None:
                    inner = type(eng).sgpr_select_inducing

                    def counted(*a, _inner=inner, _eng=eng, **kw):
                        t0 = time.perf_counter()
                        r = _inner(_eng, *a, **kw)
                        sel.append((time.perf_counter() - t0) * 1e3)
                        return r

                    eng.sgpr_select_inducing = counted
                evals0 = s.gpflow_model.num_loss_evals if s.gpflow_model is not None else 0
                t0 = time.perf_counter()
                s.gp_update()
                ms = (time.perf_counter() - t0) * 1e3
                row["updates"].append({"update": k + 1, "n": s.num_evaluated, "ms": ms, "selection_ms": sum(sel),
                                       "selections": len(sel), "num_loss_evals": s.gpflow_model.num_loss_evals - evals0,
                                       "loss": s.gpflow_model._last_nlml})
            s.gpflow_model.engine.close()
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bench_quality(maxfun):
    n, d = 2048, 12
    X, y = synthetic_problem(n, d, seed=0)
    leaves = synthetic_leaves(8192, d, seed=1)
    u = _u(d)
    gpr = HipGPEngine("float64", device=0)
    gpr.set_data(X, y)
    gpr.fit_eval_u(KERNEL, u, 1, True, 0.0)
    mean_g, var_g = gpr.predict(leaves)
    gpr.close()
    sd = float(np.std(y))
    rows = []
    for m in MS:
        eng = HipGPEngine("float64", device=0)
        eng.set_data(X, y)
        eng.sgpr_select_inducing(KERNEL, u, 1, m)
        Z0 = eng.sgpr_get_inducing()[0]

        def rms():
            eng.sgpr_posterior(KERNEL, u, 1, True, 0.0)
            mean_s, var_s = eng.predict(leaves)
            return float(np.sqrt(np.mean((mean_s - mean_g) ** 2))), float(np.sqrt(np.mean((var_s - var_g) ** 2)))

        f0 = eng.sgpr_bound_u(KERNEL, u, 1, True, 0.0, want_grad=False)[0]
        rm0, rv0 = rms()
        evals = [0]

        def fun(z):
            f, _, gz, _ = eng.sgpr_bound_uz(KERNEL, u, 1, True, 0.0, Z=z.reshape(Z0.shape))
            evals[0] += 1
            return f, gz.ravel()

        t0 = time.perf_counter()
        res = scipy.optimize.minimize(fun, Z0.ravel(), jac=True, method="L-BFGS-B", options={"maxfun": maxfun} if maxfun > 0 else {})
        ms = (time.perf_counter() - t0) * 1e3
        f1 = eng.sgpr_bound_uz(KERNEL, u, 1, True, 0.0, Z=res.x.reshape(Z0.shape), want_grad=False)[0]
        rm1, rv1 = rms()
        eng.close()
        row = {"n": n, "d": d, "m": m, "y_std": sd, "loss_greedy": f0, "loss_trained": f1, "evals": evals[0], "train_ms": ms,
               "rms_mean_greedy": rm0, "rms_mean_trained": rm1, "rms_var_greedy": rv0, "rms_var_trained": rv1,
               "rms_mean_greedy_over_std": rm0 / sd, "rms_mean_trained_over_std": rm1 / sd}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--update-sizes", default="8192:20,16384:40")
    ap.add_argument("--maxfun", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "tools/inducing_bench.py", "kernel": KERNEL}
    if a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            res.update(json.load(fh))
    if a.eval:
        res["evaluation_cost"] = bench_eval(a.reps)
    if a.update:
        res["update_cost"] = bench_update(a.maxfun, [tuple(int(v) for v in c.split(":")) for c in a.update_sizes.split(",")])
    if a.quality:
        res["model_quality"] = bench_quality(a.maxfun)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
