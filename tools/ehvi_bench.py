#!/usr/bin/env python3
"""
What a bi-objective selection costs on the device, beside what a user could do without the EHVI calls.

For (N, D, M) = (52, 2, 162) -- the optimiser's regime -- and (128, 12, 65 536) -- the set's limit in N and a full batch of
leaves --, each with a front of P = 7 and of P = 63 points and with J = 1 (objective 2 alone) and J = 4 (three further
constraints) members, two candidates timed in turn (interleaved):
  best_ehvi   ONE gpso_best_ehvi call on the context that holds the objective and the set: the constrained calls' stage 1,
              the EHVI fold (a wave a leaf), the arg-max, three gathers, one record
  columns     gpso_constrained_acq_values for the columns (the objective's and the J members': (2 + 2 J) M doubles over PCIe),
              then the EHVI by the transposed decomposition, the other members' log Phi (scipy's ndtr / log_ndtr), the weight
              and the arg-max in numpy
Both rank by EHVI x P(feasible) ("weight" mode, no gate); the winners are compared (the same leaf, or values within 1e-9
relative: another libm and another order of the sum).  gpso_last_ms(ctx, 1) of one further gpso_best_ehvi call is recorded.

Each step runs in a fresh child process under a time limit of its own (--step-limit seconds); after a step that fails or runs
out of time NOTHING further is started and the document records where it stopped.  Each figure is the median host wall time of
CALLS synchronous calls after WARMUP, repeated REPEATS times; the min and max of the repeated medians are kept beside their
median (DESIGN.md section 7q's protocol).  Nothing here has a target: the figures are recorded.  Without a GPU the script fails
(no fallback).  Writes one JSON document (default profiles/ehvi_bench.json).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((52, 2, 162), (128, 12, 65536))
PS = (7, 63)
JS = (1, 4)
INV_SQRT_2PI = 0.3989422804014327


def front_of(p, lo, hi, seed=11):
    """A front of p points inside the box (lo, hi): f1 ascending, f2 descending, uneven gaps."""
    t = np.sort(np.random.default_rng([seed, p]).uniform(0.05, 0.95, p))
    return np.column_stack([lo[0] + (hi[0] - lo[0]) * t, lo[1] + (hi[1] - lo[1]) * (1.0 - t ** 1.7)])


def excess(mean, s, x):
    """E[(Y - x)+] for Y ~ N(mean, s^2): mean, s [M], x [K] -> [K, M]."""
    from scipy.special import ndtr

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = (mean[None] - x[:, None]) / s[None]
        g = s[None] * (INV_SQRT_2PI * np.exp(-0.5 * z * z) + z * ndtr(z))
    return np.where(s[None] > 0.0, g, np.maximum(mean[None] - x[:, None], 0.0))


def ehvi_numpy(front, ref, m1, s1, m2, s2):
    """The exact EHVI [M] by strips along objective 2 (tests/ehvi_oracle.py's decomposition), all strips at once."""
    a = np.concatenate([[ref[0]], front[:, 0]])
    b = np.concatenate([front[:, 1], [ref[1]]])
    g1 = excess(m1, s1, a)
    g2 = np.vstack([np.zeros((1, m1.shape[0])), excess(m2, s2, b)])
    return np.sum((g2[1:] - g2[:-1]) * g1, axis=0)


def fold_step(n, d, m, p, j, calls, warmup, repeats):
    from scipy.special import log_ndtr

    from constraints_bench import constraint_targets
    from ensemble_bench import problem, thetas, timed
    from pygpso_amd import HipGPEngine, acquisition

    X, y, leaves = problem(n, d, m)
    th = thetas(j + 1, d, y)
    cY = constraint_targets(X, j)
    thr = np.median(cY, axis=1)
    sense = np.array([-1] + [1 if i % 2 == 0 else -1 for i in range(1, j)])  # member 0 is objective 2: a lower= constraint
    one = HipGPEngine("float64")
    src = HipGPEngine("float64")
    for i in range(j):
        ls, var, noise, _ = th[i + 1]
        src.set_data(X, cY[i])
        src.fit_eval("Matern52", [ls], var, noise, float(cY[i].mean()), want_grad=False)
        one.constraint_push(src, thr[i], int(sense[i]))
    src.close()
    ls, var, noise0, c = th[0]
    one.set_data(X, y)
    one.fit_eval("Matern52", [ls], var, noise0, c, want_grad=False)
    noise = np.array([t[2] for t in th[1:]])
    ei = acquisition.EI(xi=0.0)
    # the reference point and the front from the columns themselves: the front runs through the leaves' means
    mean, varc, _, _, mm, mv = one.constrained_acq_values(leaves, ei, "gate", -np.inf, incumbent=0.0, want_members=True)
    lo = np.array([mean.min(), mm[0].min()])
    hi = np.array([mean.max(), mm[0].max()])
    ref = lo - 0.1 * (hi - lo)
    front = front_of(p, ref, hi)

    def best_ehvi():
        return one.best_ehvi(leaves, 0, front, ref, True, "weight", -np.inf)

    def columns():
        mean, varc, _, _, mm, mv = one.constrained_acq_values(leaves, ei, "gate", -np.inf, incumbent=0.0, want_members=True)
        s1 = np.sqrt(np.maximum(varc - noise0, 0.0))
        s2 = np.sqrt(np.maximum(mv[0] - noise[0], 0.0))
        value = ehvi_numpy(front, ref, mean, s1, mm[0], s2)
        for i in range(1, j):
            value = value * np.exp(log_ndtr(sense[i] * (thr[i] - mm[i]) / np.sqrt(np.maximum(mv[i] - noise[i], 0.0))))
        k = int(np.argmax(value))
        return k, value[k]

    idx, value, logpof, _, _ = best_ehvi()
    k, v = columns()
    same = bool(int(idx[0]) == k or abs(value[0] - v) <= 1e-9 * max(abs(v), 1e-300))
    res = timed({"best_ehvi": best_ehvi, "columns": columns}, calls, warmup, repeats)
    res["same_winner"] = same
    res["winner"] = {"best_ehvi": [int(idx[0]), float(value[0])], "columns": [k, float(v)]}
    one.set_timing(True)
    best_ehvi()
    res["device_ms_best_ehvi"] = one.last_ms(1)
    one.close()
    res.update(n=n, d=d, m=m, p=p, j=j)
    return res


def steps():
    for n, d, m in SHAPES:
        for p in PS:
            for j in JS:
                yield ["--step", "fold", "--n", str(n), "--d", str(d), "--m", str(m), "--p", str(p), "--j", str(j)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ehvi_bench.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=float, default=150.0, help="seconds a step may take before it is ended")
    ap.add_argument("--step", choices=("fold",), help="(internal) run one step in this process and print its JSON line")
    for name in ("n", "d", "m", "p", "j"):
        ap.add_argument("--" + name, type=int, default=0)
    args = ap.parse_args()
    if args.step == "fold":
        print("RESULT " + json.dumps(fold_step(args.n, args.d, args.m, args.p, args.j, args.calls, args.warmup, args.repeats)), flush=True)
        return 0
    doc = {"tool": "tools/ehvi_bench.py", "calls": args.calls, "warmup": args.warmup, "repeats": args.repeats,
           "clock": "host wall time around synchronous calls", "mode": "weight", "log_pof_min": "-inf", "latent": True,
           "leaves": "host float64", "wave_packing": "not built: W = 64, a wave a leaf", "step_limit_s": args.step_limit, "fold": [],
           "stopped_at": None}
    common = ["--calls", str(args.calls), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
    for step in steps():
        cmd = [sys.executable, os.path.abspath(__file__)] + step + common
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_limit)
            line = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")]
            if done.returncode != 0 or not line:
                doc["stopped_at"] = {"step": step, "returncode": done.returncode, "stderr_tail": done.stderr[-2000:]}
        except subprocess.TimeoutExpired:
            doc["stopped_at"] = {"step": step, "returncode": None, "stderr_tail": f"no result within {args.step_limit} s"}
        if doc["stopped_at"] is not None:  # (a step failed or hung: nothing further is started on the GPU)
            print(f"step {' '.join(step)} failed: stopping here", flush=True)
            break
        r = json.loads(line[0][len("RESULT "):])
        doc["fold"].append(r)
        print(f"N={r['n']} D={r['d']} M={r['m']} P={r['p']} J={r['j']}: best_ehvi {r['best_ehvi']['median_us']:.0f} us, columns + numpy "
              f"{r['columns']['median_us']:.0f} us, device {r['device_ms_best_ehvi'] * 1e3:.0f} us, same winner {r['same_winner']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 1 if doc["stopped_at"] is not None else 0


if __name__ == "__main__":
    sys.exit(main())
