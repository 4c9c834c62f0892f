#!/usr/bin/env python3
"""
What the success member costs on the device, beside the way a user had without it; and what a training iteration of the
Bernoulli VGP costs beside the Student-t's.

Steps, each run in a fresh child process under a time limit of its own (--step-limit seconds); after a step that fails or
runs out of time NOTHING further is started and the document records where it stopped:

  fold   for (N, D, M) = (52, 2, 162) -- the optimiser's regime -- and (128, 12, 65 536) -- the member's limit in N and a full
         batch of leaves --, with J = 0 and J = 4 constraint models, two candidates timed in turn (interleaved):
           member      ONE context holding the objective's posterior, J constraint members and the success member; one
                       gpso_constrained_best_acq call (three stage-1 launches, the fold, the arg-max, the gather, one record)
           separate    the classifier's, the objective's and the J constraint models' contexts called separately (gpso_predict on
                       the classifier's, gpso_acq_values on the others: columns of M doubles over PCIe), the probit map and the
                       constraints' log Phi (scipy's log_ndtr), the gate and the arg-max in numpy
         Both rank by the reference's mean + varsigma * var in gate mode at P >= 0.5 ** (J + 1); the winners are compared, and so
         are the leaves of largest logpof in feasibility mode (which no gate can make agree trivially).
  train  for N = 50 and 128 (D = 2): 10 training iterations -- a natural-gradient step on q (gamma 0.5), then one Adam step
         on -ELBO's gradient -- of HipVGP under the Bernoulli likelihood and under the Student-t (df 4), interleaved in one run.

Each figure is the median host wall time of CALLS synchronous calls after WARMUP, repeated REPEATS times; the min and max of
the repeated medians are kept beside their median (DESIGN.md section 7q's protocol).  Nothing here has a target: the figures are
recorded.  Without a GPU the script fails (no fallback).  Writes one JSON document (default profiles/failures_bench.json).
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

VARSIGMA = 1.82138636771845
SHAPES = ((52, 2, 162), (128, 12, 65536))
JS = (0, 4)
TRAIN_NS = (50, 128)


def pof_min_of(j):
    """The gate: P >= 0.5 ** (J + 1), one coin per factor of the product -- at 0.5 four constraints at their medians and the
    member gate every leaf, and two all-gated candidates would agree on their winner trivially."""
    return 0.5 ** (j + 1)


GH_POINTS = 20


def labels_of(X, seed=5):
    """Labels in {0, 1}: the sign of a smooth function of X about its median."""
    rng = np.random.default_rng([seed, X.shape[1]])
    g = np.sin(2.0 * X @ rng.normal(size=X.shape[1]) / np.sqrt(X.shape[1])) + 0.5 * X[:, 0]
    return (g > np.median(g)).astype(np.float64)


def fold_step(n, d, m, j, calls, warmup, repeats):
    from scipy.special import log_ndtr

    from constraints_bench import constraint_targets
    from ensemble_bench import problem, thetas, timed
    from pygpso_amd import HipGPEngine, acquisition
    from pygpso_amd.model import _softplus_inv

    X, y, leaves = problem(n, d, m)
    th = thetas(j + 1, d, y)
    acq = acquisition.UCBVar(VARSIGMA)
    cY = constraint_targets(X, j) if j else np.zeros((0, n))
    thr = np.median(cY, axis=1) if j else np.zeros(0)
    sense = np.array([1 if i % 2 == 0 else -1 for i in range(j)])
    many = []
    for i, (ls, var, noise, c) in enumerate(th):
        e = HipGPEngine("float64")
        e.set_data(X, y if i == 0 else cY[i - 1])
        e.fit_eval("Matern52", [ls], var, noise, c if i == 0 else float(cY[i - 1].mean()), want_grad=False)
        many.append(e)
    one = many[0]
    for i in range(j):
        one.constraint_push(many[i + 1], thr[i], int(sense[i]))
    cls = HipGPEngine("float64")  # the classifier: four natural-gradient steps at a fixed theta, then the install
    cls.set_data(X, labels_of(X))
    cls.vgp_set_likelihood("Bernoulli", 0.0, GH_POINTS)
    cls.vgp_set_q()
    u = np.array([float(_softplus_inv(0.3 * np.sqrt(d))), float(_softplus_inv(1.0)), 0.0, 0.0])
    for _ in range(4):
        cls.vgp_natgrad("Matern52", u, 1, True, 0.0, 0.5)
    cls.vgp_posterior("Matern52", u, 1, True, 0.0)
    one.success_push(cls)
    noise = np.array([t[2] for t in th[1:]])
    LOG_POF_MIN = float(np.log(pof_min_of(j)))

    def member():
        return one.constrained_best_acq(leaves, acq, "gate", LOG_POF_MIN)

    def separate_logpof():
        sm, sv = cls.predict(leaves)
        logpof = None
        for i in range(j):
            cm, cv, _ = many[i + 1].acq_values(leaves, acq)
            lp = log_ndtr(sense[i] * (thr[i] - cm) / np.sqrt(np.maximum(cv - noise[i], 0.0)))
            logpof = lp if logpof is None else logpof + lp
        ls_ = log_ndtr(sm / np.sqrt(1.0 + np.maximum(sv, 0.0)))
        return ls_ if logpof is None else logpof + ls_

    def separate():
        value = many[0].acq_values(leaves, acq)[2]
        logpof = separate_logpof()
        value = np.where(logpof >= LOG_POF_MIN, value, -np.inf)
        k = int(np.argmax(value))
        return k, value[k]

    idx, _, _, value, logpof = member()
    k, v = separate()
    same = bool(int(idx[0]) == k and (value[0] == v or abs(value[0] - v) <= 1e-9 * max(1.0, abs(v))))
    res = timed({"member": member, "separate": separate}, calls, warmup, repeats)
    res["same_winner"] = same
    # ... and in feasibility mode, where no gate can make the comparison trivial: the leaf with the largest logpof
    fi, _, _, fv, _ = one.constrained_best_acq(leaves, acq, "feasibility", LOG_POF_MIN)
    lp_np = separate_logpof()
    res["same_most_feasible_leaf"] = bool(int(fi[0]) == int(np.argmax(lp_np)) and abs(fv[0] - lp_np.max()) <= 1e-9 * max(1.0, abs(lp_np.max())))
    res["gated_fraction"] = float(np.mean(np.isneginf(one.constrained_acq_values(leaves, acq, "gate", LOG_POF_MIN)[2])))
    one.set_timing(True)
    member()
    res["device_ms_member"] = one.last_ms(1)
    for e in many + [cls]:
        e.close()
    res.update(n=n, d=d, m=m, j=j, pof_min=pof_min_of(j))
    return res


def train_step(n, calls, warmup, repeats, iterations=10):
    from ensemble_bench import problem, timed
    from pygpso_amd import kernels as K
    from pygpso_amd.vgp import HipVGP

    X, y, _ = problem(n, 2, 8)
    models = {
        "bernoulli": HipVGP(data=(X, labels_of(X)[:, None]), kernel=K.Matern52(lengthscales=0.4, variance=1.0), mean_function=K.Constant(0.0),
                            likelihood=K.Bernoulli()),
        "student_t": HipVGP(data=(X, y[:, None]), kernel=K.Matern52(lengthscales=0.4, variance=1.0), mean_function=K.Constant(0.0),
                            likelihood=K.StudentT(scale=0.5, df=4.0)),
    }
    adams = {name: K.Adam(0.01) for name in models}

    def trainer(name):
        model, adam = models[name], adams[name]

        def run():
            for _ in range(iterations):
                model.natgrad(0.5)
                adam.minimize(model.training_loss, model.trainable_variables)
        return run

    res = timed({name: trainer(name) for name in models}, calls, warmup, repeats)
    res.update(n=n, d=2, iterations=iterations, natgrad_gamma=0.5)
    for model in models.values():
        model.engine.close()
    return res


def steps():
    for n, d, m in SHAPES:
        for j in JS:
            yield ["--step", "fold", "--n", str(n), "--d", str(d), "--m", str(m), "--j", str(j)]
    for n in TRAIN_NS:
        yield ["--step", "train", "--n", str(n)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "failures_bench.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=float, default=150.0, help="seconds a step may take before it is ended")
    ap.add_argument("--step", choices=("fold", "train"), help="(internal) run one step in this process and print its JSON line")
    for name in ("n", "d", "m", "j"):
        ap.add_argument("--" + name, type=int, default=0)
    args = ap.parse_args()
    if args.step == "fold":
        print("RESULT " + json.dumps(fold_step(args.n, args.d, args.m, args.j, args.calls, args.warmup, args.repeats)), flush=True)
        return 0
    if args.step == "train":
        print("RESULT " + json.dumps(train_step(args.n, args.calls, args.warmup, args.repeats)), flush=True)
        return 0
    doc = {"tool": "tools/failures_bench.py", "calls": args.calls, "warmup": args.warmup, "repeats": args.repeats,
           "clock": "host wall time around synchronous calls", "acquisition": "ucb_var", "mode": "gate", "pof_min": "0.5 ** (J + 1)",
           "leaves": "host float64", "step_limit_s": args.step_limit, "fold": [], "train": [], "stopped_at": None}
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
        doc[step[1]].append(r)
        if step[1] == "fold":
            print(f"N={r['n']} D={r['d']} M={r['m']} J={r['j']}: member {r['member']['median_us']:.0f} us, separate "
                  f"{r['separate']['median_us']:.0f} us, same winner {r['same_winner']} (most feasible leaf: {r['same_most_feasible_leaf']}), gated {r['gated_fraction']:.2f}", flush=True)
        else:
            print(f"N={r['n']}: 10 iterations Bernoulli {r['bernoulli']['median_us']:.0f} us, Student-t {r['student_t']['median_us']:.0f} us",
                  flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 1 if doc["stopped_at"] is not None else 0


if __name__ == "__main__":
    sys.exit(main())
