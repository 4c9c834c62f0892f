#!/usr/bin/env python3
"""The screened best-UCB call (GPSO_OPT_SCREEN) on bench.py's problems, on an MI355X:  python tools/screen_bench.py

Per landscape (C3 seeds 0-4, noise 1e-2 / 1e-6, the C4 share): survivors and verdict of the screened call, its record against
the option-0 record byte for byte, wall ms per synchronous call and gpso_last_ms(ctx, 0) with the option off and on.  FLAT: the
landscape that prunes nothing (constant targets at C3's shape, refitted before every call so that every call is screened and
refused): the worst case, one refused call against one unscreened call.  profiles/screen_ab_pairs.txt holds a run."""
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import gpr  # noqa: E402
from pygpso_amd import HipGPEngine  # noqa: E402
from tests.helpers import synthetic_leaves, synthetic_problem  # noqa: E402

VS = gpr.VARSIGMA_DEFAULT


def run(name, d, n, m, seed, flat=False, noise=1e-3, reps=20):
    X, y = synthetic_problem(n, d, seed=seed)
    if flat:
        y = np.full_like(y, 0.3)
    Xs = torch.from_numpy(synthetic_leaves(m, d, seed=seed + 1).astype(np.float32)).cuda()
    eng = HipGPEngine("float32")
    eng.set_data(X, y)
    c = 0.3 if flat else float(y.mean())
    fit = lambda: eng.fit_eval("Matern52", 0.25 * math.sqrt(d) * np.ones(1), 1.0, noise, c, want_grad=False)  # noqa: E731
    fit()
    eng.set_screen(0)
    off = eng.best_ucb(Xs, VS)
    t_off, k_off = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.best_ucb(Xs, VS)
        t_off.append((time.perf_counter() - t0) * 1e3)
        k_off.append(eng.last_ms(0))
    eng.set_screen(1)
    t_on, k_on, verdicts = [], [], []
    for _ in range(reps):
        if flat:
            fit()  # (a new posterior: screened -- and refused -- again)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        on = eng.best_ucb(Xs, VS)
        t_on.append((time.perf_counter() - t0) * 1e3)
        k_on.append(eng.last_ms(0))
        verdicts.append(eng.last_count(8))
    same = all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(on, off))
    print(f"{name} seed {seed}{' FLAT' if flat else ''}: survivors {eng.last_count(7)} of {m}, verdict {sorted(set(verdicts))}, "
          f"same bytes as option 0: {same}; wall ms/call median: option 0 {np.median(t_off):.4f} | option 1 {np.median(t_on):.4f}; "
          f"last_ms(0) median: option 0 {np.median(k_off):.4f} | option 1 {np.median(k_on):.4f}; "
          f"math {eng.precision_info()['predict_math']}", flush=True)


for seed in range(5):
    run("C3", 12, 2048, 65536, seed)
run("C3", 12, 2048, 65536, 0, flat=True)
run("C3 noise 1e-2", 12, 2048, 65536, 0, noise=1e-2)
run("C3 noise 1e-6", 12, 2048, 65536, 0, noise=1e-6)
run("C4 share", 20, 8192, 32768, 0, reps=5)
