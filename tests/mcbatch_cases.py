"""The configurations of ``gpso_paths_best_batch`` shared by tests/test_gpu_mcbatch.py (which runs them on the device) and
tests/test_mcbatch_cpu.py (which checks on the CPU, with the oracles alone, that every one of them is decided): cases of
tests/paths_cases.py cut to m candidate rows, b pending rows, and per kind and bar type an incumbent, per-draw bars and a margin
xi taken from a short grid -- the first for which every round of q = 1, 2 and 64 is decided by more than twice the case's
tolerance (tests/mcbatch_oracle.py: ``decided_by``, which is half the gap between a round's two highest gains).  Values off by at
most tol move a QEI gain and a bar by at most tol each, so a round's gap survives while it exceeds four tolerances, the round
that ends a batch while every live row misses a positive term by more than two, and a QPI count while no value lies within
tol of its threshold."""
import itertools

import numpy as np

from tests import mcbatch_oracle as mo
from tests import paths_cases as pc
from tests import paths_oracle as po

#          case of paths_cases, m, b, dtype, leaves on the device
CONFIGS = [(0, 1, 0, "float64", False),           # N = 2, S = 1, one row
           (1, 64, 3, "mixed", False),            # N = 2, S = 17, Matern-1/2
           (2, 65, 3, "float64", True),           # N = 17, S = 17, a partial block of rows
           (3, 64, 0, "mixed", True),             # N = 17, S = 16
           (4, 65, 3, "float64", False),          # N = 129, S = 129: a second block of draws in stage A
           (4, 127, 3, "mixed", False),
           (10, pc.CHUNK + 3, 0, "float64", False),  # S = 1 across stage A's chunk boundary
           (10, pc.CHUNK + 3, 3, "mixed", True)]
XI_GRID = (0.0, 0.013, 0.029, 0.051, 0.083)  # margins, in units of the values' spread
OFFSETS = (-0.25, 1.0, 2.0, 2.5, 3.0, 1.5)              # the bars against the values' median, likewise


def config_inputs(ci):
    """Rows, pending rows, the oracle's values [S, m + b] of configuration ``ci``, and per kind and bar type the (incumbent,
    bars, xi) chosen -- with the oracle alone -- so that every round of q = 1, 2 and 64 is decided by more than two
    tolerances."""
    index, m, b, dtype, on_device = CONFIGS[ci]
    r = pc.reference(index)
    rows, vals = r["Xs"][:m], r["values"][:, :m]
    if m > pc.CHUNK:  # the round-0 winner of the plain qEI into the last chunk
        win = int(mo.greedy(vals, m, 1, "qei", float(np.median(vals)))[0][0])
        perm = np.arange(m)
        perm[[win, m - 2]] = perm[[m - 2, win]]
        rows, vals = rows[perm], vals[:, perm]
    pend = pc.points_at(b, rows.shape[1], seed=9) if b else None
    V = vals if not b else np.hstack([vals, po.path_values(r["post"], r["s"], r["omega"], r["phase"], r["w"], r["eps"], pend)])
    s = V.shape[0]
    spread = float(np.std(vals)) if m > 1 else 1.0
    chosen = {}
    for kind in ("qei", "qpi"):
        for per_draw in (False, True):
            for off, xi in itertools.product(OFFSETS, XI_GRID[1:] if per_draw else XI_GRID):  # (per-draw bars: always a margin)
                inc = float(np.median(vals)) + off * spread
                bars = np.median(vals, axis=1) + off * spread * np.linspace(0.5, 1.5, s) if per_draw else None
                start = bars if per_draw else inc
                if all(mo.decided_by(V, m, q, kind, start, xi * spread) > 2.0 * r["tol"] for q in (1, 2, 64)):
                    chosen[kind, per_draw] = (inc, bars, xi * spread)
                    break
    return r, rows, pend, V, chosen
