#!/usr/bin/env python3
"""
The worst errors of gpso_cross_cov and gpso_best_batch over the cases of tests/test_gpu_batch.py, against the dense-solve
oracle of tests/batch_oracle.py: per case and engine the largest |cov - oracle| over the test's (m, b) shapes, and for six
rounds of ucb_var and ucb_std the largest |var|, |value| and |var_after| error, with the picks compared (float64) or replayed
against the oracle conditioned on the device's earlier picks (mixed, and the Matern-1/2).  Errors relative to the kernel
variance.  Writes profiles/batch_parity.json.        python tools/batch_errors.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import batch_oracle as B
    from tests import test_gpu_batch as T

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_parity.json"))
    a = ap.parse_args()
    rows = []
    cases = [(i, "Matern52", False, False) for i in range(len(B.PROBLEMS))] + [c for c in T.COV_CASES if c[1:] != ("Matern52", False, False)]
    for key in cases:
        c = T.case(*key)
        mean, Sigma = c.oracle()
        noise, scale = c.theta.noise, c.theta.variance
        for dtype in T.DTYPES:
            eng = c.engine(dtype)
            row = {"problem": list(B.PROBLEMS[key[0]]), "m": len(c.leaves), "kernel": key[1], "ard": key[2], "noise_vector": key[3],
                   "dtype": dtype}
            worst = 0.0
            for m, b in T.SHAPES:
                m, b = min(m, len(c.leaves)), min(b, len(c.leaves))
                got = eng.cross_cov(c.leaves[:m], c.leaves[len(c.leaves) - b:])
                worst = max(worst, float(np.max(np.abs(got - Sigma[len(c.leaves) - b:, :m]))))
            row["cross_cov"] = worst / scale
            for name in ("ucb_var", "ucb_std"):
                idx, mu, var, val, after = eng.best_batch(c.leaves, T._spec(name), B.ROUNDS, noise, want_var_after=True)
                want = B.greedy(mean, Sigma, c.leaves, noise, noise, name, B.ROUNDS)
                dv = dval = shortfall = 0.0
                for t in range(len(idx)):
                    var_o, val_o = B.round_state(mean, Sigma, noise, noise, name, idx[:t])
                    live = np.ones(len(mean), dtype=bool)
                    live[idx[:t]] = False
                    dv = max(dv, abs(var[t] - var_o[idx[t]]))
                    dval = max(dval, abs(val[t] - val_o[idx[t]]))
                    shortfall = max(shortfall, float(np.max(val_o[live]) - val_o[idx[t]]))
                var_o, _ = B.round_state(mean, Sigma, noise, noise, name, idx)
                row[name] = {"picks_equal_oracle": idx.tolist() == want.idx.tolist(), "min_gap": float(np.min(want.gaps)),
                             "var": dv / scale, "value": dval, "value_below_oracle_maximum": shortfall,
                             "var_after": float(np.max(np.abs(after - var_o))) / scale}
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"note": "worst errors over the cases of tests/test_gpu_batch.py against tests/batch_oracle.py (float64 numpy / scipy, "
                           "one dense solve per round); var, var_after and cross_cov relative to the kernel variance; value absolute; "
                           "value_below_oracle_maximum: how far the oracle's value of the device's pick lies below the oracle's best "
                           "live row, given the device's earlier picks", "rounds": B.ROUNDS, "rows": rows}, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
