#!/usr/bin/env python3
"""What closing a context costs and gives back, for the build of the library that GPSO_HIP_LIB names (default: the tree's):
close() times of an exact-GP context (C3: N = 2048, D = 12, float32) and of an SGPR and an SVGP context (N = 16384, D = 6,
M = 1024, float64), each after an evaluation with gradient and its posterior; the bytes ``last_count(4)`` reports while the
last one lives and after all are closed (-1 from a build without that count); and the device memory the process has not
given back at the end, from the driver's own free-memory figure.  Prints one line  CLOSE {json}.

    GPSO_HIP_LIB=$PWD/pygpso_amd/libgpso_hip_prev.so GPSO_HIP_LIB_OLDER=1 python tools/devbuf_close.py
    python tools/devbuf_close.py                                         (profiles/devbuf_ab.json quotes both)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (the driver's free-memory figure)

from pygpso_amd import HipGPEngine, model as M_  # noqa: E402
from tests.helpers import synthetic_leaves, synthetic_problem  # noqa: E402

KERNEL = "Matern52"
U = np.array([M_._softplus_inv(0.5), M_._softplus_inv(1.2), M_._softplus_inv(0.01), 0.1])  # one lengthscale, trained mean


def exact():
    X, y = synthetic_problem(2048, 12, seed=0)
    e = HipGPEngine("float32")
    e.set_data(X, y)
    e.fit_eval(KERNEL, [0.8], 1.0, 1e-3, float(y.mean()))
    e.predict(synthetic_leaves(4096, 12, seed=1))
    return e


def sparse(svgp):
    X, y = synthetic_problem(16384, 6, seed=0)
    e = HipGPEngine("float64")
    e.set_data(X, y)
    e.sgpr_set_inducing(X[::16].copy())
    if svgp:
        e.svgp_init_q(KERNEL, U, 1, True, 0.0, 0.01)
        e.svgp_elbo_u(KERNEL, U, 1, True)
        e.svgp_posterior(KERNEL, U, 1, True)
    else:
        e.sgpr_bound_u(KERNEL, U, 1, True)
        e.sgpr_posterior(KERNEL, U, 1, True)
    return e


def main():
    out = {"lib": os.path.basename(os.environ.get("GPSO_HIP_LIB", "libgpso_hip.so"))}
    exact().close()  # (first launches load code objects)
    free0 = torch.cuda.mem_get_info(0)[0]
    probe = HipGPEngine("float64")
    for name, make, reps in (("exact_c3_float32", exact, 5), ("sgpr_n16384_m1024", lambda: sparse(False), 4),
                             ("svgp_n16384_m1024", lambda: sparse(True), 4)):
        close_ms = []
        for _ in range(reps):
            e = make()
            held = probe.last_count(4)
            t0 = time.perf_counter()
            e.close()
            close_ms.append(round(1e3 * (time.perf_counter() - t0), 3))
        out[name] = {"close_ms": close_ms, "bytes_held_while_alive": held}
    out["bytes_held_after_all_closed"] = probe.last_count(4)
    probe.close()
    out["device_bytes_not_given_back"] = int(free0 - torch.cuda.mem_get_info(0)[0])
    print("CLOSE " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
