#!/usr/bin/env python3
"""
What a Monte-Carlo batch selection over the path draws costs on the device, beside the only route the
tree had before it.

At D = 12, N = 2048, Matern-5/2, float64, S = 64 draws over F = 1024 features, q = 8, qNoisyEI (per-draw bars: the draws' own
maxima over the training rows), for M = 162 host leaves -- the optimiser's loop -- and M = 65 536 device-resident leaves, two
candidates timed in turn (alternating, one process):
  device   ONE gpso_paths_best_batch call: stage A (paths_eval_kernel into the call's S x M workspace), the fold of the bars,
           q round + fold launches, one wait, one read-back of the picks
  host     gpso_paths_eval with the S x M values copied to the host (8 S M bytes over PCIe), then gpso_paths_batch_host on them
Both return the same picks and the same gain bits (checked before anything is timed).  One further timed device call gives the
split by HIP events: gpso_last_ms(ctx, 1) the call, (ctx, 0) its rounds, the difference stage A.  The rounds stream S M 8
bytes of V per round that ran; that over the rounds' event time is set against the HBM figures of the microarchitecture notes
(8.0 TB/s specified, 6.29 TB/s measured by a float4 copy).  The event span holds 2 q + 1 launches and a 1.6 KB copy, so at small M
it measures launches, not bandwidth; and a 32 MB matrix that stage A has just written may be served by the 256 MiB last-level
cache rather than HBM: the figure is a rate over the rounds, named for what it is.

Each figure is the median host wall time of CALLS synchronous calls after WARMUP, repeated REPEATS = 5 times; the min and max
of the repeated medians are kept beside their median.  Nothing here has a target: the figures are recorded.  Without a GPU
the script fails (no fallback).  Writes one JSON document (default profiles/mcbatch_bench.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, D, S, F, Q = 2048, 12, 64, 1024, 8
SIZES = ((162, False), (65536, True))  # (leaves, device-resident)
HBM_SPEC_TBS, HBM_MEASURED_TBS = 8.0, 6.29


def bench_size(eng, bars, leaves, on_device, calls, warmup, repeats):
    import torch

    from ensemble_bench import timed
    from pygpso_amd import HipGPEngine

    m = leaves.shape[0]
    xs = leaves
    if on_device:
        xs = torch.from_numpy(leaves).to(torch.device("cuda", eng.device))
        torch.cuda.synchronize()

    def device():
        return eng.paths_best_batch(xs, Q, "qnei", incumbent_s=bars)

    def host():
        values = eng.paths_eval(xs)[0]
        return HipGPEngine.paths_batch_host(values, Q, "qnei", incumbent_s=bars)[:3]

    a, b = device(), host()
    same = bool(np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes())
    res = timed({"device": device, "host": host}, calls, warmup, repeats)
    eng.set_timing(True)
    split = []
    for _ in range(repeats):
        picks = device()[0]
        split.append((eng.last_ms(1), eng.last_ms(0), len(picks)))
    call_ms, rounds_ms, rounds_run = (float(np.median([s[i] for s in split])) for i in range(3))
    bytes_rounds = rounds_run * S * m * 8.0
    rate = bytes_rounds / (rounds_ms * 1e-3) / 1e12 if rounds_ms > 0.0 else float("nan")
    res.update(m=m, leaves="device float64" if on_device else "host float64", same_picks_and_bits=same, picks=[int(i) for i in a[0]],
               batch_value=float(a[2][-1]), device_call_ms=call_ms, device_rounds_ms=rounds_ms, device_stage_a_ms=call_ms - rounds_ms,
               rounds_run=int(rounds_run), rounds_bytes=bytes_rounds, rounds_tb_per_s=rate,
               rounds_share_of_hbm_spec=rate / HBM_SPEC_TBS, rounds_share_of_hbm_measured=rate / HBM_MEASURED_TBS,
               host_route_pcie_bytes=8.0 * S * m)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcbatch_bench.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch

    torch.cuda.set_device(0)  # (torch's runtime first, as bench.py does: the device-resident leaves are a torch tensor)
    torch.zeros(1, device="cuda:0")
    from ensemble_bench import problem
    from pygpso_amd import HipGPEngine
    from pygpso_amd.paths import draw_path_inputs

    X, y, _ = problem(N, D, 1)
    eng = HipGPEngine("float64")
    eng.set_data(X, y)
    eng.fit_eval("Matern52", [0.3 * np.sqrt(D)], 1.0, 2.0e-3, float(y.mean()), want_grad=False)
    eng.paths_draw(*draw_path_inputs("Matern52", S, F, N, D, rng=3))
    bars = np.ascontiguousarray(eng.paths_eval(X, want_values=False)[2][:, 0])
    doc = {"tool": "tools/mcbatch_bench.py", "n": N, "d": D, "kernel": "Matern52", "dtype": "float64", "s": S, "f": F, "q": Q,
           "kind": "qnei (GPSO_MC_QEI under per-draw bars)", "calls": args.calls, "warmup": args.warmup, "repeats": args.repeats,
           "clock": "host wall time around synchronous calls; device_* from HIP events of one further call (median of repeats)",
           "hbm_tb_per_s": {"spec": HBM_SPEC_TBS, "measured_float4_copy": HBM_MEASURED_TBS}, "sizes": []}
    for m, on_device in SIZES:
        leaves = np.random.default_rng([1, m, D]).random((m, D))
        r = bench_size(eng, bars, leaves, on_device, args.calls, args.warmup, args.repeats)
        doc["sizes"].append(r)
        print(f"M={m}: device {r['device']['median_us']:.0f} us ({r['device']['min_us']:.0f}-{r['device']['max_us']:.0f}), host route "
              f"{r['host']['median_us']:.0f} us ({r['host']['min_us']:.0f}-{r['host']['max_us']:.0f}); events: call {r['device_call_ms'] * 1e3:.0f} us = "
              f"stage A {r['device_stage_a_ms'] * 1e3:.0f} + rounds {r['device_rounds_ms'] * 1e3:.0f} us ({r['rounds_run']} rounds, "
              f"{r['rounds_tb_per_s']:.3f} TB/s = {100 * r['rounds_share_of_hbm_spec']:.1f} % of 8.0); same picks and bits {r['same_picks_and_bits']}",
              flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0 if all(r["same_picks_and_bits"] for r in doc["sizes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
