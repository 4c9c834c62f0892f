#!/usr/bin/env python3
"""
Accuracy of the acquisition maps (csrc/acq.hpp, through gpso_acq_eval_host: no GPU) against the 60-digit truth of
tests/acq_oracle.py on its fixed grid, beside the float64 numpy / scipy yardstick's own error on the same grid and the
tolerance the tests derive from it (8 x the yardstick, floor 16 ulp).  Writes profiles/acq_accuracy.json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pygpso_amd import HipGPEngine  # noqa: E402
from pygpso_amd import acquisition as A  # noqa: E402
from tests import acq_oracle as AO  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default=None, metavar="ei=E,logei=E,pi=E",
                    help="worst errors the GPU tests printed (tests/test_gpu_acq.py, -s): the device cannot be fed the grid, "
                         "its figures are those of the tests' leaf batches, truth on the call's own mean / var")
    args = ap.parse_args()
    mean, s2, inc = AO.grid()
    doc = {"tool": "tools/acq_accuracy.py", "grid_z": list(AO.GRID_Z), "grid_s": list(AO.GRID_S), "ulp": AO.ULP,
           "measure": "worst relative error against mpmath at 60 digits; logei: absolute over max(1, |value|); below the normal "
                      "range: relative to 2^-1022", "kinds": {}}
    for name, spec in (("ei", A.EI), ("logei", A.LogEI), ("pi", A.PI)):
        kind = AO.KINDS[name]
        tol, yard = AO.tolerance(kind)
        lib = AO.error(kind, HipGPEngine.acq_eval_host(spec(incumbent=inc), mean, s2), AO.grid_truth(kind))
        doc["kinds"][name] = {"library_host": lib, "yardstick": yard, "tolerance": tol,
                              "library_host_ulp": lib / AO.ULP, "yardstick_ulp": yard / AO.ULP}
        print(name, doc["kinds"][name])
    if args.device:
        doc["device_note"] = ("library_device: worst error over the leaf batches of tests/test_gpu_acq.py on an MI355X (float64 and "
                              "mixed contexts, routes a-c), truth evaluated on the call's own returned mean / var; not the grid")
        for item in args.device.split(","):
            name, val = item.split("=")
            doc["kinds"][name]["library_device"] = float(val)
            doc["kinds"][name]["library_device_ulp"] = float(val) / AO.ULP
    out = os.path.join(ROOT, "profiles", "acq_accuracy.json")
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
