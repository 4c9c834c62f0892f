#!/usr/bin/env python3
"""
The two Chebyshev tables of pygpso_amd/csrc/acq.hpp, fitted at 50 digits with mpmath.

  erfc:   h(t) = erfc(x) exp(x^2) / t,  t = 2 / (2 + x),      over t in [0.045, 1]   (0 <= x <= 42.4)     -> acq_erfc
  mills:  p(w) = T^2 (1 - T R(T)),      w = 1 / T,            over w in [0.1, 1]     (1 <= T <= 10)       -> acq_mills_p
          R(T) = Phi(-T) / phi(T) = sqrt(pi / 2) erfc(T / sqrt 2) exp(T^2 / 2), Mills' ratio; q = 1 - T R = p / T^2

Each function is sampled at 96 Chebyshev nodes of its interval mapped to [-1, 1], the coefficients c_j = (2 / 96) sum_k
f(x_k) cos(j pi (k + 1/2) / 96) are formed at 50 digits and rounded to float64; the header keeps the first 32 (erfc) and 44 (mills) of them
and evaluates  c_0 / 2 + sum_j c_j T_j(u)  by Clenshaw's recurrence.  Prints the tables as they stand in the header and the
size of the first coefficient left out, relative to the smallest value of the function on the interval.

    python tools/fit_acq_tables.py            # print both tables
    python tools/fit_acq_tables.py --check    # exit 1 unless the header holds exactly these literals
"""
import argparse
import os
import re
import sys

import mpmath as mp

mp.mp.dps = 50
NODES = 96
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def h_erfc(t):
    x = 2 / t - 2
    return mp.exp(x * x) * mp.erfc(x) / t


def p_mills(w):
    tau = 1 / w
    R = mp.sqrt(mp.pi / 2) * mp.erfc(tau / mp.sqrt(2)) * mp.exp(tau * tau / 2)
    return tau * tau * (1 - tau * R)


TABLES = {"erfc": (h_erfc, mp.mpf("0.045"), mp.mpf(1), 32), "mills": (p_mills, mp.mpf("0.1"), mp.mpf(1), 44)}


def fit(f, lo, hi):
    nodes = [mp.cos(mp.pi * (k + mp.mpf(1) / 2) / NODES) for k in range(NODES)]
    vals = [f((hi - lo) / 2 * u + (hi + lo) / 2) for u in nodes]
    coef = [2 / mp.mpf(NODES) * sum(vals[k] * mp.cos(j * mp.pi * (k + mp.mpf(1) / 2) / NODES) for k in range(NODES))
            for j in range(NODES)]
    return coef, min(abs(v) for v in vals)


def literals(coef, keep):
    return [repr(float(c)) for c in coef[:keep]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    header = open(os.path.join(ROOT, "pygpso_amd", "csrc", "acq.hpp")).read()
    ok = True
    for name, (f, lo, hi, keep) in TABLES.items():
        coef, smallest = fit(f, lo, hi)
        lits = literals(coef, keep)
        print(f"// {name}: {keep} coefficients over [{lo}, {hi}]; first one left out {mp.nstr(abs(coef[keep]) / smallest, 2)} of the function")
        for i in range(0, keep, 4):
            print("      " + ", ".join(lits[i:i + 4]) + ",")
        if args.check:
            m = re.search(r"kAcqCheb_%s\[\d+\] = \{(.*?)\};" % name, header, re.S)
            have = [s.strip() for s in m.group(1).replace("\n", " ").split(",") if s.strip()] if m else []
            if have != lits:
                print(f"{name}: the header's table differs", file=sys.stderr)
                ok = False
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
