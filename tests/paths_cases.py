"""The parity cases of ``gpso_paths_draw`` / ``gpso_paths_eval`` shared by tests/test_gpu_paths.py (which runs them on the
device) and tests/test_paths_cpu.py (which checks on the CPU that they are well conditioned and that the arg-max gap rule
excludes few of them).  Problems as tests/test_gpu_predict_grad.py builds them.

Shapes, the smallest that reach every path: N = 2 one row; 17 a partial 16-step; 129 three 64-row blocks of the triangular
products and nine steps of the kernel part; 300 several of each; D = 1, 3, 5, 26 (D_pad = 28); F = 1, 4, 5 (a partial
16-step), 64, 257 (seventeen steps, the last with one feature); S = 1, 16, 17 (a second accumulator tile with one draw), 129
(a second block of draws with one draw); M = 1, 64, 65, 130 (a partial 64-point tile, several tiles); one case of 16384 + 3
points crosses the evaluation's chunk once.  Every other case carries a per-point noise vector.

The Matern-1/2's frequencies are Cauchy distributed: a seed's draw may hold one of 1e4 and more, whose cosine argument
loses digits to the order in which omega . x is summed.  The cases CLIP every frequency to [-50, 50] (a test input like any
other: the entry points take every finite frequency), which keeps the float64 and extended-precision oracles within a tenth
of the GPU tolerance of each other (test_paths_cpu.py checks it for every case).
"""
import numpy as np

from oracle import gpr
from pygpso_amd import paths as P
from tests import hetero_oracle as ho
from tests import paths_oracle as po
from tests.helpers import synthetic_problem

CHUNK = 16384  # kPathsChunk
OMEGA_CLIP = 50.0
#        N,   D, kernel,               F,   S,   M
CASES = [(2, 1, "Matern52", 1, 1, 1),
         (2, 1, "Matern12", 64, 17, 130),
         (17, 3, "SquaredExponential", 5, 17, 65),
         (17, 3, "Matern32", 4, 16, 64),
         (129, 3, "Matern52", 257, 129, 130),
         (129, 3, "Matern12", 64, 17, 130),
         (300, 5, "Matern12", 5, 1, 65),
         (300, 5, "Matern32", 257, 16, 130),
         (40, 26, "Matern52", 4, 16, 1),
         (40, 26, "SquaredExponential", 64, 17, 64),
         (17, 3, "Matern52", 4, 1, CHUNK + 3),
         (17, 3, "Matern32", 4, 1, 130)]
SEGMENTS = np.array([0, 1, 70, 130], dtype=np.int64)  # a single row; a boundary strictly inside the tile [64, 128)


def points_at(m, d, seed=5):
    return np.random.default_rng(seed).uniform(-0.2, 1.2, size=(m, d))


def tolerance(kernel, y, variance, w):
    """The project's float64 stage tolerance by the case's scale; 1e-4 for the Matern-1/2 (the square
    root at r = 0 amplifies the rounding of r^2, which the oracle and the device form differently)."""
    scale = max(float(np.max(np.abs(y))), float(np.sqrt(variance) * np.max(np.abs(w))))
    return (1.0e-4 if kernel == "Matern12" else 1.0e-8) * scale


def inputs(kernel, s, f, n, d, seed):
    """``paths.draw_path_inputs`` with the frequencies clipped (module docstring)."""
    omega, phase, w, eps = P.draw_path_inputs(kernel, s, f, n, d, rng=seed)
    return np.clip(omega, -OMEGA_CLIP, OMEGA_CLIP), phase, w, eps


_cache = {}


def reference(index):
    """Problem, theta, s (every other case), the oracle's posterior, the random inputs and the oracle's values of case
    ``index``; computed once and shared (never modified)."""
    if index not in _cache:
        n, d, kernel, f, s_draws, m = CASES[index]
        X, y = synthetic_problem(n, d, seed=17 + n)
        ls = 0.25 * np.sqrt(d) * (np.linspace(0.8, 1.3, d) if index % 4 < 2 else np.ones(1))
        th = gpr.Theta(kernel, ls, 1.3, 1.0e-3 if index % 3 else 1.0e-1, float(y.mean()))
        s = ho.draw_s(n, th.variance, seed=n + d) if index % 2 else None
        post = ho.posterior(th, X, y, np.zeros(n) if s is None else s)
        Xs = points_at(m, d)
        omega, phase, w, eps = inputs(kernel, s_draws, f, n, d, seed=100 + index)
        _cache[index] = dict(X=X, y=y, th=th, s=s, post=post, Xs=Xs, omega=omega, phase=phase, w=w, eps=eps,
                             values=po.path_values(post, s, omega, phase, w, eps, Xs), tol=tolerance(kernel, y, th.variance, w))
    return _cache[index]


def append_case():
    """The case of the GPU suite's append test: N = 300 + 3 points appended in place, Matern-5/2, S = 5, F = 64, M = 70 -- the
    random inputs drawn for the 303 points, the oracle's from-scratch posterior of all of them."""
    if "append" not in _cache:
        X, y = synthetic_problem(303, 5, seed=2)
        th = gpr.Theta("Matern52", 0.5 * np.linspace(0.8, 1.3, 5), 1.3, 1.0e-3, float(y.mean()))
        post = gpr.posterior(th, X, y)
        Xs = points_at(70, 5)
        omega, phase, w, eps = inputs("Matern52", 5, 64, 303, 5, seed=1)
        _cache["append"] = dict(X=X, y=y, th=th, s=None, post=post, Xs=Xs, omega=omega, phase=phase, w=w, eps=eps,
                                values=po.path_values(post, None, omega, phase, w, eps, Xs), tol=tolerance("Matern52", y, th.variance, w))
    return _cache["append"]


def name(index):
    n, d, kernel, f, s, m = CASES[index]
    return f"N={n} D={d} {kernel} F={f} S={s} M={m} s={'yes' if index % 2 else 'no'}"
