"""The parity cases of ``gpso_paths_draw_q`` shared by tests/test_gpu_paths_q.py (which runs them on the device) and
tests/test_paths_q_cpu.py (which checks on the CPU that they are well conditioned and that the arg-max gap rule leaves out
none of them), in the manner of tests/paths_cases.py, whose helpers (points, clipped inputs, tolerance, segments) they use.

Shapes, the smallest that reach every path: n = 2 resident rows; 17 a partial 16-step; 33 three of them; 129 three 64-row
blocks of the triangular products; 40 with D = 26 (D_pad = 28).  The sparse cases put N = 130 or 300 training points behind
M = 2, 17, 33, 40 and 129 inducing rows (the first M training rows).  F = 1, 5, 64, 257; S = 1, 17 (a second accumulator tile
with one draw), 129 (a third 64-column block of the triangular products, a second block of draws in the evaluation); M_eval
= 1, 65, 130 and one case of 16384 + 3 points.  The four kernels; the Gaussian likelihood for every family and one Student-t
(df = 4) each for the VGP and the SVGP, whose install may shift the served variance and must not shift a draw.

q is one natural-gradient step of the family's oracle from the prior (gamma = 0.7), set on the device with
``vgp_set_q`` / ``svgp_set_q``; the SGPR has no q of its own.

Conditioning.  v applies Lu^-1 twice at jitter 1e-6, so a rounding of relative size e in k(Zr, Zr) reaches a value as about
e |K~^-1 k*| |K~^-1 P|.  The lengthscales are 0.18 sqrt(D) on U[0, 1]^D (0.3 for the two-row case): the condition number of
K~ then runs from 6 to 3e6 over the cases -- the squared-exponential one at 129 rows sits on the jitter --, and no (draw,
segment) pair falls under the gap rule.  tests/test_paths_q_cpu.py holds every case to a tenth of the bar twice: the
float64 oracle against its extended-precision twin, and against itself with Lu from the direct-difference Gram in place of
the GEMM-form one (two roundings of the same matrix, what the device's own Gram is a third of; largest 2.2e-11 against a
bar of 4.1e-8 on the smooth kernels).
"""
import numpy as np

from pygpso_amd import paths as P  # noqa: F401  (the generator behind paths_cases.inputs)
from tests import paths_cases as pc
from tests import paths_oracle as po
from tests import paths_q_oracle as pq
from tests import svgp_oracle as SV
from tests import vgp_oracle as V
from tests import vgp_studentt_oracle as T
from tests.helpers import synthetic_problem

CHUNK = pc.CHUNK
SEGMENTS = pc.SEGMENTS
GAUSSIAN = pq.GAUSSIAN
STUDENT = ("StudentT", 4.0)
GAMMA = 0.7
#        family, n,   D,  N,   kernel,               F,   S,   M_eval,    likelihood
CASES = [("vgp", 2, 1, 2, "Matern52", 1, 1, 1, GAUSSIAN),
         ("vgp", 17, 3, 17, "SquaredExponential", 5, 17, 65, GAUSSIAN),
         ("vgp", 33, 5, 33, "Matern32", 64, 17, 130, STUDENT),
         ("vgp", 129, 3, 129, "Matern52", 257, 129, 130, GAUSSIAN),
         ("vgp", 40, 26, 40, "Matern12", 64, 17, 130, GAUSSIAN),
         ("sgpr", 17, 3, 130, "Matern32", 5, 17, 65, GAUSSIAN),
         ("sgpr", 33, 5, 300, "Matern52", 64, 129, 130, GAUSSIAN),
         ("sgpr", 129, 3, 300, "SquaredExponential", 257, 17, 130, GAUSSIAN),
         ("sgpr", 40, 26, 130, "Matern12", 5, 1, 65, GAUSSIAN),
         ("svgp", 17, 3, 130, "Matern52", 5, 1, CHUNK + 3, GAUSSIAN),
         ("svgp", 33, 5, 300, "Matern32", 64, 17, 130, STUDENT),
         ("svgp", 129, 3, 300, "Matern52", 257, 17, 130, GAUSSIAN),
         ("svgp", 2, 1, 130, "SquaredExponential", 1, 17, 1, GAUSSIAN)]
N_LS, TRAIN_MEAN = 1, True


def name(index):
    fam, n, d, big_n, kernel, f, s, m, lik = CASES[index]
    return f"{fam} n={n} D={d} N={big_n} {kernel} F={f} S={s} M={m} {lik[0]}"


def initial_u(index, y):
    fam, n, d, big_n, kernel, f, s, m, lik = CASES[index]
    ls = 0.3 if n == 2 else 0.18 * np.sqrt(d)
    p = 0.3 if lik[0] == "StudentT" else 0.05  # the Student-t scale | the Gaussian noise variance
    return SV.initial_u(ls, 1.3, p, lik, float(np.mean(y)))


def posterior(index, X, y, u):
    """(the oracle's whitened posterior, Z or None, q_mu or None, q_sqrt or None) of case ``index``."""
    fam, n, d, big_n, kernel, f, s, m, lik = CASES[index]
    if fam == "vgp":
        mu0, S0 = np.zeros(n), np.eye(n)
        if lik[0] == "StudentT":
            mu, S = T.natgrad(kernel, u, N_LS, TRAIN_MEAN, 0.0, X, y, mu0, S0, lik, GAMMA)
        else:
            mu, S = V.natgrad(kernel, u, N_LS, TRAIN_MEAN, 0.0, X, y, mu0, S0, GAMMA)
        return pq.vgp_posterior(kernel, u, N_LS, TRAIN_MEAN, 0.0, X, mu, S, lik), None, mu, S
    Z = np.ascontiguousarray(X[:n])
    if fam == "sgpr":
        return pq.sgpr_posterior(kernel, u, N_LS, TRAIN_MEAN, 0.0, X, y, Z), Z, None, None
    mu, S = SV.natgrad(kernel, u, N_LS, TRAIN_MEAN, 0.0, X, y, Z, np.zeros(n), np.eye(n), lik, GAMMA)
    return pq.svgp_posterior(kernel, u, N_LS, TRAIN_MEAN, 0.0, X, Z, mu, S, lik), Z, mu, S


_cache = {}


def reference(index):
    """Problem, u, q, the oracle's posterior, the random inputs and the oracle's values of case ``index``; computed once and
    shared (never modified)."""
    if index not in _cache:
        fam, n, d, big_n, kernel, f, s_draws, m, lik = CASES[index]
        X, y = synthetic_problem(big_n, d, seed=29 + big_n + n)
        u = initial_u(index, y)
        post, Z, mu, S = posterior(index, X, y, u)
        Xs = pc.points_at(m, d)
        omega, phase, w, eps = pc.inputs(kernel, s_draws, f, n, d, seed=200 + index)
        _cache[index] = dict(family=fam, kernel=kernel, lik=lik, X=X, y=y, u=u, Z=Z, mu=mu, S=S, post=post, Xs=Xs, omega=omega,
                             phase=phase, w=w, eps=eps, values=pq.path_values(post, omega, phase, w, eps, Xs),
                             tol=pc.tolerance(kernel, y, post.theta.variance, w))
    return _cache[index]


def segment_layouts(r):
    return [None] + ([SEGMENTS] if r["Xs"].shape[0] == 130 else [])


def undecided(r, seg_off):
    """The (draw, segment) pairs whose two highest oracle values lie within ten times the bar: their index is not compared."""
    return po.top_two_gap(r["values"], seg_off) < 10.0 * r["tol"]
