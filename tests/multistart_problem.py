"""
The multimodal toy problem the multi-start tests share (tests/test_multistart_cpu.py, tests/test_gpu_multistart.py), and a
stand-in model over the float64 oracle.

N = 10 points in 2-D, Matern-5/2, isotropic lengthscale, trained constant mean: from the surrogate's default
hyper-parameters (start 0) L-BFGS-B settles in a local optimum of the NLML at 10.2897; from START_1 (long lengthscale,
large noise) it reaches 10.1524 -- 0.137 nats lower.  Chosen with the oracle alone (seed 1 of the generator below).
"""
import functools

import numpy as np

from oracle import gpr

KERNEL = "Matern52"
THETA0 = dict(lengthscales=0.25, variance=1.0, noise=1.0e-3, mean_c=0.0)  # GPRSurrogate.default()'s


@functools.lru_cache(maxsize=None)
def problem():
    """(X [10, 2], y [10], u0 [4], starts [3, 4]): read-only arrays."""
    rng = np.random.default_rng(1)
    X = rng.uniform(0.0, 1.0, (10, 2))
    y = np.sin(9.0 * X[:, 0]) * np.cos(7.0 * X[:, 1]) + 0.3 * rng.standard_normal(10)
    u0 = gpr.Theta(KERNEL, **THETA0).pack()
    starts = np.stack([gpr.Theta(KERNEL, 2.0, 0.5, 0.5, 0.0).pack(),
                       gpr.Theta(KERNEL, 0.05, 1.0, 0.05, 0.0).pack(),
                       gpr.Theta(KERNEL, 0.7, 0.2, 0.01, 0.3).pack()])
    for a in (X, y, u0, starts):
        a.setflags(write=False)
    return X, y, u0, starts


class OracleModel:
    """Stand-in for HipGPR: ``_pack`` / ``_assign`` / ``_loss_and_grad`` / ``_loss_and_grad_batch`` over the oracle's NLML
    in the optimiser's variables.  ``fail(u) -> bool`` marks evaluations that report "not positive definite"."""

    def __init__(self, X, y, u0, kernel=KERNEL, fail=None, with_batch=True):
        self.X, self.y, self.kernel = X, y, kernel
        self.u = np.array(u0, dtype=np.float64)
        self.fail = fail
        self.single_calls = self.batch_calls = 0
        if not with_batch:
            self._loss_and_grad_batch = None

    def _pack(self):
        return self.u.copy()

    def _assign(self, u):
        self.u = np.array(u, dtype=np.float64)

    def training_loss(self):
        return gpr.loss_and_grad_unconstrained(self.kernel, self.u, self.X, self.y)[0]

    def _eval(self, u):
        if self.fail is not None and self.fail(u):
            raise np.linalg.LinAlgError("stand-in: not positive definite")
        return gpr.loss_and_grad_unconstrained(self.kernel, u, self.X, self.y)

    def _loss_and_grad(self, u):
        self.single_calls += 1
        return self._eval(u)

    def _loss_and_grad_batch(self, U):
        self.batch_calls += 1
        U = np.atleast_2d(U)
        loss, grad, ok = np.full(U.shape[0], np.nan), np.full(U.shape, np.nan), np.zeros(U.shape[0], dtype=bool)
        for b, u in enumerate(U):
            try:
                loss[b], grad[b] = self._eval(u)
                ok[b] = True
            except np.linalg.LinAlgError:
                pass
        return loss, grad, ok


@functools.lru_cache(maxsize=None)
def oracle_multistart():
    """The R = 4 multi-start on the problem, through the oracle: the OptimizeResult (with ``restarts`` and ``winner``)."""
    from pygpso_amd.kernels import Scipy

    X, y, u0, starts = problem()
    model = OracleModel(X, y, u0)
    return Scipy(restarts=4, starts=starts).minimize(model.training_loss)
