"""
Priors on the GP hyper-parameters (host side).

The reference trains by maximum marginal likelihood and has none.  A prior is attached per parameter --
``kernel.lengthscales_prior``, ``kernel.variance_prior``, ``likelihood.variance_prior``, ``mean_function.c_prior``; ``None``,
the default, means "no term" -- and enters the training loss in the optimiser's variables u as GPflow 2's
``log_prior_density`` does, the Jacobian of the transform included:

    loss(u) = objective(theta(u)) - sum_i [ log p_i(theta_i(u_i)) + log |d theta_i / d u_i| ]

so that exp(-loss) is a density IN u: what L-BFGS-B then finds is the MAP in u, and what ``hyper_sampler.sample_theta`` draws
from is the posterior of u.  The transforms are the model's: softplus for lengthscales and kernel variance
(d theta / d u = sigmoid(u)), NOISE_FLOOR + softplus for the likelihood variance -- its prior applies to the part above the
floor, softplus(u) --, identity for a trained constant mean.  Everything here is float64 numpy on the host, added after the
device has returned; with every prior ``None`` nothing is added at all.
"""
from __future__ import annotations

import math

import numpy as np

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


class Prior:
    """A density over one scalar parameter: ``log_density(x)`` and its derivative ``dlog_density(x)``, elementwise."""

    def log_density(self, x):
        raise NotImplementedError

    def dlog_density(self, x):
        raise NotImplementedError


class LogNormal(Prior):
    """log x ~ N(log median, sigma^2): for lengthscales, kernel variance and the likelihood variance above its floor."""

    def __init__(self, median, sigma):
        self.median, self.sigma = float(median), float(sigma)
        if not (self.median > 0.0 and math.isfinite(self.median)):
            raise ValueError(f"LogNormal median={median} must be positive and finite")
        if not (self.sigma > 0.0 and math.isfinite(self.sigma)):
            raise ValueError(f"LogNormal sigma={sigma} must be positive and finite")
        self.mu = math.log(self.median)

    def log_density(self, x):
        x = np.asarray(x, dtype=np.float64)
        lx = np.log(x)
        return -lx - math.log(self.sigma) - _HALF_LOG_2PI - 0.5 * ((lx - self.mu) / self.sigma) ** 2

    def dlog_density(self, x):
        x = np.asarray(x, dtype=np.float64)
        return -(1.0 + (np.log(x) - self.mu) / self.sigma ** 2) / x

    def __repr__(self):
        return f"LogNormal(median={self.median}, sigma={self.sigma})"


class Normal(Prior):
    """x ~ N(mu, sigma^2): for a trained constant mean."""

    def __init__(self, mu, sigma):
        self.mu, self.sigma = float(mu), float(sigma)
        if not math.isfinite(self.mu):
            raise ValueError(f"Normal mu={mu} must be finite")
        if not (self.sigma > 0.0 and math.isfinite(self.sigma)):
            raise ValueError(f"Normal sigma={sigma} must be positive and finite")

    def log_density(self, x):
        x = np.asarray(x, dtype=np.float64)
        return -math.log(self.sigma) - _HALF_LOG_2PI - 0.5 * ((x - self.mu) / self.sigma) ** 2

    def dlog_density(self, x):
        x = np.asarray(x, dtype=np.float64)
        return -(x - self.mu) / self.sigma ** 2

    def __repr__(self):
        return f"Normal(mu={self.mu}, sigma={self.sigma})"


SOFTPLUS, IDENTITY = "softplus", "identity"


def _softplus(u):
    return np.logaddexp(0.0, u)


def _sigmoid(u):
    return 0.5 * (1.0 + np.tanh(0.5 * u))


def neg_log_prior_u(u, slots):
    """-sum_i [log p_i(theta_i(u_i)) + log |d theta_i / d u_i|] and its gradient in u.

    ``u [nu]`` or ``[B, nu]``; ``slots``: one ``(prior or None, SOFTPLUS | IDENTITY)`` per variable.  Under SOFTPLUS the prior
    is evaluated at softplus(u_i) (for the likelihood variance that is the part above the floor) and the Jacobian term is
    log sigmoid(u_i) = -softplus(-u_i).  Returns (value, grad): a float and [nu], or [B] and [B, nu]."""
    u = np.asarray(u, dtype=np.float64)
    if u.shape[-1] != len(slots):
        raise ValueError(f"u has {u.shape[-1]} variables, {len(slots)} prior slots")
    value = np.zeros(u.shape[:-1], dtype=np.float64)
    grad = np.zeros_like(u)
    for i, (prior, transform) in enumerate(slots):
        if prior is None:
            continue
        ui = u[..., i]
        if transform == SOFTPLUS:
            x = _softplus(ui)
            value = value - (prior.log_density(x) - _softplus(-ui))
            grad[..., i] = -(prior.dlog_density(x) * _sigmoid(ui) + _sigmoid(-ui))
        elif transform == IDENTITY:
            value = value - prior.log_density(ui)
            grad[..., i] = -prior.dlog_density(ui)
        else:
            raise ValueError(f"unknown transform {transform!r}")
    if u.ndim == 1:
        return float(value), grad
    return value, grad


def default_priors():
    """What ``GPRSurrogate(hyper="marginal")`` attaches when the user passes none -- CHOICES, not measurements: on the
    unit cube a lengthscale of half the side is the median, with a decade either way inside two sigma; the kernel variance
    is centred on the normalised scores' unit scale and left wide; the noise is small but free to grow by orders."""
    return {"lengthscales": LogNormal(0.5, 1.0), "variance": LogNormal(1.0, 1.5), "noise": LogNormal(1.0e-3, 2.0)}


def attach(model, priors):
    """Attach a dictionary of priors (keys ``lengthscales``, ``variance``, ``noise``, ``mean``; missing keys: no change)
    to a ``HipGPR``'s kernel, likelihood and mean function."""
    unknown = set(priors) - {"lengthscales", "variance", "noise", "mean"}
    if unknown:
        raise ValueError(f"unknown prior keys {sorted(unknown)}: lengthscales, variance, noise, mean")
    for p in priors.values():
        if p is not None and not isinstance(p, Prior):
            raise TypeError(f"{p!r} is not a pygpso_amd.priors.Prior")
    if "lengthscales" in priors:
        model.kernel.lengthscales_prior = priors["lengthscales"]
    if "variance" in priors:
        model.kernel.variance_prior = priors["variance"]
    if "noise" in priors:
        model.likelihood.variance_prior = priors["noise"]
    if "mean" in priors:
        model.mean_function.c_prior = priors["mean"]
