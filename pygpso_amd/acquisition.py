"""
Acquisition functions: what a leaf is ranked by, as a map of the (mean, var) the predict kernels produce.

The maps themselves run on the device (``csrc/acq.hpp``, behind ``gpso_best_acq*`` / ``gpso_acq_values``) or, for checks
without a GPU, on the host through the same header (``gpso_acq_eval_host``).  This module holds the small spec objects the
Python layers pass around, their names, and a numpy restatement of the two kinds that are in SCORE UNITS -- the ones the
optimiser's loop may rank by, because ``GPSOptimiser._tree_select`` compares a leaf's value with evaluated scores:

* ``UCBVar(varsigma)``   mean + varsigma * var       the reference's rule (gpso/gp_surrogate.py:326)
* ``UCBStd(varsigma)``   mean + varsigma * sqrt(var) GP-UCB

``EI``, ``LogEI`` and ``PI`` rank leaves against an incumbent; their values are improvements, log-improvements and
probabilities, not scores, so they serve ``gp_eval_best_acq`` / ``gp_acq_values`` / ``polish`` but not the loop.

``MES`` (max-value entropy search, Wang & Jegelka 2017) ranks a leaf by the information it carries about the optimum's
VALUE, from K sampled maxima y* (``max_value_samples`` of the models): (1/K) sum_k t((y*_k - mean) / s) with
t(g) = g phi(g) / (2 Phi(g)) - log Phi(g).  Its values are nats, not scores; it serves ``gp_eval_best_acq``,
``gp_acq_values``, ``select_batch`` and ``mes_select``, not the loop and not ``polish``.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L


class Acquisition:
    """Base of the specs: ``kind`` (GPSO_ACQ_*), ``name``, ``score_units``."""

    kind = -1
    name = ""
    score_units = False
    needs_incumbent = False

    def __init__(self, varsigma=0.0, xi=0.0, latent=False, incumbent=None):
        self.varsigma = float(varsigma)
        self.xi = float(xi)
        self.latent = bool(latent)
        self.incumbent = None if incumbent is None else float(incumbent)

    def c_struct(self, incumbent=None):
        """The ``gpso_acq`` record of this spec; ``incumbent`` overrides the spec's own."""
        inc = self.incumbent if incumbent is None else float(incumbent)
        if self.needs_incumbent and inc is None:
            raise ValueError(f"{self.name}: an incumbent is needed (the best score so far, in the model's units)")
        return L.GpsoAcq(self.kind, int(self.latent), self.varsigma, 0.0 if inc is None else inc, self.xi)

    def host_value(self, mean, var):
        """numpy restatement (score-unit kinds only): the bits the device writes for the same (mean, var)."""
        raise NotImplementedError(f"{self.name} has no host restatement: use HipGPEngine.acq_eval_host")

    def __repr__(self):
        return f"{type(self).__name__}(varsigma={self.varsigma}, xi={self.xi}, latent={self.latent}, incumbent={self.incumbent})"


class UCBVar(Acquisition):
    kind, name, score_units = L.ACQ_UCB_VAR, "ucb_var", True

    def __init__(self, varsigma):
        super().__init__(varsigma=varsigma)

    def host_value(self, mean, var):
        return mean + self.varsigma * var


class UCBStd(Acquisition):
    kind, name, score_units = L.ACQ_UCB_STD, "ucb_std", True

    def __init__(self, varsigma, latent=False):
        super().__init__(varsigma=varsigma, latent=latent)

    def host_value(self, mean, var):
        return mean + self.varsigma * np.sqrt(np.maximum(var, 0.0))


class EI(Acquisition):
    kind, name, needs_incumbent = L.ACQ_EI, "ei", True

    def __init__(self, xi=0.0, latent=False, incumbent=None):
        super().__init__(xi=xi, latent=latent, incumbent=incumbent)


class LogEI(EI):
    kind, name = L.ACQ_LOGEI, "logei"


class PI(EI):
    kind, name = L.ACQ_PI, "pi"


class MES(Acquisition):
    """``maxima``: the sampled maxima y* (at most 64 finite values) the engine installs on its context before a call
    (``gpso_acq_set_maxima``); ``None``: the call reads whatever the context holds.  ``latent`` (the default): s is the
    latent standard deviation, the quantity the entropy of y* is about."""

    kind, name = L.ACQ_MES, "mes"

    def __init__(self, latent=True, maxima=None):
        super().__init__(latent=latent)
        self.maxima = None if maxima is None else np.array(maxima, dtype=np.float64).reshape(-1)

    def __repr__(self):
        return f"MES(latent={self.latent}, maxima={None if self.maxima is None else self.maxima.tolist()})"


BY_NAME = {c.name: c for c in (UCBVar, UCBStd, EI, LogEI, PI, MES)}
BY_NAME["ucb"] = UCBVar
SCORE_UNIT_NAMES = tuple(n for n, c in BY_NAME.items() if c.score_units and n != "ucb")


def resolve(acquisition, varsigma=None, **kwargs):
    """A spec from a spec or a name.  The UCB kinds take ``varsigma``; EI / LogEI / PI take ``xi``, ``latent``,
    ``incumbent``; MES takes ``latent`` and ``maxima``."""
    if isinstance(acquisition, Acquisition):
        return acquisition
    try:
        cls = BY_NAME[str(acquisition).lower()]
    except KeyError:
        raise ValueError(f"unknown acquisition {acquisition!r}: one of {sorted(BY_NAME)}") from None
    if cls.score_units:
        if varsigma is None:
            raise ValueError(f"{cls.name} needs varsigma")
        return cls(varsigma, **kwargs)
    return cls(**kwargs)


def score_unit_spec(acquisition, varsigma):
    """The spec a surrogate's loop ranks by: ``ucb_var`` or ``ucb_std`` only (see the module text)."""
    name = acquisition.name if isinstance(acquisition, Acquisition) else str(acquisition).lower()
    cls = BY_NAME.get(name)
    if cls is None:
        raise ValueError(f"unknown acquisition {acquisition!r}: one of {sorted(BY_NAME)}")
    if not cls.score_units:
        raise ValueError(f"gp_acquisition={name!r} is not in score units: the optimiser's loop compares a leaf's acquisition "
                         f"value with evaluated scores, so only {SCORE_UNIT_NAMES} can drive it (use gp_eval_best_acq / "
                         f"gp_acq_values for EI, log-EI and PI)")
    return acquisition if isinstance(acquisition, Acquisition) else cls(varsigma)


# ---- host-side value and chain rule of EI / log-EI (GPSurrogate.polish) -------------------------------------------
_SQRT2 = float(np.sqrt(2.0))
_HALF_LOG_2PI = 0.9189385332046728


def h_parts(z):
    """For h(z) = phi(z) + z Phi(z): (log h, Phi / h, phi / h), none of Phi, phi or h formed where they underflow.
    z >= -1: as written.  Below: with Mills' ratio R = Phi / phi = sqrt(pi / 2) erfcx(-z / sqrt 2) and q = 1 + z R,
    log h = -z^2 / 2 - log(2 pi) / 2 + log q,  Phi / h = R / q,  phi / h = 1 / q;  z <= -10 takes q from the asymptotic
    series sum_k (-1)^k (2k + 1)!! / z^(2k + 2), where 1 + z R has cancelled to nothing."""
    from scipy.special import erfcx, ndtr

    z = np.asarray(z, dtype=np.float64)
    log_h, phi_r, pdf_r = np.empty_like(z), np.empty_like(z), np.empty_like(z)
    up = z >= -1.0
    zu = z[up]
    pdf = np.exp(-0.5 * zu * zu) / np.sqrt(2.0 * np.pi)
    cdf = ndtr(zu)
    h = pdf + zu * cdf
    log_h[up], phi_r[up], pdf_r[up] = np.log(h), cdf / h, pdf / h
    t = -z[~up]
    mills = np.sqrt(np.pi / 2.0) * erfcx(t / _SQRT2)
    q = 1.0 - t * mills
    far = t >= 10.0
    if np.any(far):
        r = 1.0 / (t[far] * t[far])
        term, acc = r.copy(), r.copy()
        for k in range(1, 48):
            term = term * (-(2 * k + 1)) * r
            acc = acc + term
        q[far] = acc
    log_h[~up] = -0.5 * t * t - _HALF_LOG_2PI + np.log(q)
    phi_r[~up], pdf_r[~up] = mills / q, 1.0 / q
    return log_h, phi_r, pdf_r


def host_value_and_grad(name, mean, var, dmean, dvar, varsigma=0.0, incumbent=0.0, xi=0.0):
    """Value [M] and gradient [M, D] of "ucb_std", "ei" or "logei" from ``gp_predict_grad``'s four outputs (chain rule:
    dEI = Phi dmean + phi dsigma, dlogEI = (Phi dmean + phi dsigma) / (sigma h), dsigma = dvar / (2 sigma))."""
    sigma = np.sqrt(np.maximum(var, np.finfo(np.float64).tiny))
    dsigma = dvar / (2.0 * sigma)[:, None]
    if name == "ucb_std":
        return mean + varsigma * sigma, dmean + varsigma * dsigma
    z = (mean - incumbent - xi) / sigma
    log_h, phi_r, pdf_r = h_parts(z)
    dlog = (phi_r[:, None] * dmean + pdf_r[:, None] * dsigma) / sigma[:, None]
    log_ei = np.log(sigma) + log_h
    if name == "logei":
        return log_ei, dlog
    ei = np.exp(log_ei)
    return ei, ei[:, None] * dlog
