"""
Outcome constraints (NOT in the reference): what a user says about them.

A simulation often returns more than a score -- a firing rate that must stay within range, a run time under a budget.
``Constraint`` names one such output and the bound it must keep; the surrogate models every constrained output with a GP of
its own and ``ConstrainedAcq`` says how the probability that the latent constraint functions are satisfied enters the
ranking of a leaf (Gardner et al. 2014; Gelbart, Snoek & Adams 2014):

* ``"gate"``         the acquisition's own value where P(feasible) >= ``pof_min``, -inf otherwise: score units are kept, so
                     this is the mode that may drive the optimiser's loop
* ``"weight"``       EI and PI times P(feasible), log-EI plus its logarithm; leaves below ``pof_min`` get -inf
* ``"feasibility"``  log P(feasible) alone: the rule to use while no feasible point is known
"""
from __future__ import annotations

import numpy as np

from . import _lib as L

MODES = tuple(L.CON_MODES)


class Constraint:
    """``Constraint("rate", upper=40.0)``: feasible where the output is <= 40; ``lower=``: where it is >= the bound.
    Exactly one of the two (an interval is two constraints on the same output)."""

    def __init__(self, name, upper=None, lower=None):
        if (upper is None) == (lower is None):
            raise ValueError(f"Constraint {name!r}: exactly one of upper= and lower= (an interval is two constraints)")
        bound = float(upper if upper is not None else lower)
        if not np.isfinite(bound):
            raise ValueError(f"Constraint {name!r}: the bound must be finite, not {bound}")
        self.name = str(name)
        self.threshold = bound
        self.sense = 1 if upper is not None else -1

    @property
    def upper(self):
        return self.threshold if self.sense == 1 else None

    @property
    def lower(self):
        return self.threshold if self.sense == -1 else None

    def satisfied(self, values):
        """Elementwise: do observed values of this output keep the bound?"""
        values = np.asarray(values, dtype=np.float64)
        return values <= self.threshold if self.sense == 1 else values >= self.threshold

    def __repr__(self):
        return f"Constraint({self.name!r}, {'upper' if self.sense == 1 else 'lower'}={self.threshold})"


class ConstrainedAcq:
    """An acquisition (a spec or a name of ``pygpso_amd.acquisition``) under constraints: ``mode`` and the smallest
    probability of feasibility ``pof_min`` a leaf may have (0: no gate)."""

    def __init__(self, acq, mode="gate", pof_min=0.5):
        if mode not in L.CON_MODES:
            raise ValueError(f"mode must be one of {MODES}, not {mode!r}")
        pof_min = float(pof_min)
        if not 0.0 <= pof_min <= 1.0:
            raise ValueError(f"pof_min={pof_min}: a probability")
        self.acq = acq
        self.mode = mode
        self.pof_min = pof_min

    @property
    def log_pof_min(self):
        return float(np.log(self.pof_min)) if self.pof_min > 0.0 else -np.inf

    def __repr__(self):
        return f"ConstrainedAcq({self.acq!r}, mode={self.mode!r}, pof_min={self.pof_min})"


def feasible_rows(constraints, values):
    """[n] bool: the rows of ``values [n, J]`` (observed constraint outputs) that keep every bound."""
    values = np.atleast_2d(np.asarray(values, dtype=np.float64))
    ok = np.ones(values.shape[0], dtype=bool)
    for i, c in enumerate(constraints):
        ok &= c.satisfied(values[:, i])
    return ok
