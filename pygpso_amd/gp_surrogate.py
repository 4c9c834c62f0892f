"""
GP surrogate of the objective surface -- the drop-in boundary of the hot path.

Mirrors the reference's operator interface (names, argument meaning, error behaviour):

* ``GPPoint`` .............. gpso/gp_surrogate.py:24-36
* ``GPListOfPoints`` ....... gpso/gp_surrogate.py:39-118  (1e-12 L2 duplicate rule)
* ``GPSurrogate`` .......... gpso/gp_surrogate.py:121-385 (append / gp_predict / gp_eval_best_ucb /
                             gp_update / properties)
* ``GPRSurrogate`` ......... gpso/gp_surrogate.py:388-533 (exact GP regression; ``_gp_train``)

What differs is underneath: ``gpflow_model`` is a ``HipGPR`` whose training loss, gradient and
``predict_y`` run as HIP kernels on the MI355X (pygpso_amd/csrc), the point store answers the
duplicate queries with one vectorised pass over a coordinate array instead of a Python scan, and
``gp_eval_best_ucb_grow`` scores whole ternary sub-trees without materialising them on the host.
``VGPSurrogate`` (gpso/gp_surrogate.py:536-699) keeps a ``HipVGP``: natural-gradient steps on q and the
hyper-parameter steps of ``Adam`` (or ``Scipy``) run on the device, and its predictive goes through the same kernels.
"""
from __future__ import annotations

import json
import logging
import os
from collections import namedtuple

import math

import numpy as np
import scipy.optimize
from scipy.special import erfcinv

from .kernels import KERNEL_CLASSES, Adam, Constant, Gaussian, Kernel, Matern52, MeanFunction, Scipy, StudentT, Zero, _LbfgsbSearch
from .acquisition import host_value_and_grad, resolve as resolve_acquisition, score_unit_spec
from .model import HipGPR, _standard_normals
from .sgpr import HipSGPR
from .svgp import HipSVGP
from .vgp import HipVGP, carried_order
from .utils import JSON_EXT, PointLabels

DUPLICATE_TOLERANCE = 1.0e-12
NORM_PARAMS_BOUNDS = (0, 1)



class GPPoint(namedtuple("GPPoint", ["normed_coord", "score_mu", "score_sigma", "score_ucb", "label"])):
    """One stored point: normalised coordinates, mean score, VARIANCE (the field is called
    score_sigma in the reference but holds the variance, gpso/gp_surrogate.py:305), UCB, label.
    Equality compares the coordinate arrays element-wise."""

    __slots__ = ()

    def __eq__(self, other):
        if not isinstance(other, tuple) or len(other) != len(self):
            return False
        return bool(np.array_equal(self[0], other[0])) and tuple(self[1:]) == tuple(other[1:])

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None


_NONE = []


class GPListOfPoints(list):
    """List of ``GPPoint`` whose ``append`` de-duplicates by coordinates.

    Same observable behaviour as the reference: a new point within 1e-12 (L2) of stored points
    replaces every such point that is not ``evaluated`` and is not appended; the constructor does
    not de-duplicate.  ``append`` additionally RETURNS the index the point now lives at (first
    duplicate, or the new last position)."""

    # The index hashes a PROJECTION w.x of the coordinates, bucket width 1e-6: two points closer than the duplicate
    # tolerance (1e-12, L2) differ by at most |w| x 1e-12 < 1.5e-12 in it, so a duplicate of x can only sit in the bucket of
    # w.x or one of its two neighbours.  (Rounds 1-5 hashed coordinate 0 alone: the centres of a ternary tree share their
    # first coordinate -- in D = 12 the tree splits other dimensions for a long time --, nearly every point fell into ONE
    # bucket and a look-up scanned the whole list in Python: 250 us per look-up at 1 000 points, O(P^2) per gp_update.  With
    # w_i = 1 / sqrt(i-th prime) distinct grid points have distinct projections.)
    _BUCKET = 1.0e-6
    _PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107,
               109, 113, 127, 131, 137, 139, 149, 151, 157, 163, 167, 173, 179, 181, 191, 193, 197, 199, 211, 223, 227, 229,
               233, 239, 241, 251, 257, 263, 269, 271, 277, 281, 283, 293, 307, 311)
    _W = tuple(1.0 / math.sqrt(p) for p in _PRIMES)  # |w|^2 = sum 1 / p < 2.1 over these 64

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        assert all(isinstance(p, GPPoint) for p in self)
        self._rows = []      # coordinates of self[i] as a tuple of Python floats
        self._dirty = True
        self._buckets = {}   # bucket of the projection -> indices (ascending)
        # every point came in through append(): no two stored points lie within the duplicate tolerance of each other (the
        # constructor does not de-duplicate, list surgery may break it: cleared by anything but append / score updates)
        self._unique = len(self) == 0
        # known variance of a stored point's score (the variance of a mean of repeated evaluations), beside the five-field
        # GPPoint: keyed by the point's coordinate row, as the index above is; a point without an entry has variance 0
        self._noise = {}
        self.noise_given = False  # was a variance ever stored (``current_training_noise`` is None until then)
        # observed values of the constrained outputs of an evaluated point (``GPRSurrogate(constraints=...)``), kept the same
        # way: keyed by the point's coordinate row, empty unless constraints are in use
        self._cvals = {}
        # evaluated points whose objective returned no finite score (``GPRSurrogate(failures="classify")``), kept the same
        # way: the coordinate rows of the failed ones, empty unless failures are in use
        self._failed = set()
        if args and isinstance(args[0], GPListOfPoints):  # (a copy of a store keeps its variances)
            self._noise = dict(args[0]._noise)
            self.noise_given = args[0].noise_given
            self._cvals = dict(args[0]._cvals)
            self._failed = set(args[0]._failed)

    # -- failed evaluations (parallel store) ----------------------------------------------------------
    def mark_failed_at(self, index):
        """The evaluation of the point stored at ``index`` returned no finite score."""
        self._index()
        self._failed.add(self._rows[index])

    def failed_mask(self, label=None):
        """[n] bool over the stored points (of ``label`` only when given), in list order: was the evaluation a failure?"""
        if not self._failed:
            return np.zeros(sum(1 for p in self if label is None or p.label == label), dtype=bool)
        self._index()
        return np.array([self._rows[i] in self._failed for i, p in enumerate(self) if label is None or p.label == label], dtype=bool)

    # -- observed constraint outputs (parallel store) -------------------------------------------------
    def set_constraint_values_at(self, index, values):
        """The J observed constraint outputs of the point stored at ``index``."""
        values = tuple(float(v) for v in np.asarray(values, dtype=np.float64).reshape(-1))
        if not all(math.isfinite(v) for v in values):
            raise ValueError(f"constraint values {values} must be finite")
        self._index()
        self._cvals[self._rows[index]] = values

    def constraint_values_at(self, index):
        self._index()
        return self._cvals.get(self._rows[index])

    def constraint_matrix(self, label=None):
        """[n, J] observed constraint outputs of the stored points (of ``label`` only when given), in list order; a point
        without an entry raises (every evaluated point of a constrained run has one)."""
        self._index()
        rows = [self._cvals.get(self._rows[i]) for i, p in enumerate(self) if label is None or p.label == label]
        if any(r is None for r in rows):
            raise ValueError("an evaluated point has no constraint values: append(coords, scores, constraint_values=...) stores them")
        return np.array(rows, dtype=np.float64).reshape(len(rows), -1)

    # -- per-point score variances (parallel store) ---------------------------------------------------
    def set_noise_at(self, index, variance):
        """The score variance of the point stored at ``index``."""
        variance = float(variance)
        if not (math.isfinite(variance) and variance >= 0.0):
            raise ValueError(f"score variance {variance} must be finite and >= 0")
        self._index()
        self._noise[self._rows[index]] = variance
        self.noise_given = True

    def noise_at(self, index):
        self._index()
        return self._noise.get(self._rows[index], 0.0)

    def noise_by_coords(self, coords):
        """The stored variance of the point within the duplicate tolerance of ``coords`` (0.0: none stored, or no such point)."""
        i = self.find_index_by_coords(coords)
        return 0.0 if i is None else self._noise.get(self._rows[i], 0.0)

    def noise_vector(self, label=None):
        """Variances of the stored points (of ``label`` only when given), in list order."""
        self._index()
        get, rows = self._noise.get, self._rows
        return np.array([get(rows[i], 0.0) for i, p in enumerate(self) if label is None or p.label == label], dtype=np.float64)

    def save_noise(self, filename):
        """One variance per stored point, in list order -- written only when some variance is non-zero.  A store without any
        leaves the folder as it always was: nothing is written, and a file an earlier save left there is REMOVED (it would
        otherwise be read back beside points it no longer describes).  So a store that was only ever given zero variances
        loads as one that was given none (``current_training_noise`` None instead of zeros: the same model).  Returns True
        when written."""
        if not filename.endswith(JSON_EXT):
            filename += JSON_EXT
        values = self.noise_vector()
        if not np.any(values != 0.0):
            if os.path.exists(filename):
                os.remove(filename)
            return False
        with open(filename, "w") as fh:
            fh.write(json.dumps(values.tolist()))
        return True

    def load_noise(self, filename):
        """Read what ``save_noise`` wrote beside this list's points file; a missing file is a store without variances."""
        if not filename.endswith(JSON_EXT):
            filename += JSON_EXT
        if not os.path.exists(filename):
            return False
        with open(filename) as fh:
            values = json.load(fh)
        if len(values) != len(self):
            raise ValueError(f"{filename}: {len(values)} variances for {len(self)} points")
        for i, v in enumerate(values):
            if v != 0.0:
                self.set_noise_at(i, v)
        self.noise_given = True
        return True

    # -- index kept in sync ------------------------------------------------------------------------
    # (plain Python floats on purpose: a look-up touches one or two candidate rows of D numbers, and the
    # fixed cost of any numpy call is larger than that whole computation)
    def _index(self):
        if self._dirty or len(self._rows) != len(self):
            self._rows = [tuple(np.asarray(p.normed_coord, dtype=np.float64).reshape(-1).tolist()) for p in self]
            self._buckets = {}
            for i, r in enumerate(self._rows):
                self._buckets.setdefault(self._bucket_of(r), []).append(i)
            self._dirty = False

    @classmethod
    def _bucket_of(cls, row):
        """bucket of the projection w.row (dimensions beyond the 64 weights wrap around: still a valid projection)"""
        w = cls._W
        if len(row) <= len(w):
            proj = sum(a * b for a, b in zip(row, w))
        else:
            proj = sum(a * w[i % len(w)] for i, a in enumerate(row))
        return int(math.floor(proj / cls._BUCKET))

    def _matches(self, coords):
        """Indices (ascending) of the stored points within the duplicate tolerance of ``coords`` --
        the reference's linear scan (gpso/gp_surrogate.py:68-101), answered from a hash on the first
        coordinate: candidates come from three buckets, the exact distance test decides."""
        self._index()
        if not self._rows:
            return []
        c = np.asarray(coords, dtype=np.float64).reshape(-1).tolist()
        b = self._bucket_of(c)
        get = self._buckets.get
        cand = get(b - 1, _NONE) + get(b, _NONE) + get(b + 1, _NONE)
        if not cand:
            return []
        if len(cand) > 1:
            cand = sorted(cand)
        rows, hits = self._rows, []
        for i in cand:
            d2 = 0.0
            for a, x in zip(rows[i], c):
                t = a - x
                d2 += t * t
            if math.sqrt(d2) < DUPLICATE_TOLERANCE:
                hits.append(i)
        return hits

    def __setitem__(self, idx, value):
        super().__setitem__(idx, value)
        self._unique = False  # (arbitrary surgery: the store can no longer vouch for uniqueness; append() keeps it itself)
        n = len(self._rows)
        if isinstance(idx, int) and not self._dirty and n == len(self) and -n <= idx < n:
            i = idx % n
            row = tuple(np.asarray(value.normed_coord, dtype=np.float64).reshape(-1).tolist())
            old_b, new_b = self._bucket_of(self._rows[i]), self._bucket_of(row)
            self._rows[i] = row
            if old_b != new_b:
                self._buckets[old_b].remove(i)
                self._buckets.setdefault(new_b, []).append(i)
        else:
            self._dirty = True

    # -- reference API ----------------------------------------------------------------------------
    def append(self, point):
        assert isinstance(point, GPPoint)
        hits = self._matches(point.normed_coord)
        if hits:
            unique = self._unique
            for i in hits:
                if self[i].label != PointLabels.evaluated:
                    self[i] = point
            self._unique = unique  # (a point replaced by one within the tolerance of it: uniqueness is kept)
            return hits[0]
        n = len(self)
        super().append(point)
        if not self._dirty and len(self._rows) == n:
            row = tuple(np.asarray(point.normed_coord, dtype=np.float64).reshape(-1).tolist())
            self._rows.append(row)
            self._buckets.setdefault(self._bucket_of(row), []).append(n)
        else:
            self._dirty = True
        return n

    def update_scores(self, indices, mean, var, varsigma, score=None):
        """New (mean, var, ucb) for the points at ``indices``, coordinates and labels kept -- what re-appending a point with
        the SAME coordinates does (it overwrites its own entry), without the look-up.  Only valid while no two stored points
        are duplicates of each other (``_unique``); returns False otherwise and changes nothing."""
        if not self._unique:
            return False
        setitem = list.__setitem__
        for i, m, v in zip(indices, mean, var):
            p = self[i]
            m, v = float(m), float(v)
            u = float(m + varsigma * v) if score is None else score(m, v)  # (score: the surrogate's rule when it is not the reference's)
            setitem(self, i, GPPoint(p.normed_coord, m, v, u, p.label))  # (coordinates unchanged: the index stays valid)
        return True

    def find_index_by_coords(self, coords):
        hits = self._matches(coords)
        return hits[0] if hits else None

    def find_by_coords(self, coords):
        i = self.find_index_by_coords(coords)
        return None if i is None else self[i]

    # -- persistence (same JSON schema as the reference, gpso/gp_surrogate.py:103-118) ------------
    def save(self, filename):
        if not filename.endswith(JSON_EXT):
            filename += JSON_EXT
        rows = []
        for p in self:
            rows.append({
                "normed_coord": np.asarray(p.normed_coord).tolist(),
                "score_mu": float(p.score_mu),
                "score_sigma": float(p.score_sigma),
                "score_ucb": float(p.score_ucb),
                "label": p.label.name,
            })
        with open(filename, "w") as fh:
            fh.write(json.dumps(rows))

    @classmethod
    def from_file(cls, filename):
        if not filename.endswith(JSON_EXT):
            filename += JSON_EXT
        with open(filename) as fh:
            rows = json.load(fh)
        return cls([
            GPPoint(np.array(r["normed_coord"]), r["score_mu"], r["score_sigma"], r["score_ucb"],
                    PointLabels[r["label"]])
            for r in rows
        ])


def _invalidating(name):
    base = getattr(list, name)

    def method(self, *args, **kwargs):
        self._dirty = True
        self._unique = False
        return base(self, *args, **kwargs)

    method.__name__ = name
    return method


for _name in ("extend", "insert", "pop", "remove", "clear", "sort", "reverse", "__delitem__", "__iadd__"):
    setattr(GPListOfPoints, _name, _invalidating(_name))
del _name


def polish_lockstep(value_and_grad, starts, lower, upper, options=None):
    """R bounded L-BFGS-B searches (``kernels._LbfgsbSearch``) that MAXIMISE a function, advanced side by side: each round
    the points the live searches wait at are stacked and evaluated by one ``value_and_grad(X [P, D]) -> (value [P],
    grad [P, D])`` call.  ``starts``, ``lower``, ``upper``: [R, D].  Returns one ``scipy.optimize.OptimizeResult`` per start
    (``x``: the end point, ``fun``: minus the value there).  With a SciPy whose private routine has another signature the
    starts go one after another through ``scipy.optimize.minimize(method="L-BFGS-B", bounds=...)``, as ``kernels.Scipy``
    falls back: the same answers, one evaluation per call."""
    names = {"maxiter": "maxiter", "maxfun": "maxfun", "gtol": "pgtol", "maxls": "maxls"}
    for key in (options or {}):
        if key != "ftol" and key not in names:
            raise ValueError(f"polish: unknown option {key!r}")
    setulb = _LbfgsbSearch.routine()
    if setulb is None:
        def one(x):
            value, grad = value_and_grad(np.asarray(x, dtype=np.float64)[np.newaxis, :])
            return -float(value[0]), -np.asarray(grad[0], dtype=np.float64)

        return [scipy.optimize.minimize(one, np.clip(s, lo, up), jac=True, method="L-BFGS-B", bounds=list(zip(lo, up)),
                                        options=dict(options or {}))
                for s, lo, up in zip(starts, lower, upper)]
    searches = [_LbfgsbSearch(setulb, s, lower=lo, upper=up) for s, lo, up in zip(starts, lower, upper)]
    for key, val in (options or {}).items():
        for s in searches:
            if key == "ftol":
                s.factr = float(val) / np.finfo(float).eps
            else:
                setattr(s, names[key], type(getattr(s, names[key]))(val))
    live = list(range(len(searches)))
    while live:
        pending = [(i, searches[i].advance()) for i in live]
        pending = [(i, x) for i, x in pending if x is not None]
        live = [i for i, _ in pending]
        if pending:
            value, grad = value_and_grad(np.stack([x for _, x in pending]))
            for (i, _), v, g in zip(pending, value, grad):
                searches[i].feed(-float(v), -np.asarray(g, dtype=np.float64))
    return [s.result() for s in searches]


class GPSurrogate:
    """Base class: point bookkeeping + predict/UCB on top of ``self.gpflow_model``."""

    POINTS_FILE = f"points{JSON_EXT}"
    POINTS_NOISE_FILE = f"points_noise{JSON_EXT}"  # (beside the points file, only when some score variance is non-zero)
    GPR_FILE = f"GPRmodel{JSON_EXT}"
    GPR_INFO = f"GPRinfo{JSON_EXT}"

    @classmethod
    def from_saved(cls, folder):
        raise NotImplementedError

    def __init__(self, gp_kernel, gp_meanf=None, optimiser=None, varsigma=erfcinv(0.01), points=None,
                 gpflow_model=None, dtype="float64", device=0, engine_options=None, devices=None,
                 gp_acquisition="ucb_var"):
        """
        :param gp_kernel: kernel spec (``pygpso_amd.kernels.Matern52(...)`` etc.)
        :param gp_meanf: mean-function spec (``Constant(c)``) or None
        :param optimiser: object with ``minimize(closure, variables)``; default ``Scipy()`` (L-BFGS-B)
        :param varsigma: UCB = mean + varsigma * VAR (gpso/gp_surrogate.py:150-155,326)
        :param points: initial list of ``GPPoint``
        :param gpflow_model: an initialised ``HipGPR`` (used when loading a saved surrogate)
        :param dtype: arithmetic of the device kernels: "float64" (the reference's; parity), "mixed"
            (fit in float64, predictions in float32 / split bf16) or "float32" (everything in float32).
            Float predictions are guarded by a self-test; a model whose posterior fails it moves to the
            next more precise arithmetic on the device by itself (``HipGPR``).
        :param device: HIP device index
        :param devices: several HIP device indices: the fit runs on the first, every leaf-UCB / predict
            call is sharded over all of them (RCCL behind the C-ABI, ``HipGPEngineGroup``); results are
            bit-identical to a single device's
        :param engine_options: extra ``HipGPEngine`` keyword arguments (predict_math, generation, ...)
        :param gp_acquisition: what the loop ranks leaves by: "ucb_var" (the reference's mean + varsigma * VAR, the
            default) or "ucb_std" (GP-UCB, mean + varsigma * sqrt(VAR)).  Only these are in score units --
            ``GPSOptimiser._tree_select`` compares a leaf's value with evaluated scores --; "ei", "logei" and "pi" raise
            ValueError here and are served by ``gp_eval_best_acq`` / ``gp_acq_values`` / ``polish``
        """
        self.gpflow_model = gpflow_model
        self.gp_varsigma = float(varsigma)
        self.gp_acquisition = score_unit_spec(gp_acquisition, self.gp_varsigma).name
        assert isinstance(gp_kernel, Kernel)
        self.gp_kernel = gp_kernel
        assert gp_meanf is None or isinstance(gp_meanf, MeanFunction)
        self.gp_meanf = gp_meanf
        optimiser = optimiser if optimiser is not None else Scipy()
        assert hasattr(optimiser, "minimize")
        self.optimiser = optimiser
        self.dtype = dtype
        self.devices = [int(v) for v in devices] if devices is not None else None
        self.device = self.devices[0] if self.devices else device
        self.engine_options = dict(engine_options or {})
        self.points = GPListOfPoints(points or list())

    # -- bookkeeping properties (gpso/gp_surrogate.py:174-257) -----------------------------------
    def _with_label(self, label):
        return [p for p in self.points if p.label == label]

    @property
    def num_evaluated(self):
        return len(self._with_label(PointLabels.evaluated))

    @property
    def num_gp_based(self):
        return len(self._with_label(PointLabels.gp_based))

    @property
    def highest_score(self):
        cand = self._with_label(PointLabels.evaluated)
        if cand:
            return max(cand, key=lambda p: p.score_mu)  # max() keeps the first of equal maxima

    @property
    def highest_ucb(self):
        cand = self._with_label(PointLabels.gp_based)
        if cand:
            return max(cand, key=lambda p: p.score_ucb)

    @property
    def current_training_data(self):
        ev = self._with_label(PointLabels.evaluated)
        return np.array([p.normed_coord for p in ev]), np.array([p.score_mu for p in ev])

    @property
    def current_training_noise(self):
        """Known variance of each evaluated point's score, [N] aligned with ``current_training_data`` (zeros where none was
        given); None when none was ever given."""
        if not self.points.noise_given:
            return None
        return self.points.noise_vector(PointLabels.evaluated)

    def _refuse_score_variances(self, s):
        """The variational and sparse surrogates model one shared noise variance: they refuse non-zero score variances."""
        if s is not None and np.any(np.asarray(s) != 0.0):
            raise NotImplementedError(f"per-point observation noise (score_vars / eval_repeats_noise) is only modelled by "
                                      f"GPRSurrogate, not by {type(self).__name__}")

    @property
    def gp_based_coords(self):
        return np.array([p.normed_coord for p in self._with_label(PointLabels.gp_based)])

    # -- training-data intake ----------------------------------------------------------------------
    def _gp_train(self, x, y):
        raise NotImplementedError

    def append(self, coords, scores, score_vars=None):
        """Store evaluated points (normalised coordinates [n, D], scores [n]).  ``score_vars`` [n] >= 0 (not in the
        reference): the known variance of each score, kept beside the points and modelled as per-point observation noise."""
        assert coords.ndim == 2
        assert scores.ndim == 1
        assert coords.shape[0] == scores.shape[0]
        if score_vars is None:
            for c, s in zip(coords, scores):
                self.points.append(GPPoint(c, s, 0.0, 0.0, PointLabels.evaluated))
            return
        score_vars = np.asarray(score_vars, dtype=np.float64)
        assert score_vars.ndim == 1 and score_vars.shape[0] == scores.shape[0]
        if not (np.all(np.isfinite(score_vars)) and np.all(score_vars >= 0.0)):
            raise ValueError("score_vars must be finite and >= 0")
        self.points.noise_given = True
        for c, s, v in zip(coords, scores, score_vars):
            point = GPPoint(c, s, 0.0, 0.0, PointLabels.evaluated)
            i = self.points.append(point)
            if self.points[i] is point:  # (an evaluated duplicate keeps its score, and so its variance)
                self.points.set_noise_at(i, v)

    # -- predict / UCB ------------------------------------------------------------------------------
    def _acquisition_record(self):
        """What ``save`` adds to the surrogate's record: nothing for the default rule (its files stay what they were)."""
        return {} if self.gp_acquisition == "ucb_var" else {"gp_acquisition": self.gp_acquisition}

    def _loop_acquisition(self):
        return resolve_acquisition(self.gp_acquisition, varsigma=self.gp_varsigma)

    def _score_ucb(self, m, v):
        """The stored ``score_ucb`` of a point with predictive mean ``m`` and variance ``v`` (Python floats)."""
        if self.gp_acquisition == "ucb_var":
            return float(m + self.gp_varsigma * v)
        return float(self._loop_acquisition().host_value(m, v))

    def _require_model(self):
        assert isinstance(self.gpflow_model, HipGPR), "GP model not trained yet"

    def gp_predict(self, normed_coords):
        """predict_y at ``normed_coords`` and store every row as a gp_based point."""
        self._require_model()
        mean, var = self.gpflow_model.predict_y(normed_coords)
        for i in range(normed_coords.shape[0]):
            m, v = float(mean[i, 0]), float(var[i, 0])
            self.points.append(GPPoint(normed_coords[i, :], m, v, self._score_ucb(m, v), PointLabels.gp_based))

    def gp_predict_grad(self, normed_coords):
        """predict_y and its gradients in normed coordinates at the rows of ``normed_coords``: (mean [M], var [M],
        dmean [M, D], dvar [M, D]); stores nothing.  One ``gpso_predict_grad`` call (not in the reference, where it would
        be a tf.GradientTape around predict_y).  A multi-GPU engine group raises NotImplementedError."""
        self._require_model()
        from .distributed import HipGPEngineGroup

        if isinstance(self.gpflow_model.engine, HipGPEngineGroup):
            raise NotImplementedError("gp_predict_grad / polish: not offered on a multi-GPU engine group")
        return self.gpflow_model.predict_y_grad(np.ascontiguousarray(normed_coords, dtype=np.float64))

    def _joint_model(self, what):
        self._require_model()
        from .distributed import HipGPEngineGroup

        if isinstance(self.gpflow_model.engine, HipGPEngineGroup):
            raise NotImplementedError(f"{what}: not offered on a multi-GPU engine group")
        return self.gpflow_model

    def gp_predict_joint(self, normed_coords, noise=False):
        """The JOINT predictive at the rows of ``normed_coords`` (M <= 1024): (mean [M], cov [M, M]) of the latent f, or
        of y (``noise=True``: the model's predictive noise on the diagonal); stores nothing.  One ``gpso_predict_joint``
        call -- GPflow's ``predict_f(full_cov=True)`` on the reference's model."""
        model = self._joint_model("gp_predict_joint")
        coords = np.ascontiguousarray(normed_coords, dtype=np.float64)
        mean, cov = model.predict_y(coords, full_cov=True) if noise else model.predict_f(coords, full_cov=True)
        return np.asarray(mean)[:, 0], cov

    def _draw(self, model, normed_coords, n_draws, rng, diag_add, want_samples):
        coords = np.ascontiguousarray(normed_coords, dtype=np.float64)
        z = _standard_normals(rng, n_draws, coords.shape[0])
        return model._predicting(lambda: model.engine.sample_joint(coords, z, diag_add, want_samples=want_samples))

    def gp_sample(self, normed_coords, n_draws, rng=None, noise=False, jitter=1e-6):
        """``n_draws`` draws [S, M] from the joint posterior at the rows of ``normed_coords`` (M <= 1024): of the latent f,
        or of y (``noise=True``).  ``rng``: a seed or a ``numpy.random.Generator`` (the normals are drawn on the host);
        ``jitter`` is added to the diagonal before the Cholesky, as GPflow's ``predict_f_samples`` adds its default_jitter.
        Stores nothing."""
        model = self._joint_model("gp_sample")
        diag_add = jitter + (model.predictive_noise() if noise else 0.0)
        return self._draw(model, normed_coords, n_draws, rng, diag_add, True)[0]

    def thompson_select(self, normed_coords, n_draws, rng=None, jitter=1e-6):
        """Thompson sampling over the candidate rows of ``normed_coords`` (M <= 1024): (indices [S], values [S]), the
        arg-max (the first on ties) and the maximum of each of ``n_draws`` latent draws of ``gp_sample`` for the same
        ``rng`` -- S candidates for an evaluation pool in one step rather than S times the same arg-max.  The draws never
        leave the device.  Stores nothing."""
        _, idx, val = self._draw(self._joint_model("thompson_select"), normed_coords, n_draws, rng, jitter, False)
        return idx, val

    def gp_sample_paths(self, n_paths, n_features=1024, rng=None):
        """Draw ``n_paths`` posterior functions of the surrogate (pathwise conditioning, ``HipGPR.sample_paths``) and keep
        them on the device until the model changes.  ``gp_eval_paths`` and ``thompson_select_leaves`` evaluate them at any
        number of rows -- the leaves the optimiser holds, not a hand-picked 1024.  Stores nothing."""
        self._joint_model("gp_sample_paths").sample_paths(n_paths, n_features=n_features, rng=rng)

    def gp_eval_paths(self, normed_coords):
        """The drawn paths at the rows of ``normed_coords``: [S, M].  Stores nothing."""
        coords = np.ascontiguousarray(normed_coords, dtype=np.float64)
        return self._joint_model("gp_eval_paths").eval_paths(coords)[0]

    def thompson_select_leaves(self, normed_coords, seg_off=None):
        """Thompson sampling over ALL the rows of ``normed_coords`` (any M): (indices [S, nseg], values [S, nseg]), per
        drawn path of ``gp_sample_paths`` and per segment of ``seg_off`` (None: one segment) the arg-max relative to the
        segment start (the first on ties) and the maximum.  The values never leave the device.  Stores nothing."""
        coords = np.ascontiguousarray(normed_coords, dtype=np.float64)
        _, idx, val = self._joint_model("thompson_select_leaves").eval_paths(coords, seg_off, want_values=False)
        return idx, val

    def polish(self, normed_coords, objective="ucb", box=None, options=None):
        """Gradient polish of R candidate points on the surrogate: from each row of ``normed_coords`` [R, D], L-BFGS-B
        maximises ``mean + varsigma * var`` (``objective="ucb"``, the package's UCB on the variance) or the mean
        (``"mean"``) inside ``box`` -- the unit cube by default, or [R, D, 2] (lower, upper) per start, one leaf's bounds
        being the intended use.  The R searches advance in lockstep; each round their pending points are ONE
        ``gp_predict_grad`` call, and every search takes the iterates it would take alone.  ``options``: ``maxiter``,
        ``maxfun``, ``gtol``, ``ftol``, ``maxls`` as SciPy's L-BFGS-B names them; ``ftol`` defaults to ten machine epsilons
        here, so a search ends on its projected gradient (``gtol``, 1e-5).  Changes neither the point store nor
        anything saved.  Returns (coords [R, D], mean [R], var [R], value [R], results)."""
        if objective not in ("ucb", "mean", "ucb_std", "ei", "logei"):
            raise ValueError(f"objective={objective!r}: 'ucb', 'mean', 'ucb_std', 'ei' or 'logei'")
        starts = np.array(normed_coords, dtype=np.float64, ndmin=2)
        r, d = starts.shape
        if box is None:
            lower, upper = np.zeros((r, d)), np.ones((r, d))
        else:
            box = np.asarray(box, dtype=np.float64)
            if box.shape != (r, d, 2):
                raise ValueError(f"box has shape {box.shape}, expected {(r, d, 2)}")
            lower, upper = box[:, :, 0], box[:, :, 1]
        weight = self.gp_varsigma if objective == "ucb" else 0.0
        mapped = objective in ("ucb_std", "ei", "logei")  # (the chain rule on the host: acq_value_and_grad)

        def value_and_grad(x):
            if mapped:
                return self.acq_value_and_grad(x, objective)[2:]
            mean, var, dmean, dvar = self.gp_predict_grad(x)
            return mean + weight * var, dmean + weight * dvar

        # (a polish is after the last digits: SciPy's default ftol, 1e7 machine epsilons, would end it on the flat top first)
        opts = {"ftol": 10.0 * np.finfo(float).eps}
        opts.update(options or {})
        results = polish_lockstep(value_and_grad, starts, lower, upper, opts)
        coords = np.stack([np.asarray(r.x, dtype=np.float64) for r in results])
        if mapped:
            mean, var, value, _ = self.acq_value_and_grad(coords, objective)
            return coords, mean, var, value, results
        mean, var, _, _ = self.gp_predict_grad(coords)
        return coords, mean, var, mean + weight * var, results

    def acq_value_and_grad(self, normed_coords, objective, incumbent=None, xi=0.0):
        """(mean [M], var [M], value [M], dvalue [M, D]) of "ucb_std", "ei" or "logei" at the rows of ``normed_coords``: one
        ``gp_predict_grad`` call and the chain rule on the host, the quotients of log-EI in their tail-stable form
        (``pygpso_amd.acquisition.h_parts``).  The incumbent defaults to the largest training target."""
        if objective not in ("ucb_std", "ei", "logei"):
            raise ValueError(f"objective={objective!r}: 'ucb_std', 'ei' or 'logei' (MES has no gradient here: rank leaves with "
                             f"mes_select / gp_eval_best_acq)")
        mean, var, dmean, dvar = self.gp_predict_grad(normed_coords)
        if incumbent is None and objective != "ucb_std":
            incumbent = float(np.max(self.current_training_data[1]))
        value, grad = host_value_and_grad(objective, mean, var, dmean, dvar, varsigma=self.gp_varsigma,
                                          incumbent=incumbent, xi=xi)
        return mean, var, value, grad

    def gp_eval_best_ucb(self, normed_coords):
        """(mean, var, ucb) of the row with the highest ucb = mean + varsigma * var; stores nothing."""
        self._require_model()
        if self.gp_acquisition == "ucb_var":
            _, mean, var, ucb = self.gpflow_model.best_ucb(normed_coords, self.gp_varsigma)
        else:
            _, mean, var, ucb = self.gpflow_model.best_acq(normed_coords, self._loop_acquisition())
        return float(mean[0]), float(var[0]), float(ucb[0])

    def gp_eval_best_acq(self, normed_coords, acquisition, incumbent=None, seg_off=None):
        """Per segment of ``seg_off`` (None: one) the row of ``normed_coords`` with the highest value of ``acquisition`` --
        a name ("ucb_var", "ucb_std", "ei", "logei", "pi", "mes") or a spec of ``pygpso_amd.acquisition``: (idx, mean, var, value)
        arrays, idx relative to the segment start, the first on ties.  EI, log-EI and PI improve on ``incumbent``: by
        default the largest training target, in the units ``_gp_train`` saw.  Stores nothing."""
        self._require_model()
        acq = resolve_acquisition(acquisition, varsigma=self.gp_varsigma)
        if acq.name == "mes":
            self._joint_model("gp_eval_best_acq with MES")
        return self.gpflow_model.best_acq(np.ascontiguousarray(normed_coords, dtype=np.float64), acq, seg_off, incumbent)

    def gp_acq_values(self, normed_coords, acquisition, incumbent=None):
        """(mean [M], var [M], value [M]) of every row of ``normed_coords`` under ``acquisition`` (as
        ``gp_eval_best_acq``); stores nothing."""
        self._require_model()
        acq = resolve_acquisition(acquisition, varsigma=self.gp_varsigma)
        if acq.name == "mes":
            self._joint_model("gp_acq_values with MES")
        return self.gpflow_model.acq_values(np.ascontiguousarray(normed_coords, dtype=np.float64), acq, incumbent)

    def max_value_samples(self, normed_coords, k=16, method="paths", rng=None, n_features=1024):
        """``k`` samples of the optimum's value over the rows of ``normed_coords``, in the units ``_gp_train`` saw
        (``HipGPR.max_value_samples``): ``method="paths"`` -- the maxima of ``k`` drawn posterior functions (replaces a
        path set of ``gp_sample_paths``) -- or ``"gumbel"`` -- a Gumbel law fitted to the independent-leaves law of the
        maximum.  Both are clamped from below at the largest training target.  Stores nothing."""
        model = self._joint_model("max_value_samples")
        return model.max_value_samples(np.ascontiguousarray(normed_coords, dtype=np.float64), k=k, method=method, rng=rng,
                                       n_features=n_features)

    def mes_select(self, normed_coords, k=16, method="paths", rng=None, seg_off=None):
        """Max-value entropy search over the rows of ``normed_coords``: ``k`` samples of the optimum's value
        (``max_value_samples``, over ALL the rows), then per segment of ``seg_off`` (None: one) the row that tells most
        about it -- ``acquisition.MES`` on the latent variance, one ``gpso_best_acq`` call.  Returns (idx, mean, var,
        value) as ``gp_eval_best_acq``; the samples stay installed on the engine (``acq_get_maxima``).  Stores nothing."""
        from .acquisition import MES

        coords = np.ascontiguousarray(normed_coords, dtype=np.float64)
        maxima = self.max_value_samples(coords, k=k, method=method, rng=rng)
        return self.gpflow_model.best_acq(coords, MES(latent=True, maxima=maxima), seg_off)

    def gp_cross_cov(self, a, b):
        """The latent posterior covariance [B, M] between the M rows of ``a`` and the B <= 64 rows of ``b`` (normed
        coordinates): one ``gpso_cross_cov`` call; stores nothing."""
        model = self._joint_model("gp_cross_cov")
        return model.cross_cov(np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64))

    def select_batch(self, normed_coords, q, acquisition=None, incumbent=None, return_var_after=False):
        """``q`` different rows of ``normed_coords`` to evaluate at once -- a pool of workers -- by greedy selection under
        hallucinated updates (GP-BUCB, "kriging believer"; one ``gpso_best_batch`` call): the best row, then the best once
        that row counts as observed at its posterior mean with the model's predictive noise, and so on.  ``acquisition``:
        as ``gp_eval_best_acq``; None: the surrogate's own (``gp_acquisition``, by default the reference's mean +
        varsigma * var).  Returns (indices, mean, var, value) of the picks -- fewer than ``q`` when the rows run out or a
        value is NaN --: ``var`` is the predictive variance a pick was ranked by, given the earlier picks; with
        ``return_var_after`` a fifth entry holds the predictive variance of every row after all of them.  The first index
        is ``gp_eval_best_acq``'s.  Stores nothing; a multi-GPU engine group raises NotImplementedError."""
        model = self._joint_model("select_batch")
        acq = self._loop_acquisition() if acquisition is None else resolve_acquisition(acquisition, varsigma=self.gp_varsigma)
        return model.best_batch(np.ascontiguousarray(normed_coords, dtype=np.float64), acq, q, incumbent=incumbent,
                                want_var_after=return_var_after)

    def select_batch_mc(self, normed_coords, q, kind="qnei", n_paths=64, n_features=1024, rng=None, incumbent=None, pending=None,
                        xi=0.0, return_gain0=False):
        """``q`` different rows of ``normed_coords`` for a pool of workers by the Monte-Carlo batch acquisition over
        posterior draws (one ``gpso_paths_best_batch`` call): the sample-average qNoisyEI (``kind="qnei"``), qEI
        (``"qei"``) or qPI (``"qpi"``) over the drawn paths, picked by sequential greedy selection over those fixed
        draws.  Unlike ``select_batch`` a pick moves the means: a draw in which the pick is high raises that draw's bar.
        A path set is drawn (``n_paths``, ``n_features``, ``rng`` as ``gp_sample_paths``) unless a valid one is
        resident.  The bars: for "qnei" each draw's own maximum over the evaluated points (one ``eval_paths`` call, the
        values stay on the device) -- no observed score enters --; for "qei" / "qpi" ``incumbent``, by default the best
        evaluated score.  ``pending`` [B, D]: points still being evaluated; they raise the bars and are never returned.
        Returns (indices, gain, batch_value) of the picks -- fewer than ``q`` when no draw can improve any more --, in
        the paths' latent units; with ``return_gain0`` a fourth entry holds every row's round-0 gain, at ``q = 1`` the
        plain sample-average EI / PI of each row.  Stores nothing; a multi-GPU engine group raises NotImplementedError."""
        if kind not in ("qnei", "qei", "qpi"):
            raise ValueError(f"kind={kind!r}: 'qnei', 'qei' or 'qpi'")
        model = self._joint_model("select_batch_mc")
        coords = np.ascontiguousarray(normed_coords, dtype=np.float64)
        if model._predicting(lambda: model.engine.paths_info())[0] == 0:
            model.sample_paths(n_paths, n_features=n_features, rng=rng)
        bars = None
        if kind == "qnei":
            x_train, _ = self.current_training_data
            bars = np.asarray(model.eval_paths(np.ascontiguousarray(x_train, dtype=np.float64), want_values=False)[2])[:, 0]
        elif incumbent is None:
            incumbent = float(np.max(self.current_training_data[1]))
        return model.mc_batch(coords, q, kind, incumbent=incumbent if bars is None else None, incumbent_s=bars, pending=pending, xi=xi,
                              want_gain0=return_gain0)

    def gp_eval_best_ucb_grow(self, leaf_bounds, depth):
        """MI355X path of ``gp_eval_best_ucb(leaf.grow(depth))`` for several leaves at once: the
        ternary sub-tree centres are generated on the device (bit-identical to ``LeafNode.grow``)
        and never cross PCIe.  ``leaf_bounds``: [nleaf, D, 2].  Returns a list of (mean, var, ucb)."""
        self._require_model()
        bounds = np.asarray(leaf_bounds, dtype=np.float64)
        if self.gp_acquisition == "ucb_var":
            _, mean, var, ucb = self.gpflow_model.best_ucb_grow(bounds, depth, self.gp_varsigma)
        else:
            _, mean, var, ucb = self.gpflow_model.best_acq_grow(bounds, depth, self._loop_acquisition())
        return [(float(m), float(v), float(u)) for m, v, u in zip(mean, var, ucb)]

    def gp_update(self):
        """Retrain on the evaluated points, then re-predict every gp_based point."""
        x_train, y_train = self.current_training_data
        if logging.getLogger().isEnabledFor(logging.DEBUG):  # (formatting the arrays is not free)
            logging.debug(f"Retraining GPR with x data: {x_train}; y data: {y_train}")
        s_train = self.current_training_noise
        if s_train is None:
            self._gp_train(x=x_train, y=y_train[:, np.newaxis])
        else:
            self._gp_train(x=x_train, y=y_train[:, np.newaxis], s=s_train)
        # re-predict every gp-based point.  The reference re-appends them (gpso/gp_surrogate.py:341-342): each overwrites its
        # own entry -- done here by index, one predict call and no look-ups, while the store can vouch that no two points are
        # duplicates of each other; otherwise the reference's way
        idx = [i for i, p in enumerate(self.points) if p.label == PointLabels.gp_based]
        if idx:
            coords = np.array([self.points[i].normed_coord for i in idx])
            if getattr(self.points, "_unique", False):
                mean, var = self.gpflow_model.predict_y(coords)
                score = None if self.gp_acquisition == "ucb_var" else self._score_ucb
                if self.points.update_scores(idx, np.asarray(mean)[:, 0], np.asarray(var)[:, 0], self.gp_varsigma, score):
                    return
            self.gp_predict(coords)

    def save(self, folder):
        raise NotImplementedError


class GPRSurrogate(GPSurrogate):
    """Exact GP regression surrogate (the reference's default)."""

    # hook for tests / multi-GPU: a callable returning the engine object HipGPR should drive
    # (default None -> a HipGPEngine on ``device``; there is no CPU engine in this package)
    engine_factory = None

    def __init__(self, gp_kernel, gp_meanf=None, optimiser=None, varsigma=erfcinv(0.01),
                 gauss_likelihood_sigma=1.0e-3, points=None, gpflow_model=None, dtype="float64",
                 device=0, engine_options=None, devices=None, refit_every=1, refit_guard=2.0, objective="nlml", gp_acquisition="ucb_var",
                 hyper="point", n_theta=16, hyper_priors=None, hyper_seed=0, hyper_options=None,
                 constraints=None, constraint_mode="gate", pof_min=0.5, failures=None, classifier_schedule=None):
        """
        :param failures: None (default: nothing changes -- a non-finite score poisons the fit, as ever) or "classify" (NOT in
            the reference): ``append`` accepts non-finite scores.  Such points are kept with their coordinates and marked
            failed; they never enter the training set of the objective's GP or of a constraint model.  While at least one
            failure is held, ``gp_update`` also trains a GP classifier -- one ``HipVGP`` under the Bernoulli likelihood
            (exact probit) on ALL attempted points, label 0 for a failure and 1 for a finite score, on an engine of its own,
            with deep copies of ``gp_kernel`` and ``gp_meanf`` as given here and q kept across updates -- and installs it as
            the engine's success member (``HipGPR.install_success``).  While the member is resident the routes that go through
            the constrained calls under ``constraints=`` do so here too, in gate mode with ``log_pof_min = log(pof_min)`` on
            the product of the probability of success and, if there are constraints, their probabilities (Gelbart, Snoek &
            Adams 2014).  Before the first failure there is no classifier and no member and every call is the call of
            ``failures=None``.  ``highest_score`` ignores failed points.  N <= 128 attempted points, "float64" / "mixed", one
            GPU, ``refit_every`` = 1, ``hyper="point"``; nothing of it is saved.  ``close_constraint_models()`` also closes the
            classifier's engine
        :param classifier_schedule: how the classifier is trained at every update, a dictionary with the keys ``iterations``
            (natural-gradient step on q, then one optimiser step on theta, that many times), ``natgrad_gamma`` and
            ``optimiser``; None: 10 iterations, gamma 0.5, ``Adam(0.05)`` -- a choice, not a measurement
        :param constraints: a list of ``pygpso_amd.constraints.Constraint`` (NOT in the reference; None, the default: no
            constraints, nothing changes).  The objective returns J further outputs beside the score; ``append`` takes them as
            ``constraint_values`` [n, J] and keeps them beside the points.  ``gp_update`` trains one ``HipGPR`` per constraint
            on the evaluated rows -- its own engine, deep copies of ``gp_kernel`` and ``gp_meanf`` as given here, the usual
            search, warm-started from its last optimum -- and installs them as the engine's constraint set
            (``HipGPR.install_constraints``).  While the set is resident ``gp_eval_best_ucb``, ``gp_eval_best_ucb_grow``,
            ``gp_eval_best_acq``, ``gp_acq_values`` and the rescoring of ``gp_update`` go through the constrained calls
            (Gardner et al. 2014; Gelbart, Snoek & Adams 2014): a leaf whose probability of feasibility is below ``pof_min`` is
            worth -inf.  N <= 128, "float64" / "mixed", one GPU, ``refit_every`` = 1, ``hyper="point"``; MES and
            ``select_batch`` raise ValueError.  Nothing of it is saved (``save`` raises while constraints are set).  The
            constraint models are always trained on the marginal likelihood, whatever ``objective`` says of the scores' model:
            the LOO objective was added for a misspecified model of the SCORE.  EI, log-EI and PI improve by default on the
            best FEASIBLE observation (``highest_feasible_score``; Gardner et al. 2014), on the largest score while none is
            feasible.  ``close_constraint_models()`` closes the models' engines
        :param constraint_mode: how the loop's calls combine the acquisition with the probability of feasibility: "gate"
            (default: the acquisition's own value, in score units, or -inf) -- the only mode under which the loop's
            score-unit acquisition keeps its units; "weight" and "feasibility" serve ``constrained_select``
        :param pof_min: the smallest probability of feasibility a leaf may have (0: no gate)
        :param hyper: "point" (default, the reference's way): every leaf is ranked under the one hyper-parameter vector the
            search found.  "marginal" (NOT in the reference): the integrated acquisition of Snoek, Larochelle & Adams (2012)
            -- ``gp_update`` runs the search with priors in the loss (a MAP search), draws ``n_theta`` samples of
            p(theta | y) by HMC from the optimum (``HipGPR.sample_hyper``) and installs their posteriors as an ensemble on
            the engine (``HipGPR.install_ensemble``); while it is resident ``gp_eval_best_ucb``, ``gp_eval_best_ucb_grow``,
            ``gp_eval_best_acq``, ``gp_acq_values``, ``gp_predict`` (the mixture's moments) and the rescoring of
            ``gp_update`` go through the integrated calls.  Every other method keeps reading the MAP posterior.  N <= 128,
            "float64" / "mixed", one GPU, ``refit_every`` = 1, ``objective="nlml"``; MES and ``select_batch`` raise ValueError;
            ``gp_update`` raises ValueError at the 129th evaluated point (``GPSOptimiser`` warns at construction when its
            budget can get there).  ``gp_kernel`` and ``gp_meanf`` are deep-copied: the priors are attached to the copies,
            never to the caller's objects (a model passed in as ``gpflow_model`` is the caller's and gets them).  Nothing of it is
            saved: a surrogate loaded with ``from_saved`` is a "point" one until constructed otherwise
        :param n_theta: members of the ensemble (1 .. 32)
        :param hyper_priors: dictionary with the keys ``lengthscales``, ``variance``, ``noise``, ``mean`` of
            ``pygpso_amd.priors`` objects; None: ``priors.default_priors()`` -- LogNormal(median 0.5, sigma 1) on the
            lengthscales of the unit cube, LogNormal(1, 1.5) on the kernel variance, LogNormal(1e-3, 2) on the noise: choices,
            not measurements
        :param hyper_seed: seeds the sampler, together with the number of the update: the same seed gives the same run
        :param hyper_options: keyword arguments of ``hyper_sampler.sample_theta`` (chains, burn, leapfrog, step, thin, ...)
        :param objective: what ``gp_update`` minimises over the hyper-parameters (NOT in the reference, which has the
            first only): "nlml" (default), the negative log marginal likelihood, or "loo", the leave-one-out log
            pseudo-likelihood (Rasmussen & Williams 5.4.2) -- the usual alternative when the kernel family is misspecified;
            "float64" / "mixed" only
        :param gauss_likelihood_sigma: initial noise VARIANCE of the Gaussian likelihood (the
            reference passes it as ``noise_variance`` despite the name, gpso/gp_surrogate.py:494)
        :param refit_every: 1 (default): every ``gp_update`` re-optimises the hyper-parameters, as the reference does
            (gpso/gp_surrogate.py:496-503).  c > 1 (opt-in, NOT the reference's behaviour): only every c-th update
            re-optimises; the updates in between keep the hyper-parameters and extend the device posterior by the new
            points in place (``gpso_append``: O(N^2 k) instead of 10-45 O(N^3) loss evaluations)
        :param refit_guard: (with ``refit_every`` > 1) how far the kept hyper-parameters may drift before an appended
            posterior counts as stale: an append's NLML increment per new point is -log p(y_new | data, theta); when it
            exceeds the fit's own average (NLML / N) by more than ``refit_guard`` nats per point the new points are
            surprising under theta and THIS update re-optimises instead of waiting for the c-th.  None: no guard
        """
        if hyper == "marginal":
            # (the priors are attached to the kernel and the mean function: the surrogate works on copies of its own, so that
            # the caller's objects, which another surrogate or a bare HipGPR may share, never carry a prior they were not given)
            import copy

            gp_kernel = copy.deepcopy(gp_kernel)
            gp_meanf = copy.deepcopy(gp_meanf)
        super().__init__(gp_kernel=gp_kernel, gp_meanf=gp_meanf, optimiser=optimiser,
                         varsigma=varsigma, gp_acquisition=gp_acquisition, points=points, gpflow_model=gpflow_model, dtype=dtype,
                         device=device, engine_options=engine_options, devices=devices)
        if objective not in ("nlml", "loo"):
            raise ValueError(f"objective must be 'nlml' or 'loo', not {objective!r}")
        self.objective = objective
        self.gp_lik_sigma = gauss_likelihood_sigma
        self.refit_every = max(1, int(refit_every))
        self.refit_guard = None if refit_guard is None else float(refit_guard)
        self.guard_refits = 0  # updates the guard turned into re-optimisations
        self._updates = 0  # gp_update calls so far (refit_every counts them)
        if hyper not in ("point", "marginal"):
            raise ValueError(f"hyper must be 'point' or 'marginal', not {hyper!r}")
        self.hyper = hyper
        self.n_theta = int(n_theta)
        self.hyper_priors = hyper_priors
        self.hyper_seed = int(hyper_seed)
        self.hyper_options = dict(hyper_options or {})
        self._ensemble_live = False  # an ensemble drawn for the model's current data is resident on the engine
        self.last_hyper_info = None  # the sampler's info of the last update
        if hyper == "marginal":
            if dtype == "float32":
                raise ValueError("hyper='marginal' needs the dense double factor: dtype='float64' or 'mixed'")
            if objective != "nlml":
                raise ValueError("hyper='marginal' samples p(theta | y), the marginal likelihood times the priors: objective must be "
                                 "'nlml' (exp(-LOO loss) is no likelihood of theta)")
            if self.devices is not None and len(self.devices) > 1:
                raise ValueError("hyper='marginal' runs on one GPU: the ensemble is not sharded over an engine group")
            if not 1 <= self.n_theta <= 32:
                raise ValueError(f"n_theta={n_theta}: 1..32 members")
            if self.refit_every != 1:
                raise ValueError("hyper='marginal' draws a new ensemble at every update: refit_every must be 1")
            if hyper_priors is None:
                from .priors import default_priors

                self.hyper_priors = default_priors()
        self.constraints = []
        self._constraint_models = None  # one HipGPR per constraint, in order, once trained
        self._constraints_live = False  # models of the model's current rows are installed on the engine
        if constraints:
            import copy

            from .constraints import ConstrainedAcq, Constraint

            self.constraints = list(constraints)
            if not all(isinstance(c, Constraint) for c in self.constraints):
                raise TypeError("constraints must be pygpso_amd.constraints.Constraint objects")
            if len(self.constraints) > 16:
                raise ValueError(f"{len(self.constraints)} constraints: a constraint set holds at most 16 models")
            if constraint_mode != "gate":
                raise ValueError(f"constraint_mode={constraint_mode!r}: the loop's acquisition is in score units and only 'gate' keeps "
                                 "them (use constrained_select for 'weight' and 'feasibility')")
            if dtype == "float32":
                raise ValueError("constraints need the dense double factor: dtype='float64' or 'mixed'")
            if self.devices is not None and len(self.devices) > 1:
                raise ValueError("constraints run on one GPU: the constraint set is not sharded over an engine group")
            if self.refit_every != 1:
                raise ValueError("constraints: every update retrains the constraint models on the objective's rows, refit_every must be 1")
            if hyper != "point":
                raise ValueError("constraints are not integrated over a hyper-parameter ensemble: hyper must be 'point'")
            ConstrainedAcq(None, constraint_mode, pof_min)  # (validates pof_min)
            self._constraint_specs = (copy.deepcopy(gp_kernel), copy.deepcopy(gp_meanf))
        self.constraint_mode, self.pof_min = constraint_mode, float(pof_min)
        if failures not in (None, "classify"):
            raise ValueError(f"failures must be None or 'classify', not {failures!r}")
        self.failures = failures
        self._classifier = None  # the HipVGP under the Bernoulli likelihood, once a failure is held
        self._success_live = False  # a classifier of the points attempted so far is installed as the engine's success member
        if failures is not None:
            import copy

            from .constraints import ConstrainedAcq

            if dtype == "float32":
                raise ValueError("failures='classify' needs the dense double factor: dtype='float64' or 'mixed'")
            if self.devices is not None and len(self.devices) > 1:
                raise ValueError("failures='classify' runs on one GPU: the success member is not sharded over an engine group")
            if self.refit_every != 1:
                raise ValueError("failures='classify': every update retrains the classifier on the attempted points, refit_every must be 1")
            if hyper != "point":
                raise ValueError("failures='classify' is not integrated over a hyper-parameter ensemble: hyper must be 'point'")
            ConstrainedAcq(None, "gate", pof_min)  # (validates pof_min)
            self._classifier_specs = (copy.deepcopy(gp_kernel), copy.deepcopy(gp_meanf))
            sched = {"iterations": 10, "natgrad_gamma": 0.5, "optimiser": None}
            unknown = set(classifier_schedule or {}) - set(sched)
            if unknown:
                raise ValueError(f"classifier_schedule: unknown keys {sorted(unknown)}")
            sched.update(classifier_schedule or {})
            if sched["optimiser"] is None:
                sched["optimiser"] = Adam(0.05)
            if not (int(sched["iterations"]) >= 1 and 0.0 < float(sched["natgrad_gamma"]) <= 1.0):
                raise ValueError("classifier_schedule: iterations >= 1 and natgrad_gamma in (0, 1]")
            self.classifier_schedule = sched

    # -- failures="classify": failed points stay in the store (label evaluated, score -inf, marked failed) and out of every
    # regression model's training set --
    def _failed_evaluated(self):
        """[num_evaluated] bool: which evaluated points are failures (all False without ``failures=``)."""
        return self.points.failed_mask(PointLabels.evaluated)

    @property
    def num_failed(self):
        return int(self._failed_evaluated().sum()) if self.failures else 0

    @property
    def highest_score(self):
        if not self.failures:
            return super().highest_score
        cand = [p for p, bad in zip(self._with_label(PointLabels.evaluated), self._failed_evaluated()) if not bad]
        if cand:
            return max(cand, key=lambda p: p.score_mu)

    @property
    def current_training_data(self):
        if not self.failures:
            return super().current_training_data
        ev = [p for p, bad in zip(self._with_label(PointLabels.evaluated), self._failed_evaluated()) if not bad]
        return np.array([p.normed_coord for p in ev]), np.array([p.score_mu for p in ev])

    @property
    def current_training_noise(self):
        s = super().current_training_noise
        return s if s is None or not self.failures else s[~self._failed_evaluated()]

    @property
    def current_attempts(self):
        """(coords [A, D], labels [A]) of every ATTEMPTED point in list order: label 1 for a finite score, 0 for a failure --
        the classifier's training set."""
        ev = self._with_label(PointLabels.evaluated)
        return np.array([p.normed_coord for p in ev]), (~self._failed_evaluated()).astype(np.float64)

    @classmethod
    def default(cls, dtype="float64", device=0, engine_options=None, devices=None):
        """Matern-5/2 (l = 0.25, s2 = 1), constant mean 0, L-BFGS-B, noise 1e-3
        (gpso/gp_surrogate.py:418-434)."""
        return cls(
            gp_kernel=Matern52(lengthscales=np.sum(NORM_PARAMS_BOUNDS) * 0.25, variance=1.0),
            gp_meanf=Constant(0.0),
            optimiser=Scipy(),
            varsigma=erfcinv(0.01),
            gauss_likelihood_sigma=1.0e-3,
            dtype=dtype,
            device=device,
            engine_options=engine_options,
            devices=devices,
        )

    # -- constraints=[...]: the observed constraint outputs ride beside the points, the models beside the objective's --
    def append(self, coords, scores, score_vars=None, constraint_values=None):
        """``constraint_values`` [n, J] (with ``constraints=`` only, and then required): the observed outputs of the J
        constrained quantities at ``coords``, kept beside the points as the score variances are."""
        if self.failures:
            scores = np.asarray(scores, dtype=np.float64)
            ok = np.isfinite(scores)
            if not ok.all():
                return self._append_with_failures(coords, scores, ok, score_vars, constraint_values)
        if not self.constraints:
            if constraint_values is not None:
                raise ValueError("constraint_values given, but the surrogate was constructed without constraints=")
            return super().append(coords, scores, score_vars)
        if constraint_values is None:
            raise ValueError(f"the surrogate has {len(self.constraints)} constraints: append needs constraint_values [n, J]")
        cv = np.asarray(constraint_values, dtype=np.float64)
        if cv.shape != (coords.shape[0], len(self.constraints)):
            raise ValueError(f"constraint_values has shape {cv.shape}, not {(coords.shape[0], len(self.constraints))}")
        if not np.all(np.isfinite(cv)):
            raise ValueError("constraint_values must be finite")
        for i in range(coords.shape[0]):
            had = self.points.find_by_coords(coords[i])
            if had is not None and had.label == PointLabels.evaluated:
                continue  # (an evaluated duplicate keeps its score, and so its variance and its constraint values)
            super().append(coords[i:i + 1], scores[i:i + 1], None if score_vars is None else score_vars[i:i + 1])
            self.points.set_constraint_values_at(self.points.find_index_by_coords(coords[i]), cv[i])

    def _append_with_failures(self, coords, scores, ok, score_vars, constraint_values):
        """``append`` when some score is not finite: the finite rows go the usual way; a failed row is stored at its
        coordinates as an evaluated point worth -inf and marked failed (an evaluated duplicate keeps what it has).  Whatever
        came with a failed row -- a score variance, constraint outputs -- is dropped: nothing was observed there."""
        assert coords.ndim == 2 and scores.ndim == 1 and coords.shape[0] == scores.shape[0]
        if not ok.any() and self.highest_score is None:
            raise ValueError("append: no finite score, here or held: the objective's GP needs at least one evaluated point "
                             "(failures='classify' models where evaluations fail, not a run in which every one does)")
        for i in range(coords.shape[0]):  # (row by row: the store keeps the caller's order)
            if ok[i]:
                self.append(coords[i:i + 1], scores[i:i + 1], None if score_vars is None else np.asarray(score_vars)[i:i + 1],
                            None if constraint_values is None else np.asarray(constraint_values)[i:i + 1])
                continue
            c = coords[i]
            had = self.points.find_by_coords(c)
            if had is not None and had.label == PointLabels.evaluated:
                continue
            i = self.points.append(GPPoint(c, -np.inf, 0.0, -np.inf, PointLabels.evaluated))
            self.points.mark_failed_at(i)

    @property
    def current_training_constraints(self):
        """[N, J] observed constraint outputs aligned with ``current_training_data``; None without constraints."""
        if not self.constraints:
            return None
        if not self.failures or not self.num_failed:
            return self.points.constraint_matrix(PointLabels.evaluated)
        keep = set(np.flatnonzero(~self._failed_evaluated()).tolist())
        ev = [i for i, p in enumerate(self.points) if p.label == PointLabels.evaluated]
        rows = [self.points.constraint_values_at(i) for k, i in enumerate(ev) if k in keep]
        if any(r is None for r in rows):
            raise ValueError("an evaluated point has no constraint values: append(coords, scores, constraint_values=...) stores them")
        return np.array(rows, dtype=np.float64).reshape(len(rows), -1)

    @property
    def highest_feasible_score(self):
        """The best evaluated point whose OBSERVED constraint outputs all keep their bounds (None: none does); without
        constraints ``highest_score``."""
        if not self.constraints:
            return self.highest_score
        from .constraints import feasible_rows

        ev = self._with_label(PointLabels.evaluated)
        if self.failures and self.num_failed:  # (a failed point observed nothing: neither a score nor constraint outputs)
            ev = [p for p, bad in zip(ev, self._failed_evaluated()) if not bad]
        if not ev:
            return None
        ok = feasible_rows(self.constraints, self.current_training_constraints)
        cand = [p for p, good in zip(ev, ok) if good]
        return max(cand, key=lambda p: p.score_mu) if cand else None

    def _constrained_incumbent(self, acq, incumbent):
        """The incumbent of EI / log-EI / PI under constraints: the caller's, else the best score OBSERVED feasible -- an
        infeasible high score as incumbent would flatten EI over the whole feasible region.  None (the model's default,
        the largest training target) while no evaluated point is feasible or none carries constraint values."""
        if incumbent is not None or not acq.needs_incumbent or acq.incumbent is not None or not self.points._cvals:
            return incumbent
        best = self.highest_feasible_score
        return None if best is None else float(best.score_mu)

    def close_constraint_models(self):
        """Close the engines of the constraint models (each has a context of its own); the next ``gp_update`` opens new ones.
        The set already copied onto the objective's engine stays usable."""
        for model in list(self._constraint_models or []) + ([self._classifier] if self._classifier is not None else []):
            if getattr(model, "_owns_engine", False) and hasattr(model.engine, "close"):
                model.engine.close()
        self._constraint_models = None
        self._classifier = None

    def _constrained_acq(self, acq=None, mode=None):
        from .constraints import ConstrainedAcq

        return ConstrainedAcq(self._loop_acquisition() if acq is None else acq, self.constraint_mode if mode is None else mode, self.pof_min)

    def _train_constraints(self, x, c):
        """One HipGPR per constraint on the rows ``x`` with the column of ``c`` [N, J] as targets, then the set."""
        import copy

        self._constraints_live = False
        if c is None:
            raise ValueError(f"the surrogate has {len(self.constraints)} constraints: _gp_train needs their observed values c [N, J]")
        c = np.asarray(c, dtype=np.float64)
        if c.shape != (x.shape[0], len(self.constraints)):
            raise ValueError(f"c has shape {c.shape}, not {(x.shape[0], len(self.constraints))}")
        if x.shape[0] > 128:
            raise ValueError(f"constraints hold at most 128 evaluated points (N={x.shape[0]}): the constraint set's limit")
        if self._constraint_models is None:
            kernel, meanf = self._constraint_specs
            self._constraint_models = []
            for j in range(len(self.constraints)):
                engine = self.engine_factory() if self.engine_factory is not None else None
                self._constraint_models.append(HipGPR(data=(x, c[:, j:j + 1]), kernel=copy.deepcopy(kernel), mean_function=copy.deepcopy(meanf),
                                                      noise_variance=self.gp_lik_sigma, dtype=self.dtype, device=self.device, engine=engine,
                                                      engine_options=self.engine_options))
        else:
            for j, model in enumerate(self._constraint_models):
                model.data = (x, c[:, j:j + 1])  # hyper-parameters warm-start from the last optimum
        for model in self._constraint_models:
            self.optimiser.minimize(model.training_loss, model.trainable_variables)
        self.gpflow_model.install_constraints(zip(self._constraint_models, self.constraints))
        self._constraints_live = True

    def constrained_select(self, leaves, acq=None, mode="weight", incumbent=None, seg_off=None):
        """For use outside the loop: per segment of ``seg_off`` the row of ``leaves`` (normed coordinates) that the
        constrained acquisition ranks first -- ``acq`` a name or a spec (None: the surrogate's own), ``mode`` "weight",
        "gate" or "feasibility", the surrogate's ``pof_min``.  Returns (idx, mean, var, value, logpof).  Stores nothing."""
        self._require_model()
        if not self._constraints_live:
            raise ValueError("constrained_select: no constraint models are installed (constraints= and one gp_update first)")
        spec = self._loop_acquisition() if acq is None else resolve_acquisition(acq, varsigma=self.gp_varsigma)
        return self.gpflow_model.constrained_best_acq(np.ascontiguousarray(leaves, dtype=np.float64), self._constrained_acq(spec, mode),
                                                      seg_off, self._constrained_incumbent(spec, incumbent))

    # -- bi-objective search (pygpso_amd.pareto): the score and ONE lower-bounded constraint output as two
    # objectives to maximise.  Outside the loop: EHVI is not in score units --
    def _second_objective(self, second):
        """The index of the constraint that serves as objective 2: a name or an index of a ``lower=`` constraint."""
        if isinstance(second, str):
            names = [c.name for c in self.constraints]
            if second not in names:
                raise ValueError(f"no constraint named {second!r} (constraints: {names})")
            j = names.index(second)
        else:
            j = int(second)
            if not 0 <= j < len(self.constraints):
                raise ValueError(f"second={second}: the surrogate has {len(self.constraints)} constraints")
        if self.constraints[j].sense != -1:
            raise ValueError(f"{self.constraints[j]!r} is an upper bound: objective 2 is MAXIMISED above a reference value, declare it "
                             "with lower=")
        return j

    def _ehvi_reference(self, j, scores, ref):
        """(r1, r2): the caller's entries, else ``default_reference`` of the scores and the constraint's bound."""
        from .pareto import default_reference

        r1, r2 = (None, None) if ref is None else ref
        if r1 is None:
            if scores.shape[0] == 0:
                raise ValueError("no evaluated point yet: a reference value for the score (ref=(r1, None)) is needed")
            r1 = default_reference(scores.reshape(-1, 1))[0]
        if r2 is None:
            r2 = self.constraints[j].threshold
        r = np.array([r1, r2], dtype=np.float64)
        if not np.all(np.isfinite(r)):
            raise ValueError(f"the reference point {r.tolist()} must be finite")
        return r

    def pareto_front(self, second, ref=None):
        """The trade-off found so far between the score and the constraint output ``second`` (a name or an index of a
        ``lower=`` constraint), both maximised -> (coords [P, D], front [P, 2]): the evaluated points on the front in
        normed coordinates and their (score, f2) rows, score ascending.  A point counts when it is evaluated, not failed,
        its OBSERVED outputs keep every OTHER bound, and it lies strictly above the reference point ``ref`` = (r1, r2)
        (None entries: ``default_reference`` of the scores, and the constraint's own bound)."""
        from .constraints import feasible_rows
        from .pareto import pareto_front

        j = self._second_objective(second)
        x, y = self.current_training_data
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1)
        r = self._ehvi_reference(j, y, ref)
        if y.shape[0] == 0:
            return np.zeros((0, 0)), np.zeros((0, 2))
        c = self.current_training_constraints
        others = [i for i in range(len(self.constraints)) if i != j]
        ok = feasible_rows([self.constraints[i] for i in others], c[:, others]) if others else np.ones(y.shape[0], dtype=bool)
        Y = np.column_stack([y, c[:, j]])
        ok &= (Y[:, 0] > r[0]) & (Y[:, 1] > r[1])
        rows = np.flatnonzero(ok)
        front, at = pareto_front(Y[rows])
        return x[rows[at]], front

    def ehvi_select(self, leaves, second, ref=None, mode="weight", seg_off=None):
        """For use outside the loop: per segment of ``seg_off`` the row of ``leaves`` (normed coordinates) of the largest
        exact expected hypervolume improvement of (score, constraint output ``second``) over ``pareto_front(second, ref)``,
        weighted ("weight") or left as it is ("gate") by the probability that the OTHER constraints (and the evaluation
        itself, under ``failures='classify'``) hold.  The surrogate's ``pof_min`` gates in BOTH modes, as in
        ``constrained_select``: a leaf whose probability is below it is worth -inf, weighted or not (``pof_min=0``: no
        gate).  ``mode=None``: the EHVI alone, no gate.  Returns
        (idx, value, logpof, mean [2, nseg], var [2, nseg]).  Stores nothing.  A front of more than 63 points is thinned
        (``pareto.truncate_front``, with a warning)."""
        from .constraints import ConstrainedAcq
        from .distributed import HipGPEngineGroup
        from .pareto import truncate_front

        if not self._constraints_live:
            raise ValueError("ehvi_select: no constraint models are installed (constraints= with objective 2 as a lower= constraint, "
                             "and one gp_update first)")
        self._require_model()
        if isinstance(self.gpflow_model.engine, HipGPEngineGroup):
            raise NotImplementedError("ehvi_select: not offered on a multi-GPU engine group")
        if mode not in (None, "weight", "gate"):
            raise ValueError(f"mode must be None, 'weight' or 'gate', not {mode!r}")
        j = self._second_objective(second)
        r = self._ehvi_reference(j, np.asarray(self.current_training_data[1], dtype=np.float64).reshape(-1), ref)
        _, front = self.pareto_front(j, r)
        front = truncate_front(front, r)
        cspec = None if mode is None else ConstrainedAcq(None, mode, self.pof_min)
        return self.gpflow_model.best_ehvi(np.ascontiguousarray(leaves, dtype=np.float64), j, front, r, latent=True, cspec=cspec,
                                           seg_off=seg_off)

    def _gp_train(self, x, y, s=None, c=None):
        """``s`` [N] (None: none): the known variance of each score, a fixed per-point noise term beside the trained one.
        ``c`` [N, J]: the observed constraint outputs (``constraints=`` only)."""
        self._gp_train_objective(x, y, s)
        if self.constraints:
            self._train_constraints(x, c)
        if self.failures and self.num_failed:
            self._train_classifier(*self.current_attempts)

    @property
    def _gate_live(self):
        """Do the loop's calls go through the constrained ones: a constraint set or a success member is installed."""
        return self._constraints_live or self._success_live

    def _train_classifier(self, xa, labels):
        """One HipVGP under the Bernoulli likelihood on every attempted point (``xa`` [A, D], ``labels`` [A] in {0, 1}),
        trained by ``classifier_schedule``, installed and pushed as the engine's success member."""
        import copy

        self._success_live = False
        if xa.shape[0] > 128:
            raise ValueError(f"failures='classify' holds at most 128 attempted points (A={xa.shape[0]}): the success member's limit")
        y = np.asarray(labels, dtype=np.float64)[:, np.newaxis]
        if self._classifier is None:
            from .kernels import Bernoulli

            kernel, meanf = self._classifier_specs
            engine = self.engine_factory() if self.engine_factory is not None else None
            self._classifier = HipVGP(data=(xa, y), kernel=copy.deepcopy(kernel), mean_function=copy.deepcopy(meanf), likelihood=Bernoulli(),
                                      dtype=self.dtype, device=self.device, engine=engine, engine_options=self.engine_options)
        else:
            self._classifier.data = (xa, y)  # (held rows keep their q, new rows get the prior: pygpso_amd.vgp)
        model, sched = self._classifier, self.classifier_schedule
        for _ in range(int(sched["iterations"])):
            model.natgrad(float(sched["natgrad_gamma"]))
            sched["optimiser"].minimize(model.training_loss, model.trainable_variables)
        self.gpflow_model.install_success(model)
        self._success_live = True

    def _gp_train_objective(self, x, y, s=None):
        assert x.shape[0] == y.shape[0]
        assert x.ndim == 2 and y.ndim == 2
        if s is not None:
            s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
            assert s.shape[0] == x.shape[0]
        if self.gpflow_model is None:
            engine = self.engine_factory() if self.engine_factory is not None else None
            self.gpflow_model = HipGPR(data=(x, y), kernel=self.gp_kernel, mean_function=self.gp_meanf,
                                       noise_variance=self.gp_lik_sigma, dtype=self.dtype,
                                       device=self.device, engine=engine,
                                       engine_options=self.engine_options, devices=self.devices, noise_diag=s,
                                       objective=self.objective)
        else:
            n_old = self.gpflow_model.data[0].shape[0]
            new_rows = None
            if self.refit_every > 1 and self._updates % self.refit_every != 0 and x.shape[0] > n_old:
                if s is None and self.gpflow_model.noise_diag is None:
                    new_rows = self._rows_beyond(self.gpflow_model.data, x, y)
                else:
                    # (a held row must also have kept its variance: it rides as one more coordinate of the comparison)
                    old_x, old_y = self.gpflow_model.data
                    old_s = self.gpflow_model.noise_diag if self.gpflow_model.noise_diag is not None else np.zeros(n_old)
                    new_s = s if s is not None else np.zeros(x.shape[0])
                    new_rows = self._rows_beyond((np.hstack([old_x, old_s[:, np.newaxis]]), old_y),
                                                 np.hstack([x, new_s[:, np.newaxis]]), y)
            if new_rows is not None:
                # the model's points are all still there with their scores: extend the posterior at the kept
                # hyper-parameters by the others.  (The evaluated points do NOT only grow at the end of the list: an
                # evaluation of a point that was stored gp-based overwrites that entry in place, gpso/gp_surrogate.py:
                # 68-101 -- the model then holds the points in ITS order of arrival, a permutation of the list's; the next
                # re-optimisation sets the list's order again.)
                try:
                    model = self.gpflow_model
                    model._ensure_resident()
                    nlml_before = float(model._last_nlml)
                    if s is None:
                        model.append_data(x[new_rows], y[new_rows])
                    else:
                        model.append_data(x[new_rows], y[new_rows], s_new=s[new_rows])
                    per_new = (float(model._last_nlml) - nlml_before) / (x.shape[0] - n_old)
                    if self.refit_guard is None or not (per_new > nlml_before / n_old + self.refit_guard):
                        self._updates += 1
                        return
                    # the new points are much less likely under the kept hyper-parameters than the old ones were on
                    # average: theta has drifted -- re-optimise now (the model already holds all points)
                    self.guard_refits += 1
                    logging.info(f"appended points cost {per_new:.2f} nats each against {nlml_before / n_old:.2f} on average: "
                                 "re-optimising the hyper-parameters on this update")
                except np.linalg.LinAlgError as err:
                    # the appended block is not positive definite at the kept hyper-parameters (in the engine's
                    # arithmetic): the model holds the N + k points with no posterior -- this update re-optimises instead
                    logging.warning(f"{err}; this update re-optimises the hyper-parameters instead of appending")
            else:
                self.gpflow_model.data = (x, y)  # hyper-parameters warm-start from the last optimum
                if s is not None:
                    self.gpflow_model.noise_diag = s
        self._updates += 1
        if self.hyper != "marginal":
            self.optimiser.minimize(self.gpflow_model.training_loss, self.gpflow_model.trainable_variables)
            return
        # the search with the priors in the loss (MAP), the samples from its optimum, their posteriors on the engine
        from . import priors

        self._ensemble_live = False
        model = self.gpflow_model
        if x.shape[0] > 128:
            raise ValueError(f"hyper='marginal' holds at most 128 evaluated points (N={x.shape[0]}): the ensemble's limit")
        priors.attach(model, self.hyper_priors if self.hyper_priors is not None else priors.default_priors())
        self.optimiser.minimize(model.training_loss, model.trainable_variables)
        rng = np.random.default_rng([self.hyper_seed, self._updates])
        U, self.last_hyper_info = model.sample_hyper(self.n_theta, rng=rng, **self.hyper_options)
        installed, skipped = model.install_ensemble(U)
        self.last_hyper_info["installed"], self.last_hyper_info["skipped"] = installed, skipped
        self._ensemble_live = installed > 0

    # -- hyper="marginal": the calls that rank or score leaves go through the integrated ones while an ensemble is resident --
    def _refuse_unserved(self, what):
        """What neither a hyper-parameter ensemble nor a constraint set serves (MES, batch selection) is refused in words."""
        if self.hyper == "marginal":
            raise ValueError(f"{what} is not available with hyper='marginal': it reads one hyper-parameter vector")
        if self.constraints:
            raise ValueError(f"{what} is not available with constraints: it is not served under a constraint set")
        if self.failures:
            raise ValueError(f"{what} is not available with failures='classify': it is not served under a success member")

    def gp_eval_best_ucb(self, normed_coords):
        if self._gate_live:
            _, mean, var, ucb, _ = self.gpflow_model.constrained_best_acq(np.ascontiguousarray(normed_coords, dtype=np.float64),
                                                                          self._constrained_acq())
            return float(mean[0]), float(var[0]), float(ucb[0])
        if not self._ensemble_live:
            return super().gp_eval_best_ucb(normed_coords)
        _, mean, var, ucb = self.gpflow_model.ensemble_best_acq(np.ascontiguousarray(normed_coords, dtype=np.float64), self._loop_acquisition())
        return float(mean[0]), float(var[0]), float(ucb[0])

    def gp_eval_best_ucb_grow(self, leaf_bounds, depth):
        if self._gate_live:
            # (as below: the constrained call takes rows, the centres come from gpso_grow and go back as one segment per box)
            bounds = np.asarray(leaf_bounds, dtype=np.float64)
            bounds = bounds[None] if bounds.ndim == 2 else bounds
            coords = np.asarray(self.gpflow_model.engine.grow(bounds, depth))
            nseg, rows, d = coords.shape
            seg_off = np.arange(nseg + 1, dtype=np.int64) * rows
            _, mean, var, ucb, _ = self.gpflow_model.constrained_best_acq(coords.reshape(nseg * rows, d), self._constrained_acq(), seg_off)
            return [(float(m), float(v), float(u)) for m, v, u in zip(mean, var, ucb)]
        if not self._ensemble_live:
            return super().gp_eval_best_ucb_grow(leaf_bounds, depth)
        # (the integrated call takes rows, not boxes: the centres come from gpso_grow -- LeafNode.grow's bits -- and go back as
        # one segment per box)
        bounds = np.asarray(leaf_bounds, dtype=np.float64)
        bounds = bounds[None] if bounds.ndim == 2 else bounds
        coords = self.gpflow_model.engine.grow(bounds, depth)
        nseg, rows, d = coords.shape
        seg_off = np.arange(nseg + 1, dtype=np.int64) * rows
        _, mean, var, ucb = self.gpflow_model.ensemble_best_acq(coords.reshape(nseg * rows, d), self._loop_acquisition(), seg_off)
        return [(float(m), float(v), float(u)) for m, v, u in zip(mean, var, ucb)]

    def gp_eval_best_acq(self, normed_coords, acquisition, incumbent=None, seg_off=None):
        acq = resolve_acquisition(acquisition, varsigma=self.gp_varsigma)
        if acq.name == "mes":
            self._refuse_unserved("MES")
        if self._gate_live:
            return self.gpflow_model.constrained_best_acq(np.ascontiguousarray(normed_coords, dtype=np.float64), self._constrained_acq(acq),
                                                          seg_off, self._constrained_incumbent(acq, incumbent))[:4]
        if not self._ensemble_live:
            return super().gp_eval_best_acq(normed_coords, acquisition, incumbent, seg_off)
        return self.gpflow_model.ensemble_best_acq(np.ascontiguousarray(normed_coords, dtype=np.float64), acq, seg_off, incumbent)

    def gp_acq_values(self, normed_coords, acquisition, incumbent=None):
        acq = resolve_acquisition(acquisition, varsigma=self.gp_varsigma)
        if acq.name == "mes":
            self._refuse_unserved("MES")
        if self._gate_live:
            return self.gpflow_model.constrained_acq_values(np.ascontiguousarray(normed_coords, dtype=np.float64), self._constrained_acq(acq),
                                                            self._constrained_incumbent(acq, incumbent))[:3]
        if not self._ensemble_live:
            return super().gp_acq_values(normed_coords, acquisition, incumbent)
        return self.gpflow_model.ensemble_acq_values(np.ascontiguousarray(normed_coords, dtype=np.float64), acq, incumbent)

    def mes_select(self, *args, **kwargs):
        self._refuse_unserved("mes_select")
        return super().mes_select(*args, **kwargs)

    def max_value_samples(self, *args, **kwargs):
        self._refuse_unserved("max_value_samples")
        return super().max_value_samples(*args, **kwargs)

    def select_batch(self, *args, **kwargs):
        self._refuse_unserved("select_batch")
        return super().select_batch(*args, **kwargs)

    def select_batch_mc(self, *args, **kwargs):
        self._refuse_unserved("select_batch_mc")
        return super().select_batch_mc(*args, **kwargs)

    def gp_predict(self, normed_coords):
        """``hyper="marginal"``: the moments of the ensemble's mixture at ``normed_coords`` and the integrated value of the
        loop's acquisition -- what ``gp_eval_best_ucb`` ranks by --, stored as gp_based points."""
        if self._gate_live:  # (a gated point is stored with -inf: the loop never evaluates it)
            coords = np.ascontiguousarray(normed_coords, dtype=np.float64)
            mean, var, val, _ = self.gpflow_model.constrained_acq_values(coords, self._constrained_acq())
            for i in range(coords.shape[0]):
                self.points.append(GPPoint(normed_coords[i, :], float(mean[i]), float(var[i]), float(val[i]), PointLabels.gp_based))
            return
        if not self._ensemble_live:
            return super().gp_predict(normed_coords)
        coords = np.ascontiguousarray(normed_coords, dtype=np.float64)
        mean, var, val = self.gpflow_model.ensemble_acq_values(coords, self._loop_acquisition())
        for i in range(coords.shape[0]):
            self.points.append(GPPoint(normed_coords[i, :], float(mean[i]), float(var[i]), float(val[i]), PointLabels.gp_based))

    def gp_update(self):
        if self.constraints or (self.failures and self.num_failed):
            x_train, y_train = self.current_training_data
            self._gp_train(x=x_train, y=y_train[:, np.newaxis], s=self.current_training_noise, c=self.current_training_constraints)
            # the gp-based points are rescored under the new models and the gate: re-appended, each overwrites its own entry
            # (the base class's in-place ``update_scores`` recomputes a score from (mean, var) alone and cannot gate)
            idx = [i for i, p in enumerate(self.points) if p.label == PointLabels.gp_based]
            if idx:
                self.gp_predict(np.array([self.points[i].normed_coord for i in idx]))
            return
        if self.hyper != "marginal":
            return super().gp_update()
        x_train, y_train = self.current_training_data
        s_train = self.current_training_noise
        if s_train is None:
            self._gp_train(x=x_train, y=y_train[:, np.newaxis])
        else:
            self._gp_train(x=x_train, y=y_train[:, np.newaxis], s=s_train)
        # the gp-based points are rescored under the new ensemble: re-appended, each overwrites its own entry (the reference's way)
        idx = [i for i, p in enumerate(self.points) if p.label == PointLabels.gp_based]
        if idx:
            self.gp_predict(np.array([self.points[i].normed_coord for i in idx]))

    def loo_diagnostics(self):
        """Does the surrogate predict its own data?  The leave-one-out predictive of every evaluated point at the current
        hyper-parameters (``HipGPR.loo``; O(N) behind the resident posterior, no refits): a dict of arrays over the
        evaluated points in ``current_training_data`` order -- ``coords`` [N, D], ``score`` [N], ``mean`` / ``var`` [N] of
        the prediction for each score from all the others (``var`` includes the noise), ``z`` = (score - mean) / sqrt(var)
        (standard normal under a well-specified model) and ``lpd``, the log predictive density of each score."""
        self._require_model()
        mean, var, lpd, _, z = self.gpflow_model.loo()
        x, y = self.gpflow_model.data
        return {"coords": x.copy(), "score": y[:, 0].copy(), "mean": mean, "var": var, "z": z, "lpd": lpd}

    @staticmethod
    def _rows_beyond(data, x, y):
        """Indices of the rows of (x, y) that the model's data does not hold, when EVERY row of the model's data is among
        (x, y) bit for bit with its score (any order) -- else None: the update cannot be an append."""
        old_x, old_y = data
        if old_x.shape[1] != x.shape[1] or x.shape[0] <= old_x.shape[0]:
            return None
        rec = np.dtype([("", np.float64)] * (x.shape[1] + 1))
        new_v = np.ascontiguousarray(np.hstack([x, y.reshape(-1, 1)]), dtype=np.float64).view(rec).ravel()
        old_v = np.ascontiguousarray(np.hstack([old_x, old_y.reshape(-1, 1)]), dtype=np.float64).view(rec).ravel()
        held = np.isin(new_v, old_v)
        if int(held.sum()) != old_v.shape[0] or np.unique(old_v).shape[0] != old_v.shape[0]:
            return None
        return np.flatnonzero(~held)

    # -- persistence: points JSON (reference schema) + hyper-parameters as plain JSON ---------------
    def _optimiser_record(self):
        """["Scipy"] as ever; a multi-start optimiser adds its settings (explicit ``starts`` are not kept: they belong to one
        problem).  A record without them loads as ``restarts=1``."""
        opt = self.optimiser
        if isinstance(opt, Scipy) and getattr(opt, "restarts", 1) > 1:
            return ["Scipy", {"restarts": opt.restarts, "restart_scale": opt.restart_scale, "seed": opt.seed}]
        return [type(opt).__name__]

    @staticmethod
    def _optimiser_from_record(record):
        extra = record[1] if len(record) > 1 and isinstance(record[1], dict) else {}
        return Scipy(restarts=extra.get("restarts", 1), restart_scale=extra.get("restart_scale", 1.0),
                     seed=extra.get("seed", 0))

    def save(self, folder):
        """Points, hyper-parameters and settings as JSON.  ``points_noise.json`` exists in ``folder`` afterwards exactly when
        some stored score variance is non-zero: it is written then, and otherwise a copy left by an earlier save is deleted
        (``GPListOfPoints.save_noise``)."""
        if self.failures:
            raise ValueError("a surrogate with failures='classify' is not saved: the failed points and the classifier have no place in "
                             "the saved folder")
        if self.constraints:
            raise ValueError("a surrogate with constraints is not saved: the observed constraint outputs and the constraint models have "
                             "no place in the saved folder")
        os.makedirs(folder, exist_ok=True)
        self.points.save(os.path.join(folder, self.POINTS_FILE))
        self.points.save_noise(os.path.join(folder, self.POINTS_NOISE_FILE))
        model = self.gpflow_model
        params = {k: np.asarray(v).tolist() for k, v in model.parameter_dict().items()}
        with open(os.path.join(folder, self.GPR_FILE), "w") as fh:
            fh.write(json.dumps(params))
        info = {
            "gpr_kernel": model.kernel.name,
            "gpr_kernel_shape": list(np.shape(model.kernel.lengthscales)),
            "gpr_meanf": type(model.mean_function).__name__,
            "gpr_meanf_shape": [],
            "gp_varsigma": self.gp_varsigma, **self._acquisition_record(),
            "gp_likelihood": self.gp_lik_sigma,
            "optimiser": self._optimiser_record(),
            "dtype": self.dtype,
            "refit_every": self.refit_every,  # (not in the reference's schema: an extra key; 1 = the reference's behaviour)
            "refit_guard": self.refit_guard,
        }
        if self.objective != "nlml":  # (an extra key only where it says something: a default run's folder is as ever)
            info["objective"] = self.objective
        with open(os.path.join(folder, self.GPR_INFO), "w") as fh:
            fh.write(json.dumps(info))

    @classmethod
    def from_saved(cls, folder, device=0, devices=None):
        points = GPListOfPoints.from_file(os.path.join(folder, cls.POINTS_FILE))
        has_noise = points.load_noise(os.path.join(folder, cls.POINTS_NOISE_FILE))  # (an older folder has none)
        ev = [p for p in points if p.label == PointLabels.evaluated]
        x = np.array([p.normed_coord for p in ev])
        y = np.array([p.score_mu for p in ev])[:, np.newaxis]
        with open(os.path.join(folder, cls.GPR_INFO)) as fh:
            info = json.load(fh)
        with open(os.path.join(folder, cls.GPR_FILE)) as fh:
            params = json.load(fh)
        assert info["gpr_kernel"] in KERNEL_CLASSES
        kernel = KERNEL_CLASSES[info["gpr_kernel"]](
            lengthscales=np.array(params[".kernel.lengthscales"]), variance=params[".kernel.variance"])
        meanf = Constant(params[".mean_function.c"]) if info["gpr_meanf"] == "Constant" else Zero()
        assert info["optimiser"][0] == "Scipy", f"{info['optimiser']} not currently supported."
        engine = cls.engine_factory() if cls.engine_factory is not None else None
        model = HipGPR(data=(x, y), kernel=kernel, mean_function=meanf,
                       noise_variance=params[".likelihood.variance"], dtype=info.get("dtype", "float64"),
                       device=device, engine=engine, devices=devices,
                       noise_diag=points.noise_vector(PointLabels.evaluated) if has_noise else None,
                       objective=info.get("objective", "nlml"))
        return cls(gp_kernel=kernel, gp_meanf=meanf, optimiser=cls._optimiser_from_record(info["optimiser"]),
                   gauss_likelihood_sigma=info["gp_likelihood"], varsigma=info["gp_varsigma"], gp_acquisition=info.get("gp_acquisition", "ucb_var"),
                   points=points, gpflow_model=model, dtype=info.get("dtype", "float64"), device=device,
                   devices=devices, refit_every=info.get("refit_every", 1), refit_guard=info.get("refit_guard", 2.0),
                   objective=info.get("objective", "nlml"))


class SGPRSurrogate(GPSurrogate):
    """Sparse GP regression surrogate on inducing points (GPflow's ``SGPR``, Titsias 2009): M points Z summarise the N
    evaluated points, an update costs O(N M^2) per loss evaluation and every leaf-UCB prediction O(M^2) whatever N -- the
    surrogate for runs whose N outgrows the exact GPR.  While N <= M, Z is the data and the model is the exact GPR up to
    GPflow's 1e-6 jitter on Kuu.  With ``train_inducing=False`` (the default) Z is not trained: each ``_gp_train`` chooses it
    again (``"greedy"``: the conditional-variance selection on the device at the hyper-parameters the search starts from;
    or an array used as given) and keeps it fixed while L-BFGS-B searches the hyper-parameters (``HipSGPR``).  With
    ``train_inducing=True`` that choice only names where Z starts: once N > M, L-BFGS-B searches the hyper-parameters and
    Z jointly (GPflow's default for ``SGPR``), and later updates warm-start from the trained Z without a selection."""

    def __init__(self, gp_kernel, gp_meanf=None, optimiser=None, varsigma=erfcinv(0.01), gauss_likelihood_sigma=1.0e-3,
                 num_inducing=256, inducing="greedy", points=None, gpflow_model=None, dtype="float64", device=0,
                 engine_options=None, train_inducing=False, gp_acquisition="ucb_var"):
        """
        :param gauss_likelihood_sigma: initial noise VARIANCE of the Gaussian likelihood (as ``GPRSurrogate``)
        :param num_inducing: M (ignored when ``inducing`` is an array)
        :param inducing: "greedy" or an [M, D] array of normed coordinates used as given
        :param train_inducing: train Z beside the hyper-parameters once N > M (``inducing`` then names where Z starts)
        """
        if not isinstance(train_inducing, (bool, np.bool_)):
            raise TypeError(f"train_inducing must be True or False, not {train_inducing!r}")
        if dtype not in ("float64", "mixed"):
            raise ValueError(f"SGPR trains in float64: dtype must be 'float64' or 'mixed', not {dtype!r}")
        if isinstance(inducing, str):
            if inducing != "greedy":
                raise ValueError(f"inducing must be 'greedy' or an [M, D] array, not {inducing!r}")
            if int(num_inducing) < 1:
                raise ValueError(f"num_inducing={num_inducing}: need at least one inducing point")
        else:
            inducing = np.ascontiguousarray(inducing, dtype=np.float64)
            if inducing.ndim != 2 or inducing.shape[0] < 1 or not np.all(np.isfinite(inducing)):
                raise ValueError("inducing must be a finite [M, D] array with M >= 1")
            num_inducing = inducing.shape[0]
        super().__init__(gp_kernel=gp_kernel, gp_meanf=gp_meanf, optimiser=optimiser, varsigma=varsigma, gp_acquisition=gp_acquisition, points=points,
                         gpflow_model=gpflow_model, dtype=dtype, device=device, engine_options=engine_options)
        self.gp_lik_sigma = gauss_likelihood_sigma
        self.num_inducing = int(num_inducing)
        self.inducing = inducing
        self.train_inducing = bool(train_inducing)

    @classmethod
    def default(cls, num_inducing=256, dtype="float64", device=0, engine_options=None, train_inducing=False):
        """``GPRSurrogate.default()``'s specification with M inducing points."""
        return cls(gp_kernel=Matern52(lengthscales=np.sum(NORM_PARAMS_BOUNDS) * 0.25, variance=1.0), gp_meanf=Constant(0.0),
                   optimiser=Scipy(), varsigma=erfcinv(0.01), gauss_likelihood_sigma=1.0e-3, num_inducing=num_inducing,
                   dtype=dtype, device=device, engine_options=engine_options, train_inducing=train_inducing)

    def _gp_train(self, x, y, s=None):
        self._refuse_score_variances(s)
        assert x.shape[0] == y.shape[0]
        assert x.ndim == 2 and y.ndim == 2
        if self.gpflow_model is None:
            self.gpflow_model = HipSGPR(data=(x, y), kernel=self.gp_kernel, mean_function=self.gp_meanf,
                                        noise_variance=self.gp_lik_sigma, num_inducing=self.num_inducing,
                                        inducing=self.inducing, dtype=self.dtype, device=self.device,
                                        engine_options=self.engine_options, train_inducing=self.train_inducing)
        else:
            # Z chosen again at the hyper-parameters the search warm-starts from (or, trained, kept as it is)
            self.gpflow_model.data = (x, y)
        self.optimiser.minimize(self.gpflow_model.training_loss, self.gpflow_model.trainable_variables)

    # -- persistence: the GPR schema plus num_inducing, the policy and Z ----------------------------
    def save(self, folder):
        os.makedirs(folder, exist_ok=True)
        self.points.save(os.path.join(folder, self.POINTS_FILE))
        model = self.gpflow_model
        params = {k: np.asarray(v).tolist() for k, v in model.parameter_dict().items()}
        with open(os.path.join(folder, self.GPR_FILE), "w") as fh:
            fh.write(json.dumps(params))
        info = {
            "gpr_kernel": model.kernel.name,
            "gpr_kernel_shape": list(np.shape(model.kernel.lengthscales)),
            "gpr_meanf": type(model.mean_function).__name__,
            "gpr_meanf_shape": [],
            "gp_varsigma": self.gp_varsigma, **self._acquisition_record(),
            "gp_likelihood": self.gp_lik_sigma,
            "optimiser": VGPSurrogate._serialise_optimiser(self),
            "dtype": self.dtype,
            "model": "SGPR",
            "num_inducing": self.num_inducing,
            "inducing": "greedy" if isinstance(self.inducing, str) else "given",
        }
        if self.train_inducing:  # (absent: False -- a surrogate that does not train Z writes the file it always wrote)
            info["train_inducing"] = True
        with open(os.path.join(folder, self.GPR_INFO), "w") as fh:
            fh.write(json.dumps(info))

    @classmethod
    def from_saved(cls, folder, device=0):
        points = GPListOfPoints.from_file(os.path.join(folder, cls.POINTS_FILE))
        ev = [p for p in points if p.label == PointLabels.evaluated]
        x = np.array([p.normed_coord for p in ev])
        y = np.array([p.score_mu for p in ev])[:, np.newaxis]
        with open(os.path.join(folder, cls.GPR_INFO)) as fh:
            info = json.load(fh)
        with open(os.path.join(folder, cls.GPR_FILE)) as fh:
            params = json.load(fh)
        assert info.get("model") == "SGPR", "not a saved SGPRSurrogate"
        assert info["gpr_kernel"] in KERNEL_CLASSES
        kernel = KERNEL_CLASSES[info["gpr_kernel"]](
            lengthscales=np.array(params[".kernel.lengthscales"]), variance=params[".kernel.variance"])
        meanf = Constant(params[".mean_function.c"]) if info["gpr_meanf"] == "Constant" else Zero()
        assert info["optimiser"][0] == "Scipy", f"{info['optimiser']} not currently supported."
        z = np.array(params[".inducing_variable.Z"], dtype=np.float64).reshape(-1, x.shape[1])
        inducing = z if info["inducing"] == "given" else "greedy"
        dtype = info.get("dtype", "float64")
        train_z = bool(info.get("train_inducing", False))
        model = HipSGPR(data=(x, y), kernel=kernel, mean_function=meanf, noise_variance=params[".likelihood.variance"],
                        num_inducing=info["num_inducing"], inducing=inducing, dtype=dtype, device=device,
                        train_inducing=train_z)
        # the Z the saved posterior was built on (the next update chooses again, or -- trained -- continues from it)
        model.set_inducing(z)
        return cls(gp_kernel=kernel, gp_meanf=meanf, optimiser=VGPSurrogate._deserialise_optimiser(info["optimiser"]),
                   gauss_likelihood_sigma=info["gp_likelihood"], varsigma=info["gp_varsigma"], gp_acquisition=info.get("gp_acquisition", "ucb_var"),
                   num_inducing=info["num_inducing"], inducing=inducing, points=points, gpflow_model=model, dtype=dtype,
                   device=device, train_inducing=train_z)


VGP_TRAIN_ITERATIONS = 10


class VGPSurrogate(GPSurrogate):
    """Variational GP surrogate (gpso/gp_surrogate.py:536-699): per ``_gp_train`` iteration one natural-gradient step on
    the variational state q, then one step of the hyper-parameter optimiser (``Adam``, or ``Scipy``) on -ELBO at fixed q
    -- all on the device (``HipVGP``).  Gaussian or Student-t likelihood: the Student-t (GPflow's ``StudentT``, heavy
    tails) keeps gross outliers among the scores -- a diverged simulation, a bad seed -- from dragging the mean and the UCB
    of their whole neighbourhood; its per-point terms come from GPflow's 20-point Gauss-Hermite quadrature.

    The natural-gradient step of a non-Gaussian likelihood is formed at the current q and can be indefinite where a point
    lies far out in the tails (|y - f| > sqrt(df) scale): with ``natgrad_learning_rate`` = 1 heavy outliers can make it
    fail with ``numpy.linalg.LinAlgError``, leaving q as it was -- exactly as GPflow's NaturalGradient fails in its
    Cholesky before assigning q.  gamma of about 0.1 is the usual choice for a non-conjugate likelihood.

    The model keeps its rows in their order of arrival between updates and grows q by the prior for new rows; when a held
    row disappears or its score changes, q restarts at the prior in the caller's order (``pygpso_amd.vgp``)."""

    def __init__(self, gp_kernel, gp_meanf=None, likelihood=None, optimiser=None, varsigma=erfcinv(0.01), points=None,
                 gpflow_model=None, natgrad_learning_rate=1.0, train_iterations=VGP_TRAIN_ITERATIONS, dtype="float64",
                 device=0, engine_options=None, gp_acquisition="ucb_var"):
        """
        :param likelihood: ``Gaussian(variance)`` (default ``Gaussian(1e-3)``) or ``StudentT(scale, df)``; any other
            likelihood raises NotImplementedError
        :param optimiser: hyper-parameter optimiser, default ``Adam(0.01)`` (its moments persist across updates)
        :param natgrad_learning_rate: step length gamma in (0, 1] of the natural gradient
        :param train_iterations: natgrad / optimiser iterations per ``_gp_train``
        :param dtype: "float64" (default) or "mixed" (float64 training, float predict arithmetic); "float32" raises
        """
        likelihood = likelihood if likelihood is not None else Gaussian(1.0e-3)
        if not isinstance(likelihood, (Gaussian, StudentT)):
            raise NotImplementedError(f"{type(likelihood).__name__}: only the Gaussian and Student-t likelihoods are supported")
        gamma = float(natgrad_learning_rate)
        if not (0.0 < gamma <= 1.0):
            raise ValueError(f"natgrad_learning_rate {gamma} outside (0, 1]")
        if dtype not in ("float64", "mixed"):
            raise ValueError(f"VGP trains in float64: dtype must be 'float64' or 'mixed', not {dtype!r}")
        super().__init__(gp_kernel=gp_kernel, gp_meanf=gp_meanf,
                         optimiser=optimiser if optimiser is not None else Adam(0.01), varsigma=varsigma, gp_acquisition=gp_acquisition,
                         points=points, gpflow_model=gpflow_model, dtype=dtype, device=device,
                         engine_options=engine_options)
        self.likelihood = likelihood
        self.natgrad_gamma = gamma
        self.train_iters = int(train_iterations)

    def _gp_train(self, x, y, s=None):
        self._refuse_score_variances(s)
        assert x.shape[0] == y.shape[0]
        assert x.ndim == 2 and y.ndim == 2
        if self.gpflow_model is None:
            self.gpflow_model = HipVGP(data=(x, y), kernel=self.gp_kernel, mean_function=self.gp_meanf,
                                       likelihood=self.likelihood, dtype=self.dtype, device=self.device,
                                       engine_options=self.engine_options)
        else:
            self.gpflow_model.data = (x, y)
        model = self.gpflow_model
        for i in range(self.train_iters):
            model.natgrad(self.natgrad_gamma)
            self.optimiser.minimize(model.training_loss, model.trainable_variables)
            if logging.getLogger().isEnabledFor(logging.DEBUG):
                logging.debug(f"VGP iteration {i + 1}. ELBO: {model.elbo():.04f}")

    def _serialise_optimiser(self):
        if isinstance(self.optimiser, Adam):
            return ["Adam", self.optimiser.learning_rate]
        if isinstance(self.optimiser, Scipy) and self.optimiser.options:  # (absent: SciPy's defaults, the file of before)
            return ["Scipy", dict(self.optimiser.options)]
        return [type(self.optimiser).__name__]

    @staticmethod
    def _deserialise_optimiser(info):
        if info[0] == "Adam":
            return Adam(info[1])
        if info[0] == "Scipy":
            return Scipy(options=info[1] if len(info) > 1 else None)
        raise ValueError(f"{info} not currently supported.")

    def save(self, folder):
        os.makedirs(folder, exist_ok=True)
        self.points.save(os.path.join(folder, self.POINTS_FILE))
        model = self.gpflow_model
        params = {k: np.asarray(v).tolist() for k, v in model.parameter_dict().items()}
        with open(os.path.join(folder, self.GPR_FILE), "w") as fh:
            fh.write(json.dumps(params))
        # the model's rows as indices into the evaluated points (its order of arrival may differ from the list's)
        ev_x, ev_y = self.current_training_data
        order = carried_order(model.data[0], model.data[1], ev_x, ev_y[:, np.newaxis])
        info = {
            "vgp_kernel": model.kernel.name,
            "vgp_kernel_shape": list(np.shape(model.kernel.lengthscales)),
            "vgp_meanf": type(model.mean_function).__name__,
            "vgp_meanf_shape": [1] if isinstance(model.mean_function, Constant) else [],  # (the shape of c)
            "vgp_likelihood": self.likelihood.name,
            "gp_varsigma": self.gp_varsigma, **self._acquisition_record(),
            "optimiser": self._serialise_optimiser(),
            "vgp_iters": self.train_iters,
            "vgp_natgrad_lr": self.natgrad_gamma,
            "dtype": self.dtype,  # (extra keys, not in the reference's schema)
            "vgp_row_order": None if order is None else order[: model.data[0].shape[0]].tolist(),
        }
        if isinstance(self.likelihood, StudentT):  # (df is no GPflow Parameter: the reference's from_saved resets it to 3)
            info["vgp_likelihood_df"] = model.likelihood.df
        with open(os.path.join(folder, self.GPR_INFO), "w") as fh:
            fh.write(json.dumps(info))

    @classmethod
    def from_saved(cls, folder, device=0):
        points = GPListOfPoints.from_file(os.path.join(folder, cls.POINTS_FILE))
        ev = [p for p in points if p.label == PointLabels.evaluated]
        x = np.array([p.normed_coord for p in ev])
        y = np.array([p.score_mu for p in ev])[:, np.newaxis]
        with open(os.path.join(folder, cls.GPR_INFO)) as fh:
            info = json.load(fh)
        with open(os.path.join(folder, cls.GPR_FILE)) as fh:
            params = json.load(fh)
        assert info["vgp_kernel"] in KERNEL_CLASSES
        lik_name = info.get("vgp_likelihood", "Gaussian")
        if lik_name not in ("Gaussian", "StudentT"):
            raise NotImplementedError(f"{lik_name}: only the Gaussian and Student-t likelihoods are supported")
        kernel = KERNEL_CLASSES[info["vgp_kernel"]](
            lengthscales=np.array(params[".kernel.lengthscales"]), variance=params[".kernel.variance"])
        meanf = Constant(params[".mean_function.c"]) if info["vgp_meanf"] == "Constant" else Zero()
        if lik_name == "StudentT":
            likelihood = StudentT(params[".likelihood.scale"], info.get("vgp_likelihood_df", 3.0))
        else:
            likelihood = Gaussian(params[".likelihood.variance"])
        dtype = info.get("dtype", "float64")
        order = info.get("vgp_row_order")
        if order is not None:
            x, y = x[order], y[order]
        model = HipVGP(data=(x, y), kernel=kernel, mean_function=meanf, likelihood=likelihood, dtype=dtype,
                       device=device, q_mu=np.array(params[".q_mu"]), q_sqrt=np.array(params[".q_sqrt"]))
        return cls(gp_kernel=kernel, gp_meanf=meanf, likelihood=likelihood,
                   optimiser=cls._deserialise_optimiser(info["optimiser"]), varsigma=info["gp_varsigma"], gp_acquisition=info.get("gp_acquisition", "ucb_var"),
                   points=points, gpflow_model=model, natgrad_learning_rate=info["vgp_natgrad_lr"],
                   train_iterations=info["vgp_iters"], dtype=dtype, device=device)


SVGP_TRAIN_ITERATIONS = 10


class SVGPSurrogate(GPSurrogate):
    """Sparse variational GP surrogate on inducing points (GPflow's ``SVGP``, whitened, full ``q_sqrt``, full batch):
    the Student-t likelihood of ``VGPSurrogate`` at the scale of ``SGPRSurrogate`` -- an update costs O(N M^2) per
    natural-gradient step or -ELBO evaluation, a leaf-UCB prediction O(M^2), whatever the number N of evaluated points.

    Each ``_gp_train`` chooses Z as ``SGPRSurrogate`` does (the data itself while N <= M, else the greedy conditional-
    variance selection at the current kernel hyper-parameters, or an array used as given; with ``train_inducing=True``
    that is only where Z starts, the hyper-parameter optimiser then moves Z too, at fixed q, and later updates keep the
    trained Z without a selection), starts q (the prior under the
    Gaussian likelihood; under the Student-t the conjugate start, one Gaussian natural-gradient step at the noise variance
    scale^2 df / (df - 2)), then runs ``train_iterations`` times one natural-gradient step on q and one step of the
    hyper-parameter optimiser on -ELBO at fixed q (``HipSVGP``).  An indefinite natural-gradient step raises
    ``numpy.linalg.LinAlgError`` and leaves q as it was (GPflow's behaviour); gamma of about 0.1 is the usual choice for
    the Student-t."""

    def __init__(self, gp_kernel, gp_meanf=None, likelihood=None, num_inducing=256, inducing="greedy",
                 natgrad_learning_rate=1.0, train_iterations=SVGP_TRAIN_ITERATIONS, optimiser=None,
                 varsigma=erfcinv(0.01), points=None, gpflow_model=None, dtype="float64", device=0, engine_options=None,
                 train_inducing=False, gp_acquisition="ucb_var"):
        """
        :param likelihood: ``Gaussian(variance)`` (default ``Gaussian(1e-3)``) or ``StudentT(scale, df)``; any other
            likelihood raises NotImplementedError
        :param num_inducing: M (ignored when ``inducing`` is an array)
        :param inducing: "greedy" or an [M, D] array of normed coordinates used as given
        :param train_inducing: train Z beside the hyper-parameters once N > M (``inducing`` then names where Z starts)
        :param natgrad_learning_rate: step length gamma in (0, 1] of the natural gradient
        :param train_iterations: natgrad / optimiser iterations per ``_gp_train``
        :param optimiser: hyper-parameter optimiser, default ``Adam(0.01)`` (its moments persist across updates), or
            ``Scipy()``
        :param dtype: "float64" (default) or "mixed" (float64 training, float predict arithmetic); "float32" raises
        """
        likelihood = likelihood if likelihood is not None else Gaussian(1.0e-3)
        if not isinstance(likelihood, (Gaussian, StudentT)):
            raise NotImplementedError(f"{type(likelihood).__name__}: only the Gaussian and Student-t likelihoods are supported")
        if not isinstance(train_inducing, (bool, np.bool_)):
            raise TypeError(f"train_inducing must be True or False, not {train_inducing!r}")
        gamma = float(natgrad_learning_rate)
        if not (0.0 < gamma <= 1.0):
            raise ValueError(f"natgrad_learning_rate {gamma} outside (0, 1]")
        if dtype not in ("float64", "mixed"):
            raise ValueError(f"SVGP trains in float64: dtype must be 'float64' or 'mixed', not {dtype!r}")
        if isinstance(inducing, str):
            if inducing != "greedy":
                raise ValueError(f"inducing must be 'greedy' or an [M, D] array, not {inducing!r}")
            if int(num_inducing) < 1:
                raise ValueError(f"num_inducing={num_inducing}: need at least one inducing point")
        else:
            inducing = np.ascontiguousarray(inducing, dtype=np.float64)
            if inducing.ndim != 2 or inducing.shape[0] < 1 or not np.all(np.isfinite(inducing)):
                raise ValueError("inducing must be a finite [M, D] array with M >= 1")
            num_inducing = inducing.shape[0]
        super().__init__(gp_kernel=gp_kernel, gp_meanf=gp_meanf,
                         optimiser=optimiser if optimiser is not None else Adam(0.01), varsigma=varsigma, gp_acquisition=gp_acquisition,
                         points=points, gpflow_model=gpflow_model, dtype=dtype, device=device,
                         engine_options=engine_options)
        self.likelihood = likelihood
        self.num_inducing = int(num_inducing)
        self.inducing = inducing
        self.train_inducing = bool(train_inducing)
        self.natgrad_gamma = gamma
        self.train_iters = int(train_iterations)

    def _gp_train(self, x, y, s=None):
        self._refuse_score_variances(s)
        assert x.shape[0] == y.shape[0]
        assert x.ndim == 2 and y.ndim == 2
        if self.gpflow_model is None:
            self.gpflow_model = HipSVGP(data=(x, y), kernel=self.gp_kernel, mean_function=self.gp_meanf,
                                        likelihood=self.likelihood, num_inducing=self.num_inducing,
                                        inducing=self.inducing, dtype=self.dtype, device=self.device,
                                        engine_options=self.engine_options, train_inducing=self.train_inducing)
        else:
            self.gpflow_model.data = (x, y)  # Z chosen again at the current hyper-parameters (or, trained, kept as it is)
        model = self.gpflow_model
        model.start_q()
        for i in range(self.train_iters):
            model.natgrad(self.natgrad_gamma)
            self.optimiser.minimize(model.training_loss, model.trainable_variables)
            if logging.getLogger().isEnabledFor(logging.DEBUG):
                logging.debug(f"SVGP iteration {i + 1}. ELBO: {model.elbo():.04f}")

    # -- persistence: the VGP's schema plus the SGPR's num_inducing, policy and Z ---------------------
    def save(self, folder):
        os.makedirs(folder, exist_ok=True)
        self.points.save(os.path.join(folder, self.POINTS_FILE))
        model = self.gpflow_model
        params = {k: np.asarray(v).tolist() for k, v in model.parameter_dict().items()}
        with open(os.path.join(folder, self.GPR_FILE), "w") as fh:
            fh.write(json.dumps(params))
        info = {
            "model": "SVGP",
            "svgp_kernel": model.kernel.name,
            "svgp_kernel_shape": list(np.shape(model.kernel.lengthscales)),
            "svgp_meanf": type(model.mean_function).__name__,
            "svgp_likelihood": self.likelihood.name,
            "gp_varsigma": self.gp_varsigma, **self._acquisition_record(),
            "optimiser": VGPSurrogate._serialise_optimiser(self),
            "svgp_iters": self.train_iters,
            "svgp_natgrad_lr": self.natgrad_gamma,
            "num_inducing": self.num_inducing,
            "inducing": "greedy" if isinstance(self.inducing, str) else "given",
            "dtype": self.dtype,
        }
        if self.train_inducing:  # (absent: False)
            info["train_inducing"] = True
        if isinstance(self.likelihood, StudentT):
            info["svgp_likelihood_df"] = model.likelihood.df
        with open(os.path.join(folder, self.GPR_INFO), "w") as fh:
            fh.write(json.dumps(info))

    @classmethod
    def from_saved(cls, folder, device=0):
        points = GPListOfPoints.from_file(os.path.join(folder, cls.POINTS_FILE))
        ev = [p for p in points if p.label == PointLabels.evaluated]
        x = np.array([p.normed_coord for p in ev])
        y = np.array([p.score_mu for p in ev])[:, np.newaxis]
        with open(os.path.join(folder, cls.GPR_INFO)) as fh:
            info = json.load(fh)
        with open(os.path.join(folder, cls.GPR_FILE)) as fh:
            params = json.load(fh)
        assert info.get("model") == "SVGP", "not a saved SVGPSurrogate"
        assert info["svgp_kernel"] in KERNEL_CLASSES
        kernel = KERNEL_CLASSES[info["svgp_kernel"]](
            lengthscales=np.array(params[".kernel.lengthscales"]), variance=params[".kernel.variance"])
        meanf = Constant(params[".mean_function.c"]) if info["svgp_meanf"] == "Constant" else Zero()
        if info["svgp_likelihood"] == "StudentT":
            likelihood = StudentT(params[".likelihood.scale"], info.get("svgp_likelihood_df", 3.0))
        elif info["svgp_likelihood"] == "Gaussian":
            likelihood = Gaussian(params[".likelihood.variance"])
        else:
            raise NotImplementedError(f"{info['svgp_likelihood']}: only the Gaussian and Student-t likelihoods are supported")
        z = np.array(params[".inducing_variable.Z"], dtype=np.float64).reshape(-1, x.shape[1])
        inducing = z if info["inducing"] == "given" else "greedy"
        dtype = info.get("dtype", "float64")
        train_z = bool(info.get("train_inducing", False))
        model = HipSVGP(data=(x, y), kernel=kernel, mean_function=meanf, likelihood=likelihood,
                        num_inducing=info["num_inducing"], inducing=inducing, dtype=dtype, device=device,
                        train_inducing=train_z)
        model.set_inducing(z)  # the Z the saved q belongs to (the next update chooses again, or -- trained -- continues from it)
        model.set_q(np.array(params[".q_mu"]), np.array(params[".q_sqrt"]))
        return cls(gp_kernel=kernel, gp_meanf=meanf, likelihood=likelihood, num_inducing=info["num_inducing"],
                   inducing=inducing, natgrad_learning_rate=info["svgp_natgrad_lr"], train_iterations=info["svgp_iters"],
                   optimiser=VGPSurrogate._deserialise_optimiser(info["optimiser"]), varsigma=info["gp_varsigma"], gp_acquisition=info.get("gp_acquisition", "ucb_var"),
                   points=points, gpflow_model=model, dtype=dtype, device=device, train_inducing=train_z)
