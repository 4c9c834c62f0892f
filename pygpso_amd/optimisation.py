"""
GPSO loop: the caller of the hot path (update -> explore -> select).

Mirrors ``GPSOptimiser`` of the reference (gpso/optimisation.py:54-718) -- same constructor
arguments, ``run`` / ``resume_run`` / ``save_state`` / ``resume_from_saved``, and the same three
steps with the same quirks:

* ``_gp_update`` ...... optimisation.py:314-340   retrain + re-score every gp_based cell
* ``_tree_explore`` ... optimisation.py:342-403   split best cell per flagged level, score children
* ``_tree_select`` .... optimisation.py:405-462   evaluate the objective at promising cells

MI355X-first differences (results unchanged): both new children of a level are scored by ONE
device call that also generates their ternary sub-trees on the GPU
(``GPRSurrogate.gp_eval_best_ucb_grow`` -> ``gpso_best_ucb_grow``); cells remember the index of
their centre in the point store instead of re-searching it on every update; objective workers are
spawned (never forked) because a process that has initialised HIP must not fork.
"""
from __future__ import annotations

import json
import logging
import os
from enum import Enum, unique
from functools import partial

import numpy as np

from .gp_surrogate import GPPoint, GPRSurrogate, GPSurrogate
from .param_space import NORM_PARAMS_BOUNDS, ParameterSpace
from .utils import JSON_EXT, PKL_EXT, PointLabels


@unique
class CallbackTypes(Enum):
    post_initialise = "post_initialise"
    pre_iteration = "pre_iteration"
    post_iteration = "post_iteration"
    post_update = "post_update"
    pre_finalise = "pre_finalise"


class GPSOCallback:
    """Base class for user hooks: set ``callback_type`` and implement ``run(optimiser)``."""

    callback_type = None

    def run(self, optimiser):
        assert isinstance(optimiser, GPSOptimiser)


class GPSOptimiser:
    SAVE_ATTRS = ["iterations", "budget", "eval_repeats", "last_explored_levels", "last_update_idx",
                  "method", "max_depth", "stop_cond", "update_cycle", "n_eval_counter", "n_workers",
                  "expl_seed"]
    PARAM_SPACE_FILE = f"parameter_space{PKL_EXT}"
    OPT_ATTRS_FILE = f"opt_attributes{JSON_EXT}"

    def __init__(self, parameter_space, gp_surrogate=None, exploration_method="tree",
                 exploration_depth=5, budget=100, stopping_condition="evaluations", update_cycle=1,
                 n_workers=1, callbacks=None, saver=None):
        assert isinstance(parameter_space, ParameterSpace)
        self.param_space = parameter_space
        self.method = exploration_method
        if self.method == "tree":
            self.max_depth = exploration_depth
        elif self.method == "sample":
            self.max_depth = exploration_depth * self.param_space.ndim ** 2
        else:
            raise ValueError(f"Unknown exploration method: {self.method}")
        self.budget = budget
        assert stopping_condition in ["evaluations", "iterations", "depth"]
        self.stop_cond = stopping_condition
        self.update_cycle = update_cycle
        self.n_eval_counter = 0
        self.iterations = 0
        self.eval_repeats_noise = False  # (``run``: store the variance of each aggregated score with its point)
        self.constraints = []  # (``run(objective, constraints=[...])``: the objective returns (score, c_1 .. c_J))
        self._last_constraint_values = None  # [n, J] of the evaluation just made, aggregated over the repeats like the scores
        self.failures = None  # (``run(objective, failures="classify")``: a non-finite score is a failed evaluation, not a score)
        self.n_workers = n_workers
        callbacks = callbacks or []
        assert all(isinstance(cb, GPSOCallback) for cb in callbacks)
        self.callbacks = callbacks
        self.gp_surr = gp_surrogate or GPRSurrogate.default()
        assert isinstance(self.gp_surr, GPSurrogate)
        if getattr(self.gp_surr, "hyper", "point") == "marginal" and stopping_condition == "evaluations" and budget > 128:
            logging.warning(f"hyper='marginal' holds at most 128 evaluated points and the budget is {budget} evaluations: the update "
                            "after the 128th will raise ValueError")
        self.saver = saver
        if saver is not None:
            assert callable(getattr(saver, "save_runs", None))
        # batch both children of a level into one on-device grow+score call when the surrogate can
        self.device_grow = hasattr(self.gp_surr, "gp_eval_best_ucb_grow")

    # -- helpers ---------------------------------------------------------------------------------
    def _run_callbacks(self, callback_type):
        assert callback_type in CallbackTypes
        for cb in self.callbacks:
            if cb.callback_type == callback_type:
                cb.run(self)

    @staticmethod
    def _centre(node):
        return np.array(node.get_center_as_list(normed=True))

    def _point_of(self, node):
        pts = self.gp_surr.points
        if node.point_index is None and hasattr(pts, "find_index_by_coords"):
            node.point_index = pts.find_index_by_coords(self._centre(node))
        if node.point_index is not None:
            return pts[node.point_index]
        return pts.find_by_coords(self._centre(node))

    # -- initial design ----------------------------------------------------------------------------
    def _initialise(self, init_samples):
        d = self.param_space.ndim
        mid, rad = np.mean(NORM_PARAMS_BOUNDS), np.sum(NORM_PARAMS_BOUNDS) * 0.25
        if init_samples is None:
            logging.info("Sampling 2 vertices per dimension within L1 ball of 0.25 of the domain size "
                         f"radius in normalised coordinates using {self.n_workers} worker(s)...")
            normed = np.vstack([mid - rad * np.eye(d), mid + rad * np.eye(d)])
            orig_coords = self.param_space.denormalise_coords(normed)
        elif isinstance(init_samples, np.ndarray):
            assert init_samples.ndim == 2 and init_samples.shape[1] == d
            if init_samples.shape[0] <= 2:
                logging.warning(f"Only {init_samples.shape[0]} points selected for sampling, you "
                                "might want to add more...")
            elif init_samples.shape[0] > 2 * d:
                logging.warning("Too many initial points obtained, you will run out of budget of "
                                "objective function evaluations!")
            logging.info(f"Got {init_samples.shape[0]} points for initial sampling. Note that these "
                         "are interpreted in the original parameter space coordinates!")
            orig_coords = init_samples.copy()
        else:
            raise TypeError("init_samples must be None or a numpy array of original coordinates")
        centre_orig = self.param_space.denormalise_coords(np.array([[mid] * d]))
        all_coords = np.vstack([orig_coords, centre_orig])
        if self.eval_repeats_noise:
            all_scores, all_vars = self.evaluate_objective_function(all_coords)
        else:
            all_scores = self.evaluate_objective_function(all_coords)
        self.param_space.score = float(all_scores[-1])
        if self.failures and not np.isfinite(self.param_space.score):
            self.param_space.score = -np.inf  # (a failed centre: evaluated, worth -inf)
        self.param_space.label = PointLabels.evaluated
        if self.constraints:
            self.gp_surr.append(self.param_space.normalise_coords(all_coords), all_scores, constraint_values=self._last_constraint_values)
        elif self.eval_repeats_noise:
            self.gp_surr.append(self.param_space.normalise_coords(all_coords), all_scores, score_vars=all_vars)
        else:
            self.gp_surr.append(self.param_space.normalise_coords(all_coords), all_scores)
        logging.debug(f"Initialised with {all_coords.shape[0]} points")

    # -- update --------------------------------------------------------------------------------
    def _gp_update(self, update_idx):
        if (self.gp_surr.num_evaluated - update_idx) >= self.update_cycle:
            logging.info("Update step: retraining GP model and updating scores...")
            self.gp_surr.gp_update()
            for node in self.param_space.iter_preorder():
                point = self._point_of(node)
                assert point is not None
                if point.label == PointLabels.gp_based:
                    node.score = point.score_ucb
            self._run_callbacks(CallbackTypes.post_update)
        return self.gp_surr.num_evaluated

    # -- explore -------------------------------------------------------------------------------
    def _score_children(self, fresh, kwargs):
        """best (mean, var, ucb) over the exploration samples of each fresh child."""
        if not fresh:
            return []
        if self.method == "tree":
            if self.device_grow:
                bounds = np.stack([ch.bounds_array() for ch in fresh])
                return self.gp_surr.gp_eval_best_ucb_grow(bounds, self.max_depth)
            return [self.gp_surr.gp_eval_best_ucb(ch.grow(depth=self.max_depth)) for ch in fresh]
        out = []
        for ch in fresh:  # "sample": only the first child of a pass sees the seed (reference quirk)
            coords = ch.sample_uniformly(n_points=self.max_depth, seed=kwargs.pop("seed", None))
            out.append(self.gp_surr.gp_eval_best_ucb(coords))
        return out

    def _tree_explore(self, levels_to_explore, **kwargs):
        logging.info("Exploration step: sampling children in the ternary tree...")
        n_levels = self.param_space.max_depth + 1
        assert len(levels_to_explore) == n_levels
        points = self.gp_surr.points
        for level in range(n_levels):
            if not levels_to_explore[level]:
                continue
            logging.debug(f"Exploring {level} level...")
            parent = self.param_space.get_best_score_leaf(depth=level)
            children = parent.ternary_split()
            centres = [self._centre(ch) for ch in children]
            known = [points.find_index_by_coords(c) for c in centres]
            fresh = [ch for ch, idx in zip(children, known) if idx is None]
            scores = iter(self._score_children(fresh, kwargs))
            for ch, c, idx in zip(children, centres, known):
                if idx is None:
                    mu, var, ucb = next(scores)
                    ch.score = ucb
                    ch.label = PointLabels.gp_based
                    # stored at the child's CENTRE, with the values of its best sub-leaf
                    ch.point_index = points.append(GPPoint(c, mu, var, ucb, PointLabels.gp_based))
                else:
                    ch.score = parent.score
                    ch.label = parent.label
                    ch.point_index = idx
                logging.debug(f"{ch.name} best score: {ch.score}")
            parent.sampled = True

    # -- select --------------------------------------------------------------------------------
    def _tree_select(self):
        logging.info("Selecting step: evaluating best leaves...")
        max_score = -np.inf
        n_levels = self.param_space.max_depth + 1
        levels_to_explore = [False] * n_levels
        for level in range(n_levels):
            leaf = self.param_space.get_best_score_leaf(depth=level, only_not_sampled=True)
            if leaf is None or not leaf.score > max_score:
                continue
            levels_to_explore[level] = True
            max_score = float(leaf.score)  # the pre-evaluation score drives the comparison
            point = self._point_of(leaf)
            if point.label == PointLabels.gp_based:
                orig = self.param_space.denormalise_coords(point.normed_coord[np.newaxis, :])
                if self.constraints:
                    new_score = float(self.evaluate_objective_function(orig)[0])
                    self.gp_surr.append(point.normed_coord[np.newaxis, :], np.array([new_score]),
                                        constraint_values=self._last_constraint_values)
                elif self.failures:
                    new_score = float(self.evaluate_objective_function(orig)[0])
                    self.gp_surr.append(point.normed_coord[np.newaxis, :], np.array([new_score]))
                elif self.eval_repeats_noise:
                    scores, variances = self.evaluate_objective_function(orig)
                    new_score = float(scores[0])
                    self.gp_surr.append(point.normed_coord[np.newaxis, :], np.array([new_score]),
                                        score_vars=np.array([float(variances[0])]))
                else:
                    new_score = float(self.evaluate_objective_function(orig)[0])
                    self.gp_surr.points.append(
                        GPPoint(point.normed_coord, new_score, 0.0, 0.0, PointLabels.evaluated))
                if self.failures and not np.isfinite(new_score):
                    new_score = -np.inf  # a failed evaluation: the leaf is evaluated, worth -inf, and never selected for splitting
                leaf.score = new_score
                leaf.label = PointLabels.evaluated
                logging.debug(f"Leaf {leaf.name} updated to new evaluated score: {leaf.score}")
        logging.debug(f"Level to explore in the next iteration: {levels_to_explore}")
        return levels_to_explore

    def _all_candidates_gated(self):
        """Is every leaf the loop could still evaluate -- unsampled, gp-based -- worth -inf (or NaN)?"""
        for node in self.param_space.iter_preorder():
            if not node.sampled and node.label == PointLabels.gp_based and node.score > -np.inf:
                return False
        return True

    # -- objective -----------------------------------------------------------------------------
    def evaluate_objective_function(self, orig_coords):
        assert orig_coords.ndim == 2 and orig_coords.shape[1] == self.param_space.ndim
        repeated = np.vstack(self.eval_repeats * [orig_coords])
        if self.n_workers > 1 and repeated.shape[0] > 1:
            import multiprocessing as mp
            from concurrent.futures import ProcessPoolExecutor

            # spawn, never fork: this process may already hold a HIP context
            with ProcessPoolExecutor(self.n_workers, mp_context=mp.get_context("spawn")) as pool:
                scores = list(pool.map(self.obj_func, repeated))
        else:
            scores = [self.obj_func(c) for c in repeated]
        self.n_eval_counter += orig_coords.shape[0]
        if self.saver is not None:
            results = [s[0] for s in scores]
            scores = [s[1] for s in scores]
            n = orig_coords.shape[0]
            for i, coords in enumerate(orig_coords):
                self.saver.save_runs(results[i::n], scores[i::n],
                                     dict(zip(self.param_space.parameter_names, coords)))
        if self.constraints:
            # every evaluation returned (score, c_1 .. c_J): the repeats of each column are aggregated by the same function
            cube = np.array(scores).astype(float).reshape((self.eval_repeats, orig_coords.shape[0], -1))
            if cube.shape[2] != 1 + len(self.constraints):
                raise ValueError(f"the objective must return (score, c_1 .. c_{len(self.constraints)}): got {cube.shape[2]} numbers")
            agg = np.asarray(self.eval_repeats_function(cube))
            if self.failures:  # (one non-finite number in any repeat: the evaluation failed, whatever the aggregate makes of it)
                agg = np.array(agg, dtype=np.float64)
                agg[~np.isfinite(cube).all(axis=(0, 2)), 0] = np.nan
            self._last_constraint_values = agg[:, 1:]
            return agg[:, 0]
        table = np.array(scores).astype(float).reshape((self.eval_repeats, -1))
        if self.failures:
            agg = np.array(self.eval_repeats_function(table), dtype=np.float64)
            agg[~np.isfinite(table).all(axis=0)] = np.nan
            return agg
        if self.eval_repeats_noise:
            # the variance of the MEAN of the repeats: what the aggregated score is known to, a fixed per-point noise term
            return self.eval_repeats_function(table), np.var(table, axis=0, ddof=1) / self.eval_repeats
        return self.eval_repeats_function(table)

    def _stopping_condition(self):
        if self.stop_cond == "evaluations":
            return self.n_eval_counter < self.budget
        if self.stop_cond == "iterations":
            return self.iterations < self.budget
        return self.param_space.max_depth <= self.budget

    # -- main loops ------------------------------------------------------------------------------
    def _iterate(self, explore_levels, update_idx):
        cond = True
        while cond:
            self._run_callbacks(CallbackTypes.pre_iteration)
            self._tree_explore(levels_to_explore=explore_levels, seed=self.expl_seed)
            evals_before = self.n_eval_counter
            explore_levels = self._tree_select()
            if (self.constraints or self.failures) and self.n_eval_counter == evals_before and self._all_candidates_gated():
                # nothing was evaluated and no unsampled gp-based leaf is worth more than -inf: every candidate is gated.  The
                # evaluated centres would go on being split without an evaluation ever being made, so the run ends here
                logging.warning(f"every unsampled leaf has a probability of feasibility below pof_min={self.gp_surr.pof_min}: "
                                f"nothing left to evaluate, ending the run after {self.iterations} iteration(s) (lower pof_min, or "
                                "relax the constraints)")
                break
            update_idx = self._gp_update(update_idx)
            self.iterations += 1
            highest_ucb = self.gp_surr.highest_ucb
            logging.info(
                f"After {self.iterations}th iteration: \n\t number of obj. func. evaluations: "
                f"{self.n_eval_counter} \n\t highest score: {self.gp_surr.highest_score.score_mu} "
                f"\n\t highest UCB: {highest_ucb.score_ucb if highest_ucb else None}")
            self.trace.append((self.n_eval_counter, self.gp_surr.highest_score.score_mu,
                               highest_ucb.score_ucb if highest_ucb else None))
            self._run_callbacks(CallbackTypes.post_iteration)
            cond = self._stopping_condition()
        logging.info(f"Done. Highest evaluated score: {self.gp_surr.highest_score.score_mu}")
        self._run_callbacks(CallbackTypes.pre_finalise)
        self.last_explored_levels = explore_levels
        self.last_update_idx = update_idx
        if self.constraints:  # (the best point that was OBSERVED to keep every bound; None when none did)
            return self.gp_surr.highest_feasible_score
        return self.gp_surr.highest_score

    @staticmethod
    def _check_repeats_noise(eval_repeats_noise, eval_repeats, eval_repeats_function):
        """s = var(scores, ddof=1) / eval_repeats is the variance of a mean, and of nothing else."""
        if not eval_repeats_noise:
            return
        if eval_repeats < 2:
            raise ValueError(f"eval_repeats_noise needs eval_repeats >= 2 to estimate a variance (eval_repeats={eval_repeats})")
        if eval_repeats_function is not np.mean:
            raise ValueError("eval_repeats_noise is the variance of the mean of the repeats: eval_repeats_function must be np.mean")

    def _set_constraints(self, constraints):
        """``run``'s constraints: what does not go together with them is refused in words."""
        self.constraints = list(constraints or [])
        surr_has = list(getattr(self.gp_surr, "constraints", None) or [])
        if not self.constraints:
            if surr_has:
                raise ValueError(f"the surrogate was constructed with {len(surr_has)} constraints: pass them to run(objective, constraints=[...]) "
                                 "too (the objective must return their values)")
            return
        if not isinstance(self.gp_surr, GPRSurrogate):
            raise ValueError(f"constraints are modelled by GPRSurrogate, not by {type(self.gp_surr).__name__}")
        if self.saver is not None:
            raise ValueError("constraints and a saver: the saver's (result, score) pairs have no place for the constraint outputs")
        if self.eval_repeats_noise:
            raise ValueError("constraints and eval_repeats_noise: per-point noise of the constraint outputs is not modelled")
        if self.gp_surr.refit_every != 1:
            raise ValueError("constraints: refit_every must be 1 (every update retrains the constraint models)")
        if getattr(self.gp_surr, "hyper", "point") != "point":
            raise ValueError("constraints are not integrated over a hyper-parameter ensemble: hyper must be 'point'")
        if self.method != "tree":
            raise ValueError("constraints drive the tree exploration only")
        if surr_has:
            same = len(surr_has) == len(self.constraints) and all(
                (a.name, a.threshold, a.sense) == (b.name, b.threshold, b.sense) for a, b in zip(surr_has, self.constraints))
            if not same:
                raise ValueError("run(constraints=...) differs from the list the surrogate was constructed with")
        else:
            raise ValueError("run(constraints=...) needs a surrogate that models them: construct it as GPRSurrogate(constraints=[...]) "
                             "with the same list")

    def _set_failures(self, failures):
        """``run``'s failures: what does not go together with them is refused in words."""
        if failures not in (None, "classify"):
            raise ValueError(f"failures must be None or 'classify', not {failures!r}")
        self.failures = failures
        surr_has = getattr(self.gp_surr, "failures", None)
        if failures is None:
            if surr_has:
                raise ValueError("the surrogate was constructed with failures='classify': pass it to run(objective, failures='classify') too")
            return
        if not isinstance(self.gp_surr, GPRSurrogate):
            raise ValueError(f"failed evaluations are modelled by GPRSurrogate, not by {type(self.gp_surr).__name__}")
        if self.saver is not None:
            raise ValueError("failures='classify' and a saver: the saver's (result, score) pairs have no place for a failed evaluation")
        if self.eval_repeats_noise:
            raise ValueError("failures='classify' and eval_repeats_noise: a failed evaluation has no score variance")
        if self.gp_surr.refit_every != 1:
            raise ValueError("failures='classify': refit_every must be 1 (every update retrains the classifier)")
        if getattr(self.gp_surr, "hyper", "point") != "point":
            raise ValueError("failures='classify' is not integrated over a hyper-parameter ensemble: hyper must be 'point'")
        if self.method != "tree":
            raise ValueError("failures='classify' drives the tree exploration only")
        if not surr_has:
            raise ValueError("run(failures='classify') needs a surrogate that models them: construct it as GPRSurrogate(failures='classify')")

    def run(self, objective_function, init_samples=None, eval_repeats=1, eval_repeats_function=np.mean,
            eval_repeats_noise=False, constraints=None, failures=None, **kwargs):
        """``failures`` (not in the reference): None, or "classify" -- an evaluation whose score is not finite (NaN, +-inf; any
        repeat of it under ``eval_repeats``) is recorded as FAILED: its leaf is evaluated, carries the score -inf and is never
        selected for splitting, and the surrogate (constructed as ``GPRSurrogate(failures="classify")``) models the
        probability of success and gates the leaves by it, together with ``constraints`` if there are any.  An iteration in
        which nothing was evaluated and every unsampled gp-based leaf is gated ends the run with a warning.  Returns the best
        finite score.  Refused with failures: a saver, ``save_state`` / ``resume_from_saved``, ``refit_every`` > 1,
        ``eval_repeats_noise``, ``hyper="marginal"``, a surrogate other than ``GPRSurrogate``, ``exploration_method="sample"`` (as
        with constraints: the gate is the tree loop's).
        ``constraints`` (not in the reference): a list of ``pygpso_amd.constraints.Constraint``.  The objective then
        returns ``(score, c_1 .. c_J)``; initial samples and selected leaves store both, repeats aggregate the constraint
        outputs with the same function as the scores, and leaves are ranked in gate mode under the surrogate's score-unit
        acquisition (the surrogate must have been constructed with the same list: ``GPRSurrogate(constraints=...)``).  A gated leaf is never evaluated.
        A leaf is scored by the best centre of its sub-tree (``exploration_depth`` levels) and evaluated at its own centre, as
        without constraints: with ``exploration_depth`` > 1 the gate a leaf passed is its best sub-leaf's, so the evaluated
        point itself may have a probability of feasibility below ``pof_min``; only with ``exploration_depth`` = 1 is every
        evaluated point one that passed the gate.  An iteration in which every candidate is gated ends the run with a warning.  Returns the best point observed feasible (None: none was).  Refused with
        constraints: a saver, ``save_state``, ``refit_every`` > 1, ``hyper="marginal"``, ``eval_repeats_noise``.
        ``eval_repeats_noise`` (not in the reference): with ``eval_repeats`` >= 2 and the mean as the aggregate, store
        the variance of each mean score, var(repeats, ddof=1) / eval_repeats, with its point; the surrogate then models it
        as a fixed per-point noise term beside the trained one (``GPRSurrogate``).  False: the reference's behaviour."""
        assert callable(objective_function)
        self._check_repeats_noise(eval_repeats_noise, eval_repeats, eval_repeats_function)
        self.eval_repeats_noise = bool(eval_repeats_noise)
        self._set_constraints(constraints)
        self._set_failures(failures)
        self.obj_func = objective_function
        self.eval_repeats = eval_repeats
        assert callable(eval_repeats_function)
        self.eval_repeats_function = partial(eval_repeats_function, axis=0)
        self.expl_seed = kwargs.pop("seed", None)
        self.trace = []  # (evaluations, highest score, highest UCB) per iteration
        logging.info(f"Starting {self.param_space.ndim}-dimensional optimisation with budget of "
                     f"{self.budget} objective function evaluations...")
        self._initialise(init_samples)
        self._run_callbacks(CallbackTypes.post_initialise)
        update_idx = self._gp_update(0)
        return self._iterate([True], update_idx)

    def resume_run(self, additional_budget):
        assert callable(self.obj_func) and callable(self.eval_repeats_function)
        assert self.iterations > 0
        self.budget += additional_budget
        if not hasattr(self, "trace"):
            self.trace = []
        logging.info(f"Resuming optimisation for with additional budget of {additional_budget}")
        return self._iterate(self.last_explored_levels, self.last_update_idx)

    # -- persistence -----------------------------------------------------------------------------
    def save_state(self, folder):
        if self.failures:
            raise ValueError("a run with failures='classify' is not saved (save_state / resume_from_saved): the failed points and the "
                             "classifier have no place in the saved folder")
        if self.constraints:
            raise ValueError("a run with constraints is not saved (save_state / resume_from_saved): the constraint outputs and models "
                             "have no place in the saved folder")
        os.makedirs(folder, exist_ok=True)
        logging.warning("When saving, all callbacks and saver will be lost!")
        self.param_space.save(os.path.join(folder, self.PARAM_SPACE_FILE))
        self.gp_surr.save(folder)
        attrs = {a: getattr(self, a) for a in self.SAVE_ATTRS}
        if self.eval_repeats_noise:  # (absent: False -- a run without it writes the file it always wrote)
            attrs["eval_repeats_noise"] = True
        with open(os.path.join(folder, self.OPT_ATTRS_FILE), "w") as fh:
            fh.write(json.dumps(attrs))
        logging.info(f"Saved optimiser to {folder}")

    @classmethod
    def resume_from_saved(cls, folder, additional_budget, objective_function, gp_surrogate=GPRSurrogate,
                          eval_repeats_function=np.mean, callbacks=None, saver=None, eval_repeats_noise=None):
        """``eval_repeats_noise``: None (default) continues as the saved run did (a state file without the key: False);
        True / False overrides it."""
        space = ParameterSpace.from_file(os.path.join(folder, cls.PARAM_SPACE_FILE))
        surr = gp_surrogate.from_saved(folder)
        with open(os.path.join(folder, cls.OPT_ATTRS_FILE)) as fh:
            attrs = json.load(fh)
        opt = cls(parameter_space=space, gp_surrogate=surr, callbacks=callbacks, saver=saver)
        for name, value in attrs.items():
            setattr(opt, name, value)
        if eval_repeats_noise is not None:
            opt.eval_repeats_noise = bool(eval_repeats_noise)
        cls._check_repeats_noise(opt.eval_repeats_noise, opt.eval_repeats, eval_repeats_function)
        assert callable(objective_function)
        opt.obj_func = objective_function
        assert callable(eval_repeats_function)
        opt.eval_repeats_function = partial(eval_repeats_function, axis=0)
        return opt.resume_run(additional_budget=additional_budget), opt
