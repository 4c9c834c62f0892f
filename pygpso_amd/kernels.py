"""
Kernel / mean-function / optimiser SPEC objects.

The reference is configured with GPflow objects (``gpflow.kernels.Matern52(lengthscales=..,
variance=..)``, ``gpflow.mean_functions.Constant(c)``, ``gpflow.optimizers.Scipy()`` --
gpso/gp_surrogate.py:393-434).  These are the drop-in stand-ins: they only carry names and
initial hyper-parameter values; the arithmetic is in the HIP kernels.
"""
from __future__ import annotations

import numpy as np
import scipy.optimize


class Kernel:
    """Stationary kernel spec: ``lengthscales`` scalar (isotropic) or [D] (ARD), ``variance``."""

    name = None
    # priors on the hyper-parameters (pygpso_amd.priors; None: no term in the training loss)
    lengthscales_prior = None
    variance_prior = None

    def __init__(self, variance=1.0, lengthscales=1.0):
        self.variance = float(variance)
        ls = np.asarray(lengthscales, dtype=np.float64)
        self.lengthscales = ls.copy() if ls.ndim else float(ls)

    @property
    def ard(self):
        return np.ndim(self.lengthscales) > 0

    def __repr__(self):
        return f"{self.name}(variance={self.variance}, lengthscales={self.lengthscales})"


class Matern52(Kernel):
    name = "Matern52"


class Matern32(Kernel):
    name = "Matern32"


class Matern12(Kernel):
    name = "Matern12"


class SquaredExponential(Kernel):
    name = "SquaredExponential"


RBF = SquaredExponential
Exponential = Matern12

KERNEL_CLASSES = {c.name: c for c in (Matern52, Matern32, Matern12, SquaredExponential)}


class MeanFunction:
    c_prior = None  # prior on a trained constant (pygpso_amd.priors; None: no term)


class Constant(MeanFunction):
    """m(x) = c"""

    name = "Constant"

    def __init__(self, c=0.0):
        self.c = float(np.asarray(c).reshape(-1)[0]) if np.ndim(c) else float(c)

    def __repr__(self):
        return f"Constant(c={self.c})"


class Zero(MeanFunction):
    name = "Zero"
    c = 0.0


class Gaussian:
    """Gaussian likelihood spec (``gpflow.likelihoods.Gaussian(variance=...)``): the initial noise variance."""

    name = "Gaussian"

    def __init__(self, variance=1.0e-3):
        self.variance = float(variance)

    def __repr__(self):
        return f"Gaussian(variance={self.variance})"


class StudentT:
    """Student-t likelihood spec (``gpflow.likelihoods.StudentT(scale=..., df=...)``): the initial scale (trained, through
    GPflow's softplus ``positive()``) and the fixed degrees of freedom.  df <= 2 raises ValueError, where GPflow would
    build a model whose ``predict_y`` variance scale^2 df / (df - 2) is negative or infinite."""

    name = "StudentT"

    def __init__(self, scale=1.0, df=3.0):
        self.scale, self.df = float(scale), float(df)
        if not self.df > 2.0:
            raise ValueError(f"StudentT df={self.df}: need df > 2 (a finite predictive variance)")
        if not self.scale > 0.0:
            raise ValueError(f"StudentT scale={self.scale} must be positive")

    def __repr__(self):
        return f"StudentT(scale={self.scale}, df={self.df})"


class Bernoulli:
    """Bernoulli likelihood spec for a GP classifier: labels in {0, 1}, p(y = 1 | f) = Phi(f), the EXACT probit link (not
    ``gpflow.likelihoods.Bernoulli``'s ``inv_probit``, which mixes a 1e-3 jitter in).  No parameters."""

    name = "Bernoulli"

    def __repr__(self):
        return "Bernoulli()"


class Adam:
    """Keras's Adam (``tf.optimizers.Adam(learning_rate)``, the VGP surrogate's default optimiser,
    gpso/gp_surrogate.py:543): ``minimize(closure, variables)`` takes ONE step on the model's unconstrained vector,
    u -= lr sqrt(1 - beta2^t) / (1 - beta1^t) m / (sqrt(v) + epsilon).  The moments m, v and the step count t live in this
    object and persist across calls, as in Keras."""

    def __init__(self, learning_rate=0.01, beta_1=0.9, beta_2=0.999, epsilon=1.0e-7):
        self.learning_rate = float(learning_rate)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.m = self.v = None
        self.iterations = 0

    def step(self, u, g):
        g = np.asarray(g, dtype=np.float64)
        if self.m is None or self.m.shape != g.shape:
            self.m = np.zeros_like(g)
            self.v = np.zeros_like(g)
        self.iterations += 1
        t = self.iterations
        self.m = self.beta_1 * self.m + (1.0 - self.beta_1) * g
        self.v = self.beta_2 * self.v + (1.0 - self.beta_2) * g * g
        a = self.learning_rate * np.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)
        return np.asarray(u, dtype=np.float64) - a * self.m / (np.sqrt(self.v) + self.epsilon)

    def minimize(self, closure, variables=None):
        model = getattr(closure, "__self__", None)
        if model is None or not hasattr(model, "_loss_and_grad"):
            raise TypeError("Adam.minimize expects the bound training_loss of a pygpso_amd model")
        u = model._pack()
        _, g = model._loss_and_grad(u)
        model._assign(self.step(u, g))

    def __repr__(self):
        return f"Adam(learning_rate={self.learning_rate})"


class _LbfgsbSearch:
    """One L-BFGS-B search as a resumable state: the loop of scipy.optimize._lbfgsb_py._minimize_lbfgsb (SciPy 1.15) for a
    problem with an exact gradient and default options -- unbounded (the hyper-parameter searches) or inside a box
    (``lower=`` / ``upper=``: ``GPSurrogate.polish``) --, cut open where it asks for f and g.  ``advance()`` runs
    the routine until it wants an evaluation (returns a copy of x) or ends (returns None); ``feed(f, g)`` hands the
    evaluation back.  One ``setulb`` workspace per search, so any number of them advance side by side
    (``Scipy(restarts=R)``)."""

    _SETULB_DOC = "setulb(m,x,l,u,nbd,f,g,factr,pgtol,wa,iwa,task,lsave,isave,dsave,maxls,ln_task)"
    NOT_PD = "not positive definite"

    @classmethod
    def routine(cls):
        """scipy's private ``setulb`` when it is the expected one, else None."""
        try:
            from scipy.optimize import _lbfgsb
        except ImportError:
            return None
        if (getattr(_lbfgsb.setulb, "__doc__", None) or "").strip() != cls._SETULB_DOC:
            return None
        return _lbfgsb.setulb

    def __init__(self, setulb, x0, lower=None, upper=None):
        """``lower`` / ``upper`` (each None or [n], +-inf where open): box bounds as ``scipy.optimize.minimize(bounds=...)``
        hands them to the routine, x0 clipped into them.  Both None: the unbounded setup (nbd = 0)."""
        self.setulb = setulb
        self.m, self.maxls, self.maxfun, self.maxiter = 10, 20, 15000, 15000
        self.factr = 2.2204460492503131e-09 / np.finfo(float).eps
        self.pgtol = 1e-5
        m = self.m
        self.x = np.array(np.asarray(x0).ravel(), dtype=np.float64)
        n = self.x.shape[0]
        self.nbd = np.zeros(n, np.int32)
        self.low_bnd = np.zeros(n, np.float64)
        self.upper_bnd = np.zeros(n, np.float64)
        if lower is not None or upper is not None:
            lo = np.full(n, -np.inf) if lower is None else np.array(np.asarray(lower).ravel(), dtype=np.float64)
            up = np.full(n, np.inf) if upper is None else np.array(np.asarray(upper).ravel(), dtype=np.float64)
            if lo.shape != (n,) or up.shape != (n,) or np.any(lo > up):
                raise ValueError("bounds must be [n] arrays with lower <= upper")
            has_lo, has_up = np.isfinite(lo), np.isfinite(up)
            # setulb's codes: 0 unbounded, 1 only a lower bound, 2 both, 3 only an upper bound
            self.nbd[:] = np.where(has_lo & has_up, 2, np.where(has_lo, 1, np.where(has_up, 3, 0)))
            self.low_bnd[has_lo] = lo[has_lo]
            self.upper_bnd[has_up] = up[has_up]
            self.x = np.clip(self.x, lo, up)
        self.f = np.array(0.0, dtype=np.int32)
        self.g = np.zeros((n,), dtype=np.int32)
        self.wa = np.zeros(2 * m * n + 5 * n + 11 * m * m + 8 * m, np.float64)
        self.iwa = np.zeros(3 * n, dtype=np.int32)
        self.task = np.zeros(2, dtype=np.int32)
        self.ln_task = np.zeros(2, dtype=np.int32)
        self.lsave = np.zeros(4, dtype=np.int32)
        self.isave = np.zeros(44, dtype=np.int32)
        self.dsave = np.zeros(29, dtype=np.float64)
        self.nfev = self.nit = 0
        self.done = False
        self.failed = False

    def advance(self):
        while not self.done:
            self.g = self.g.astype(np.float64)
            self.setulb(self.m, self.x, self.low_bnd, self.upper_bnd, self.nbd, self.f, self.g, self.factr, self.pgtol,
                        self.wa, self.iwa, self.task, self.lsave, self.isave, self.dsave, self.maxls, self.ln_task)
            if self.task[0] == 3:  # the routine wants f and g at the current x
                return np.copy(self.x)
            if self.task[0] == 1:  # new iteration
                self.nit += 1
                if self.nit >= self.maxiter:
                    self.task[0], self.task[1] = 5, 504
                elif self.nfev > self.maxfun:
                    self.task[0], self.task[1] = 5, 502
            else:
                self.done = True
        return None

    def feed(self, f, g):
        self.f = float(f)
        self.g = np.array(g, dtype=np.float64).ravel()
        self.nfev += 1

    def fail(self):
        """The evaluation the search asked for has no value (matrix not positive definite): the search is over."""
        self.done = self.failed = True

    def result(self):
        task, nfev, nit = self.task, self.nfev, self.nit
        status = 0 if task[0] == 4 else (1 if (nfev > self.maxfun or nit >= self.maxiter) else 2)
        return scipy.optimize.OptimizeResult(fun=self.f, jac=self.g, nfev=nfev, njev=nfev, nit=nit, status=status,
                                             x=self.x, success=(status == 0),
                                             message=f"L-BFGS-B task {int(task[0])}/{int(task[1])}")


class Scipy:
    """L-BFGS-B through SciPy with SciPy's defaults -- what
    ``gpflow.optimizers.Scipy().minimize(model.training_loss, model.trainable_variables)`` does
    (gpso/gp_surrogate.py:500-503).  ``closure`` must be the bound ``training_loss`` of a model that
    offers ``_loss_and_grad(u)`` / ``_pack()`` / ``_assign(u)`` (pygpso_amd.model.HipGPR).

    With the defaults the L-BFGS-B routine itself (``scipy.optimize._lbfgsb.setulb``, the code
    ``scipy.optimize.minimize`` drives) is called in the same reverse-communication loop
    ``scipy.optimize._lbfgsb_py._minimize_lbfgsb`` runs, minus the per-evaluation wrappers of
    ``minimize`` (``ScalarFunction``, ``OptimizeResult`` per iteration): same routine, same inputs, same
    iterates bit for bit -- at N <= 100 those wrappers cost as much as the device evaluation.  Any option,
    another method, or a SciPy whose private routine has another signature goes through
    ``scipy.optimize.minimize``.

    ``restarts=R`` > 1 (multi-start; the marginal likelihood of a GP on a few dozen points is multimodal): R searches, the
    first from the model's current hyper-parameters as ever, advance in lockstep; each round their pending evaluations go
    to the model as ONE ``_loss_and_grad_batch(U)`` call (one launch, one workgroup per search, where N <= 128) and the
    lowest local optimum found is kept.  Every search takes exactly the iterates it would take alone."""

    _SETULB_DOC = _LbfgsbSearch._SETULB_DOC

    def __init__(self, options=None, restarts=1, restart_scale=1.0, seed=0, starts=None):
        """``options``: SciPy's ``options`` dictionary for every ``minimize`` of this object that is given none of its own,
        e.g. ``Scipy(options={"maxfun": 200})`` to cap the evaluations of an update (a search over (u, Z) with
        ``train_inducing=True`` has M D more dimensions and can use thousands).  None: SciPy's defaults.
        ``restarts``: searches per ``minimize`` (1: the single warm-started search, exactly as without the keyword).
        Searches 1 .. R-1 start at the rows of ``starts`` ``[R-1, nu]`` (unconstrained vectors) when given, otherwise at
        u0 + ``restart_scale`` * N(0, 1) draws of a generator made from (``seed``, minimize calls of this object so far)."""
        self.options = dict(options) if options else None
        self.restarts = int(restarts)
        if self.restarts < 1:
            raise ValueError(f"restarts={restarts} must be at least 1")
        self.restart_scale = float(restart_scale)
        self.seed = int(seed)
        self.starts = None if starts is None else np.array(starts, dtype=np.float64, ndmin=2)
        if self.starts is not None and self.starts.shape[0] != self.restarts - 1:
            raise ValueError(f"starts has {self.starts.shape[0]} rows for restarts={self.restarts}: need restarts - 1")
        self.minimize_calls = 0

    def _start_points(self, x0):
        """[R, nu]: row 0 the warm start, the others the explicit ``starts`` or the seeded draws around it."""
        r, nu = self.restarts, x0.shape[0]
        if self.starts is not None:
            if self.starts.shape[1] != nu:
                raise ValueError(f"starts has {self.starts.shape[1]} columns, the model has {nu} variables")
            extra = self.starts
        else:
            rng = np.random.default_rng([self.seed, self.minimize_calls])
            extra = x0 + self.restart_scale * rng.standard_normal((r - 1, nu))
        return np.vstack([x0[np.newaxis, :], extra])

    def minimize(self, closure, variables=None, method="L-BFGS-B", **scipy_kwargs):
        if getattr(self, "options", None) and "options" not in scipy_kwargs:
            scipy_kwargs["options"] = dict(self.options)
        model = getattr(closure, "__self__", None)
        if model is None or not hasattr(model, "_loss_and_grad"):
            raise TypeError("Scipy.minimize expects the bound training_loss of a HipGPR model")
        x0 = model._pack()  # (the model's hyper-parameters are assigned only at the end: a restart begins here again)
        starts = None
        if getattr(self, "restarts", 1) > 1:
            if getattr(model, "_loss_and_grad_batch", None) is None:
                raise NotImplementedError(f"Scipy(restarts={self.restarts}): {type(model).__name__} has no "
                                          "_loss_and_grad_batch; restarts > 1 needs a model that evaluates a batch")
            starts = self._start_points(x0)
            self.minimize_calls += 1
        while True:
            try:
                res = None
                if starts is not None:
                    res = self._multistart(model, starts, method, scipy_kwargs)
                elif method == "L-BFGS-B" and not scipy_kwargs:
                    res = self._lbfgsb_direct(model._loss_and_grad, x0)
                if res is None:
                    res = scipy.optimize.minimize(model._loss_and_grad, x0, jac=True, method=method, **scipy_kwargs)
                break
            except np.linalg.LinAlgError as err:
                # GPSO_E_NOTPD inside the search.  The reference's search runs in float64 (gpflow.default_float,
                # gpso/gp_surrogate.py:490-503) and loses positive definiteness only on a genuinely singular matrix; a
                # float32 factorisation loses it where the line search steps into small noise at large N.  The model then
                # reopens its engine as "mixed" (float64 fit, on the device) and THIS update's search starts over from its
                # theta_0 -- one history in one arithmetic.  Nowhere to go (float64 / mixed engine, escalate=False, an engine
                # the model does not own): the error is the caller's, as in the reference.
                escalate = getattr(model, "_escalate", None)
                if escalate is None or not escalate(err, fit=True):
                    raise
                model.fit_escalations = getattr(model, "fit_escalations", 0) + 1
        model._assign(res.x)
        self.last_result = res  # (callers such as GPRSurrogate._gp_train drop the return value)
        return res

    @classmethod
    def _lbfgsb_direct(cls, fun_and_grad, x0):
        """One resumable search (``_LbfgsbSearch``) run alone; None when the private routine is not the expected one."""
        setulb = _LbfgsbSearch.routine()
        if setulb is None or _LbfgsbSearch._SETULB_DOC != cls._SETULB_DOC:
            return None
        search = _LbfgsbSearch(setulb, x0)
        while True:
            x = search.advance()
            if x is None:
                break
            search.feed(*fun_and_grad(x))
        return search.result()

    # -- multi-start ---------------------------------------------------------------------------------------------------
    @classmethod
    def _lockstep(cls, batch, starts):
        """The searches from the rows of ``starts`` advanced side by side: each round the x every live search waits at are
        stacked into U and evaluated by one ``batch(U) -> (loss, grad, ok)`` call.  A search whose evaluation failed is
        over (start 0: ``LinAlgError``, as when it runs alone).  Returns the list of searches, or None when SciPy's private
        routine is not the expected one."""
        setulb = _LbfgsbSearch.routine()
        if setulb is None or _LbfgsbSearch._SETULB_DOC != cls._SETULB_DOC:
            return None
        searches = [_LbfgsbSearch(setulb, s) for s in starts]
        live = list(range(len(searches)))
        while live:
            pending = [(i, searches[i].advance()) for i in live]
            pending = [(i, x) for i, x in pending if x is not None]
            if not pending:
                break
            loss, grad, ok = batch(np.stack([x for _, x in pending]))
            live = []
            for (i, _), f, g, fine in zip(pending, loss, grad, ok):
                if fine:
                    searches[i].feed(f, g)
                    live.append(i)
                elif i == 0:
                    raise np.linalg.LinAlgError("multi-start: the warm-started search met a matrix that is not positive definite")
                else:
                    searches[i].fail()
        return searches

    def _multistart(self, model, starts, method, scipy_kwargs):
        records, results = [], []
        searches = self._lockstep(model._loss_and_grad_batch, starts) if method == "L-BFGS-B" and not scipy_kwargs else None
        if searches is not None:
            for s in searches:
                results.append(None if s.failed else s.result())
                records.append({"fun": float("nan") if s.failed else float(s.f), "nfev": s.nfev, "nit": s.nit,
                                "status": _LbfgsbSearch.NOT_PD if s.failed else int(results[-1].status)})
        else:  # options, another method or another SciPy: the starts one after another through scipy.optimize.minimize
            for i, s in enumerate(starts):
                try:
                    r = scipy.optimize.minimize(model._loss_and_grad, s, jac=True, method=method, **scipy_kwargs)
                except np.linalg.LinAlgError:
                    if i == 0:
                        raise
                    r = None
                results.append(r)
                records.append({"fun": float("nan"), "nfev": 0, "nit": 0, "status": _LbfgsbSearch.NOT_PD} if r is None else
                               {"fun": float(r.fun), "nfev": int(r.nfev), "nit": int(r.get("nit", 0)), "status": int(r.status)})
        winner = None  # the lowest final loss among the searches that ended; ties: the lowest index
        for i, r in enumerate(results):
            if r is None or np.isnan(r.fun):
                continue
            if winner is None or r.fun < results[winner].fun:
                winner = i
        if winner is None:
            winner = 0  # (every loss NaN: the warm start's result, as a single search would return it)
        res = results[winner]
        res["restarts"] = records
        res["winner"] = winner
        return res
