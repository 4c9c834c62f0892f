"""
``HipGPR``: the object the surrogate keeps in ``.gpflow_model``.

Stands where ``gpflow.models.GPR`` stands in the reference (gpso/gp_surrogate.py:488-503,
298, 325; gpso/plotting.py:351-356 reaches it through ``gp_surr.gpflow_model.predict_y``):
holds data + hyper-parameters, evaluates ``training_loss`` and answers ``predict_y`` -- by calling
the HIP engine.  The parameter transforms are GPflow-2's: softplus for
lengthscales / kernel variance, 1e-6 + softplus for the likelihood variance, identity for the mean.
"""
from __future__ import annotations

import logging
import math
import types

import numpy as np

from . import _lib as L
from .engine import HipGPEngine
from .kernels import Constant, Kernel, MeanFunction, Zero

NOISE_FLOOR = 1.0e-6  # gpflow.likelihoods.Gaussian DEFAULT_VARIANCE_LOWER_BOUND
# what a model does when the device reports GPSO_E_PRECISION: reopen the posterior in the next more
# precise arithmetic ON THE DEVICE (never on the CPU, never in the test oracle)
PRECISION_ESCALATION = {"float32": "mixed", "mixed": "float64"}
# ... and when a float32 FACTORISATION loses positive definiteness (GPSO_E_NOTPD inside a hyper-parameter search or a fit at
# the stored hyper-parameters): "mixed" fits in float64, as the reference does; there is no further step
FIT_ESCALATION = {"float32": "mixed"}


def _softplus1(u):
    """softplus(u) = numpy's ``logaddexp(0, u)``, spelled out with its case split on libm's log1p / exp (what numpy's
    scalar loop calls) so that this module and ``gpso_fit_eval_u`` (csrc/theta.hpp: gpso_softplus) give the same bits."""
    if u == 0.0:
        return 0.693147180559945309417232121458176568
    if u < 0.0:
        return 0.0 + math.log1p(math.exp(u))
    if u > 0.0:
        return u + math.log1p(math.exp(-u))
    return u


def _softplus(u):
    u = np.asarray(u, dtype=np.float64)
    if u.ndim == 0:
        return np.float64(_softplus1(float(u)))
    return np.array([_softplus1(float(v)) for v in u.ravel()], dtype=np.float64).reshape(u.shape)


def _softplus_inv(x):
    x = np.asarray(x, dtype=np.float64)
    return x + np.log(-np.expm1(-x))


def _sigmoid(u):
    """(1 + tanh(u / 2)) / 2 on libm's tanh (the same bits as csrc/theta.hpp: gpso_sigmoid)."""
    u = np.asarray(u, dtype=np.float64)
    return np.array([0.5 * (1.0 + math.tanh(0.5 * float(v))) for v in u.ravel()], dtype=np.float64).reshape(u.shape)


class _Result(np.ndarray):
    """ndarray that also answers ``.numpy()`` like the tf.Tensor the reference's callers index."""

    def numpy(self):
        return np.asarray(self)


def _as_result(a):
    return np.asarray(a, dtype=np.float64).reshape(-1, 1).view(_Result)


def _standard_normals(rng, num_samples, m):
    """[S, M] standard normals from a seed or a ``numpy.random.Generator`` (None: a fresh generator)."""
    if int(num_samples) < 1:
        raise ValueError(f"num_samples={num_samples}: at least one draw")
    gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    return gen.standard_normal((int(num_samples), int(m)))


class HipGPR:
    def __init__(self, data, kernel, mean_function=None, noise_variance=1.0e-3, dtype="float64",
                 device=0, engine=None, engine_options=None, escalate=True, devices=None, noise_diag=None,
                 objective="nlml"):
        """``objective``: what the hyper-parameter search minimises -- "nlml" (default: the negative log marginal
        likelihood, as the reference) or "loo" (the leave-one-out log pseudo-likelihood, Rasmussen & Williams 5.4.2:
        -sum of the log predictive density of every point under the fit without it; ``gpso_fit_eval_loo``; "float64" and
        "mixed" engines).  No counterpart in the reference.
        ``noise_diag`` [N] >= 0 (or None): the known variance of each observation, a fixed per-point term beside the
        trained likelihood variance -- the fits factorise K + diag(likelihood.variance + noise_diag); ``predict_y`` adds
        the likelihood variance only.
        ``dtype``: "float64" | "mixed" | "float32" (see ``HipGPEngine``).  ``engine_options``: extra
        keyword arguments of ``HipGPEngine`` (predict_math, generation, tolerances).  ``escalate``:
        when the device reports that float predictions fail their self-test on the current posterior
        (GPSO_E_PRECISION), reopen it as "mixed", then "float64", with a logged warning, instead of
        raising."""
        if not isinstance(kernel, Kernel):
            raise TypeError("kernel must be a pygpso_amd.kernels.Kernel")
        if mean_function is not None and not isinstance(mean_function, MeanFunction):
            raise TypeError("mean_function must be a pygpso_amd.kernels.MeanFunction or None")
        self.kernel = kernel
        # [gpflow] GPR(mean_function=None) uses Zero(): a fixed mean, nothing to train
        self.mean_function = mean_function if mean_function is not None else Zero()
        self._train_mean = isinstance(self.mean_function, Constant)
        self.likelihood = types.SimpleNamespace(variance=float(noise_variance))
        self._engine_options = dict(engine_options or {})
        self._device = device
        self._devices = list(devices) if devices is not None else None
        self._owns_engine = engine is None
        self.escalate = bool(escalate)
        self.fit_escalations = 0  # hyper-parameter searches restarted on a more precise engine (Scipy.minimize)
        self.fused_transforms = True  # loss evaluations through gpso_fit_eval_u (False: transforms in Python)
        if objective not in ("nlml", "loo"):
            raise ValueError(f"objective must be 'nlml' or 'loo', not {objective!r}")
        self.objective = objective
        self.engine = engine if engine is not None else self._open_engine(dtype)
        if objective == "loo":
            if getattr(self.engine, "dtype_name", None) == "float32":
                raise NotImplementedError("objective='loo' needs a float64 fit: use dtype='float64' or 'mixed'")
            if not hasattr(self.engine, "fit_eval_loo_u"):
                raise NotImplementedError(f"objective='loo' is not available on {type(self.engine).__name__}")
        self._data = None
        self._resident = False  # posterior on the device matches (data, hyper-parameters)?
        self.num_loss_evals = 0
        self._noise_diag = None
        self.data = data
        if noise_diag is not None:
            self.noise_diag = noise_diag

    def _open_engine(self, dtype):
        """One engine on ``device``, or -- ``devices=[...]`` -- a group that shards every predict-type
        call over several GPUs of this process (pygpso_amd/distributed.py)."""
        if self._devices is not None and len(self._devices) > 1:
            from .distributed import HipGPEngineGroup

            return HipGPEngineGroup(dtype=dtype, devices=self._devices, **self._engine_options)
        eng = HipGPEngine(dtype=dtype, device=self._device, **self._engine_options)
        eng.set_timing(False)  # nobody reads last_ms behind the drop-in surrogate: 10 - 45 small evaluations per update
        return eng

    # -- data ---------------------------------------------------------------------------------
    @property
    def data(self):
        return self._data

    @data.setter
    def data(self, value):
        x, y = value
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1, 1)
        assert x.ndim == 2 and x.shape[0] == y.shape[0]
        self._data = (x, y)
        self._noise_diag = None  # (it belonged to the rows just replaced: set ``noise_diag`` again behind new data)
        self.engine.set_data(x, y[:, 0])
        self._resident = False
        self._device_theta = None  # hyper-parameters of the posterior on the device (None: none / unknown)

    @property
    def noise_diag(self):
        """Per-point observation variance [N] beside the current data, or None."""
        return self._noise_diag

    @noise_diag.setter
    def noise_diag(self, value):
        if value is not None:
            value = np.ascontiguousarray(value, dtype=np.float64).reshape(-1)
            if value.shape[0] != self._data[0].shape[0]:
                raise ValueError(f"noise_diag has {value.shape[0]} entries, the data {self._data[0].shape[0]} points")
            if not (np.all(np.isfinite(value)) and np.all(value >= 0.0)):
                raise ValueError("noise_diag must be finite and >= 0")
        had = self._noise_diag is not None
        self._noise_diag = value
        if value is not None or had:
            self._upload_noise_diag()
            self._resident = False
            self._device_theta = None

    def _upload_noise_diag(self):
        """The per-point term goes wherever the data goes: every engine this model opens gets it behind ``set_data``."""
        if not hasattr(self.engine, "set_noise_diag"):
            if self._noise_diag is not None and np.any(self._noise_diag != 0.0):
                raise NotImplementedError(f"per-point observation noise (noise_diag) is not available on {type(self.engine).__name__}")
            return
        self.engine.set_noise_diag(self._noise_diag)

    def append_data(self, x_new, y_new, s_new=None):
        """Extend the training data by ``x_new [k, D]``, ``y_new [k]`` or ``[k, 1]`` WITHOUT touching the hyper-parameters
        (``gpso_append``): when the posterior on the device is the one of the current hyper-parameters it is extended in
        place -- O(N^2 k) -- instead of refactorised.  Returns True when the device posterior was extended (or refitted at
        the same hyper-parameters by the library: pad crossing, N <= 128), False for engines without ``append``.
        ``s_new`` [k]: the new points' per-point noise (``gpso_append_noise``); None = zeros."""
        x_new = np.ascontiguousarray(np.atleast_2d(x_new), dtype=np.float64)
        y_new = np.ascontiguousarray(y_new, dtype=np.float64).reshape(-1, 1)
        assert x_new.shape[0] == y_new.shape[0] and x_new.shape[1] == self._data[0].shape[1]
        x = np.concatenate([self._data[0], x_new])
        y = np.concatenate([self._data[1], y_new])
        s = None  # the per-point noise of the N + k points; stays None while none was ever given
        if s_new is not None:
            s_new = np.ascontiguousarray(s_new, dtype=np.float64).reshape(-1)
            assert s_new.shape[0] == x_new.shape[0]
        if self._noise_diag is not None or (s_new is not None and np.any(s_new != 0.0)):
            s_old = self._noise_diag if self._noise_diag is not None else np.zeros(self._data[0].shape[0])
            s_new = s_new if s_new is not None else np.zeros(x_new.shape[0])
            s = np.concatenate([s_old, s_new])
        if not hasattr(self.engine, "append"):
            self.data = (x, y)
            if s is not None:
                self.noise_diag = s
            return False
        self._ensure_resident()  # the posterior of the data so far at the current hyper-parameters (a fit only if it is not there)
        try:
            if s is None:
                nlml, _ = self.engine.append(x_new, y_new[:, 0])
            else:
                nlml, _ = self.engine.append(x_new, y_new[:, 0], s_new)
        except np.linalg.LinAlgError:
            # the appended block is not positive definite in this arithmetic (GPSO_E_NOTPD): whatever the device still
            # holds, the model's state must be ONE consistent thing -- the N + k points as data, no resident posterior,
            # nothing known about the device's hyper-parameters -- so that the caller's next step (GPRSurrogate: a
            # re-optimisation, which may reopen a float32 engine as "mixed") starts from a plain ``model.data = (x, y)``
            self.data = (x, y)
            if s is not None:
                self.noise_diag = s
            raise
        # only a successful append changes what the model claims
        self._data = (x, y)
        self._noise_diag = s
        self._last_nlml = nlml
        self._resident = True
        return True

    # -- hyper-parameters ---------------------------------------------------------------------
    @property
    def n_ls(self):
        return int(np.size(self.kernel.lengthscales))

    def _pack(self):
        """Unconstrained vector in tf.Module's sorted order: kernel.lengthscales, kernel.variance,
        likelihood.variance, mean_function.c."""
        parts = [
            np.atleast_1d(_softplus_inv(self.kernel.lengthscales)),
            [float(_softplus_inv(self.kernel.variance))],
            [float(_softplus_inv(self.likelihood.variance - NOISE_FLOOR))],
        ]
        if self._train_mean:
            parts.append([self.mean_function.c])
        return np.concatenate(parts).astype(np.float64)

    def _unpack(self, u):
        u = np.asarray(u, dtype=np.float64)
        k = self.n_ls
        ls = _softplus(u[:k])
        var = float(_softplus(u[k]))
        noise = NOISE_FLOOR + float(_softplus(u[k + 1]))
        c = float(u[k + 2]) if self._train_mean else float(self.mean_function.c)
        return ls, var, noise, c

    def _assign(self, u):
        ls, var, noise, c = self._unpack(u)
        self.kernel.lengthscales = ls.copy() if self.kernel.ard else float(ls[0])
        self.kernel.variance = var
        self.likelihood.variance = noise
        if self._train_mean:
            self.mean_function.c = c
        self._resident = False

    @property
    def trainable_variables(self):
        return self._pack()

    def _theta(self):
        return (self.kernel.name, np.atleast_1d(np.asarray(self.kernel.lengthscales, dtype=np.float64)),
                self.kernel.variance, self.likelihood.variance, float(self.mean_function.c))

    # -- priors (pygpso_amd/priors.py) --------------------------------------------------------------
    def _prior_slots(self):
        """One (prior, transform) per optimiser variable in ``_pack``'s order, or None when no prior is attached -- the
        default, under which the loss is the device's number and nothing is added to it."""
        from . import priors as P

        ls, var = self.kernel.lengthscales_prior, self.kernel.variance_prior
        noise = getattr(self.likelihood, "variance_prior", None)
        mean = self.mean_function.c_prior if self._train_mean else None
        if ls is None and var is None and noise is None and mean is None:
            return None
        slots = [(ls, P.SOFTPLUS)] * self.n_ls + [(var, P.SOFTPLUS), (noise, P.SOFTPLUS)]
        if self._train_mean:
            slots.append((mean, P.IDENTITY))
        return slots

    def neg_log_prior(self, u=None):
        """-log p(theta(u)) - log |d theta / d u| at ``u`` (None: the current hyper-parameters); 0.0 without priors."""
        from . import priors as P

        slots = self._prior_slots()
        if slots is None:
            return 0.0
        return P.neg_log_prior_u(self._pack() if u is None else u, slots)[0]

    # -- loss ---------------------------------------------------------------------------------
    def _loss_and_grad(self, u):
        """f(u), df/du for L-BFGS-B: one device evaluation, plus -- where priors are attached -- the prior term and its
        u-gradient, added on the host after the device has returned (GPflow 2's ``log_prior_density``, Jacobian included).
        Without priors the device's numbers are returned as they came."""
        f, gu = self._device_loss_and_grad(u)
        slots = self._prior_slots()
        if slots is None:
            return f, gu
        from . import priors as P

        p, gp = P.neg_log_prior_u(u, slots)
        return f + p, gu + gp

    def _device_loss_and_grad(self, u):
        """The objective and its u-gradient from the device: Gram -> Cholesky -> ... -> gradient."""
        self._device_theta = None
        k = self.n_ls
        if self.objective == "loo":
            # the LOO-CV loss: the same factorisation, the same posterior left on the device, another loss and gradient
            f, gu, th, nlml = self.engine.fit_eval_loo_u(self.kernel.name, u, k, self._train_mean, float(self.mean_function.c))
            self._device_theta = self._theta_key(self.kernel.name, th[:k], th[k], th[k + 1], th[k + 2])
            self._last_nlml = nlml
            self.num_loss_evals += 1
            self._resident = False
            return f, gu
        if self.fused_transforms and hasattr(self.engine, "fit_eval_u"):
            # transforms + chain rule inside the library: one C-ABI call per evaluation (bit-identical to the branch
            # below: tests/test_gpu_goldens.py::test_loss_evaluation_in_the_optimisers_variables)
            f, gu, th = self.engine.fit_eval_u(self.kernel.name, u, k, self._train_mean, float(self.mean_function.c))
            self._device_theta = self._theta_key(self.kernel.name, th[:k], th[k], th[k + 1], th[k + 2])
            self._last_nlml = f
            self.num_loss_evals += 1
            self._resident = False
            return f, gu
        ls, var, noise, c = self._unpack(u)
        f, g = self.engine.fit_eval(self.kernel.name, ls, var, noise, c, want_grad=True)
        self._device_theta = self._theta_key(self.kernel.name, ls, var, noise, c)
        self._last_nlml = f
        self.num_loss_evals += 1
        self._resident = False  # resident for u, not necessarily for the stored hyper-parameters
        gu = np.empty(k + 2 + (1 if self._train_mean else 0))
        gu[: k + 2] = g[: k + 2] * _sigmoid(np.asarray(u[: k + 2]))
        if self._train_mean:
            gu[k + 2] = g[k + 2]
        return f, gu

    def _loss_and_grad_batch(self, U):
        """``_loss_and_grad`` at every row of ``U [B, nu]`` -- the pending evaluations of a multi-start search
        (``Scipy(restarts=R)``) in one launch where the one-launch fit applies.  Returns (loss [B], grad [B, nu], ok [B]);
        a failed row (not positive definite) has ok False.  The batched launch leaves the device's posterior alone, so
        what the model knows about it stands; the row-by-row fallbacks (N > 128, an engine without the batched call) replace
        it as any fit does.  The prior term is added as in ``_loss_and_grad``."""
        loss, grad, ok = self._device_loss_and_grad_batch(U)
        slots = self._prior_slots()
        if slots is None:
            return loss, grad, ok
        from . import priors as P

        p, gp = P.neg_log_prior_u(np.atleast_2d(np.asarray(U, dtype=np.float64)), slots)
        return loss + p, grad + gp, ok

    def _device_loss_and_grad_batch(self, U):
        U = np.atleast_2d(np.asarray(U, dtype=np.float64))
        if self.objective == "loo" or not hasattr(self.engine, "fit_eval_u_batch"):
            # an engine without the batched call (a multi-GPU group, a test double), or the LOO objective (the batched
            # kernel evaluates the NLML): the rows one after another
            loss, grad, ok = np.full(U.shape[0], np.nan), np.full(U.shape, np.nan), np.zeros(U.shape[0], dtype=bool)
            for b, u in enumerate(U):
                try:
                    loss[b], grad[b] = self._device_loss_and_grad(u)
                    ok[b] = True
                except np.linalg.LinAlgError:
                    self._device_theta = None
            return loss, grad, ok
        if self.engine.fit_batch_max() == 0:
            self._device_theta = None
            self._resident = False
        loss, grad, ok = self.engine.fit_eval_u_batch(self.kernel.name, U, self.n_ls, self._train_mean,
                                                      float(self.mean_function.c))
        self.num_loss_evals += U.shape[0]
        return loss, grad, ok

    @staticmethod
    def _theta_key(name, ls, var, noise, c):
        return (name, np.asarray(ls, dtype=np.float64).tobytes(), float(var), float(noise), float(c))

    def _ensure_resident(self):
        if not self._resident:
            name, ls, var, noise, c = self._theta()
            # L-BFGS-B's last loss evaluation is, as a rule, at the point it returns: the posterior that
            # evaluation left on the device is then the one asked for (an evaluation with the gradient builds
            # the same factor, L^-1 and alpha, bit for bit) and no further fit is needed
            if self._device_theta != self._theta_key(name, ls, var, noise, c):
                self._last_nlml, _ = self._fitting(lambda: self.engine.fit_eval(name, ls, var, noise, c, want_grad=False))
                self._device_theta = self._theta_key(name, ls, var, noise, c)
            self._resident = True

    def training_loss(self):
        """The objective at the current hyper-parameters: the negative log marginal likelihood, or -- objective="loo" --
        the LOO-CV loss."""
        self._resident = False
        self._ensure_resident()
        # (with priors attached the loss carries their term, as GPflow's training_loss does; log_marginal_likelihood never)
        prior = self.neg_log_prior() if self._prior_slots() is not None else None
        if self.objective == "loo":
            loss = self.engine.loo()[3]
            return loss if prior is None else loss + prior
        return self._last_nlml if prior is None else self._last_nlml + prior

    def log_marginal_likelihood(self):
        self._resident = False
        self._ensure_resident()
        return -self._last_nlml

    def loo(self):
        """Leave-one-out predictive of the training points at the current hyper-parameters (``gpso_loo``; O(N) behind
        the resident posterior, whatever the objective).  Returns (mean [N], var [N], lpd [N], loss, z [N]): what the fit
        without point i predicts for y_i (the variance includes its noise), the log predictive density of y_i,
        loss = -sum lpd, and the standardised residuals z = (y - mean) / sqrt(var)."""
        if not hasattr(self.engine, "loo"):
            raise NotImplementedError(f"the leave-one-out predictive is not available on {type(self.engine).__name__}")
        self._ensure_resident()
        mean, var, lpd, loss = self.engine.loo()
        return mean, var, lpd, loss, (self._data[1][:, 0] - mean) / np.sqrt(var)

    # -- predict ------------------------------------------------------------------------------
    def _escalate(self, err, fit=False):
        """GPSO_E_PRECISION (predict) or -- ``fit=True`` -- GPSO_E_NOTPD out of a FLOAT factorisation: move data +
        hyper-parameters to an engine of the next more precise arithmetic (still on the device).  Returns False when
        there is nowhere left to go: a fit error has one step only, "float32" -> "mixed" (whose fit is the float64 one,
        the reference's arithmetic: gpso/gp_surrogate.py:490-503 -- a matrix that is not positive definite THERE is the
        caller's to see, as in the reference)."""
        cur = getattr(self.engine, "dtype_name", None)
        nxt = FIT_ESCALATION.get(cur) if fit else PRECISION_ESCALATION.get(cur)
        if nxt is None or not self.escalate or not self._owns_engine:
            return False
        logging.warning(f"{err}; reopening the GP posterior as a {nxt!r} engine on device {self._device}")
        old = self.engine
        self.engine = self._open_engine(nxt)
        old.close()
        x, y = self._data
        self.engine.set_data(x, y[:, 0])
        if self._noise_diag is not None:
            self._upload_noise_diag()
        self._resident = False
        self._device_theta = None
        return True

    def _fitting(self, call):
        """Run a fit-type engine call; a float32 engine whose factorisation is not positive definite is replaced by a
        "mixed" one (float64 fit) and the call repeated -- ``escalate=False`` keeps the raise."""
        while True:
            try:
                return call()
            except np.linalg.LinAlgError as err:
                if not self._escalate(err, fit=True):
                    raise

    def _predicting(self, call):
        """Run a predict-type engine call; a float engine that reports GPSO_E_PRECISION is replaced by
        a more precise one and the call repeated."""
        while True:
            try:
                self._ensure_resident()
                return call()
            except L.GpsoPrecisionError as err:
                if not self._escalate(err):
                    raise

    def predict_y(self, Xnew, full_cov=False):
        """(mean [M,1], var [M,1]); the variance includes the likelihood (noise) variance.  ``full_cov=True``:
        (mean [M,1], cov [M,M]) with ``predictive_noise()`` on the diagonal (M <= 1024)."""
        Xnew = np.asarray(Xnew)
        if full_cov:
            return self._predict_joint(Xnew, self.predictive_noise())
        mean, var = self._predicting(lambda: self.engine.predict(Xnew))
        return _as_result(mean), _as_result(var)

    def predict_f(self, Xnew, full_cov=False):
        """Latent mean and variance; ``full_cov=True``: (mean [M,1], cov [M,M]), GPflow's ``predict_f(Xnew, full_cov=True)``."""
        if full_cov:
            return self._predict_joint(np.asarray(Xnew), 0.0)
        mean, var = self.predict_y(Xnew)
        return mean, _as_result(np.asarray(var) - self.likelihood.variance)

    def _predict_joint(self, Xnew, diag_add):
        mean, cov = self._predicting(lambda: self.engine.predict_joint(Xnew, diag_add))
        return _as_result(mean), cov

    def predict_f_samples(self, Xnew, num_samples=1, jitter=1e-6, rng=None):
        """``num_samples`` draws [S, M] of the latent f at the rows of Xnew (M <= 1024) from their JOINT posterior: mean +
        chol(cov + jitter I) z, GPflow's ``predict_f_samples`` (1e-6 is its default_jitter).  ``rng``: a seed or a
        ``numpy.random.Generator`` -- the normals are drawn on the host, so a seed reproduces the draws."""
        Xnew = np.asarray(Xnew)
        z = _standard_normals(rng, num_samples, Xnew.shape[0])
        return self._predicting(lambda: self.engine.sample_joint(Xnew, z, jitter))[0]

    def sample_paths(self, n_paths, n_features=1024, rng=None):
        """Draw ``n_paths`` posterior FUNCTIONS of the latent f (pathwise conditioning over ``n_features`` random Fourier
        features; ``gpso_paths_draw``) and keep them on the engine until the posterior changes; ``eval_paths`` evaluates
        them at any number of points.  ``rng``: a seed or a ``numpy.random.Generator`` -- every random input is drawn on
        the host (``pygpso_amd.paths``), so a seed reproduces the set.  No counterpart in the reference."""
        from .paths import draw_path_inputs

        x, _ = self._data
        omega, phase, w, eps = draw_path_inputs(self._theta()[0], n_paths, n_features, x.shape[0], x.shape[1], rng)
        self._predicting(lambda: self.engine.paths_draw(omega, phase, w, eps))

    def _sample_paths_q(self, n_rows, n_paths, n_features, rng):
        """``sample_paths`` of the variational families (``gpso_paths_draw_q``): the same generator in the same order, the
        normals being the whitened ones over the ``n_rows`` rows the installed posterior lives on."""
        from .paths import draw_path_inputs

        omega, phase, w, eps = draw_path_inputs(self.kernel.name, n_paths, n_features, n_rows, self._data[0].shape[1], rng)
        self._predicting(lambda: self.engine.paths_draw_q(omega, phase, w, eps))

    def eval_paths(self, Xnew, seg_off=None, want_values=True):
        """The path set of ``sample_paths`` at the rows of Xnew (any M): (values [S, M] or None, best_idx [S, nseg],
        best_val [S, nseg]) -- per draw and segment of ``seg_off`` the first arg-max relative to the segment start and
        the maximum.  A posterior that changed since ``sample_paths`` raises: draw again."""
        Xnew = np.asarray(Xnew)
        return self._predicting(lambda: self.engine.paths_eval(Xnew, seg_off, want_values=want_values))

    def mc_batch(self, Xnew, q, kind, incumbent=None, incumbent_s=None, pending=None, xi=0.0, want_gain0=False):
        """``q`` rows of Xnew picked greedily by the sample-average qEI / qNoisyEI / qPI over the path set of
        ``sample_paths`` (``kind``: "qei", "qnei", "qpi"; ``gpso_paths_best_batch``): (idx, gain, batch_value) of the
        picks made, plus every row's round-0 gain [M] with ``want_gain0``.  The bars are ``incumbent_s`` [S] per draw or
        the scalar ``incumbent`` (None: the largest training target); ``pending`` [B, D] are points still being
        evaluated.  In the paths' latent units.  A posterior that changed since ``sample_paths`` raises: draw again."""
        if not hasattr(self.engine, "paths_best_batch"):
            raise NotImplementedError(f"mc_batch is not available on {type(self.engine).__name__}")
        if incumbent is None and incumbent_s is None:
            incumbent = float(np.max(self._data[1]))
        Xnew = np.asarray(Xnew)
        return self._predicting(lambda: self.engine.paths_best_batch(Xnew, q, kind, incumbent=incumbent, incumbent_s=incumbent_s,
                                                                     pending=pending, xi=xi, want_gain0=want_gain0))

    def predictive_noise(self):
        """The likelihood's variance in ``predict_y`` (the families with another likelihood override this)."""
        return self.likelihood.variance

    def predict_y_grad(self, Xnew):
        """``predict_y`` and its gradients in the rows of Xnew: (mean [M], var [M], dmean [M, D], dvar [M, D]), float64
        from the dense double factor on float64 and mixed engines (what a GPflow user gets from tf.GradientTape).  Plain
        arrays, mean and var FLAT [M] -- not the [M, 1] results of ``predict_y``."""
        Xnew = np.asarray(Xnew)
        return self._predicting(lambda: self.engine.predict_grad(Xnew))

    def predict_f_grad(self, Xnew):
        """As ``predict_y_grad`` with the likelihood's variance taken off ``var``; the gradients are the same."""
        mean, var, dmean, dvar = self.predict_y_grad(Xnew)
        return mean, var - self.predictive_noise(), dmean, dvar

    def best_ucb(self, Xnew, varsigma, seg_off=None):
        return self._predicting(lambda: self.engine.best_ucb(Xnew, varsigma, seg_off))

    def best_ucb_grow(self, bounds, depth, varsigma):
        return self._predicting(lambda: self.engine.best_ucb_grow(bounds, depth, varsigma))

    def _incumbent(self, acq, incumbent):
        """EI / log-EI / PI improve on the largest training target unless told otherwise."""
        if incumbent is None and acq.needs_incumbent and acq.incumbent is None:
            return float(np.max(self._data[1]))
        return incumbent

    def best_acq(self, Xnew, acq, seg_off=None, incumbent=None):
        """``best_ucb`` ranked by an acquisition spec (``pygpso_amd.acquisition``): (idx, mean, var, value) per segment."""
        inc = self._incumbent(acq, incumbent)
        return self._predicting(lambda: self.engine.best_acq(Xnew, acq, seg_off, incumbent=inc))

    def best_acq_grow(self, bounds, depth, acq, incumbent=None):
        inc = self._incumbent(acq, incumbent)
        return self._predicting(lambda: self.engine.best_acq_grow(bounds, depth, acq, incumbent=inc))

    def acq_values(self, Xnew, acq, incumbent=None):
        """(mean [M], var [M], value [M]): ``predict_y`` with the acquisition column, flat float64 arrays."""
        inc = self._incumbent(acq, incumbent)
        return self._predicting(lambda: self.engine.acq_values(np.asarray(Xnew), acq, incumbent=inc))

    def max_logcdf(self, mean, var, y, var_sub=0.0):
        """log P(max_j f_j < y_i) over independent leaves with the given (mean, var - var_sub): ``gpso_max_logcdf``."""
        return self._predicting(lambda: self.engine.max_logcdf(mean, var, y, var_sub))

    def max_value_samples(self, Xnew, k=16, method="paths", rng=None, n_features=1024):
        """``k`` samples of the optimum's value y* = max f over the rows of Xnew, for ``acquisition.MES(maxima=...)``
        (``pygpso_amd.mes``).  ``"paths"``: draws ``k`` posterior functions (``sample_paths``, which replaces a resident
        path set) and takes their maxima over the rows, ``eval_paths``'s ``best_val``.  ``"gumbel"``: one ``acq_values``
        call, two ``max_logcdf`` calls of 64 thresholds each (more only where the coarse grid over [max mean,
        max(mean + 6 s)] does not hold the quartiles) and a Gumbel law fitted to the 25 / 50 / 75 % points, sampled by
        inversion.  Either way the samples are CLAMPED from below at the largest training target, as Wang & Jegelka do:
        max f is at least the best value seen.  ``rng``: a seed or a ``numpy.random.Generator``; a seed reproduces them."""
        from . import mes
        from .acquisition import UCBVar

        Xnew = np.asarray(Xnew)
        k = int(k)
        if not 1 <= k <= L.ACQ_MAX_MAXIMA:
            raise ValueError(f"k={k}: 1..{L.ACQ_MAX_MAXIMA} maxima")
        best = float(np.max(self._data[1]))
        if method == "paths":
            self.sample_paths(k, n_features=n_features, rng=rng)
            return mes.clamp_at(np.asarray(self.eval_paths(Xnew, want_values=False)[2]).reshape(-1), best)
        if method != "gumbel":
            raise ValueError(f"method={method!r}: 'paths' or 'gumbel'")
        mean, var, _ = self.acq_values(Xnew, UCBVar(0.0))
        noise = float(self.predictive_noise())
        ok = ~(np.isnan(mean) | np.isnan(var))
        if not np.any(ok):
            raise ValueError("max_value_samples: every row has a NaN prediction")
        s = np.sqrt(np.maximum(var[ok] - noise, 0.0))
        a, b, _, _ = mes.gumbel_fit(lambda y: self.max_logcdf(mean, var, y, noise), np.max(mean[ok]), np.max(mean[ok] + 6.0 * s))
        return mes.clamp_at(mes.gumbel_draw(a, b, k, rng), best)

    def cross_cov(self, Xa, Xb):
        """The latent posterior covariance [B, M] between the M rows of Xa and the B <= 64 rows of Xb, cov[c, j] =
        Cov(f(Xa_j), f(Xb_c)); float64 and mixed engines."""
        Xa, Xb = np.asarray(Xa), np.asarray(Xb)
        return self._predicting(lambda: self.engine.cross_cov(Xa, Xb))

    def best_batch(self, Xnew, acq, q, obs_noise=None, incumbent=None, want_var_after=False):
        """``q`` rows of Xnew picked greedily under hallucinated updates (GP-BUCB, "kriging believer"): (idx, mean, var,
        value) of the picks made -- at most ``q`` --, plus the predictive variance [M] after them with ``want_var_after``.
        ``obs_noise``: the variance of the fantasy observations (None: ``predictive_noise()``)."""
        inc = self._incumbent(acq, incumbent)
        noise = self.predictive_noise() if obs_noise is None else obs_noise
        Xnew = np.asarray(Xnew)
        return self._predicting(lambda: self.engine.best_batch(Xnew, acq, q, float(noise), incumbent=inc, want_var_after=want_var_after))

    # -- hyper-parameter uncertainty: samples of p(theta | y) and the ensemble of their posteriors --
    def sample_hyper(self, n_samples, rng=None, **sampler_options):
        """``n_samples`` draws U [K, nu] of the posterior over the optimiser's variables, by HMC from the current
        hyper-parameters (``hyper_sampler.sample_theta`` over ``_loss_and_grad_batch``: one launch per leapfrog step for
        all chains where ``fit_batch_max() > 0``; elsewhere -- N > 128, a multi-GPU group -- the same chains through the
        row-by-row fallback: correct, and slower by the number of chains).  Needs a prior on at least one trained
        parameter (``ValueError`` otherwise).  The model's hyper-parameters are not changed; the device's posterior may be
        (the fallback fits row by row), and the next predict-type call refits where it has to.  Returns (U, info)."""
        from .hyper_sampler import sample_theta

        if self._loss_and_grad_batch is None:
            raise NotImplementedError(f"sample_hyper is not available on {type(self).__name__}")
        slots = self._prior_slots()
        proper = slots is not None and any(p is not None for p, _ in slots)
        return sample_theta(self._loss_and_grad_batch, self._pack(), n_samples, proper=proper, rng=rng, **sampler_options)

    def install_ensemble(self, U):
        """Make the posteriors at the rows of ``U [K, nu]`` (K <= 32) the engine's ensemble: per row one ``fit_eval_u`` and
        one ``ensemble_push``, then one fit back at the model's own hyper-parameters, so that the resident posterior, its
        hash and what the model knows of it are what they were.  A row whose matrix is not positive definite is skipped.
        Returns (installed, skipped)."""
        U = np.atleast_2d(np.asarray(U, dtype=np.float64))
        if not hasattr(self.engine, "ensemble_push"):
            raise NotImplementedError(f"the hyper-parameter ensemble is not available on {type(self.engine).__name__}")
        if U.shape[0] > L.ENSEMBLE_MAX:
            raise ValueError(f"install_ensemble: {U.shape[0]} rows, at most {L.ENSEMBLE_MAX}")
        self.engine.ensemble_clear()
        installed = skipped = 0
        c_fixed = float(self.mean_function.c)
        for u in U:
            try:
                self.engine.fit_eval_u(self.kernel.name, u, self.n_ls, self._train_mean, c_fixed)
            except np.linalg.LinAlgError:
                skipped += 1
                continue
            self.engine.ensemble_push()
            installed += 1
        # back at the model's own theta: the same fit the model would make, the same bits
        self._device_theta = None
        self._resident = False
        self._ensure_resident()
        return installed, skipped

    def ensemble_size(self):
        return self.engine.ensemble_info()[0] if hasattr(self.engine, "ensemble_info") else 0

    def ensemble_best_acq(self, Xnew, acq, seg_off=None, incumbent=None):
        """``best_acq`` under the integrated acquisition of the installed ensemble: (idx, mean_mix, var_mix, value)."""
        inc = self._incumbent(acq, incumbent)
        return self.engine.ensemble_best_acq(np.asarray(Xnew), acq, seg_off, incumbent=inc)

    def ensemble_acq_values(self, Xnew, acq, incumbent=None, want_members=False):
        """(mean_mix [M], var_mix [M], value [M]) of the installed ensemble (+ the members' columns [K, M])."""
        inc = self._incumbent(acq, incumbent)
        return self.engine.ensemble_acq_values(np.asarray(Xnew), acq, incumbent=inc, want_members=want_members)

    # -- outcome constraints: GP models of other outputs on this model's rows -----------------------
    def install_constraints(self, models):
        """Make ``models`` -- pairs ``(HipGPR, pygpso_amd.constraints.Constraint)``, each model trained on THIS model's
        rows with the constrained output as its targets, on an engine of its own -- the engine's constraint set: per pair
        one ``constraint_push`` (a device-to-device copy of the model's resident posterior; a fit there only if it is not
        resident).  This model's own posterior is not touched.  Returns the number installed."""
        if not hasattr(self.engine, "constraint_push"):
            raise NotImplementedError(f"outcome constraints are not available on {type(self.engine).__name__}")
        models = list(models)
        if not 1 <= len(models) <= L.CONSTRAINTS_MAX:
            raise ValueError(f"install_constraints: {len(models)} models, 1..{L.CONSTRAINTS_MAX}")
        x = self._data[0]
        for model, con in models:
            if model._data[0].shape != x.shape or not np.array_equal(model._data[0], x):
                raise ValueError(f"install_constraints: the model of {con.name!r} was trained on other rows than the objective's")
        self.engine.constraint_clear()
        for model, con in models:
            model._ensure_resident()
            self.engine.constraint_push(model.engine, con.threshold, con.sense)
        return len(models)

    def install_success(self, classifier):
        """Make ``classifier`` -- a ``HipVGP`` under the Bernoulli likelihood on an engine of its own, trained on every
        ATTEMPTED point with label 1 where the score was finite -- the engine's success member (``success_push``: a
        device-to-device copy of its installed posterior; the install there only if it is not resident).  The constrained
        calls then add its log-probability of success to logpof.  This model's own posterior is not touched."""
        if not hasattr(self.engine, "success_push"):
            raise NotImplementedError(f"a success member is not available on {type(self.engine).__name__}")
        if not getattr(classifier, "_bernoulli", False):
            raise ValueError("install_success: the classifier must be a HipVGP with likelihood=Bernoulli()")
        classifier._ensure_resident()
        self.engine.success_push(classifier.engine)

    def constraint_count(self):
        return self.engine.constraint_info()[0] if hasattr(self.engine, "constraint_info") else 0

    @staticmethod
    def _constrained_args(cacq):
        from .constraints import ConstrainedAcq

        if not isinstance(cacq, ConstrainedAcq):
            raise TypeError("a pygpso_amd.constraints.ConstrainedAcq is needed")
        return cacq.acq, cacq.mode, cacq.log_pof_min

    def constrained_best_acq(self, Xnew, cacq, seg_off=None, incumbent=None):
        """``best_acq`` under the installed constraints (``cacq``: a ``ConstrainedAcq`` over an acquisition spec):
        (idx, mean, var, value, logpof) per segment."""
        acq, mode, lpm = self._constrained_args(cacq)
        inc = self._incumbent(acq, incumbent)
        return self._predicting(lambda: self.engine.constrained_best_acq(np.asarray(Xnew), acq, mode, lpm, seg_off, incumbent=inc))

    def constrained_acq_values(self, Xnew, cacq, incumbent=None, want_members=False):
        """(mean [M], var [M], value [M], logpof [M]) under the installed constraints (+ the models' columns [J, M])."""
        acq, mode, lpm = self._constrained_args(cacq)
        inc = self._incumbent(acq, incumbent)
        return self._predicting(lambda: self.engine.constrained_acq_values(np.asarray(Xnew), acq, mode, lpm, incumbent=inc,
                                                                          want_members=want_members))

    def _ehvi_args(self, cspec):
        """``cspec``: None (value = EHVI) or a ``ConstrainedAcq`` whose mode and ``pof_min`` enter (its acquisition does not)."""
        if cspec is None:
            return None, -np.inf
        self._constrained_args(cspec)
        return cspec.mode, cspec.log_pof_min

    def ehvi_values(self, Xnew, member, front, ref, latent=True, cspec=None):
        """The exact EHVI of (this model, installed constraint model ``member``) over ``front`` [P, 2] and ``ref`` at
        ``Xnew``: (value [M], logpof [M], mean [2, M], var [2, M])."""
        if not hasattr(self.engine, "ehvi_values"):
            raise NotImplementedError(f"EHVI is not available on {type(self.engine).__name__}")
        mode, lpm = self._ehvi_args(cspec)
        return self._predicting(lambda: self.engine.ehvi_values(np.asarray(Xnew), member, front, ref, latent, mode, lpm))

    def best_ehvi(self, Xnew, member, front, ref, latent=True, cspec=None, seg_off=None):
        """Per segment the row of ``Xnew`` of the largest ``ehvi_values`` value: (idx, value, logpof, mean [2, nseg],
        var [2, nseg])."""
        if not hasattr(self.engine, "best_ehvi"):
            raise NotImplementedError(f"EHVI is not available on {type(self.engine).__name__}")
        mode, lpm = self._ehvi_args(cspec)
        return self._predicting(lambda: self.engine.best_ehvi(np.asarray(Xnew), member, front, ref, latent, mode, lpm, seg_off))

    # -- reporting ----------------------------------------------------------------------------
    def parameter_dict(self):
        return {
            ".kernel.lengthscales": np.asarray(self.kernel.lengthscales, dtype=np.float64),
            ".kernel.variance": np.float64(self.kernel.variance),
            ".likelihood.variance": np.float64(self.likelihood.variance),
            ".mean_function.c": np.float64(self.mean_function.c),
        }

    def summary(self):
        """Plain-text parameter table in the column order GPflow's print_summary uses."""
        rows = [
            ("GPR.mean_function.c", "", self.mean_function.c),
            ("GPR.kernel.variance", "Softplus", self.kernel.variance),
            ("GPR.kernel.lengthscales", "Softplus", self.kernel.lengthscales),
            ("GPR.likelihood.variance", "Softplus + Shift", self.likelihood.variance),
        ]
        lines = [f"{'name':<24} {'transform':<17} {'value'}"]
        for name, tr, val in rows:
            v = np.array2string(np.asarray(val), precision=6) if np.ndim(val) else f"{val:.6g}"
            lines.append(f"{name:<24} {tr:<17} {v}")
        return "\n".join(lines)
