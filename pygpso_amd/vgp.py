"""
``HipVGP``: the variational GP the ``VGPSurrogate`` keeps in ``.gpflow_model``.

Stands where ``gpflow.models.VGP`` (Gaussian or Student-t likelihood) stands in the reference (gpso/gp_surrogate.py:536-699):
whitened variational state q(v) = N(q_mu, q_sqrt q_sqrt^T) on the device beside the training data, the -ELBO and its
gradient in the hyper-parameters (``training_loss`` / ``_loss_and_grad``, driven by ``Adam`` or ``Scipy``), one natural-
gradient step on q (``natgrad``) and ``predict_y`` / ``best_ucb`` through the predict kernels of the GPR path: the
predictive is installed as (C = R L^-1, beta = L^-T mu, sigma^2, c) with I - S S^T = R^T R (include/gpso_hip.h:
gpso_vgp_posterior).  Hyper-parameters and their transforms are ``HipGPR``'s; under ``StudentT`` the likelihood's slot of
the optimiser's vector holds softplus^-1(scale) (GPflow's ``positive()``) and df stays fixed, and the per-point terms of
the ELBO and of the natural-gradient step come from GPflow's 20-point Gauss-Hermite quadrature on the device.

Data that grows between updates.  GPflow's VGP keeps q sized to the data it was built with; here the model keeps its rows
in their order of arrival: when every row it holds is still among the new data with its score, the new rows go behind
the old ones and q grows by mu = 0 and an identity block of S for them (Cholesky factors keep their leading block, so at
fixed theta this is the GP's conditional for the new rows).  When a held row disappears or its score changes, the model
takes the caller's rows in the caller's order and q restarts at the prior.
"""
from __future__ import annotations

import json
import os
import types

import numpy as np

from .kernels import KERNEL_CLASSES, Bernoulli, Constant, Gaussian, StudentT, Zero
from .model import HipGPR, _as_result, _softplus, _softplus_inv

GH_POINTS = 20  # gpflow.likelihoods.ScalarLikelihood's Gauss-Hermite points


def _row_keys(x, y):
    return [xr.tobytes() + yr.tobytes() for xr, yr in zip(np.ascontiguousarray(x), np.ascontiguousarray(y))]


def carried_order(old_x, old_y, x, y):
    """Row order of the model after new data (x, y): indices into (x, y), the rows the model held first (in its order),
    then the others in the caller's order -- or None when a held row (coordinates and score, bit for bit) is missing."""
    if old_x is None or old_x.shape[1] != x.shape[1] or x.shape[0] < old_x.shape[0]:
        return None
    where = {}
    for i, k in enumerate(_row_keys(x, y)):
        where.setdefault(k, []).append(i)
    taken = np.zeros(x.shape[0], dtype=bool)
    order = []
    for k in _row_keys(old_x, old_y):
        cand = where.get(k)
        if not cand:
            return None
        i = cand.pop(0)
        taken[i] = True
        order.append(i)
    order.extend(np.flatnonzero(~taken).tolist())
    return np.asarray(order, dtype=np.int64)


class HipVGP(HipGPR):
    _loss_and_grad_batch = None  # no batched evaluation of this loss: Scipy(restarts > 1) refuses the model

    def __init__(self, data, kernel, mean_function=None, likelihood=None, dtype="float64", device=0, engine=None,
                 engine_options=None, q_mu=None, q_sqrt=None):
        """``dtype``: "float64" or "mixed" (float64 training, float predict arithmetic).  ``q_mu`` [N] / [N, 1] and
        ``q_sqrt`` [N, N] / [1, N, N] (optional): the variational state for ``data`` in its row order."""
        if dtype not in ("float64", "mixed"):
            raise ValueError(f"VGP trains in float64: dtype must be 'float64' or 'mixed', not {dtype!r}")
        likelihood = likelihood if likelihood is not None else Gaussian()
        if not isinstance(likelihood, (Gaussian, StudentT, Bernoulli)):
            raise NotImplementedError("the device VGP supports the Gaussian, the Student-t and the Bernoulli likelihoods")
        self._student = isinstance(likelihood, StudentT)
        self._bernoulli = isinstance(likelihood, Bernoulli)
        if self._bernoulli:
            self._check_labels(data[1])
        super().__init__(data, kernel, mean_function=mean_function,
                         noise_variance=1.0 if (self._student or self._bernoulli) else likelihood.variance, dtype=dtype,
                         device=device, engine=engine, engine_options=engine_options, escalate=False)
        if self._student:
            self.likelihood = types.SimpleNamespace(scale=likelihood.scale, df=likelihood.df)
            self.engine.vgp_set_likelihood("StudentT", likelihood.df, GH_POINTS)
        if self._bernoulli:
            self.likelihood = types.SimpleNamespace(name="Bernoulli")
            self.engine.vgp_set_likelihood("Bernoulli", 0.0, GH_POINTS)
        if q_mu is not None:
            self.set_q(q_mu, q_sqrt)

    # -- data and q -------------------------------------------------------------------------------
    @property
    def data(self):
        return self._data

    @data.setter
    def data(self, value):
        x, y = value
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1, 1)
        assert x.ndim == 2 and x.shape[0] == y.shape[0]
        if self._bernoulli:
            self._check_labels(y)
        old = self._data
        order = None if old is None else carried_order(old[0], old[1], x, y)
        if order is not None:
            x, y = x[order], y[order]
        self._data = (x, y)
        self.engine.set_data(x, y[:, 0])
        if order is not None:
            self.engine.vgp_extend_q()  # q of the held rows kept, the prior for the new ones: on the device
        else:
            self.engine.vgp_set_q()
        self.q_carried = order is not None
        self._resident = False
        self._device_theta = None

    def set_q(self, q_mu, q_sqrt):
        n = self._data[0].shape[0]
        self.engine.vgp_set_q(np.asarray(q_mu, dtype=np.float64).reshape(n),
                              np.asarray(q_sqrt, dtype=np.float64).reshape(n, n))
        self._resident = False

    def get_q(self):
        """(q_mu [N], q_sqrt [N, N]) in the model's row order."""
        return self.engine.vgp_get_q()

    def append_data(self, x_new, y_new):
        """New rows behind the held ones; q grows by the prior for them (no in-place posterior update for a VGP)."""
        x = np.concatenate([self._data[0], np.atleast_2d(x_new)])
        y = np.concatenate([self._data[1], np.asarray(y_new, dtype=np.float64).reshape(-1, 1)])
        self.data = (x, y)
        return False

    @staticmethod
    def _check_labels(y):
        y = np.asarray(y, dtype=np.float64)
        if not np.all((y == 0.0) | (y == 1.0)):
            raise ValueError("the Bernoulli likelihood takes labels that are exactly 0 or 1")

    # -- hyper-parameters: the likelihood's slot ------------------------------------------------
    # Under the Bernoulli likelihood there is no likelihood parameter: the optimiser's vector (``_pack``, ``_assign``,
    # ``_loss_and_grad``) leaves the slot out; the device's layout keeps it (``_device_u``), at a fixed value nothing reads.
    def _device_u(self, u=None):
        """The vector the engine takes: the optimiser's, with the likelihood slot put back under the Bernoulli kind."""
        u = self._pack() if u is None else np.asarray(u, dtype=np.float64)
        return np.insert(u, self.n_ls + 1, 0.0) if self._bernoulli else u

    def _prior_slots(self):
        slots = super()._prior_slots()
        if slots is not None and self._bernoulli:
            del slots[self.n_ls + 1]
        return slots

    def _pack(self):
        if self._bernoulli:
            parts = [np.atleast_1d(_softplus_inv(self.kernel.lengthscales)), [float(_softplus_inv(self.kernel.variance))]]
            if self._train_mean:
                parts.append([self.mean_function.c])
            return np.concatenate(parts).astype(np.float64)
        if not self._student:
            return super()._pack()
        parts = [np.atleast_1d(_softplus_inv(self.kernel.lengthscales)), [float(_softplus_inv(self.kernel.variance))],
                 [float(_softplus_inv(self.likelihood.scale))]]
        if self._train_mean:
            parts.append([self.mean_function.c])
        return np.concatenate(parts).astype(np.float64)

    def _unpack(self, u):
        """(lengthscales, variance, likelihood parameter, c): the parameter is the Gaussian's variance or the Student-t's
        scale."""
        ls, var, p, c = super()._unpack(self._device_u(u))
        if self._student:
            p = float(_softplus(np.asarray(u, dtype=np.float64)[self.n_ls + 1]))
        return ls, var, p, c

    def _assign(self, u):
        if not (self._student or self._bernoulli):
            return super()._assign(u)
        ls, var, scale, c = self._unpack(u)
        self.kernel.lengthscales = ls.copy() if self.kernel.ard else float(ls[0])
        self.kernel.variance = var
        if self._student:
            self.likelihood.scale = scale
        if self._train_mean:
            self.mean_function.c = c
        self._resident = False

    def predictive_noise(self):
        """The likelihood's variance in ``predict_y``: sigma^2, or scale^2 df / (df - 2) for the Student-t (the closed
        form of GPflow's quadrature E[y^2] - E[y]^2)."""
        if self._student:
            return self.likelihood.scale ** 2 * self.likelihood.df / (self.likelihood.df - 2.0)
        if self._bernoulli:
            return 0.0  # (the install serves the latent f: ``predict_prob`` maps it to a probability)
        return self.likelihood.variance

    def predict_y(self, Xnew, full_cov=False):
        if self._bernoulli:
            raise NotImplementedError("a Bernoulli VGP has no Gaussian predict_y: predict_f returns the latent moments, "
                                      "predict_prob the probability of success")
        return super().predict_y(Xnew, full_cov)

    def predict_f(self, Xnew, full_cov=False):
        if full_cov:
            return self._predict_joint(np.asarray(Xnew), 0.0)
        if self._bernoulli:
            mean, var = self._predicting(lambda: self.engine.predict(np.asarray(Xnew)))
            return _as_result(mean), _as_result(var)
        mean, var = self.predict_y(Xnew)
        return mean, _as_result(np.asarray(var) - self.predictive_noise())

    def predict_prob(self, Xnew):
        """(prob [M, 1], logprob [M, 1]): P(success) = Phi(mean_f / sqrt(1 + var_f)) at the rows of Xnew (``gpso_predict_prob``)."""
        if not self._bernoulli:
            raise NotImplementedError("predict_prob needs likelihood=Bernoulli()")
        prob, logprob = self._predicting(lambda: self.engine.predict_prob(np.asarray(Xnew)))
        return _as_result(prob), _as_result(logprob)

    def sample_paths(self, n_paths, n_features=1024, rng=None):
        """``HipGPR.sample_paths`` for the installed q (``gpso_paths_draw_q``): the normals are the N whitened ones.  The
        draws come from q itself -- a Student-t install's shift is in the served variance only."""
        self._sample_paths_q(self._data[0].shape[0], n_paths, n_features, rng)

    # -- training -------------------------------------------------------------------------------
    def _args(self):
        return self.kernel.name, self.n_ls, self._train_mean, float(self.mean_function.c)

    def natgrad(self, gamma=1.0):
        """One natural-gradient step of length gamma in (0, 1] on q at the current hyper-parameters."""
        if not (0.0 < gamma <= 1.0):
            raise ValueError(f"natural-gradient step {gamma} outside (0, 1]")
        name, k, tm, c = self._args()
        self.engine.vgp_natgrad(name, self._device_u(), k, tm, c, gamma)
        self._resident = False

    def _loss_and_grad(self, u):
        """-ELBO and its gradient in u at fixed q (one device evaluation)."""
        name, k, tm, c = self._args()
        f, gu, _ = self.engine.vgp_elbo_u(name, self._device_u(u), k, tm, c)
        if self._bernoulli:
            gu = np.delete(gu, k + 1)  # (exactly 0.0 from the device: the slot is no variable of the optimiser's)
        self._last_nlml = f
        self.num_loss_evals += 1
        self._resident = False
        return f, gu

    def training_loss(self):
        """-ELBO at the current hyper-parameters and q."""
        name, k, tm, c = self._args()
        f, _, _ = self.engine.vgp_elbo_u(name, self._device_u(), k, tm, c, want_grad=False)
        self._resident = False
        return f

    def elbo(self):
        return -self.training_loss()

    def log_marginal_likelihood(self):
        raise NotImplementedError("a VGP has no exact marginal likelihood: use elbo()")

    def _ensure_resident(self):
        if not self._resident:
            name, k, tm, c = self._args()
            self.engine.vgp_posterior(name, self._device_u(), k, tm, c)
            self._resident = True

    def _escalate(self, err, fit=False):
        return False

    # -- reporting -----------------------------------------------------------------------------
    def parameter_dict(self):
        mu, S = self.get_q()
        if self._bernoulli:
            d = {".kernel.lengthscales": np.asarray(self.kernel.lengthscales, dtype=np.float64),
                 ".kernel.variance": np.float64(self.kernel.variance),
                 ".mean_function.c": np.float64(self.mean_function.c)}
        elif self._student:
            d = {".kernel.lengthscales": np.asarray(self.kernel.lengthscales, dtype=np.float64),
                 ".kernel.variance": np.float64(self.kernel.variance),
                 ".likelihood.scale": np.float64(self.likelihood.scale),
                 ".mean_function.c": np.float64(self.mean_function.c)}
        else:
            d = super().parameter_dict()
        d[".q_mu"] = mu.reshape(-1, 1)
        d[".q_sqrt"] = S.reshape(1, S.shape[0], S.shape[1])
        return d

    def summary(self):
        rows = [
            ("VGP.mean_function.c", "", self.mean_function.c),
            ("VGP.kernel.variance", "Softplus", self.kernel.variance),
            ("VGP.kernel.lengthscales", "Softplus", self.kernel.lengthscales),
        ]
        if self._student:
            rows.append(("VGP.likelihood.scale", "Softplus", self.likelihood.scale))
        elif not self._bernoulli:  # (the Bernoulli likelihood has no parameter)
            rows.append(("VGP.likelihood.variance", "Softplus + Shift", self.likelihood.variance))
        lines = [f"{'name':<24} {'transform':<17} {'value'}"]
        for name, tr, val in rows:
            v = np.array2string(np.asarray(val), precision=6) if np.ndim(val) else f"{val:.6g}"
            lines.append(f"{name:<24} {tr:<17} {v}")
        n = self._data[0].shape[0]
        lines.append(f"{'VGP.q_mu':<24} {'':<17} shape ({n}, 1)")
        lines.append(f"{'VGP.q_sqrt':<24} {'FillTriangular':<17} shape (1, {n}, {n})")
        return "\n".join(lines)

    # -- persistence of the model alone (a surrogate's folder holds more: gp_surrogate.py) -----------
    MODEL_FILE = "vgp_model.json"

    def likelihood_spec(self):
        """The likelihood as a ``pygpso_amd.kernels`` spec at its current parameters."""
        if self._bernoulli:
            return Bernoulli()
        if self._student:
            return StudentT(self.likelihood.scale, self.likelihood.df)
        return Gaussian(self.likelihood.variance)

    def save(self, folder):
        """Kernel, mean, likelihood kind and parameters, data and q as one JSON file in ``folder``."""
        os.makedirs(folder, exist_ok=True)
        lik = self.likelihood_spec()
        rec = {
            "kernel": self.kernel.name,
            "mean_function": type(self.mean_function).__name__,
            "likelihood": lik.name,
            "likelihood_args": {"Gaussian": lambda: {"variance": lik.variance}, "StudentT": lambda: {"scale": lik.scale, "df": lik.df},
                                "Bernoulli": dict}[lik.name](),
            "dtype": getattr(self.engine, "dtype_name", "float64"),
            "params": {k: np.asarray(v).tolist() for k, v in self.parameter_dict().items()},
            "x": self._data[0].tolist(), "y": self._data[1][:, 0].tolist(),
        }
        with open(os.path.join(folder, self.MODEL_FILE), "w") as fh:
            fh.write(json.dumps(rec))

    @classmethod
    def from_saved(cls, folder, device=0):
        with open(os.path.join(folder, cls.MODEL_FILE)) as fh:
            rec = json.load(fh)
        p = rec["params"]
        kernel = KERNEL_CLASSES[rec["kernel"]](lengthscales=np.array(p[".kernel.lengthscales"]), variance=p[".kernel.variance"])
        meanf = Constant(p[".mean_function.c"]) if rec["mean_function"] == "Constant" else Zero()
        likelihood = {"Gaussian": Gaussian, "StudentT": StudentT, "Bernoulli": Bernoulli}[rec["likelihood"]](**rec["likelihood_args"])
        x, y = np.array(rec["x"], dtype=np.float64), np.array(rec["y"], dtype=np.float64)[:, np.newaxis]
        return cls(data=(x, y), kernel=kernel, mean_function=meanf, likelihood=likelihood, dtype=rec.get("dtype", "float64"),
                   device=device, q_mu=np.array(p[".q_mu"]), q_sqrt=np.array(p[".q_sqrt"]))
