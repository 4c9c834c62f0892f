"""
``HipSGPR``: sparse GP regression on inducing points, the model the ``SGPRSurrogate`` keeps in ``.gpflow_model``.

Stands where ``gpflow.models.SGPR`` (Titsias 2009, Gaussian likelihood) would: M inducing points Z summarise the N training
rows, ``training_loss`` is the negative collapsed bound and costs O(N M^2) on the device, and a prediction costs O(M^2)
whatever N: the predictive is installed as a whitened Gaussian over the M rows Z (include/gpso_hip.h: gpso_sgpr_posterior),
so ``predict_y`` / ``best_ucb`` / ``best_ucb_grow`` run through the predict kernels of the GPR path.  Hyper-parameters and
their transforms are ``HipGPR``'s.  Z is chosen by ``choose_inducing`` -- the data itself while N <= M, beyond that the
greedy conditional-variance selection on the device (pivoted partial Cholesky of k(X, X)) at the current kernel
hyper-parameters, or an array given by the caller.  With ``train_inducing=False`` (the default) that Z stays fixed (GPflow's
``set_trainable(model.inducing_variable, False)``) and is chosen again at every change of the data.  With
``train_inducing=True`` it is GPflow's default: the choice only names where Z starts, the optimiser's vector is (u, Z) and
the bound is maximised over both (include/gpso_hip.h: gpso_sgpr_bound_uz); the trained Z is kept across changes of the
data, so the selection runs once, when N first exceeds M.  While N <= M, Z is the data and is not trained.
"""
from __future__ import annotations

import numpy as np

from .model import HipGPR, _as_result


class HipSGPR(HipGPR):
    _loss_and_grad_batch = None  # no batched evaluation of this loss: Scipy(restarts > 1) refuses the model

    def __init__(self, data, kernel, mean_function=None, noise_variance=1.0e-3, num_inducing=256, inducing="greedy",
                 dtype="float64", device=0, engine=None, engine_options=None, train_inducing=False):
        """``num_inducing``: M.  ``inducing``: "greedy" or an [M, D] array used as given (with ``train_inducing``: where Z
        starts).  ``dtype``: "float64" or "mixed" (float64 training, float predict arithmetic).  ``train_inducing``: search
        (u, Z) jointly whenever N > M."""
        if dtype not in ("float64", "mixed"):
            raise ValueError(f"SGPR trains in float64: dtype must be 'float64' or 'mixed', not {dtype!r}")
        if isinstance(inducing, str):
            if inducing != "greedy":
                raise ValueError(f"inducing must be 'greedy' or an [M, D] array, not {inducing!r}")
            if int(num_inducing) < 1:
                raise ValueError(f"num_inducing={num_inducing}: need at least one inducing point")
            self.inducing_policy, self._z_given = "greedy", None
            self.num_inducing = int(num_inducing)
        else:
            z = np.ascontiguousarray(inducing, dtype=np.float64)
            if z.ndim != 2 or z.shape[0] < 1 or not np.all(np.isfinite(z)):
                raise ValueError("inducing must be a finite [M, D] array with M >= 1")
            self.inducing_policy, self._z_given = "given", z
            self.num_inducing = int(z.shape[0])
        if not isinstance(train_inducing, (bool, np.bool_)):
            raise TypeError(f"train_inducing must be True or False, not {train_inducing!r}")
        self.train_inducing = bool(train_inducing)
        self._z = None  # Z as the optimiser sees it, [M, D], while it is trained (N > M); None: Z is fixed
        self._z_device = None  # the Z the device is known to hold while Z is trained (None: unknown)
        self.inducing_index = None  # rows of the data the greedy selection picked (None: Z is the data or was given)
        self.install_delta = 0.0    # shift of the last install (0: the served variance is exact)
        super().__init__(data, kernel, mean_function=mean_function, noise_variance=noise_variance, dtype=dtype,
                         device=device, engine=engine, engine_options=engine_options, escalate=False)

    # -- data and Z -------------------------------------------------------------------------------
    @property
    def data(self):
        return self._data

    @data.setter
    def data(self, value):
        x, y = value
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1, 1)
        assert x.ndim == 2 and x.shape[0] == y.shape[0]
        if self._z_given is not None and self._z_given.shape[1] != x.shape[1]:
            raise ValueError(f"inducing points have D={self._z_given.shape[1]}, the data D={x.shape[1]}")
        self._data = (x, y)
        self._resident = False
        self._device_theta = None
        self.choose_inducing()

    def choose_inducing(self):
        """(Re-)choose Z for the current data at the current kernel hyper-parameters and put both on the device.  With
        ``train_inducing`` and N > M a trained Z of shape [M, D] that is held is kept instead, and nothing is selected."""
        x, y = self._data
        self.engine.set_data(x, y[:, 0])
        self.inducing_index = None
        trains = self.train_inducing and x.shape[0] > self.num_inducing
        if trains and self._z is not None and self._z.shape == (self.num_inducing, x.shape[1]):
            self.engine.sgpr_set_inducing(self._z)
        else:
            self._z = None
            if self._z_given is not None:
                self.engine.sgpr_set_inducing(self._z_given)
            elif x.shape[0] <= self.num_inducing:
                self.engine.sgpr_set_inducing(x)
            else:
                self.inducing_index = self.engine.sgpr_select_inducing(self.kernel.name, self._pack_theta(), self.n_ls,
                                                                       self.num_inducing)
            if trains:
                self._z = self.engine.sgpr_get_inducing()[0]
        self._z_device = None if self._z is None else self._z.copy()
        self._resident = False

    @property
    def inducing_points(self):
        """Z [M, D] as the device holds it."""
        return self.engine.sgpr_get_inducing()[0]

    def set_inducing(self, Z):
        """Use Z [M, D] as given for the current data (kept until the data changes, unless the policy is an array)."""
        z = np.ascontiguousarray(Z, dtype=np.float64)
        x, y = self._data
        self.engine.set_data(x, y[:, 0])
        self.engine.sgpr_set_inducing(z)
        self.inducing_index = None
        self._resident = False
        trains = self.train_inducing and x.shape[0] > self.num_inducing and z.shape == (self.num_inducing, x.shape[1])
        self._z = z.copy() if trains else None
        self._z_device = None if self._z is None else self._z.copy()

    def append_data(self, x_new, y_new):
        """New rows behind the held ones; Z is chosen again, or a trained Z kept (no in-place posterior update for an
        SGPR)."""
        x = np.concatenate([self._data[0], np.atleast_2d(x_new)])
        y = np.concatenate([self._data[1], np.asarray(y_new, dtype=np.float64).reshape(-1, 1)])
        self.data = (x, y)
        return False

    # -- the optimiser's vector: u, and behind it Z row by row while Z is trained ----------------------
    def _pack_theta(self):
        return super()._pack()

    def _assign_theta(self, u):
        super()._assign(u)

    def _n_theta(self):
        return self.n_ls + 2 + (1 if self._train_mean else 0)

    def _pack(self):
        u = self._pack_theta()
        return u if self._z is None else np.concatenate([u, self._z.ravel()])

    def _assign(self, u):
        u = np.asarray(u, dtype=np.float64)
        nt = self._n_theta()
        self._assign_theta(u[:nt])
        if self._z is not None:
            self._z = u[nt:].reshape(self._z.shape).copy()
            self._put_z()

    def _put_z(self):
        """Make the device's inducing rows the model's Z, unless they already are (L-BFGS-B's last evaluation is, as a
        rule, at the point it returns)."""
        if self._z_device is None or not np.array_equal(self._z_device, self._z):
            self.engine.sgpr_move_inducing(self._z)
            self._z_device = self._z.copy()

    # -- training -------------------------------------------------------------------------------
    def _args(self):
        return self.kernel.name, self.n_ls, self._train_mean, float(self.mean_function.c)

    def _eval_fixed(self, *args, **kwargs):
        return self.engine.sgpr_bound_u(*args, **kwargs)

    def _eval_moving(self, *args, **kwargs):
        return self.engine.sgpr_bound_uz(*args, **kwargs)

    def _loss_and_grad(self, u):
        """The loss and its gradient in the optimiser's vector (one device evaluation): in u at fixed Z, or -- while Z is
        trained -- in (u, Z)."""
        name, k, tm, c = self._args()
        if self._z is None:
            f, g, _ = self._eval_fixed(name, u, k, tm, c)
        else:
            u = np.asarray(u, dtype=np.float64)
            nt = self._n_theta()
            z = u[nt:].reshape(self._z.shape)
            same = self._z_device is not None and np.array_equal(self._z_device, z)
            try:  # (Z travels only when the device holds another one)
                f, gu, gz, _ = self._eval_moving(name, u[:nt], k, tm, c, Z=None if same else z)
            except Exception:
                # an evaluation that fails (Kuu not positive definite where rows of Z collapse) has already replaced the
                # device's rows: put the Z the model holds back, so that model and device speak of the same Z
                self._z_device = None
                self._put_z()
                raise
            self._z_device = z.copy()
            g = np.concatenate([gu, gz.ravel()])
        self._last_nlml = f
        self.num_loss_evals += 1
        self._resident = False
        return f, g

    def training_loss(self):
        """-bound at the current hyper-parameters and Z."""
        name, k, tm, c = self._args()
        f, _, _ = self.engine.sgpr_bound_u(name, self._pack_theta(), k, tm, c, want_grad=False)
        self._resident = False
        return f

    def elbo(self):
        return -self.training_loss()

    def log_marginal_likelihood(self):
        raise NotImplementedError("an SGPR has a lower bound of the marginal likelihood: use elbo()")

    def _ensure_resident(self):
        if not self._resident:
            name, k, tm, c = self._args()
            self.install_delta = self.engine.sgpr_posterior(name, self._pack_theta(), k, tm, c)
            self._resident = True

    def _escalate(self, err, fit=False):
        return False

    def predict_f(self, Xnew, full_cov=False):
        """Latent mean and variance.  After a shifted install (``install_delta`` > 0) the variance keeps the shift's
        surplus delta (k** - |Lu^-1 k*u|^2) >= 0: never below the exact latent variance."""
        if full_cov:
            return self._predict_joint(np.asarray(Xnew), 0.0)
        mean, var = self.predict_y(Xnew)
        return mean, _as_result(np.asarray(var) - self.likelihood.variance)

    def sample_paths(self, n_paths, n_features=1024, rng=None):
        """``HipGPR.sample_paths`` for the installed posterior over Z (``gpso_paths_draw_q``; ``HipSVGP`` inherits it): the
        normals are the M whitened ones, and a path costs O(M + F) a point whatever N."""
        self._sample_paths_q(int(self.engine.n), n_paths, n_features, rng)

    # -- reporting -----------------------------------------------------------------------------
    def _z_note(self):
        return "(trained)" if self._z is not None else "(not trained)"

    def parameter_dict(self):
        d = super().parameter_dict()
        d[".inducing_variable.Z"] = self.inducing_points
        return d

    def summary(self):
        lines = super().summary().replace("GPR.", "SGPR.").split("\n")
        z = self.inducing_points
        lines.append(f"{'SGPR.inducing_variable.Z':<24} {self._z_note():<17} shape {z.shape}")
        return "\n".join(lines)
