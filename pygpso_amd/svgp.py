"""
``HipSVGP``: the sparse variational GP on inducing points, the model the ``SVGPSurrogate`` keeps in ``.gpflow_model``.

Stands where ``gpflow.models.SVGP`` (whitened, full ``q_sqrt``, full batch) would: M inducing points Z summarise the N
training rows as in ``HipSGPR`` (chosen the same way; trained beside the hyper-parameters with ``train_inducing=True``,
at fixed q -- q is whitened, so it stays valid while Z moves), and a whitened variational state q(v) = N(q_mu,
q_sqrt q_sqrt^T) over the M inducing values is trained against the Gaussian or the Student-t likelihood -- the robust
likelihood of ``HipVGP`` at the cost of the SGPR: O(N M^2) per natural-gradient step or -ELBO evaluation on the device,
O(M^2) per prediction.  The predictive is installed over the rows Z as the VGP's is over its training rows
(include/gpso_hip.h: gpso_svgp_posterior), so ``predict_y`` / ``best_ucb`` / ``best_ucb_grow`` run through the predict
kernels of the GPR path.  Hyper-parameters and their transforms are ``HipVGP``'s (under ``StudentT`` the likelihood's
slot of the optimiser's vector holds softplus^-1(scale), df stays fixed).

q starts at the prior whenever Z is set.  ``start_q`` puts it at the conjugate start for a non-Gaussian likelihood: one
natural-gradient step of length 1 as if the likelihood were Gaussian with the Student-t's predictive variance scale^2 df /
(df - 2).  From the prior, the Student-t's first steps are often indefinite wherever gross outliers sit.
"""
from __future__ import annotations

import types

import numpy as np

from .kernels import Gaussian, StudentT
from .model import _as_result, _softplus, _softplus_inv
from .sgpr import HipSGPR
from .vgp import GH_POINTS


class HipSVGP(HipSGPR):
    def __init__(self, data, kernel, mean_function=None, likelihood=None, num_inducing=256, inducing="greedy",
                 dtype="float64", device=0, engine=None, engine_options=None, q_mu=None, q_sqrt=None,
                 train_inducing=False):
        """``likelihood``: ``Gaussian(variance)`` (default ``Gaussian(1e-3)``) or ``StudentT(scale, df)``.
        ``num_inducing`` / ``inducing`` / ``train_inducing``: as ``HipSGPR``.  ``dtype``: "float64" or "mixed".  ``q_mu`` [M] / [M, 1] and
        ``q_sqrt`` [M, M] / [1, M, M] (optional): the variational state for the Z the data leads to."""
        if dtype not in ("float64", "mixed"):
            raise ValueError(f"SVGP trains in float64: dtype must be 'float64' or 'mixed', not {dtype!r}")
        likelihood = likelihood if likelihood is not None else Gaussian(1.0e-3)
        if not isinstance(likelihood, (Gaussian, StudentT)):
            raise NotImplementedError("the device SVGP supports the Gaussian and the Student-t likelihoods")
        self._student = isinstance(likelihood, StudentT)
        super().__init__(data, kernel, mean_function=mean_function,
                         noise_variance=1.0 if self._student else likelihood.variance, num_inducing=num_inducing,
                         inducing=inducing, dtype=dtype, device=device, engine=engine, engine_options=engine_options,
                         train_inducing=train_inducing)
        if self._student:
            self.likelihood = types.SimpleNamespace(scale=likelihood.scale, df=likelihood.df)
            self.engine.vgp_set_likelihood("StudentT", likelihood.df, GH_POINTS)
        else:
            self.engine.vgp_set_likelihood("Gaussian")
        if q_mu is not None:
            self.set_q(q_mu, q_sqrt)

    # -- q ------------------------------------------------------------------------------------------
    def start_q(self):
        """q at the prior (Gaussian likelihood) or at the conjugate start (Student-t: one Gaussian natural-gradient step
        of length 1 at the noise variance scale^2 df / (df - 2))."""
        if not self._student:
            self.engine.svgp_init_q()
        else:
            name, k, tm, c = self._args()
            self.engine.svgp_init_q(name, self._pack_theta(), k, tm, c, self.predictive_noise())
        self._resident = False

    def set_q(self, q_mu, q_sqrt):
        m = self.engine.n
        self.engine.svgp_set_q(np.asarray(q_mu, dtype=np.float64).reshape(m),
                               np.asarray(q_sqrt, dtype=np.float64).reshape(m, m))
        self._resident = False

    def get_q(self):
        """(q_mu [M], q_sqrt [M, M])."""
        return self.engine.svgp_get_q()

    # -- hyper-parameters: the likelihood's slot (as HipVGP) ----------------------------------------
    def _pack_theta(self):
        # (while HipGPR.__init__ chooses Z the likelihood is not yet the Student-t's: the selection reads only the kernel's
        # slots of u)
        if not self._student or not hasattr(self.likelihood, "scale"):
            return super()._pack_theta()
        parts = [np.atleast_1d(_softplus_inv(self.kernel.lengthscales)), [float(_softplus_inv(self.kernel.variance))],
                 [float(_softplus_inv(self.likelihood.scale))]]
        if self._train_mean:
            parts.append([self.mean_function.c])
        return np.concatenate(parts).astype(np.float64)

    def _unpack(self, u):
        ls, var, p, c = super()._unpack(u)
        if self._student:
            p = float(_softplus(np.asarray(u, dtype=np.float64)[self.n_ls + 1]))
        return ls, var, p, c

    def _assign_theta(self, u):
        if not self._student:
            return super()._assign_theta(u)
        ls, var, scale, c = self._unpack(u)
        self.kernel.lengthscales = ls.copy() if self.kernel.ard else float(ls[0])
        self.kernel.variance = var
        self.likelihood.scale = scale
        if self._train_mean:
            self.mean_function.c = c
        self._resident = False

    def predictive_noise(self):
        """The likelihood's variance in ``predict_y``: sigma^2, or scale^2 df / (df - 2) for the Student-t."""
        if self._student:
            return self.likelihood.scale ** 2 * self.likelihood.df / (self.likelihood.df - 2.0)
        return self.likelihood.variance

    # -- training -------------------------------------------------------------------------------
    def natgrad(self, gamma=1.0):
        """One natural-gradient step of length gamma in (0, 1] on q at the current hyper-parameters and Z.  An indefinite
        step raises numpy.linalg.LinAlgError and leaves q as it was."""
        if not (0.0 < gamma <= 1.0):
            raise ValueError(f"natural-gradient step {gamma} outside (0, 1]")
        name, k, tm, c = self._args()
        self._resident = False
        self.engine.svgp_natgrad(name, self._pack_theta(), k, tm, c, gamma)

    # (``_loss_and_grad`` is HipSGPR's: -ELBO at fixed q and its gradient in u, or in (u, Z) while Z is trained)
    def _eval_fixed(self, *args, **kwargs):
        return self.engine.svgp_elbo_u(*args, **kwargs)

    def _eval_moving(self, *args, **kwargs):
        return self.engine.svgp_elbo_uz(*args, **kwargs)

    def training_loss(self):
        """-ELBO at the current hyper-parameters, q and Z."""
        name, k, tm, c = self._args()
        f, _, _ = self.engine.svgp_elbo_u(name, self._pack_theta(), k, tm, c, want_grad=False)
        self._resident = False
        return f

    def log_marginal_likelihood(self):
        raise NotImplementedError("an SVGP has a lower bound of the marginal likelihood: use elbo()")

    def _ensure_resident(self):
        if not self._resident:
            name, k, tm, c = self._args()
            self.install_delta = self.engine.svgp_posterior(name, self._pack_theta(), k, tm, c)
            self._resident = True

    def predict_f(self, Xnew, full_cov=False):
        if full_cov:
            return self._predict_joint(np.asarray(Xnew), 0.0)
        mean, var = self.predict_y(Xnew)
        return mean, _as_result(np.asarray(var) - self.predictive_noise())

    # -- reporting -----------------------------------------------------------------------------
    def parameter_dict(self):
        mu, S = self.get_q()
        d = {".kernel.lengthscales": np.asarray(self.kernel.lengthscales, dtype=np.float64),
             ".kernel.variance": np.float64(self.kernel.variance)}
        if self._student:
            d[".likelihood.scale"] = np.float64(self.likelihood.scale)
        else:
            d[".likelihood.variance"] = np.float64(self.likelihood.variance)
        d[".mean_function.c"] = np.float64(self.mean_function.c)
        d[".inducing_variable.Z"] = self.inducing_points
        d[".q_mu"] = mu.reshape(-1, 1)
        d[".q_sqrt"] = S.reshape(1, S.shape[0], S.shape[1])
        return d

    def summary(self):
        rows = [
            ("SVGP.mean_function.c", "", self.mean_function.c),
            ("SVGP.kernel.variance", "Softplus", self.kernel.variance),
            ("SVGP.kernel.lengthscales", "Softplus", self.kernel.lengthscales),
            ("SVGP.likelihood.scale", "Softplus", self.likelihood.scale) if self._student else
            ("SVGP.likelihood.variance", "Softplus + Shift", self.likelihood.variance),
        ]
        lines = [f"{'name':<25} {'transform':<17} {'value'}"]
        for name, tr, val in rows:
            v = np.array2string(np.asarray(val), precision=6) if np.ndim(val) else f"{val:.6g}"
            lines.append(f"{name:<25} {tr:<17} {v}")
        m = self.engine.n
        lines.append(f"{'SVGP.inducing_variable.Z':<25} {self._z_note():<17} shape ({m}, {self._data[0].shape[1]})")
        lines.append(f"{'SVGP.q_mu':<25} {'':<17} shape ({m}, 1)")
        lines.append(f"{'SVGP.q_sqrt':<25} {'FillTriangular':<17} shape (1, {m}, {m})")
        return "\n".join(lines)
