"""
The stand-in engine of the CPU loop tests of ``failures="classify"``: tests/constraints_oracle.py's
stand-in with the variational calls under the Bernoulli likelihood (tests/vgp_bernoulli_oracle.py), ``predict_prob`` and the
success member.  The constrained calls apply the LIBRARY's host fold (``gpso_constrained_success_fold_host``) to the oracle's
columns -- the device applies the same header to its own.  Test infrastructure only.
"""
import numpy as np

from tests import vgp_bernoulli_oracle as B
from tests.constraints_oracle import ConstraintOracleEngine


class FailuresOracleEngine(ConstraintOracleEngine):
    dtype_name = "float64"

    def __init__(self, dtype="float64", device=0):
        super().__init__(dtype, device)
        self._lik = "Gaussian"
        self._q = None       # (mu, S) of the variational state
        self.bpost = None    # the Bernoulli install: a B.Posterior
        self._suc = None     # the success member: a copy of a source's B.Posterior
        self.closed = False

    def close(self):
        self.closed = True

    # -- data: whatever posterior was resident is dropped, the success member stays (it is the context's)
    def set_data(self, X, y):
        super().set_data(X, y)
        self.bpost = None

    def fit_eval(self, *args, **kwargs):
        self.bpost = None
        return super().fit_eval(*args, **kwargs)

    # -- the variational GP under the Bernoulli likelihood
    def vgp_set_likelihood(self, kind="Gaussian", df=3.0, n_gh=20):
        assert kind == "Bernoulli" and n_gh == B.N_GH, "the stand-in serves the Bernoulli kind only"
        self._lik = kind

    def vgp_set_q(self, mu=None, S=None):
        self._q = (np.zeros(self.n), np.eye(self.n)) if mu is None else (np.array(mu, dtype=np.float64), np.array(S, dtype=np.float64))
        self.bpost = None

    def vgp_extend_q(self):
        mu0, S0 = self._q
        n0 = mu0.shape[0]
        assert n0 <= self.n
        mu, S = np.zeros(self.n), np.eye(self.n)
        mu[:n0], S[:n0, :n0] = mu0, S0
        self._q = (mu, S)
        self.bpost = None

    def vgp_get_q(self):
        return self._q[0].copy(), self._q[1].copy()

    def vgp_natgrad(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, gamma=1.0):
        assert self._lik == "Bernoulli"
        self._q = B.natgrad(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, *self._q, gamma)
        self.bpost = None

    def vgp_elbo_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, want_grad=True):
        assert self._lik == "Bernoulli"
        f, g, th = B.neg_elbo_and_grad_u(kernel, u, n_ls, train_mean, mean_c_fixed, self.X, self.y, *self._q)
        self.bpost = None
        return f, (g if want_grad else None), th

    def vgp_posterior(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        assert self._lik == "Bernoulli"
        self.bpost = B.Posterior(kernel, np.array(u, dtype=np.float64), n_ls, train_mean, mean_c_fixed, self.X.copy(), *self.vgp_get_q())
        self.post = None

    def predict(self, xs, out=None):
        if self.bpost is not None:  # (a Bernoulli install serves the latent moments)
            return self.bpost.predict_f(np.asarray(xs, dtype=np.float64))
        return super().predict(xs, out)

    def predict_prob(self, xs, want_latent=False):
        from pygpso_amd import HipGPEngine

        assert self.bpost is not None
        mean, var = self.bpost.predict_f(np.asarray(xs, dtype=np.float64))
        pr, lp = HipGPEngine.success_prob_host(mean, var)
        return (pr, lp, mean, var) if want_latent else (pr, lp)

    # -- the success member
    def success_push(self, src):
        assert src.bpost is not None and src.bpost.X.shape[0] <= 128 and (self.n == 0 or src.bpost.X.shape[1] == self.d)
        self._suc = src.bpost

    def success_clear(self):
        self._suc = None

    def success_info(self):
        return self._suc is not None, (0 if self._suc is None else self._suc.X.shape[0]), None

    def constrained_acq_values(self, xs, acq, mode="gate", log_pof_min=-np.inf, incumbent=None, want_members=False):
        from pygpso_amd import HipGPEngine

        if self._suc is None:
            return super().constrained_acq_values(xs, acq, mode, log_pof_min, incumbent, want_members)
        xs = np.asarray(xs, dtype=np.float64)
        mean, var = self.predict(xs)
        mm, mv = self.member_columns(xs) if self._con else (np.zeros((0, xs.shape[0])), np.zeros((0, xs.shape[0])))
        sm, sv = self._suc.predict_f(xs)
        val, lp = HipGPEngine.constrained_success_fold_host(
            acq, mean, var, self.post.theta.noise, mm, mv, [p.theta.noise for p, _, _ in self._con], [c[1] for c in self._con],
            [c[2] for c in self._con], sm, sv, mode, log_pof_min, incumbent)
        if want_members:
            return mean, var, val, lp, np.vstack([mm, sm[None]]), np.vstack([mv, sv[None]])
        return mean, var, val, lp
