"""CPU-only checks of the Bernoulli likelihood: the oracle of tests/vgp_bernoulli_oracle.py against
its own finite differences and against mpmath at 60 digits, the case table of the device tests, the probit map of
csrc/success.hpp through ``gpso_success_prob_host`` against mpmath, the fold with a success column through
``gpso_constrained_success_fold_host`` to the bit, and ``HipVGP(likelihood=Bernoulli())`` over the CPU stand-in engine."""
import os
from shutil import rmtree

import mpmath as mp
import numpy as np
import pytest

from pygpso_amd import HipGPEngine
from pygpso_amd import _lib as L
from pygpso_amd import acquisition as A
from pygpso_amd import kernels as K
from tests import constraints_oracle as co, mes_oracle
from tests import vgp_bernoulli_oracle as B
from tests.failures_oracle import FailuresOracleEngine

mp.mp.dps = 60
ULP = mes_oracle.ULP
VS = 2.326347874040841
HERE = os.path.dirname(os.path.abspath(__file__))
TMP = os.path.join(HERE, "_tmp_vgp_bernoulli")


# ---- the oracle ------------------------------------------------------------------------------------------------------
def _small_problem(train_mean=True):
    rng = np.random.default_rng(3)
    n, d = 9, 2
    X = rng.random((n, d))
    y = (np.sin(4.0 * X[:, 0]) + X[:, 1] > 0.9).astype(np.float64)
    assert 2 <= y.sum() <= n - 2
    u = B.initial_u([0.3, 0.45], 1.3, 0.15 if train_mean else None)
    mu = 0.3 * rng.normal(size=n)
    S = np.tril(0.1 * rng.normal(size=(n, n)), -1) + np.diag(0.5 + 0.4 * rng.random(n))
    return X, y, u, mu, S


@pytest.mark.parametrize("kernel", ("Matern52", "SquaredExponential", "Matern32"))
def test_oracle_gradient_against_central_differences(kernel):
    X, y, u, mu, S = _small_problem()
    f, g, th = B.neg_elbo_and_grad_u(kernel, u, 2, True, 0.0, X, y, mu, S)
    assert f == pytest.approx(B.neg_elbo(kernel, u, 2, True, 0.0, X, y, mu, S), rel=1e-14)
    assert g[3] == 0.0 and not np.signbit(g[3])  # the likelihood slot: exactly 0.0
    h = 1e-5
    for k in range(u.shape[0]):
        e = np.zeros_like(u)
        e[k] = h
        fd = (B.neg_elbo(kernel, u + e, 2, True, 0.0, X, y, mu, S) - B.neg_elbo(kernel, u - e, 2, True, 0.0, X, y, mu, S)) / (2 * h)
        # (central differences of a smooth function: error O(h^2 f''') + O(eps f / h), about 1e-9 here)
        assert abs(fd - g[k]) <= 1e-7 * max(1.0, abs(g[k])), (kernel, k, fd, g[k])
    # the slot is read by nothing: another value leaves loss and gradient as they are
    u2 = u.copy()
    u2[3] = 2.5
    f2, g2, _ = B.neg_elbo_and_grad_u(kernel, u2, 2, True, 0.0, X, y, mu, S)
    assert f2 == f and np.array_equal(g2, g)


def test_oracle_psi_against_mpmath():
    """psi = log Phi(s f) and psi' = s phi(f) / Phi(s f) for s f from 8 down to -40, both labels."""
    sf = np.concatenate([np.linspace(8.0, -40.0, 97), [1e-3, -1e-3, 0.0, -39.999]])
    worst = [0.0, 0.0]
    for s in (1.0, -1.0):
        f = s * sf
        psi, dpsi = B.logdensity(np.full_like(f, s), f)
        for fi, p, dp in zip(f, psi, dpsi):
            z = mp.mpf(s) * mp.mpf(float(fi))
            want = mes_oracle._log_ncdf_mp(z)
            dwant = mp.mpf(s) * mp.exp(-mp.mpf(float(fi)) ** 2 / 2) / mp.sqrt(2 * mp.pi) / mp.exp(want)
            worst[0] = max(worst[0], float(abs(mp.mpf(float(p)) - want) / abs(want)))
            worst[1] = max(worst[1], float(abs(mp.mpf(float(dp)) - dwant) / abs(dwant)))
    print(f"oracle psi: worst relative error {worst[0]:.2e}; psi': {worst[1]:.2e}")
    # psi is scipy's log_ndtr: a few ulp.  psi' exponentiates -f^2/2 - log sqrt(2 pi) - psi, a difference of numbers up to 805
    # each known to a relative 1e-15 or so: an absolute 2e-12 in the exponent at the far end, the same relative in psi'
    assert worst[0] <= 1e-13 and worst[1] <= 5e-12, worst


@pytest.mark.parametrize("n,d,kernel,ard", B.CASES)
def test_case_table_of_the_device_tests(n, d, kernel, ard):
    """Every case has at least 20 % of each label, and the oracle's Lambda of both steps keeps its smallest eigenvalue >= 1
    (the likelihood is log-concave: a >= 0, and Lambda = I + L^T diag(a) L mixed with Sigma^-1 >= I)."""
    X, y, u, n_ls = B.case_problem(n, d, kernel, ard)
    assert set(np.unique(y)) == {0.0, 1.0} and 0.2 <= y.mean() <= 0.8
    mu, S = np.zeros(n), np.eye(n)
    for gamma, shift in B.STEPS:
        lam, _ = B.natural_params(kernel, u + shift, n_ls, True, 0.0, X, y, mu, S, gamma)
        ev = np.linalg.eigvalsh(lam)
        # (>= 1 up to the rounding of the symmetric eigensolver, n eps |Lambda|)
        assert ev.min() >= 1.0 - 4.0 * n * ULP * ev.max(), (gamma, ev.min())
        mu, S = B.natgrad(kernel, u + shift, n_ls, True, 0.0, X, y, mu, S, gamma)
        assert np.linalg.eigvalsh(S @ S.T).max() <= 1.0 + 4.0 * n * ULP  # Sigma below I: the install's shift is 0


# ---- the probit map ----------------------------------------------------------------------------------------------------
GRID_Z = (40.0, 38.5, 30.0, 12.0, 8.0, 5.0, 3.0, 1.0, 0.5, 1e-3, 0.0, -1e-3, -0.5, -1.0, -1.0000001, -2.0, -5.0, -6.0, -9.999, -10.0,
          -12.0, -30.0, -38.0, -39.0, -40.0)
GRID_VAR = (0.0, 1e-12, 1e-3, 0.5, 1.0, 10.0, 1e3, 1e6)


MEASURED_LOGPROB_ERROR = 1.0e-13  # the figure in DESIGN.md section 7s: twice it is allowed, a regression of the map fails


def _prob_grid():
    mean, var = [], []
    for v in GRID_VAR:
        for z in GRID_Z:
            mean.append(float(np.float64(z) * np.sqrt(np.float64(1.0) + np.float64(v))))
            var.append(v)
    return np.array(mean), np.array(var)


def _prob_truth(mean, var):
    """(log Phi(z), its condition number in z) at z = mean / sqrt(1 + max(var, 0)), on the float64 inputs as they are."""
    lp, cond = [], []
    for m, v in zip(mean, var):
        z = mp.mpf(float(m)) / mp.sqrt(1 + max(mp.mpf(float(v)), mp.mpf(0)))
        w = mes_oracle._log_ncdf_mp(z)
        lp.append(w)
        cond.append(abs(z * mp.exp(-z * z / 2 - w) / mp.sqrt(2 * mp.pi) / w))
    return lp, cond


def test_success_prob_host_against_mpmath():
    """logprob through the host entry on a grid that puts z = mean / sqrt(1 + var) from 40 down to -40 with var from 0 to 1e6.
    Section 7r's rule: the worst relative error is MEASURED, twice that is allowed, floor 16 ulp.  Beside it a bound that is
    reasoned, per point: the library's own log Phi error (measured on section 7r's grid, constraints_oracle.log_ncdf_error) plus
    what the three roundings of z (1 + var, sqrt, the division: 1.5 ulp together) become through the condition number of
    log Phi at z -- which is z^2 in the upper tail, where log Phi(z) = -Phi(-z) is tiny and an ulp of z moves it by z^2 ulp."""
    mean, var = _prob_grid()
    z = mean / np.sqrt(1.0 + var)
    assert z.max() >= 40.0 - 1e-12 and z.min() <= -40.0 + 1e-12 and var.min() == 0.0 and var.max() == 1e6
    prob, logprob = HipGPEngine.success_prob_host(mean, var)
    want, cond = _prob_truth(mean, var)
    measured = mes_oracle.error(logprob, want)
    # (measured when this test was written, x86-64: 1.014e-13 = 457 ulp, at z = 30, var = 0.5; DESIGN.md section 7s records it)
    tol = max(2.0 * MEASURED_LOGPROB_ERROR, 16.0 * ULP)
    own = co.log_ncdf_error()
    print(f"success_prob_host: logprob worst relative error {measured:.3e} ({measured / ULP:.2f} ulp); allowed {tol / ULP:.2f} ulp; "
          f"log Phi's own error {own / ULP:.2f} ulp")
    assert np.isfinite(measured) and measured <= tol
    tiny = mp.mpf(2) ** -1022
    for j in range(mean.shape[0]):
        e = float(abs(mp.mpf(float(logprob[j])) - want[j]) / max(abs(want[j]), tiny))
        bound = max(2.0 * own, 16.0 * ULP) + 1.5 * ULP * float(cond[j])
        assert e <= bound, (mean[j], var[j], e / ULP, bound / ULP)
    # the probability is acq_exp of logprob: in [0, 1], 1/2 at mean 0, monotone in z along a row of the grid
    assert np.all((prob >= 0.0) & (prob <= 1.0))
    assert abs(HipGPEngine.success_prob_host([0.0], [3.0])[0][0] - 0.5) <= 2.0 * ULP  # (exp of a rounded log 1/2)
    for v in GRID_VAR:
        row = prob[var == v]
        assert np.all(np.diff(row) <= 0.0)
    pe = max(float(abs(mp.mpf(float(p)) - mp.exp(w)) / max(mp.exp(w), tiny)) for p, w in zip(prob, want) if mp.exp(w) > tiny)
    print(f"success_prob_host: prob worst relative error {pe:.3e}")
    # NaN in, NaN out; a negative variance is clamped; an infinite variance is the coin
    pr, lp = HipGPEngine.success_prob_host([np.nan, 1.0, 1.5, 2.0], [1.0, np.nan, -3.0, np.inf])
    assert np.isnan(lp[0]) and np.isnan(lp[1]) and np.isnan(pr[0]) and np.isnan(pr[1])
    assert lp[2] == HipGPEngine.success_prob_host([1.5], [0.0])[1][0] and lp[3] == HipGPEngine.success_prob_host([0.0], [0.0])[1][0]


# ---- the fold with a success column --------------------------------------------------------------------------------
def _columns(seed=0, m=400, nj=3):
    rng = np.random.default_rng(seed)
    mean, var = rng.standard_normal(m), rng.random(m) * 10.0 ** rng.integers(-6, 2, m) + 1e-3
    cm, cv = rng.standard_normal((nj, m)) * 2.0, rng.random((nj, m)) * 10.0 ** rng.integers(-4, 1, (nj, m)) + 2e-3
    cn = np.array([1e-3, 2e-3, 0.0])[:nj]
    thr, sense = rng.standard_normal(nj), np.array([1, -1, 1])[:nj]
    sm, sv = 2.0 * rng.standard_normal(m), rng.random(m) * 10.0 ** rng.integers(-3, 2, m)
    return mean, var, 1e-3, cm, cv, cn, thr, sense, sm, sv


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("mode", ("gate", "weight", "feasibility"))
def test_success_fold_host(mode):
    mean, var, noise, cm, cv, cn, thr, sense, sm, sv = _columns()
    acq = A.EI(xi=0.01)
    term = HipGPEngine.success_prob_host(sm, sv)[1]
    # J = 0: the success term IS logpof, bit for bit
    lp0 = HipGPEngine.constrained_success_fold_host(acq, mean, var, noise, None, None, None, None, None, sm, sv, "feasibility", incumbent=0.3)[1]
    assert np.array_equal(_bits(lp0), _bits(term))
    # J > 0: gpso_constrained_fold_host's logpof plus the success term, in that association
    for nj in (1, 3):
        base = HipGPEngine.constrained_fold_host(acq, mean, var, noise, cm[:nj], cv[:nj], cn[:nj], thr[:nj], sense[:nj], "feasibility",
                                                 incumbent=0.3)[1]
        lp = HipGPEngine.constrained_success_fold_host(acq, mean, var, noise, cm[:nj], cv[:nj], cn[:nj], thr[:nj], sense[:nj], sm, sv,
                                                       "feasibility", incumbent=0.3)[1]
        assert np.array_equal(_bits(lp), _bits(base + term)), nj
        # the mode's value is what section 7r's fold makes of that logpof: checked against the plain fold of ONE member whose
        # log-probability of feasibility is exactly this logpof cannot be arranged, so the rules are restated here
        gate = float(np.median(lp))
        val, lp2 = HipGPEngine.constrained_success_fold_host(acq, mean, var, noise, cm[:nj], cv[:nj], cn[:nj], thr[:nj], sense[:nj], sm, sv,
                                                             mode, gate, incumbent=0.3)
        assert np.array_equal(_bits(lp2), _bits(lp))
        a0 = HipGPEngine.acq_eval_host(acq, mean, var, noise, incumbent=0.3)
        keep = lp >= gate
        assert keep.any() and (~keep).any()
        if mode == "feasibility":
            assert np.array_equal(_bits(val), _bits(lp))
        elif mode == "gate":
            assert np.array_equal(_bits(val[keep]), _bits(a0[keep])) and np.all(np.isneginf(val[~keep]))
            open_gate = HipGPEngine.constrained_success_fold_host(acq, mean, var, noise, cm[:nj], cv[:nj], cn[:nj], thr[:nj], sense[:nj],
                                                                  sm, sv, "gate", -np.inf, incumbent=0.3)[0]
            assert np.array_equal(_bits(open_gate), _bits(a0))
        else:
            assert np.all(np.isneginf(val[~keep])) and np.all(np.isfinite(val[keep])) and np.all(val[keep] <= a0[keep])
            lval = HipGPEngine.constrained_success_fold_host(A.LogEI(xi=0.01), mean, var, noise, cm[:nj], cv[:nj], cn[:nj], thr[:nj],
                                                             sense[:nj], sm, sv, "weight", gate, incumbent=0.3)[0]
            l0 = HipGPEngine.acq_eval_host(A.LogEI(xi=0.01), mean, var, noise, incumbent=0.3)
            assert np.array_equal(_bits(lval[keep]), _bits((l0 + lp)[keep]))
    # a NaN in any column gives NaN; -inf is preserved (a UCB kind cannot be weighted: EI there)
    one = np.ones(1)
    acq1, inc = (A.EI(), 0.0) if mode == "weight" else (A.UCBVar(VS), None)
    for kw in (dict(sm=[np.nan]), dict(sv=[np.nan]), dict(cm=[[np.nan]])):
        a = dict(cm=[[0.0]], cv=[[1.0]], sm=[0.5], sv=[1.0])
        a.update(kw)
        val, lp = HipGPEngine.constrained_success_fold_host(acq1, one, one, 0.0, a["cm"], a["cv"], [0.0], [0.0], [1], a["sm"], a["sv"],
                                                            mode, -1.0, incumbent=inc)
        assert np.isnan(lp[0]) and np.isnan(val[0]), kw
    val, lp = HipGPEngine.constrained_success_fold_host(acq1, one, one, 0.0, [[0.5]], [[0.0]], [0.0], [0.0], [1], [0.5], [1.0], mode, -1.0, incumbent=inc)
    assert lp[0] == -np.inf and val[0] == -np.inf  # (the constraint is violated with certainty: s2 = 0 beyond the threshold)
    val, lp = HipGPEngine.constrained_success_fold_host(acq1, one, one, 0.0, None, None, None, None, None, [-1e200], [0.0], mode, -1.0, incumbent=inc)
    assert lp[0] == -np.inf and val[0] == -np.inf  # (log Phi of -1e200 overflows its square: -inf, not NaN)
    # refusals of the record
    with pytest.raises(L.GpsoHipError):
        HipGPEngine.constrained_success_fold_host(A.MES(), mean, var, noise, None, None, None, None, None, sm, sv, mode)
    with pytest.raises(L.GpsoHipError):
        HipGPEngine.constrained_success_fold_host(A.UCBVar(VS), mean, var, noise, None, None, None, None, None, sm, sv, "weight")


# ---- HipVGP(likelihood=Bernoulli()) over the stand-in ---------------------------------------------------------------------
def _model(X, y, lengthscales=0.3, **kw):
    from pygpso_amd.vgp import HipVGP

    return HipVGP(data=(X, y[:, None]), kernel=K.Matern52(lengthscales=lengthscales, variance=1.2), mean_function=K.Constant(0.1),
                  likelihood=K.Bernoulli(), engine=FailuresOracleEngine(), **kw)


def test_hipvgp_bernoulli_host_layer():
    X, y, _, _ = B.case_problem(60, 2, "Matern52", False)
    with pytest.raises(ValueError, match="exactly 0 or 1"):
        _model(X, y + 0.25)
    model = _model(X, y)
    # the likelihood slot is no variable of the optimiser's: (lengthscale, variance, c)
    u = model.trainable_variables
    assert u.shape == (3,)
    f, g = model._loss_and_grad(u)
    assert g.shape == (3,)
    u_dev = model._device_u(u)
    assert u_dev.shape == (4,) and u_dev[2] == 0.0
    f_ref, g_ref, _ = B.neg_elbo_and_grad_u("Matern52", u_dev, 1, True, 0.0, X, y, np.zeros(60), np.eye(60))
    assert f == f_ref and np.array_equal(g, np.delete(g_ref, 2))
    adam = K.Adam(0.05)
    for _ in range(3):
        model.natgrad(0.5)
        adam.minimize(model.training_loss, model.trainable_variables)
    assert not np.array_equal(model.trainable_variables, u)
    Xs = np.random.default_rng(0).random((50, 2))
    with pytest.raises(NotImplementedError, match="predict_f"):
        model.predict_y(Xs)
    mean, var = model.predict_f(Xs)
    post = model.engine.bpost
    m_ref, v_ref = post.predict_f(Xs)
    assert np.array_equal(np.asarray(mean)[:, 0], m_ref) and np.array_equal(np.asarray(var)[:, 0], v_ref)
    prob, logprob = model.predict_prob(Xs)
    p_ref, lp_ref = post.predict_prob(Xs)
    np.testing.assert_allclose(np.asarray(logprob)[:, 0], lp_ref, rtol=1e-13)
    np.testing.assert_allclose(np.asarray(prob)[:, 0], p_ref, rtol=1e-13)
    # the classifier has learnt the labels' side of the boundary at its own training points
    pt = np.asarray(model.predict_prob(X)[0])[:, 0]
    assert np.mean((pt > 0.5) == (y > 0.5)) >= 0.85
    pd = model.parameter_dict()
    assert ".likelihood.variance" not in pd and ".likelihood.scale" not in pd and "likelihood" not in model.summary()
    # growing data keeps q for the held rows; labels that are not 0 / 1 are refused there too
    with pytest.raises(ValueError, match="exactly 0 or 1"):
        model.append_data(Xs[:1], [0.5])
    mu0, _ = model.get_q()
    model.append_data(Xs[:2], [1.0, 0.0])
    mu1, _ = model.get_q()
    assert model.q_carried and np.array_equal(mu1[:60], mu0) and np.all(mu1[60:] == 0.0)


@pytest.mark.parametrize("ard", (False, True))
def test_hipvgp_save_and_from_saved_round_trip_the_kind(monkeypatch, ard):
    from pygpso_amd import vgp

    X, y, _, _ = B.case_problem(*((60, 2, "Matern52", True) if ard else (7, 1, "Matern12", False)))
    model = _model(X, y, lengthscales=np.array([0.3, 0.45]) if ard else 0.3)
    model.natgrad(1.0)
    model.save(TMP)
    try:
        # (from_saved opens an engine of its own: the stand-in here, a HipGPEngine on the device)
        monkeypatch.setattr(vgp.HipVGP, "_open_engine", lambda self, dtype: FailuresOracleEngine())
        back = vgp.HipVGP.from_saved(TMP)
        assert back._bernoulli and isinstance(back.likelihood_spec(), K.Bernoulli) and back.kernel.name == "Matern52"
        assert back.kernel.ard == ard and back.n_ls == (2 if ard else 1)
        a, b = model.parameter_dict(), back.parameter_dict()
        assert sorted(a) == sorted(b)
        for k in a:
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]))
        np.testing.assert_array_equal(back.data[1], model.data[1])
        Xs = np.random.default_rng(4).random((11, X.shape[1]))
        for p, q in zip(model.predict_prob(Xs), back.predict_prob(Xs)):
            np.testing.assert_array_equal(np.asarray(p), np.asarray(q))
    finally:
        rmtree(TMP, ignore_errors=True)
