"""
Restatements for the hyper-parameter ensemble's tests, independent of pygpso_amd:

* ``fold_numpy``     the fold of csrc/ensemble.hpp written out in numpy for the UCB kinds and the moments -- the expression
                     the library must match bit for bit: every sum starts at its first term, index order, one division
* ``fold_truth``     the fold in mpmath at 60 digits over tests/acq_oracle.py's ``truth`` of every member's value: the mean
                     of the members' EI / PI, the LOG OF THE MEAN EI for LOGEI (finite where float64 EI is 0.0)
* ``neg_log_prior``  -sum [log p(theta(u)) + log |d theta / d u|] from scipy.stats densities
* ``members``        the float64 oracle posterior's predict_y at every theta_k (tests/hetero_oracle.py with a noise vector)
"""
import mpmath as mp
import numpy as np
from scipy import stats

from oracle import gpr
from tests import acq_oracle, hetero_oracle

UCB_VAR, UCB_STD, EI, LOGEI, PI = 0, 1, 2, 3, 4


def _seq_sum(cols):
    """((c0 + c1) + c2) + ...: numpy adds whole rows, so the order per leaf is the index order."""
    s = cols[0].copy()
    for c in cols[1:]:
        s = s + c
    return s


def moments_numpy(member_mean, member_var):
    mm, mv = np.asarray(member_mean, dtype=np.float64), np.asarray(member_var, dtype=np.float64)
    k = mm.shape[0]
    mean_mix = _seq_sum(mm) / float(k)
    var_mix = _seq_sum([mv[i] + (mm[i] - mean_mix) * (mm[i] - mean_mix) for i in range(k)]) / float(k)
    return mean_mix, var_mix


def fold_numpy(kind, member_mean, member_var, varsigma):
    """(mean_mix, var_mix, value) for UCB_VAR / UCB_STD: the written-out expression."""
    mm, mv = np.asarray(member_mean, dtype=np.float64), np.asarray(member_var, dtype=np.float64)
    k = mm.shape[0]
    if kind == UCB_VAR:
        a = [mm[i] + varsigma * mv[i] for i in range(k)]
    elif kind == UCB_STD:
        a = [mm[i] + varsigma * np.sqrt(np.maximum(mv[i], 0.0)) for i in range(k)]
    else:
        raise ValueError(kind)
    mean_mix, var_mix = moments_numpy(mm, mv)
    return mean_mix, var_mix, _seq_sum(a) / float(k)


def fold_truth(kind, member_mean, member_var, noise=None, latent=False, varsigma=0.0, incumbent=0.0, xi=0.0):
    """mpmath values [M] (mp.mpf, or -inf / nan) of the integrated acquisition."""
    mm, mv = np.asarray(member_mean, dtype=np.float64), np.asarray(member_var, dtype=np.float64)
    k, m = mm.shape
    per = []
    for i in range(k):
        add = (-float(noise[i]),) if (latent and kind != UCB_VAR) else ()
        per.append(acq_oracle.truth(EI if kind == LOGEI else kind, mm[i], mv[i], varsigma=varsigma, incumbent=incumbent, xi=xi, s2_add=add))
    out = []
    for j in range(m):
        vals = [per[i][j] for i in range(k)]
        if any(mp.isnan(v) for v in vals):
            out.append(mp.nan)
            continue
        mean = sum(vals) / k
        if kind == LOGEI:
            out.append(mp.log(mean) if mean > 0 else mp.mpf("-inf"))
        else:
            out.append(mean)
    return out


def neg_log_prior(u, slots):
    """``slots``: per variable (None | ("lognormal", median, sigma) | ("normal", mu, sigma), "softplus" | "identity")."""
    u = np.asarray(u, dtype=np.float64)
    total = 0.0
    for ui, (prior, transform) in zip(u, slots):
        if prior is None:
            continue
        x = np.logaddexp(0.0, ui) if transform == "softplus" else ui
        if prior[0] == "lognormal":
            lp = stats.lognorm(s=prior[2], scale=prior[1]).logpdf(x)
        else:
            lp = stats.norm(loc=prior[1], scale=prior[2]).logpdf(x)
        log_jac = -np.logaddexp(0.0, -ui) if transform == "softplus" else 0.0  # log sigmoid(u)
        total -= float(lp + log_jac)
    return total


def theta_from_info(kernel, row, n_ls):
    """gpso_ensemble_info's row (48 lengthscales, variance, noise, mean_c) -> the oracle's Theta."""
    ls = row[:n_ls].copy() if n_ls > 1 else float(row[0])
    return gpr.Theta(kernel, ls, float(row[48]), float(row[49]), float(row[50]))


def members(thetas, X, y, leaves, s=None):
    """(member_mean [K, M], member_var [K, M]) of the float64 oracle posteriors."""
    mean, var = [], []
    for th in thetas:
        if s is None:
            m_, v_ = gpr.predict_y(gpr.posterior(th, X, y), leaves)
        else:
            m_, v_ = hetero_oracle.predict_y(hetero_oracle.posterior(th, X, y, s), leaves)
        mean.append(m_)
        var.append(v_)
    return np.array(mean), np.array(var)
