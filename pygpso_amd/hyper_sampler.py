"""
Samples of p(u | y): plain Hamiltonian Monte Carlo over the optimiser's variables, C chains in lockstep (host side;
DESIGN.md section 7q).

The target is exp(-loss(u)), loss the model's training loss WITH its prior term (``priors.neg_log_prior_u``: the Jacobian
makes it a density in u).  The only coupling to the device is one callable,

    loss_and_grad_batch(U [C, nu]) -> (loss [C], grad [C, nu], ok [C])

``HipGPR._loss_and_grad_batch``: at N <= 128 that is ONE launch of the batched one-launch fit whatever C is (up to 256
rows), so C chains cost what one chain costs.  Every leapfrog step is one such call.  A row that comes back ``ok == False``
(not positive definite) or with a non-finite loss or gradient makes its chain's proposal a rejected one -- never an
exception.  Identity mass; the step size is adapted towards a target acceptance during burn-in only (Robbins-Monro on
log step, frozen at the average of the second half of burn-in); afterwards every iteration uses the frozen step times a
uniform factor in [0.8, 1.2] drawn from the same generator, so the kept draws come from one fixed mixture of kernels and no
trajectory length can sit on a period of the target.  Every random number comes from the caller's ``rng``.

The defaults (8 chains, 60 burn-in iterations, 10 leapfrog steps of 0.1, every 5th iteration kept, target acceptance 0.8)
are design choices for 3 .. 50 variables whose posterior scale in u is of order one; they are not measurements.
"""
from __future__ import annotations

import numpy as np


def _evaluate(batch, U, info):
    loss, grad, ok = batch(U)
    info["batch_calls"] += 1
    loss = np.array(loss, dtype=np.float64).reshape(-1)
    grad = np.array(grad, dtype=np.float64).reshape(U.shape)
    fine = np.asarray(ok, dtype=bool).reshape(-1) & np.isfinite(loss) & np.all(np.isfinite(grad), axis=1)
    return loss, grad, fine


def _keep_schedule(n_samples, chains, thin):
    """Per chain the post-burn-in iterations whose state is kept: n_samples spread over the chains as evenly as it goes
    (the first n_samples % chains chains keep one more), each chain's draws spread evenly over the T iterations."""
    per = [n_samples // chains + (1 if c < n_samples % chains else 0) for c in range(chains)]
    total = thin * max(per)
    return total, [set(((j + 1) * total) // n - 1 for j in range(n)) if n else set() for n in per]


def sample_theta(loss_and_grad_batch, u0, n_samples, *, proper, chains=8, burn=60, leapfrog=10, step=0.1, thin=5,
                 target_accept=0.8, init_scale=0.1, rng=None):
    """``n_samples`` draws U [K, nu] of the density exp(-loss(u)) and an ``info`` dictionary.

    ``proper``: whether the target has a prior on at least one trained parameter; the caller must say.  False raises
    ``ValueError``: the likelihood alone is flat in some directions of u (a lengthscale going to infinity) and the chains
    would wander off.  ``u0``: where chain 0 starts; the others start at u0 + ``init_scale`` * N(0, 1), and one whose start
    does not evaluate is put back at u0.  ``burn`` = 0 keeps ``step`` as given.  ``rng``: a seed or a
    ``numpy.random.Generator``; the same seed gives the same samples.
    ``info``: ``accept_rate`` [chains] (after burn-in), ``step`` (the frozen BASE step: an iteration runs at it times its
    own uniform factor in [0.8, 1.2], so no iteration uses exactly this number), ``batch_calls``, ``restarted`` (chains
    put back at u0), ``failed_rows`` (proposals rejected because a row did not evaluate)."""
    if not proper:
        raise ValueError("sample_theta: the target has no prior on any trained parameter -- a flat prior in u is improper; "
                         "attach priors (pygpso_amd.priors) first")
    n_samples, chains, burn, leapfrog, thin = int(n_samples), int(chains), int(burn), int(leapfrog), int(thin)
    if n_samples < 1 or chains < 1 or burn < 0 or leapfrog < 1 or thin < 1:
        raise ValueError("sample_theta: n_samples, chains, leapfrog, thin >= 1 and burn >= 0")
    if not (step > 0.0 and np.isfinite(step)) or not 0.0 < target_accept < 1.0:
        raise ValueError("sample_theta: step must be positive and finite, target_accept inside (0, 1)")
    gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    u0 = np.array(u0, dtype=np.float64).reshape(-1)
    nu = u0.shape[0]
    info = {"batch_calls": 0, "restarted": 0, "failed_rows": 0}

    q = u0 + init_scale * gen.standard_normal((chains, nu))
    q[0] = u0
    f, g, fine = _evaluate(loss_and_grad_batch, q, info)
    if not fine[0]:  # (chain 0 stands at u0)
        raise ValueError("sample_theta: the loss does not evaluate at u0")
    bad = ~fine  # a chain whose start does not evaluate starts at u0, with chain 0's loss and gradient there
    info["restarted"] = int(np.sum(bad))
    q[bad], f[bad], g[bad] = u0, f[0], g[0]

    total, keep = _keep_schedule(n_samples, chains, thin)
    log_step, log_steps = float(np.log(step)), []
    kept = [[] for _ in range(chains)]
    accepted = np.zeros(chains)
    for it in range(burn + total):
        # (the iteration's step: the adapted one, times a uniform factor in [0.8, 1.2] -- a fixed trajectory length that
        # happens to be a period of the target would bring every chain back to where it started)
        eps = float(np.exp(log_step)) * float(gen.uniform(0.8, 1.2))
        p = gen.standard_normal((chains, nu))
        h0 = f + 0.5 * np.sum(p * p, axis=1)
        qn, fn, gn = q.copy(), f.copy(), g.copy()
        alive = np.ones(chains, dtype=bool)
        p = p - 0.5 * eps * gn
        for l in range(leapfrog):
            qn = np.where(alive[:, None], qn + eps * p, q)  # (a dead chain's row goes back to its state: it evaluates, and is ignored)
            fn, gn, fine = _evaluate(loss_and_grad_batch, qn, info)
            info["failed_rows"] += int(np.sum(alive & ~fine))
            alive &= fine
            gn = np.where(alive[:, None], gn, 0.0)
            p = p - (eps if l + 1 < leapfrog else 0.5 * eps) * gn
        with np.errstate(over="ignore", invalid="ignore"):
            h1 = np.where(alive, fn + 0.5 * np.sum(p * p, axis=1), np.inf)
            prob = np.where(alive, np.minimum(1.0, np.exp(np.minimum(h0 - h1, 0.0))), 0.0)
        prob = np.where(np.isfinite(prob), prob, 0.0)
        take = gen.random(chains) < prob
        q[take], f[take], g[take] = qn[take], fn[take], gn[take]
        if it < burn:
            log_step += (float(np.mean(prob)) - target_accept) / (1.0 + it) ** 0.6
            log_steps.append(log_step)
            if it == burn - 1:
                log_step = float(np.mean(log_steps[burn // 2:]))
        else:
            accepted += take
            for c in range(chains):
                if it - burn in keep[c]:
                    kept[c].append(q[c].copy())
    samples = np.array([row for c in range(chains) for row in kept[c]], dtype=np.float64).reshape(n_samples, nu)
    info["accept_rate"] = accepted / max(total, 1)
    info["step"] = float(np.exp(log_step))
    return samples, info
