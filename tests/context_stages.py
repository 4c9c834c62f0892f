"""
Stages of a context's life, and the comparison that holds them to the bit.

A *stage* is ``stage(eng) -> dict`` of observables: it starts from its own ``set_data``, sets every persistent option it
depends on (the variational stages call ``vgp_set_likelihood`` themselves), makes its calls and returns everything the API
lets a caller see of them.  It never changes predict-math, generation or contraction options.  The property the tests
built on this module assert: a stage run on a context with ANY earlier history returns the bits of the same stage on a
fresh context (tests/test_gpu_context_reuse.py on the device; tests/test_context_stages_cpu.py on CPU doubles: one
without history, on which every stage runs and passes, and stand-ins that leak, which prove the harness can fail).

An observable the engine does not offer (a test double without ``get_matrix``, say) is absent from the dict, not an
error; a call the library refuses with a status is recorded as ``"<exception type>: <message>"`` -- a status is an
observable too.

Inputs: tests.helpers.synthetic_problem / synthetic_leaves with fixed seeds; hyper-parameters: the ones the family's GPU
test file uses (``_problem`` of tests/test_gpu_parity.py, ``_theta`` of tests/test_gpu_append.py, ``initial_u`` of the
family's oracle).  The shapes are the smallest that still reach each dispatch branch.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np

from oracle import gpr
from tests import sgpr_oracle as S
from tests import svgp_oracle as O
from tests import vgp_oracle as V
from tests import vgp_studentt_oracle as T
from tests.helpers import synthetic_leaves, synthetic_problem

VS = gpr.VARSIGMA_DEFAULT
MAT_CHOL, MAT_LINV, MAT_KINV = 0, 1, 2  # (pygpso_amd._lib's ids, restated: this module never loads the HIP library)
VEC_ALPHA = 0
KERNEL = "Matern52"
LIK_VGP_T = ("StudentT", 4.0)  # tests/test_gpu_vgp_studentt.py: LIK_P
LIK_SVGP_T = ("StudentT", 5.0)  # tests/test_gpu_svgp.py: STUDENT
GAUSS = ("Gaussian", None)
N_GH = T.N_GH


# ---- inputs (made once, never written to) ---------------------------------------------------------------------------
def _problem(n, d, kernel="Matern52", noise=1e-3, ard=False, seed=0, variance=1.3):
    """tests/test_gpu_parity.py: _problem."""
    X, y = synthetic_problem(n, d, seed=seed)
    ls = 0.25 * np.sqrt(d) * (np.linspace(0.8, 1.3, d) if ard else np.ones(1))
    return X, y, gpr.Theta(kernel, ls, variance, noise, float(y.mean()) if n > 1 else 0.1)


def grow_bounds(d, nseg=3, seed=5):
    """The boxes the families' best_ucb_grow tests use."""
    rng = np.random.default_rng(seed)
    lo = rng.random((nseg, d)) * 0.5
    return np.stack([lo, lo + 0.3 + 0.2 * rng.random((nseg, d))], axis=-1)


def u_rows(b, d, n_ls, train_mean, seed, y_mean=0.0):
    """tests/test_gpu_multistart.py: _u_rows."""
    rng = np.random.default_rng(seed)
    nu = n_ls + 2 + (1 if train_mean else 0)
    centre = np.concatenate([np.full(n_ls, gpr.softplus_inv(0.25 * np.sqrt(d))), [gpr.softplus_inv(1.3)],
                             [gpr.softplus_inv(1.0e-2)], [y_mean] if train_mean else []])
    return np.ascontiguousarray(centre + 0.3 * rng.standard_normal((b, nu)))


def _ls(d, ard):
    return 0.3 * np.sqrt(d) * (1.0 + 0.5 * np.arange(d) / d) if ard else 0.3 * np.sqrt(d)


SEG_RAGGED = np.array([0, 0, 1, 130, 257, 257], dtype=np.int64)  # empty, single, ragged, empty


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Everything stage ``name`` feeds the engine (and its oracle check needs to restate it)."""
    if name in ("gpr_small", "gpr_general", "gpr_nograd", "gpr_wide", "gpr_shrunk_pad"):
        n, d, ard, seed, grad = {"gpr_small": (50, 3, False, 0, True), "gpr_general": (200, 3, True, 0, True),
                                 "gpr_nograd": (200, 3, False, 1, False), "gpr_wide": (300, 12, True, 0, True),
                                 "gpr_shrunk_pad": (250, 3, False, 2, True)}[name]
        X, y, th = _problem(n, d, ard=ard, seed=seed)
        return NS(X=X, y=y, th=th, grad=grad, d=d, leaves=synthetic_leaves(257, d), bounds=grow_bounds(d), depth=4)
    if name in ("append_in_place", "append_pad_crossing"):
        n, k, seed = {"append_in_place": (193, 7, 3), "append_pad_crossing": (250, 7, 9)}[name]
        d = 3
        X, y = synthetic_problem(n + k, d, seed=seed)
        th = gpr.Theta("Matern52", 0.25 * np.sqrt(d) * np.ones(1), 1.3, 1e-3, float(y.mean()))  # tests/test_gpu_append.py: _theta
        return NS(X=X, y=y, th=th, n=n, k=k, d=d, leaves=synthetic_leaves(257, d))
    if name == "batch":
        d = 3
        X, y = synthetic_problem(100, d, seed=0)
        return NS(X=X, y=y, d=d, U={tm: u_rows(5, d, 1, tm, seed=5, y_mean=float(y.mean())) for tm in (True, False)}, c_fixed=0.1)
    if name == "set_posterior":
        X, y, th = _problem(100, 3, seed=4)
        return NS(X=X, y=y, th=th, d=3, post=gpr.posterior(th, X, y), leaves=synthetic_leaves(257, 3))
    if name == "failed_fit":  # tests/test_gpu_parity.py: test_not_positive_definite_raises_linalgerror
        return NS(X=np.array([[0.1, 0.2], [0.1, 0.2], [0.4, 0.4], [0.7, 0.1]]), y=np.zeros(4))
    if name in ("vgp_gauss", "vgp_studentt"):
        n, d = 150, 3
        X, y = synthetic_problem(n, d, seed=0)
        if name == "vgp_gauss":  # tests/test_gpu_vgp.py: the steps of test_device_natgrad_elbo_against_oracle at _vgp_engine's theta
            lik, u, steps = GAUSS, V.initial_u(0.3 * np.sqrt(d), 1.1, 0.01, 0.05), ((1.0, 0.0), (0.5, 0.2))
        else:  # tests/test_gpu_vgp_studentt.py: _st_engine
            lik, u, steps = LIK_VGP_T, T.initial_u(0.3 * np.sqrt(d), 1.1, 1.0, 0.05), ((0.5, 0.0), (0.5, 0.0))
        return NS(X=X, y=y, d=d, lik=lik, u=u, steps=steps, leaves=synthetic_leaves(257, d, seed=11), bounds=grow_bounds(d), depth=4)
    if name in ("sgpr", "sgpr_small_m", "sgpr_moved"):
        n, m, d, ard, seed = {"sgpr": (300, 40, 3, False, 0), "sgpr_small_m": (140, 9, 12, True, 0),
                              "sgpr_moved": (300, 40, 3, False, 1)}[name]
        X, y = synthetic_problem(n, d, seed=seed)
        n_ls = d if ard else 1
        u = S.initial_u(_ls(d, ard), 1.1, 0.01, 0.05)
        ns = NS(X=X, y=y, d=d, m=m, n_ls=n_ls, u=u, leaves=synthetic_leaves(257, d, seed=11))
        if name == "sgpr_moved":
            ls, var, _, _ = S.unpack(u, n_ls, True)
            ns.Z0 = S.choose_inducing(KERNEL, X, ls, var, m)
            ns.Z1 = ns.Z0 + 0.04 * np.random.default_rng(3).standard_normal(ns.Z0.shape)
        return ns
    if name in ("svgp", "svgp_gauss_uz"):
        n, m, d, lik, p = {"svgp": (300, 40, 3, LIK_SVGP_T, 1.0), "svgp_gauss_uz": (140, 9, 12, GAUSS, 0.01)}[name]
        X, y = synthetic_problem(n, d, seed=2)
        u = O.initial_u(0.3 * np.sqrt(d), 1.1, p, lik, c=0.05)
        ls, var, pp, _ = O.unpack(u, 1, True, 0.0, lik)
        Z0 = S.choose_inducing(KERNEL, X, ls, var, m)
        Z1 = Z0 + 0.04 * np.random.default_rng(4).standard_normal(Z0.shape)
        return NS(X=X, y=y, d=d, m=m, lik=lik, u=u, Z0=Z0, Z1=Z1, s2=O.predictive_noise(lik, pp),
                  leaves=synthetic_leaves(257, d, seed=11))
    if name == "calls_grown_tickets":  # N_pad = 256: the one-launch kernel applies to a float64 context
        X, y, th = _problem(200, 3)
        # grow_bounds(3) at depth 4: 87 bit-distinct rows against 81 analytic slots -- centre children that differ from their
        # parents in the last bit, which the one-launch kernel has no slot for (it asks for the append-counter sequence).
        # near: the ``arbitrary`` boxes of tests/test_gpu_parity.py::test_small_call_sequence_gives_the_bits_of_the_general_one
        # for its (d, depth) = (3, 8) case (4 455 distinct rows against 4 374 slots)
        rng = np.random.default_rng(8)
        lo = rng.random((2, 3)) * 0.5
        near = np.stack([lo, lo + 0.1 + 0.4 * rng.random((2, 3))], axis=2)
        return NS(X=X, y=y, th=th, grad=False, d=3, leaves=synthetic_leaves(257, 3), bounds=grow_bounds(3), depth=4, near=near, near_depth=8)
    if name in ("calls_screened", "calls_refused_ticket"):  # tests/test_gpu_screen.py: its shape, its theta, its batches
        n, d = 768, 12
        X, y = synthetic_problem(n, d, seed=0)
        th = gpr.Theta("Matern52", 0.25 * np.sqrt(d) * np.ones(1), 1.0, 1e-3, float(y.mean()))
        f32 = lambda m, seed: synthetic_leaves(m, d, seed=seed).astype(np.float32)  # noqa: E731
        return NS(X=X, y=y, th=th, grad=False, d=d, leaves=synthetic_leaves(257, d), a1000=f32(1000, 11), b512=f32(512, 12),
                  big=f32(BIG_M, 13), big_vs=50.0)
    raise KeyError(name)


# ---- recording ---------------------------------------------------------------------------------------------------------
def _try(obs, key, fn, names=None):
    """Record what ``fn()`` returns under ``key`` (a tuple: under ``key.<name>``); a refusal is recorded as its exception
    type and message, setters included: a status after some history is an observable, and the stage goes on so that the
    run's other mismatches are still collected.  Anything else the call raises -- an AttributeError inside a wrapper,
    say -- escapes."""
    try:
        val = fn()
    except (np.linalg.LinAlgError, ValueError, RuntimeError) as e:
        obs[key] = f"{type(e).__name__}: {e}"
        return None
    if names is None:
        if val is not None:  # (a call that returns nothing leaves nothing to record unless it is refused)
            obs[key] = val
    else:
        for nm, v in zip(names, val):
            if v is not None:
                obs[f"{key}.{nm}"] = v
    return val


def _offers(eng, method):
    """Asked BEFORE the call, so that an AttributeError raised inside it is not mistaken for a missing method."""
    return hasattr(type(eng), method)


WIN = ("idx", "mean", "var", "ucb")


def _set_likelihood(eng, obs, lik):
    if lik[0] == "StudentT":
        _try(obs, "set_likelihood", lambda: eng.vgp_set_likelihood("StudentT", lik[1], N_GH))
    else:
        _try(obs, "set_likelihood", lambda: eng.vgp_set_likelihood("Gaussian"))


def posterior_observables(eng, obs, leaves, prefix="", chol=True, kinv=True):
    """What a caller can see of the resident posterior."""
    if _offers(eng, "get_matrix"):
        if chol:
            _try(obs, prefix + "chol", lambda: eng.get_matrix(MAT_CHOL))
        _try(obs, prefix + "linv", lambda: eng.get_matrix(MAT_LINV))
        if kinv:
            _try(obs, prefix + "kinv", lambda: eng.get_matrix(MAT_KINV))
    if _offers(eng, "get_vector"):
        _try(obs, prefix + "alpha", lambda: eng.get_vector(VEC_ALPHA))
    _try(obs, prefix + "predict", lambda: eng.predict(leaves), ("mean", "var"))
    if _offers(eng, "posterior_hash"):
        _try(obs, prefix + "hash", lambda: eng.posterior_hash())
    if _offers(eng, "padded_n"):
        _try(obs, prefix + "padded_n", lambda: eng.padded_n)


def _fit(eng, obs, X, y, th, grad):
    _try(obs, "set_data", lambda: eng.set_data(X, y))
    _try(obs, "fit", lambda: eng.fit_eval(th.kernel, th.lengthscales, th.variance, th.noise, th.mean_c, want_grad=grad), ("nlml", "grad"))


# ---- the stages ---------------------------------------------------------------------------------------------------------
def _gpr_stage(name):
    def stage(eng):
        p, obs = inputs(name), {}
        _fit(eng, obs, p.X, p.y, p.th, p.grad)
        if name == "gpr_nograd":  # (the winners before anything else asks for L^-1's packed form)
            _try(obs, "best_ucb", lambda: eng.best_ucb(p.leaves, VS, SEG_RAGGED), WIN)
        posterior_observables(eng, obs, p.leaves, kinv=p.grad)
        if name in ("gpr_small", "gpr_general"):
            _try(obs, "grow", lambda: eng.best_ucb_grow(p.bounds, p.depth, VS), WIN)
        if name == "gpr_general":
            _try(obs, "best_ucb", lambda: eng.best_ucb(p.leaves, VS, SEG_RAGGED), WIN)
        return obs

    stage.__name__ = name
    return stage


def _append_stage(name):
    def stage(eng):
        p, obs = inputs(name), {}
        _fit(eng, obs, p.X[:p.n], p.y[:p.n], p.th, False)
        _try(obs, "append", lambda: eng.append(p.X[p.n:], p.y[p.n:]), ("nlml", "in_place"))
        posterior_observables(eng, obs, p.leaves, kinv=False)
        return obs

    stage.__name__ = name
    return stage


def batch(eng):
    p, obs = inputs("batch"), {}
    _try(obs, "set_data", lambda: eng.set_data(p.X, p.y))
    for tm in (True, False) if _offers(eng, "fit_eval_u_batch") else ():
        _try(obs, f"batch.mean_{'trained' if tm else 'fixed'}", lambda: eng.fit_eval_u_batch(KERNEL, p.U[tm], 1, tm, p.c_fixed),
             ("loss", "grad", "ok"))
    return obs


def set_posterior(eng):
    p, obs = inputs("set_posterior"), {}
    th = p.th
    if not _offers(eng, "set_posterior"):
        return obs
    _try(obs, "set_posterior", lambda: eng.set_posterior(p.X, p.post.L, p.post.alpha, th.kernel, th.lengthscales, th.variance,
                                                         th.noise, th.mean_c))
    posterior_observables(eng, obs, p.leaves, kinv=False)
    return obs


def failed_fit(eng):
    p, obs = inputs("failed_fit"), {}
    _try(obs, "set_data", lambda: eng.set_data(p.X, p.y))
    _try(obs, "fit", lambda: eng.fit_eval("SquaredExponential", [0.3], 1.0, -1.0e-3, 0.0), ("nlml", "grad"))
    return obs


def _vgp_stage(name):
    def stage(eng):
        p, obs = inputs(name), {}
        _try(obs, "set_data", lambda: eng.set_data(p.X, p.y))
        _set_likelihood(eng, obs, p.lik)
        _try(obs, "set_q", lambda: eng.vgp_set_q())
        uu = p.u
        for k, (gamma, shift) in enumerate(p.steps):
            uu = p.u + shift
            _try(obs, f"natgrad{k}", lambda: eng.vgp_natgrad(KERNEL, uu, 1, True, 0.0, gamma))
            _try(obs, f"q{k}", lambda: eng.vgp_get_q(), ("mu", "S"))
        _try(obs, "elbo", lambda: eng.vgp_elbo_u(KERNEL, uu, 1, True, 0.0), ("loss", "grad", "theta"))
        _try(obs, "posterior", lambda: eng.vgp_posterior(KERNEL, uu, 1, True, 0.0))
        posterior_observables(eng, obs, p.leaves, chol=False, kinv=False)
        _try(obs, "grow", lambda: eng.best_ucb_grow(p.bounds, p.depth, VS), WIN)
        return obs

    stage.__name__ = name
    return stage


def _sgpr_stage(name):
    def stage(eng):
        p, obs = inputs(name), {}
        _try(obs, "set_data", lambda: eng.set_data(p.X, p.y))
        if name == "sgpr_moved":
            _try(obs, "set_inducing", lambda: eng.sgpr_set_inducing(p.Z0))
            _try(obs, "move_inducing", lambda: eng.sgpr_move_inducing(p.Z1))
            _try(obs, "bound", lambda: eng.sgpr_bound_uz(KERNEL, p.u, p.n_ls, True, 0.0, Z=None), ("loss", "grad_u", "grad_z", "theta"))
        else:
            _try(obs, "picks", lambda: eng.sgpr_select_inducing(KERNEL, p.u, p.n_ls, p.m))
            _try(obs, "bound", lambda: eng.sgpr_bound_u(KERNEL, p.u, p.n_ls, True, 0.0), ("loss", "grad_u", "theta"))
        _try(obs, "inducing", lambda: eng.sgpr_get_inducing(), ("Z", "n_data"))
        for which in ("Kuf", "Lu", "LB", "cv"):
            _try(obs, which, lambda: eng.sgpr_get_factor(which))
        _try(obs, "delta", lambda: eng.sgpr_posterior(KERNEL, p.u, p.n_ls, True, 0.0))
        posterior_observables(eng, obs, p.leaves, chol=False, kinv=False)
        return obs

    stage.__name__ = name
    return stage


def _svgp_stage(name):
    def stage(eng):
        p, obs = inputs(name), {}
        _try(obs, "set_data", lambda: eng.set_data(p.X, p.y))
        _set_likelihood(eng, obs, p.lik)
        _try(obs, "set_inducing", lambda: eng.sgpr_set_inducing(p.Z0))
        _try(obs, "init_q", lambda: eng.svgp_init_q(KERNEL, p.u, 1, True, 0.0, p.s2))
        _try(obs, "q0", lambda: eng.svgp_get_q(), ("mu", "S"))
        if name == "svgp":
            for k in (1, 2):
                _try(obs, f"natgrad{k}", lambda: eng.svgp_natgrad(KERNEL, p.u, 1, True, 0.0, 0.5))
                _try(obs, f"q{k}", lambda: eng.svgp_get_q(), ("mu", "S"))
            _try(obs, "elbo", lambda: eng.svgp_elbo_u(KERNEL, p.u, 1, True, 0.0), ("loss", "grad_u", "theta"))
        else:
            _try(obs, "elbo", lambda: eng.svgp_elbo_uz(KERNEL, p.u, 1, True, 0.0, Z=p.Z1), ("loss", "grad_u", "grad_z", "theta"))
            _try(obs, "q1", lambda: eng.svgp_get_q(), ("mu", "S"))
        _try(obs, "delta", lambda: eng.svgp_posterior(KERNEL, p.u, 1, True, 0.0))
        posterior_observables(eng, obs, p.leaves, chol=False, kinv=False)
        return obs

    stage.__name__ = name
    return stage


# ---- call kinds crossed on one context (csrc/best_call.hpp) -----------------------------------------------
# Synchronous, ticket and group-half calls, one-launch / small / general / screened sequences, in the orders in which one
# call's record could be mistaken for another's.  Records that must be equal whatever the history are asserted equal here.
def _device(eng, a):
    """float32 leaves where a screened call reads them in place: on the device (a CPU double takes the array itself)."""
    if getattr(eng, "HOST_LEAVES", False):
        return a
    import torch

    return torch.from_numpy(a).cuda()


def _counted(eng, call, counters):
    rec = call()
    return tuple(rec) + tuple(np.int64(eng.last_count(k)) for k in counters)


def _same_record(obs, *keys):
    for k in WIN:
        words = [_bits(obs[f"{key}.{k}"]).tobytes() for key in keys]
        assert all(w == words[0] for w in words), (keys, k, [obs[f"{key}.{k}"] for key in keys])


def calls_grown_tickets(eng):
    """A grown call; a ticket pair -- the same grown call and a ragged batch --, another grown call (near-duplicate centres)
    while both are open, ended out of order; the grown call again."""
    p, obs = inputs("calls_grown_tickets"), {}
    _fit(eng, obs, p.X, p.y, p.th, p.grad)
    posterior_observables(eng, obs, p.leaves, kinv=p.grad)
    rows = WIN + ("scored", "asked")
    grown = lambda: _counted(eng, lambda: eng.best_ucb_grow(p.bounds, p.depth, VS), (0, 1))  # noqa: E731
    _try(obs, "grow", grown, rows)
    t_grow = eng.best_ucb_grow_begin(p.bounds, p.depth, VS)
    t_leaves = eng.best_ucb_begin(p.leaves, VS, SEG_RAGGED)
    _try(obs, "grow_near", lambda: _counted(eng, lambda: eng.best_ucb_grow(p.near, p.near_depth, VS), (0, 1)), rows)
    _try(obs, "best_ucb", lambda: eng.best_ucb_end(t_leaves), WIN)
    _try(obs, "grow_ticket", lambda: _counted(eng, lambda: eng.best_ucb_end(t_grow), (0,)), WIN + ("scored",))
    _try(obs, "grow_again", grown, rows)
    _same_record(obs, "grow", "grow_ticket", "grow_again")
    assert obs["grow.scored"] == obs["grow_ticket.scored"] == obs["grow_again.scored"]
    return obs


SCREEN_ACCEPTED, SCREEN_REFUSED = 1, 2  # (pygpso_amd._lib's ids of last_count(8), restated)
BIG_M = 24000  # tests/test_gpu_screen.py: with varsigma = 50 every leaf survives, more than a call on 256 CUs has room for
SCREENED = WIN + ("survivors", "verdict")


def calls_screened(eng):
    """Every call screened (option 2): a ticket on 1 000 leaves, a synchronous call on 512 while it is open, its end; then
    rank 0's half of the 1 000 -- whose record nobody finishes -- and the synchronous call on them straight behind it."""
    p, obs = inputs("calls_screened"), {}
    _fit(eng, obs, p.X, p.y, p.th, p.grad)
    posterior_observables(eng, obs, p.leaves, kinv=p.grad)
    a, b = _device(eng, p.a1000), _device(eng, p.b512)
    eng.set_screen(2)
    try:
        t = eng.best_ucb_begin(a, VS)
        _try(obs, "sync_512", lambda: _counted(eng, lambda: eng.best_ucb(b, VS), (7, 8)), SCREENED)
        _try(obs, "ticket_1000", lambda: _counted(eng, lambda: eng.best_ucb_end(t), (7, 8)), SCREENED)
        _try(obs, "half", lambda: eng.shard_winners(0, 2, a[:500], 1000, VS))
        _try(obs, "sync_1000", lambda: _counted(eng, lambda: eng.best_ucb(a, VS), (7, 8)), SCREENED)
    finally:
        eng.set_screen(1)
    _same_record(obs, "ticket_1000", "sync_1000")
    assert obs["ticket_1000.survivors"] == obs["sync_1000.survivors"] and obs["ticket_1000.verdict"] == obs["sync_1000.verdict"]
    return obs


def calls_refused_ticket(eng):
    """A screened call the launch has no room for, through a ticket, ended second behind a small accepted one: the record of
    the call with the option off.  (Either verdict where the room is at least the batch, as tests/test_gpu_screen.py has it.)"""
    p, obs = inputs("calls_refused_ticket"), {}
    _fit(eng, obs, p.X, p.y, p.th, p.grad)
    posterior_observables(eng, obs, p.leaves, kinv=p.grad)
    a, big = _device(eng, p.a1000), _device(eng, p.big)
    eng.set_screen(0)
    try:
        _try(obs, "off", lambda: eng.best_ucb(big, p.big_vs), WIN)
        eng.set_screen(2)
        cap = eng.screen_probe(big, p.big_vs)[3]["cap"]
        t_small, t_big = eng.best_ucb_begin(a, VS), eng.best_ucb_begin(big, p.big_vs)
        _try(obs, "small", lambda: _counted(eng, lambda: eng.best_ucb_end(t_small), (7, 8)), SCREENED)
        _try(obs, "big", lambda: _counted(eng, lambda: eng.best_ucb_end(t_big), (7, 8)), SCREENED)
    finally:
        eng.set_screen(1)
    _same_record(obs, "big", "off")
    assert obs["big.verdict"] in (SCREEN_ACCEPTED, SCREEN_REFUSED) and (cap >= BIG_M or obs["big.verdict"] == SCREEN_REFUSED), (cap, obs["big.verdict"])
    return obs


# the dtype each runs in: the one-launch kernel needs native (double) predict math, the screen the default float kernels
CALL_STAGES = {"float64": ("calls_grown_tickets",), "mixed": (), "float32": ("calls_screened", "calls_refused_ticket")}
GPR_STAGES = ("gpr_small", "gpr_general", "gpr_nograd", "gpr_wide", "gpr_shrunk_pad", "append_in_place",
              "append_pad_crossing", "batch", "set_posterior", "failed_fit")
VAR_STAGES = ("vgp_gauss", "vgp_studentt", "sgpr", "sgpr_small_m", "sgpr_moved", "svgp", "svgp_gauss_uz")
STAGES = {}
for _n in GPR_STAGES[:5]:
    STAGES[_n] = _gpr_stage(_n)
for _n in GPR_STAGES[5:7]:
    STAGES[_n] = _append_stage(_n)
STAGES.update(batch=batch, set_posterior=set_posterior, failed_fit=failed_fit)
STAGES.update(calls_grown_tickets=calls_grown_tickets, calls_screened=calls_screened, calls_refused_ticket=calls_refused_ticket)
for _n in VAR_STAGES[:2]:
    STAGES[_n] = _vgp_stage(_n)
for _n in VAR_STAGES[2:5]:
    STAGES[_n] = _sgpr_stage(_n)
for _n in VAR_STAGES[5:]:
    STAGES[_n] = _svgp_stage(_n)
NO_POSTERIOR = ("batch", "failed_fit")  # stages that leave no predict-ready posterior behind


def stages_for(dtype):
    """The variational and sparse families refuse float32 contexts by design."""
    return GPR_STAGES + CALL_STAGES[dtype] + (() if dtype == "float32" else VAR_STAGES)


# ---- comparison -----------------------------------------------------------------------------------------------------
class Mismatch:
    def __init__(self, stage, observable, n_diff, max_diff, note=""):
        self.stage, self.observable, self.n_diff, self.max_diff, self.note = stage, observable, n_diff, max_diff, note

    def __str__(self):
        return (f"stage {self.stage}: {self.observable}: {self.n_diff} element(s) differ, largest difference "
                f"{self.max_diff:.3e}" + (f" ({self.note})" if self.note else ""))

    __repr__ = __str__


def _bits(a):
    """Floats as their 64-bit words: NaN payloads and the sign of zero count."""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return a


def compare(stage, got, want):
    """Every observable of ``got`` against ``want``, bit for bit -> list of Mismatch (all of them, not the first)."""
    out = []
    for key in sorted(set(got) | set(want)):
        if key not in got or key not in want:
            out.append(Mismatch(stage, key, 1, float("nan"), "absent from the " + ("history" if key not in got else "fresh") + " run"))
            continue
        g, w = got[key], want[key]
        if isinstance(g, str) or isinstance(w, str):
            if not (isinstance(g, str) and isinstance(w, str) and g == w):
                out.append(Mismatch(stage, key, 1, float("nan"), f"{str(g)[:80]!r} against {str(w)[:80]!r}"))
            continue
        ga, wa = np.asarray(g), np.asarray(w)
        if ga.shape != wa.shape or ga.dtype.kind != wa.dtype.kind:
            out.append(Mismatch(stage, key, max(ga.size, wa.size), float("nan"), f"shape {ga.shape} {ga.dtype} against {wa.shape} {wa.dtype}"))
            continue
        gb, wb = _bits(ga), _bits(wa)
        if np.array_equal(gb, wb):
            continue
        note = ""
        if ga.dtype.kind in "iub":  # integers (picks, winners, the 64-bit hash): the values themselves, exactly
            k = int(np.flatnonzero((gb != wb).reshape(-1))[0])
            a, b = ga.reshape(-1)[k].item(), wa.reshape(-1)[k].item()
            big, note = float(abs(int(a) - int(b))), f"first: {a} against {b}"
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                diff = np.abs(ga.astype(np.float64) - wa.astype(np.float64))
            big = float(np.nanmax(diff)) if np.any(np.isfinite(diff)) else float("nan")
        out.append(Mismatch(stage, key, int(np.count_nonzero(gb != wb)), big, note))
    return out


def run_stage(make_engine, name, history=()):
    """Stage ``name`` on a context that ran the stages of ``history`` first -> its observables."""
    eng = make_engine()
    try:
        for h in history:
            STAGES[h](eng)
        return STAGES[name](eng)
    finally:
        close = getattr(eng, "close", None)
        if close:
            close()


def pair_mismatches(make_engine, first, seconds, fresh):
    """For every stage B of ``seconds``: a context runs ``first`` then B; B against ``fresh[B]``.  One context per pair."""
    out = []
    for b in seconds:
        for m in compare(b, run_stage(make_engine, b, history=(first,)), fresh[b]):
            m.note = (m.note + "; " if m.note else "") + f"after {first}"
            out.append(m)
    return out


def walk_sequence(names, seed, steps=12):
    rng = np.random.default_rng(seed)
    return [names[int(i)] for i in rng.integers(0, len(names), size=steps)]


def walk_mismatches(make_engine, sequence, fresh):
    """One context runs the whole sequence; every step against its fresh result.  A mismatch names the step and the two
    stages before it."""
    out = []
    eng = make_engine()
    try:
        for k, name in enumerate(sequence):
            for m in compare(name, STAGES[name](eng), fresh[name]):
                before = ", ".join(sequence[max(0, k - 2):k]) or "nothing"
                m.note = (m.note + "; " if m.note else "") + f"step {k} of the walk, after {before}"
                out.append(m)
    finally:
        close = getattr(eng, "close", None)
        if close:
            close()
    return out


def report(mismatches, limit=40):
    lines = [str(m) for m in mismatches[:limit]]
    if len(mismatches) > limit:
        lines.append(f"... and {len(mismatches) - limit} more")
    return f"{len(mismatches)} observable(s) depend on the context's history:\n  " + "\n  ".join(lines)
