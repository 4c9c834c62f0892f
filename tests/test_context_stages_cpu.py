"""
The context-reuse harness (tests/context_stages.py) can fail: proved without a device.

The GPR stages run through the CPU test double ``tests.oracle_engine.OracleEngine`` -- which keeps no state between fits,
so pairs and walks pass -- and through two deliberately leaky stand-ins that restate the kinds of bug a context can
have: buffers that only grow and keep their old bytes, and a choice remembered from an earlier posterior.  The
pair test and the walk must report each leak and name the stage it shows in.  A third double offers the whole surface
(getters, batch, set_posterior, the variational and sparse calls) with the families' oracles behind it, so that every
one of the 17 stages runs here, and a leaky variant of it remembers the previous likelihood.  The HIP library is never
loaded here.
"""
import numpy as np
import pytest

from oracle import gpr
from tests import context_stages as CS
from tests import inducing_oracle as I
from tests import sgpr_oracle as S
from tests import svgp_oracle as O
from tests import vgp_oracle as V
from tests import vgp_studentt_oracle as T
from tests.oracle_engine import OracleEngine

NAMES = list(CS.GPR_STAGES)


@pytest.fixture(scope="module")
def fresh():
    return {n: CS.run_stage(OracleEngine, n) for n in NAMES}


class StaleRowsEngine(OracleEngine):
    """Leak 1: X and alpha live in buffers that only grow and keep their old bytes, and predict reads whole 128-row
    blocks: after a larger problem of the same D, the rows between N and the padded N still hold the previous inputs and
    the tail of the previous alpha."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._x_buf = np.zeros((0, 0))
        self._alpha_buf = np.zeros(0)

    def _store(self):
        n, d = self.post.X.shape
        if self._x_buf.shape[1] != d:  # (a change of D lays the buffers out anew)
            self._x_buf, self._alpha_buf = np.zeros((0, d)), np.zeros(0)
        if self._x_buf.shape[0] < n:
            self._x_buf = np.vstack([self._x_buf, np.zeros((n - self._x_buf.shape[0], d))])
            self._alpha_buf = np.concatenate([self._alpha_buf, np.zeros(n - self._alpha_buf.shape[0])])
        self._x_buf[:n], self._alpha_buf[:n] = self.post.X, self.post.alpha  # (nothing zeroes the rows behind n)

    def fit_eval(self, *a, **k):
        out = super().fit_eval(*a, **k)
        self._store()
        return out

    def append(self, *a, **k):
        out = super().append(*a, **k)
        self._store()
        return out

    def predict(self, xs, out=None):
        mean, var = super().predict(xs, out)
        n = self.post.X.shape[0]
        npad = min(-(-n // 128) * 128, self._x_buf.shape[0])
        if npad > n:
            th = self.post.theta
            ls = np.broadcast_to(np.atleast_1d(th.lengthscales), (self.post.X.shape[1],))
            mean = mean + gpr.gram(th.kernel, np.asarray(xs, dtype=np.float64), self._x_buf[n:npad], ls, th.variance) @ self._alpha_buf[n:npad]
        return mean, var


class StickyChoiceEngine(OracleEngine):
    """Leak 2: a choice made for the first posterior and never made again (the shape of ``gen_decided``): the context
    decides once, from the first posterior it serves, whether the short path applies -- which is exact for a wide problem
    and rounds to float for a narrow one -- and every later posterior inherits the answer."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._decided = None

    def predict(self, xs, out=None):
        if self._decided is None:
            self._decided = self.post.X.shape[1] > 8
        mean, var = super().predict(xs, out)
        if self._decided and self.post.X.shape[1] <= 8:
            mean, var = mean.astype(np.float32).astype(np.float64), var.astype(np.float32).astype(np.float64)
        return mean, var


class WholeSurfaceEngine(OracleEngine):
    """Every call the stages make, answered by the oracles of the families' test files; it keeps nothing between stages
    but what the API says persists (the likelihood)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.lik, self.mode, self.grad = CS.GAUSS, None, False

    def set_data(self, X, y):
        super().set_data(X, y)
        self.Xd, self.yd, self.mode = self.X, self.y, None

    def fit_eval(self, *a, want_grad=True):
        self.grad, self.mode = want_grad, None
        return super().fit_eval(*a, want_grad=want_grad)

    def fit_eval_u_batch(self, kernel, U, n_ls, train_mean, c=0.0):
        rows = [gpr.loss_and_grad_unconstrained(kernel, u if train_mean else np.append(u, c), self.X, self.y) for u in U]
        return (np.array([f for f, _ in rows]), np.array([g if train_mean else g[:-1] for _, g in rows]), np.ones(len(U), dtype=bool))

    def set_posterior(self, X, L, alpha, kernel, ls, variance, noise, mean_c):
        post = gpr.Posterior()
        post.theta = gpr.Theta(kernel, ls, variance, noise, mean_c)
        post.X, post.L, post.alpha, post.y, post.nlml = np.asarray(X), np.asarray(L), np.asarray(alpha), None, float("nan")
        self.post, self.mode, self.grad = post, None, False
        self.n, self.d = post.X.shape

    def get_matrix(self, which):
        if self.mode is not None:
            if which != CS.MAT_LINV or self._C is None:
                raise RuntimeError("not offered for this posterior")
            return self._C
        if self.post is None or (which == CS.MAT_KINV and not self.grad):
            raise RuntimeError("not resident")
        Li = np.linalg.inv(self.post.L)
        return {CS.MAT_CHOL: self.post.L, CS.MAT_LINV: Li, CS.MAT_KINV: Li.T @ Li}[which]

    def get_vector(self, which):
        if self.mode is not None:
            if self._C is None:
                raise RuntimeError("not offered for this posterior")
            return self._beta
        if self.post is None:
            raise RuntimeError("not resident")
        return self.post.alpha

    def posterior_hash(self):
        mean, var = self.predict(np.full((1, self.d), 0.5))
        return int(np.float64(mean[0] + var[0]).view(np.uint64))

    @property
    def padded_n(self):
        return -(-self.n // 128) * 128

    def predict(self, xs, out=None):
        return super().predict(xs, out) if self.mode is None else self._predict(np.asarray(xs, dtype=np.float64))

    def best_ucb(self, xs, varsigma, seg_off=None):
        if self.mode is None:
            return super().best_ucb(xs, varsigma, seg_off)
        mean, var = self.predict(xs)
        ucb = mean + varsigma * var
        i = int(np.argmax(ucb))  # (the variational stages ask for whole batches only)
        return np.array([i]), mean[i:i + 1], var[i:i + 1], ucb[i:i + 1]

    def best_ucb_grow(self, bounds, depth, varsigma):
        rows = self.grow(bounds, depth)
        got = [self.best_ucb(r, varsigma) for r in rows]
        return tuple(np.concatenate([g[j] for g in got]) for j in range(4))

    # -- the call kinds (tests/context_stages.py: CALL_STAGES) pass through: a ticket holds the record of the blocking call,
    # every screened call is accepted whole (the room is the batch), a half's payload is its winners' records behind one another
    HOST_LEAVES = True

    def best_ucb_begin(self, xs, varsigma, seg_off=None):
        return self._open(self.best_ucb(xs, varsigma, seg_off))

    def best_ucb_grow_begin(self, bounds, depth, varsigma):
        return self._open(self.best_ucb_grow(bounds, depth, varsigma))

    def _open(self, record):
        self._tickets = getattr(self, "_tickets", {})
        ticket = min(k for k in (0, 1) if k not in self._tickets)  # (a third call in flight: ValueError, a refusal)
        self._tickets[ticket] = record
        return ticket

    def best_ucb_end(self, ticket):
        return self._tickets.pop(ticket)

    def set_screen(self, mode):
        pass

    def last_count(self, what=0):
        return CS.SCREEN_ACCEPTED if what == 8 else 0

    def screen_probe(self, xs, varsigma):
        return None, None, None, {"survivors": len(xs), "threshold": -np.inf, "cap": len(xs)}

    def shard_winners(self, rank, world, local_leaves, m_global, varsigma, seg_off=None):
        idx, mean, var, ucb = self.best_ucb(local_leaves, varsigma, seg_off)
        return np.concatenate([np.column_stack([mean, var, ucb, idx.astype(np.float64)]).reshape(-1), [0.0, 0.0]])

    # -- variational GP
    def vgp_set_likelihood(self, kind="Gaussian", df=3.0, n_gh=20):
        self.lik = (kind, df if kind == "StudentT" else None)

    def vgp_set_q(self, mu=None, Sq=None):
        self.q = (np.zeros(self.n), np.eye(self.n)) if mu is None else (np.array(mu), np.array(Sq))

    def vgp_get_q(self):
        return self.q[0].copy(), self.q[1].copy()

    def _student(self):
        return self.lik[0] == "StudentT"

    def vgp_natgrad(self, k, u, n_ls, tm, c=0.0, gamma=1.0):
        a = (k, u, n_ls, tm, c, self.Xd, self.yd, *self.q)
        self.q = T.natgrad(*a, self.lik, gamma) if self._student() else V.natgrad(*a, gamma)

    def vgp_elbo_u(self, k, u, n_ls, tm, c=0.0, want_grad=True):
        a = (k, u, n_ls, tm, c, self.Xd, self.yd, *self.q)
        return T.neg_elbo_and_grad_u(*a, self.lik) if self._student() else V.neg_elbo_and_grad_u(*a)

    def vgp_posterior(self, k, u, n_ls, tm, c=0.0):
        a = (k, u, n_ls, tm, c, self.Xd, *self.q)
        post = T.Posterior(*a, self.lik, installed=True) if self._student() else V.Posterior(*a)
        self.mode, self._predict, self._C = "vgp", post.predict_y, None

    # -- sparse
    def sgpr_set_inducing(self, Z):
        self.Z = np.array(Z)
        self.n = len(self.Z)

    def sgpr_move_inducing(self, Z):
        self.Z = np.array(Z)

    def sgpr_select_inducing(self, k, u, n_ls, m):
        ls, var, _, _ = S.unpack(u, n_ls, True)
        idx = S.greedy_select(k, self.Xd, ls, var, m)
        self.sgpr_set_inducing(self.Xd[idx])
        return idx

    def sgpr_get_inducing(self):
        return self.Z.copy(), self.Xd.shape[0]

    def sgpr_bound_u(self, k, u, n_ls, tm, c=0.0, want_grad=True):
        self._fac = S.factors(k, u, n_ls, tm, c, self.Xd, self.yd, self.Z)
        return S.neg_bound_and_grad_u(k, u, n_ls, tm, c, self.Xd, self.yd, self.Z)

    def sgpr_bound_uz(self, k, u, n_ls, tm, c=0.0, Z=None, want_grad=True):
        f, g, th = self.sgpr_bound_u(k, u, n_ls, tm, c)
        return f, g, I.sgpr_grad_z(k, u, n_ls, tm, c, self.Xd, self.yd, self.Z), th

    def sgpr_get_factor(self, which):
        return getattr(self._fac, which)

    def sgpr_posterior(self, k, u, n_ls, tm, c=0.0):
        post = S.Posterior(k, u, n_ls, tm, c, self.Xd, self.yd, self.Z)
        self._C, self._beta, _, delta = post.installed()
        self.mode, self._predict = "sgpr", post.predict_y
        return delta

    def svgp_init_q(self, k=None, u=None, n_ls=1, tm=False, c=0.0, noise_variance=0.0):
        self.sq = O.conjugate_start(k, u, n_ls, tm, c, self.Xd, self.yd, self.Z, self.lik, noise_variance)

    def svgp_get_q(self):
        return self.sq[0].copy(), self.sq[1].copy()

    def svgp_natgrad(self, k, u, n_ls, tm, c=0.0, gamma=1.0):
        self.sq = O.natgrad(k, u, n_ls, tm, c, self.Xd, self.yd, self.Z, *self.sq, self.lik, gamma)

    def svgp_elbo_u(self, k, u, n_ls, tm, c=0.0, want_grad=True):
        return O.neg_elbo_and_grad_u(k, u, n_ls, tm, c, self.Xd, self.yd, self.Z, *self.sq, self.lik)

    def svgp_elbo_uz(self, k, u, n_ls, tm, c=0.0, Z=None, want_grad=True):
        if Z is not None:
            self.Z = np.array(Z)
        f, g, th = self.svgp_elbo_u(k, u, n_ls, tm, c)
        return f, g, I.svgp_grad_z(k, u, n_ls, tm, c, self.Xd, self.yd, self.Z, *self.sq, self.lik), th

    def svgp_posterior(self, k, u, n_ls, tm, c=0.0):
        post = O.Posterior(k, u, n_ls, tm, c, self.Xd, self.Z, *self.sq, self.lik)
        self._C, self._beta, _, delta = post.installed()
        self.mode, self._predict = "svgp", post.predict_y_installed
        return delta


class RemembersLikelihoodEngine(WholeSurfaceEngine):
    """Leak 3: once a Student-t likelihood was set, a later ``vgp_set_likelihood("Gaussian")`` changes the kind's name
    but the quadrature path stays switched on."""

    def vgp_set_likelihood(self, kind="Gaussian", df=3.0, n_gh=20):
        if self.lik[0] == "StudentT" and kind == "Gaussian":
            return  # (the previous likelihood stays)
        super().vgp_set_likelihood(kind, df, n_gh)


ALL = list(CS.GPR_STAGES + CS.VAR_STAGES)


@pytest.fixture(scope="module")
def fresh_all():
    return {n: CS.run_stage(WholeSurfaceEngine, n) for n in ALL}


def test_all_seventeen_stages_run_and_return_their_observables(fresh_all):
    refused = {n: sorted(k for k, v in obs.items() if isinstance(v, str)) for n, obs in fresh_all.items()}
    assert refused.pop("failed_fit") == ["fit"]
    assert refused.pop("vgp_gauss") == refused.pop("vgp_studentt") == ["alpha", "linv"]  # (this double installs no C for the VGP)
    assert not any(refused.values()), refused
    assert set(fresh_all["batch"]) == {f"batch.mean_{t}.{k}" for t in ("trained", "fixed") for k in ("loss", "grad", "ok")}
    assert {"predict.mean", "linv", "alpha", "hash", "padded_n"} <= set(fresh_all["set_posterior"])
    assert {"q0.mu", "q1.S", "elbo.loss", "elbo.grad", "elbo.theta", "predict.var", "grow.idx"} <= set(fresh_all["vgp_studentt"])
    for n in ("sgpr", "sgpr_small_m"):
        assert {"picks", "bound.loss", "bound.grad_u", "inducing.Z", "Kuf", "Lu", "LB", "cv", "delta", "linv", "alpha"} <= set(fresh_all[n])
    assert "bound.grad_z" in fresh_all["sgpr_moved"] and fresh_all["sgpr_moved"]["inducing.Z"].shape == (40, 3)
    assert {"q0.mu", "q1.mu", "q2.S", "elbo.grad_u", "delta"} <= set(fresh_all["svgp"])
    assert {"elbo.grad_z", "q1.mu"} <= set(fresh_all["svgp_gauss_uz"]) and fresh_all["svgp_gauss_uz"]["alpha"].shape == (9,)


def test_the_call_stages_run_on_the_whole_surface_double_and_a_ticket_mix_up_is_reported():
    """CALL_STAGES: every dtype's list is what stages_for adds; each stage runs on the pass-through, asserts its own equal
    records, and returns the same observables after any other of them.  A double that hands a ticket the record of the call
    begun BEFORE it fails the stage's own assertion."""
    calls = [n for names in CS.CALL_STAGES.values() for n in names]
    assert sorted(calls) == ["calls_grown_tickets", "calls_refused_ticket", "calls_screened"]
    for dt in ("float64", "mixed", "float32"):
        assert [n for n in CS.stages_for(dt) if n in calls] == list(CS.CALL_STAGES[dt])
    fresh_calls = {n: CS.run_stage(WholeSurfaceEngine, n) for n in calls}
    assert not any(isinstance(v, str) for obs in fresh_calls.values() for v in obs.values())
    assert {"grow.idx", "grow_near.scored", "best_ucb.ucb", "grow_ticket.mean", "grow_again.asked"} <= set(fresh_calls["calls_grown_tickets"])
    assert {"sync_512.verdict", "ticket_1000.survivors", "half", "sync_1000.idx"} <= set(fresh_calls["calls_screened"])
    assert {"off.idx", "small.verdict", "big.ucb"} <= set(fresh_calls["calls_refused_ticket"])
    assert fresh_calls["calls_grown_tickets"]["best_ucb.idx"][0] == -1  # (the ragged batch's empty segment, through the ticket)
    assert CS.pair_mismatches(WholeSurfaceEngine, "calls_screened", ["calls_grown_tickets"], fresh_calls) == []
    assert CS.pair_mismatches(WholeSurfaceEngine, "calls_grown_tickets", ["calls_refused_ticket"], fresh_calls) == []

    class SwapsTickets(WholeSurfaceEngine):
        def best_ucb_end(self, ticket):
            other = 1 - ticket
            return self._tickets.pop(other if other in self._tickets else ticket)

    with pytest.raises((AssertionError, ValueError)):
        CS.run_stage(SwapsTickets, "calls_grown_tickets")


def test_a_walk_over_all_stages_passes_on_the_whole_surface_double(fresh_all):
    assert CS.walk_mismatches(WholeSurfaceEngine, ALL[::-1] + ["sgpr", "gpr_small", "vgp_gauss"], fresh_all) == []


def test_the_pair_test_reports_a_remembered_likelihood(fresh_all):
    """... and the stages' own ``vgp_set_likelihood`` is what protects them on an engine that honours it."""
    var = list(CS.VAR_STAGES)
    bad = CS.pair_mismatches(RemembersLikelihoodEngine, "vgp_studentt", var, fresh_all)
    assert {m.stage for m in bad} == {"vgp_gauss", "svgp_gauss_uz"}, bad  # the Gaussian stages; SGPR has no likelihood
    assert any(m.observable == "q0.mu" for m in bad if m.stage == "vgp_gauss")
    assert CS.pair_mismatches(WholeSurfaceEngine, "vgp_studentt", ["vgp_gauss", "svgp_gauss_uz"], fresh_all) == []
    assert CS.pair_mismatches(RemembersLikelihoodEngine, "vgp_gauss", ["vgp_gauss", "vgp_studentt"], fresh_all) == []  # nothing to remember yet


def test_a_refused_setter_is_an_observable_and_the_run_goes_on(fresh_all):
    class RefusesData(WholeSurfaceEngine):
        def set_data(self, X, y):
            if self.post is not None and np.asarray(X).shape[0] == 50:
                raise ValueError("refused after history")
            super().set_data(X, y)

    bad = CS.pair_mismatches(RefusesData, "gpr_general", ["gpr_small", "gpr_nograd"], fresh_all)
    assert bad and {m.stage for m in bad} == {"gpr_small"}
    assert any(m.observable == "set_data" and "absent from the fresh run" in m.note for m in bad)  # the status itself
    assert any(m.observable == "predict.mean" for m in bad)  # ... and the stage went on: the rest of it is still compared


def test_an_attribute_error_inside_a_call_escapes():
    class Broken(WholeSurfaceEngine):
        def get_vector(self, which):
            return self.no_such_member

    with pytest.raises(AttributeError):
        CS.run_stage(Broken, "gpr_small")


def test_every_gpr_stage_runs_and_absent_observables_are_absent(fresh):
    assert set(fresh["gpr_general"]) >= {"fit.nlml", "fit.grad", "predict.mean", "predict.var", "grow.idx", "best_ucb.ucb"}
    assert "hash" not in fresh["gpr_general"] and "linv" not in fresh["gpr_general"]  # the double offers neither
    assert "fit.grad" not in fresh["gpr_nograd"]
    assert fresh["batch"] == {} and fresh["set_posterior"] == {}
    assert fresh["failed_fit"]["fit"].startswith("LinAlgError")  # a status is an observable
    seg = fresh["gpr_general"]
    assert seg["best_ucb.idx"][0] == -1 and np.isnan(seg["best_ucb.ucb"][0])  # the empty segment


def test_pairs_and_walks_pass_on_an_engine_without_history(fresh):
    for first in ("gpr_general", "append_pad_crossing", "failed_fit"):
        assert CS.pair_mismatches(OracleEngine, first, NAMES, fresh) == []
    for seed in range(3):
        assert CS.walk_mismatches(OracleEngine, CS.walk_sequence(NAMES, seed), fresh) == []


def test_the_comparison_is_bitwise_and_collects_everything():
    a = {"x": np.array([0.0, np.nan, 1.0]), "i": np.array([1, 2]), "s": "LinAlgError: pivot 1", "only_here": 1.0}
    nan2 = np.array([np.nan]).view(np.uint64)
    nan2[0] ^= 1  # another NaN payload
    b = {"x": np.array([-0.0, nan2.view(np.float64)[0], 1.0 + 2.0 ** -52]), "i": np.array([1, 3]), "s": "LinAlgError: pivot 2"}
    assert CS.compare("st", a, dict(a)) == []
    bad = {m.observable: m for m in CS.compare("st", a, b)}
    assert sorted(bad) == ["i", "only_here", "s", "x"]  # all of them, not the first
    assert bad["x"].n_diff == 3 and bad["x"].max_diff == 2.0 ** -52  # signed zero, NaN payload, one ulp
    assert bad["i"].n_diff == 1 and "st" in str(bad["i"]) and "i:" in str(bad["i"])
    assert CS.compare("st", {"x": np.zeros(3)}, {"x": np.zeros(4)})[0].note.startswith("shape")
    h = CS.compare("st", {"hash": 2 ** 63 + 1}, {"hash": 2 ** 63})[0]  # integers are reported exactly, not through float64
    assert h.n_diff == 1 and h.max_diff == 1.0 and str(2 ** 63 + 1) in h.note


def test_the_pair_test_reports_stale_rows_and_names_the_stage(fresh):
    # 200 rows, then 50 at the same D: rows 50 .. 127 of the block still hold the old problem
    bad = CS.pair_mismatches(StaleRowsEngine, "gpr_general", NAMES, fresh)
    hit = {(m.stage, m.observable) for m in bad}
    assert ("gpr_small", "predict.mean") in hit
    assert all("after gpr_general" in m.note for m in bad)
    assert not any(m.stage == "gpr_wide" for m in bad)  # another D: the buffers were laid out anew
    assert not any(m.observable == "predict.var" for m in bad)  # only what the leak touches is reported
    m = next(m for m in bad if (m.stage, m.observable) == ("gpr_small", "predict.mean"))
    assert m.n_diff > 200 and m.max_diff > 1e-6, m
    # the other order leaks nothing: the larger problem overwrites every row the smaller one left
    assert not [m for m in CS.pair_mismatches(StaleRowsEngine, "gpr_small", NAMES, fresh) if m.stage == "gpr_general"]


def test_the_pair_test_reports_a_remembered_choice_and_names_the_stage(fresh):
    bad = CS.pair_mismatches(StickyChoiceEngine, "gpr_wide", NAMES, fresh)
    stages = {m.stage for m in bad}
    assert {"gpr_small", "gpr_general", "append_in_place"} <= stages
    assert all(m.observable.startswith(("predict", "grow", "best_ucb")) for m in bad)
    assert CS.pair_mismatches(StickyChoiceEngine, "gpr_small", [n for n in NAMES if n != "gpr_wide"], fresh) == []


@pytest.mark.parametrize("engine,sequence,stage,where", [
    (StaleRowsEngine, ["gpr_small", "gpr_wide", "gpr_general", "gpr_small", "batch", "gpr_nograd"], "gpr_small",
     "step 3 of the walk, after gpr_wide, gpr_general"),
    (StickyChoiceEngine, ["failed_fit", "gpr_wide", "batch", "gpr_shrunk_pad", "gpr_small"], "gpr_shrunk_pad",
     "step 3 of the walk, after gpr_wide, batch")])
def test_the_walk_reports_the_leak_with_its_step_and_the_stages_before_it(engine, sequence, stage, where, fresh):
    bad = CS.walk_mismatches(engine, sequence, fresh)
    assert bad and bad[0].stage == stage and where in bad[0].note, bad[:1]
    assert not any(f"step {k} " in m.note for m in bad for k in range(3))  # nothing is reported before the leak shows
    assert where in CS.report(bad)


def test_the_helper_never_loads_the_hip_library():
    assert not any(getattr(v, "__name__", "").startswith("pygpso_amd") for v in vars(CS).values())
    assert not any(getattr(v, "__name__", "").startswith("pygpso_amd") for v in globals().values())
