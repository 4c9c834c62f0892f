"""
The one path of the hyper-parameters from the optimiser's vector u to the engine and back (csrc/theta.hpp) on the MI355X:
every entry point in u decodes u to the bits of the Python transform (pygpso_amd/model.py: _softplus, _sigmoid), evaluates
what the constrained entry point evaluates at that theta, and carries the gradient back by the chain rule -- all held to
equality, not to a tolerance -- and every theta the engine cannot use is refused with the status, the message and the
effect on the resident posterior that the library had before the path was made one.
"""
import functools

import numpy as np
import pytest

from pygpso_amd import model as M_
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu
N, D, M, KERNEL = 40, 3, 8, "Matern52"
GAUSS, STUDENT = ("Gaussian", 0.0), ("StudentT", 5.0)
SHAPES = [(1, False), (1, True), (D, False), (D, True)]  # (n_ls, train_mean)
SHAPE_IDS = ["iso", "iso-mean", "ard", "ard-mean"]


@functools.lru_cache(maxsize=None)
def _problem():
    X, y = synthetic_problem(N, D, seed=7)
    for a in (X, y):
        a.setflags(write=False)
    return X, y, X[::5][:M].copy(), synthetic_leaves(16, D, seed=11)


def _u(n_ls, train_mean, which):
    """ordinary: every slot positive and moderate.  branches: a negative slot and one above 30, so softplus takes both of
    its branches (lengthscale 0.2, kernel variance 31.5, likelihood parameter 0.049)."""
    inv = M_._softplus_inv
    if which == "ordinary":
        u = [inv(0.5 + 0.1 * k) for k in range(n_ls)] + [inv(1.2), inv(0.01), 0.1]
    else:
        u = [-1.5, 0.4, 0.9][:n_ls] + [31.5, -3.0, -0.25]
    return np.array(u[:n_ls + 2 + (1 if train_mean else 0)], dtype=np.float64)


def _theta_py(u, n_ls, train_mean, mean_c_fixed, floor=1.0e-6):
    th = np.empty(n_ls + 3)
    th[:n_ls + 2] = M_._softplus(u[:n_ls + 2])
    th[n_ls + 1] = floor + th[n_ls + 1]
    th[n_ls + 2] = u[n_ls + 2] if train_mean else mean_c_fixed
    return th


def _grad_u_py(u, n_ls, train_mean, g):
    gu = g[:n_ls + 2] * M_._sigmoid(u[:n_ls + 2])
    return np.append(gu, g[n_ls + 2]) if train_mean else gu


def _engine(dtype="float64", lik=None, inducing=False):
    from pygpso_amd import HipGPEngine

    X, y, Z, _ = _problem()
    eng = HipGPEngine(dtype, device=0)
    eng.set_data(X, y)
    if lik is not None:
        eng.vgp_set_likelihood(lik[0], lik[1], 20)
    if inducing:
        eng.sgpr_set_inducing(Z)
    return eng


# ---- the exact GP: the calls in u against the constrained entry points ------------------------------------------------------
@pytest.mark.parametrize("which", ["ordinary", "branches"])
@pytest.mark.parametrize("n_ls,train_mean", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
def test_fit_eval_u_is_fit_eval_at_the_python_theta(dtype, n_ls, train_mean, which):
    u, c_fixed = _u(n_ls, train_mean, which), 0.375
    eng = _engine(dtype)
    th_py = _theta_py(u, n_ls, train_mean, c_fixed)
    f, gu, th = eng.fit_eval_u(KERNEL, u, n_ls, train_mean, c_fixed)
    f_c, g_c = eng.fit_eval(KERNEL, th_py[:n_ls], th_py[n_ls], th_py[n_ls + 1], th_py[n_ls + 2])
    print(f"THETA fit_eval_u {dtype} n_ls={n_ls} mean={train_mean} {which}: f={f!r} f_c={f_c!r} "
          f"max|th - py|={np.max(np.abs(th - th_py)):.3e} max|gu - chain|={np.max(np.abs(gu - _grad_u_py(u, n_ls, train_mean, g_c))):.3e}")
    assert np.array_equal(th, th_py), (th, th_py)
    if not train_mean:
        assert th[n_ls + 2] == c_fixed
    assert f == f_c, (f, f_c)
    assert np.array_equal(gu, _grad_u_py(u, n_ls, train_mean, g_c)), (gu, g_c)
    eng.close()


@pytest.mark.parametrize("which", ["ordinary", "branches"])
@pytest.mark.parametrize("n_ls,train_mean", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_fit_eval_loo_u_is_fit_eval_loo_at_the_python_theta(dtype, n_ls, train_mean, which):
    u, c_fixed = _u(n_ls, train_mean, which), 0.375
    eng = _engine(dtype)
    th_py = _theta_py(u, n_ls, train_mean, c_fixed)
    f, gu, th, nlml = eng.fit_eval_loo_u(KERNEL, u, n_ls, train_mean, c_fixed)
    f_c, g_c, nlml_c = eng.fit_eval_loo(KERNEL, th_py[:n_ls], th_py[n_ls], th_py[n_ls + 1], th_py[n_ls + 2])
    print(f"THETA fit_eval_loo_u {dtype} n_ls={n_ls} mean={train_mean} {which}: f={f!r} f_c={f_c!r} nlml={nlml!r} nlml_c={nlml_c!r}")
    assert np.array_equal(th, th_py), (th, th_py)
    if not train_mean:
        assert th[n_ls + 2] == c_fixed
    assert f == f_c and nlml == nlml_c, (f, f_c, nlml, nlml_c)
    assert np.array_equal(gu, _grad_u_py(u, n_ls, train_mean, g_c)), (gu, g_c)
    eng.close()


@pytest.mark.parametrize("n_ls,train_mean", SHAPES, ids=SHAPE_IDS)
def test_batch_rows_are_the_single_calls_and_a_refused_row_stands_alone(n_ls, train_mean):
    a, b = _u(n_ls, train_mean, "ordinary"), _u(n_ls, train_mean, "branches")
    bad = a.copy()
    bad[n_ls - 1] = -800.0  # softplus gives exactly 0: a lengthscale the single call refuses
    assert M_._softplus(bad)[n_ls - 1] == 0.0
    U = np.stack([a, b, bad, 0.5 * (a + b), a + 0.25])
    good = [0, 1, 3, 4]
    eng = _engine("float64")
    assert eng.fit_batch_max() >= len(U)
    loss, grad, ok = eng.fit_eval_u_batch(KERNEL, U, n_ls, train_mean, 0.375)
    assert ok.tolist() == [True, True, False, True, True]
    assert np.isnan(loss[2]) and np.all(np.isnan(grad[2]))
    for r in good:
        f, gu, _ = eng.fit_eval_u(KERNEL, U[r], n_ls, train_mean, 0.375)
        assert loss[r] == f and np.array_equal(grad[r], gu), (r, loss[r], f)
    loss4, grad4, ok4 = eng.fit_eval_u_batch(KERNEL, U[good], n_ls, train_mean, 0.375)
    assert ok4.all() and np.array_equal(loss4, loss[good]) and np.array_equal(grad4, grad[good])
    eng.close()


# ---- the families: theta is the Python transform's, with the shift the likelihood asks for ----------------------------------
def _family_calls(eng, Z):
    """entry point -> callable (kernel, u, n_ls, train_mean, mean_c_fixed) -> theta"""
    return {
        "vgp_elbo_u": lambda *a: eng.vgp_elbo_u(*a)[2],
        "sgpr_bound_u": lambda *a: eng.sgpr_bound_u(*a)[2],
        "svgp_elbo_u": lambda *a: eng.svgp_elbo_u(*a)[2],
        "sgpr_bound_uz": lambda *a: eng.sgpr_bound_uz(*a, Z=Z)[3],
        "svgp_elbo_uz": lambda *a: eng.svgp_elbo_uz(*a, Z=Z)[3],
    }


FAMILY = [("vgp_elbo_u", GAUSS), ("vgp_elbo_u", STUDENT), ("sgpr_bound_u", GAUSS), ("svgp_elbo_u", GAUSS),
          ("svgp_elbo_u", STUDENT), ("sgpr_bound_uz", GAUSS), ("svgp_elbo_uz", GAUSS), ("svgp_elbo_uz", STUDENT)]


@pytest.mark.parametrize("entry,lik", FAMILY, ids=[f"{e}-{l[0]}" for e, l in FAMILY])
def test_family_theta_is_the_python_transform(entry, lik):
    Z = _problem()[2]
    eng = _engine("float64", lik, inducing=not entry.startswith("vgp"))
    call = _family_calls(eng, Z)[entry]
    floor = 0.0 if lik == STUDENT else 1.0e-6
    for n_ls, train_mean in SHAPES:
        for which in ("ordinary", "branches"):
            u = _u(n_ls, train_mean, which)
            th = call(KERNEL, u, n_ls, train_mean, 0.375)
            th_py = _theta_py(u, n_ls, train_mean, 0.375, floor)
            assert np.array_equal(th, th_py), (entry, lik, n_ls, train_mean, which, th, th_py)
            assert th[n_ls + 1] == floor + M_._softplus(u[n_ls + 1])
    eng.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
# One bad call per rule that can be reached and entry point.  What is expected -- the exception, its message, and what
# `predict` at 16 leaves does afterwards -- was recorded from this same table run against the library as it was before
# csrc/theta.hpp existed (the parent commit of that change), and is written down here as literals.
def _bad_calls(student):
    """rule -> (kernel, u, n_ls) of a call that breaks it alone (train_mean True)"""
    good = _u(D, True, "ordinary")

    def at(slot):
        u = good.copy()
        u[slot] = -800.0  # softplus: exactly 0
        return u

    rules = {"kernel id 7": (7, good, D), "n_ls = 2 with D = 3": (KERNEL, _u(2, True, "ordinary"), 2),
             "lengthscale slot -800": (KERNEL, at(1), D), "variance slot -800": (KERNEL, at(D), D),
             "n_ls = 0": (KERNEL, good[:3], 0)}
    if student:
        rules["Student-t scale slot -800"] = (KERNEL, at(D + 1), D)
    return rules


def _install_exact(eng):
    eng.fit_eval(KERNEL, [0.5], 1.2, 0.01, 0.1, want_grad=False)


def _install_vgp(eng):
    eng.vgp_set_q(np.zeros(N), 0.5 * np.eye(N))  # (a q below the prior: I - S S^T factors under either likelihood)
    eng.vgp_posterior(KERNEL, _u(D, True, "ordinary"), D, True, 0.0)


def _install_sgpr(eng):
    eng.sgpr_posterior(KERNEL, _u(D, True, "ordinary"), D, True, 0.0)


def _install_svgp(eng):
    u = _u(D, True, "ordinary")
    eng.svgp_init_q(KERNEL, u, D, True, 0.0, 0.01)
    eng.svgp_posterior(KERNEL, u, D, True, 0.0)


# family -> (engine arguments, how its posterior becomes resident, {entry point: call(eng, kernel, u, n_ls)})
FAMILIES = {
    "exact": (dict(), _install_exact, {
        "fit_eval_u": lambda e, k, u, n: e.fit_eval_u(k, u, n, True),
        "fit_eval_loo_u": lambda e, k, u, n: e.fit_eval_loo_u(k, u, n, True),
        "fit_eval_u_batch": lambda e, k, u, n: e.fit_eval_u_batch(k, u[None], n, True)}),
    "vgp-Gaussian": (dict(lik=GAUSS), _install_vgp, {
        "vgp_natgrad": lambda e, k, u, n: e.vgp_natgrad(k, u, n, True),
        "vgp_elbo_u": lambda e, k, u, n: e.vgp_elbo_u(k, u, n, True),
        "vgp_posterior": lambda e, k, u, n: e.vgp_posterior(k, u, n, True)}),
    "sgpr": (dict(lik=GAUSS, inducing=True), _install_sgpr, {
        "sgpr_select_inducing": lambda e, k, u, n: e.sgpr_select_inducing(k, u[:n + 2], n, M),
        "sgpr_bound_u": lambda e, k, u, n: e.sgpr_bound_u(k, u, n, True),
        "sgpr_posterior": lambda e, k, u, n: e.sgpr_posterior(k, u, n, True),
        "sgpr_bound_uz": lambda e, k, u, n: e.sgpr_bound_uz(k, u, n, True)}),
    "svgp-Gaussian": (dict(lik=GAUSS, inducing=True), _install_svgp, {
        "svgp_init_q": lambda e, k, u, n: e.svgp_init_q(k, u, n, True, 0.0, 0.01),
        "svgp_natgrad": lambda e, k, u, n: e.svgp_natgrad(k, u, n, True),
        "svgp_elbo_u": lambda e, k, u, n: e.svgp_elbo_u(k, u, n, True),
        "svgp_posterior": lambda e, k, u, n: e.svgp_posterior(k, u, n, True),
        "svgp_elbo_uz": lambda e, k, u, n: e.svgp_elbo_uz(k, u, n, True)}),
}
FAMILIES["vgp-StudentT"] = (dict(lik=STUDENT),) + FAMILIES["vgp-Gaussian"][1:]
FAMILIES["svgp-StudentT"] = (dict(lik=STUDENT, inducing=True),) + FAMILIES["svgp-Gaussian"][1:]
# (a batch row with a refused value is that row's status, not a refusal of the call: test_batch_rows_...; the VGP takes any
# scale, and gpso_svgp_init_q puts its noise variance in the scale's place)
NOT_A_REFUSAL = {("fit_eval_u_batch", "lengthscale slot -800"), ("fit_eval_u_batch", "variance slot -800"),
                 ("vgp_natgrad", "Student-t scale slot -800"), ("vgp_elbo_u", "Student-t scale slot -800"),
                 ("vgp_posterior", "Student-t scale slot -800"), ("svgp_init_q", "Student-t scale slot -800")}


def observe(family):
    """Every bad call of the family's table -> [(entry, rule, exception type name or None, message, what predict does then)];
    the last: "kept" (the bits it returned before the call), "changed", or the exception it raises, as (name, message)."""
    kwargs, install, entries = FAMILIES[family]
    leaves = _problem()[3]
    eng = _engine("float64", **kwargs)
    rows = []
    for entry, call in entries.items():
        for rule, (kernel, u, n_ls) in _bad_calls("StudentT" in family).items():
            if (entry, rule) in NOT_A_REFUSAL:
                continue
            install(eng)
            before = eng.predict(leaves)
            try:
                call(eng, kernel, u, n_ls)
                raised = (None, "")
            except Exception as e:  # noqa: BLE001 (the type is what is recorded)
                raised = (type(e).__name__, str(e))
            try:
                after = eng.predict(leaves)
                then = "kept" if all(np.array_equal(p, q) for p, q in zip(before, after)) else "changed"
            except Exception as e:  # noqa: BLE001
                then = (type(e).__name__, str(e))
            rows.append((entry, rule) + raised + (then,))
    eng.close()
    return rows


MESSAGE = {  # the refusal of each rule: always a ValueError (GPSO_E_ARG)
    "kernel id 7": "unknown kernel id 7",
    "n_ls = 2 with D = 3": "n_ls=2 must be 1 or D=3",
    "lengthscale slot -800": "lengthscale[1]=0 must be positive",
    "variance slot -800": "kernel variance 0 must be positive",
    "Student-t scale slot -800": "likelihood parameter 0 must be positive",
    "n_ls = 0": "n_ls=0 outside [1, 64]",
}
# What predict does after the refused call.  The exact GP, the SGPR and the SVGP validate before they touch anything: "kept".
# The VGP's entry points declare the posterior replaced (vgp_begin) before set_theta looks at the kernel's values, so a
# refusal that is set_theta's leaves no posterior behind; one made while u is decoded (n_ls = 0) comes before that.
NO_POSTERIOR = ("GpsoHipError", "libgpso_hip error -5: no posterior resident: call gpso_fit_eval / gpso_set_posterior first")
THEN = {(family, entry, rule): NO_POSTERIOR for family in ("vgp-Gaussian", "vgp-StudentT")
        for entry in ("vgp_natgrad", "vgp_elbo_u", "vgp_posterior")
        for rule in ("kernel id 7", "n_ls = 2 with D = 3", "lengthscale slot -800", "variance slot -800")}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_refusals_are_the_recorded_ones(family):
    rows = observe(family)
    for entry, rule, exc, msg, then in rows:
        print(f"THETA_REFUSAL {family} {entry} | {rule} | {exc}: {msg} | then {then}")
    for entry, rule, exc, msg, then in rows:
        assert (exc, msg) == ("ValueError", MESSAGE[rule]), (family, entry, rule, exc, msg)
        assert then == THEN.get((family, entry, rule), "kept"), (family, entry, rule, then)
