"""
The entry points that read a float64 factor -- the point calls on the dense factor (predict_grad, the joint predictive, the
pathwise draws, cross-covariance, batch selection) and the variational and sparse families (VGP, SGPR, SVGP) -- on a
"float32" context: each is refused with GPSO_E_ARG and the message below, word for word, and none of the refusals touches
the resident posterior: a predict behind them returns the bits it returned before.  The messages were recorded from the
library as it stood before the engine's untyped families moved out of the typed class template (csrc/engine_core.hpp).
"""
import numpy as np
import pytest

from pygpso_amd import acquisition as A
from pygpso_amd import model as M_
from tests.helpers import synthetic_leaves, synthetic_problem

pytestmark = pytest.mark.gpu
N, D, M, DRAWS, FEATURES, KERNEL = 8, 2, 3, 2, 4, "Matern52"

_DENSE = ' needs a GPSO_F64 or GPSO_MIXED context -- dtype="float64" or "mixed" -- (the dense factor in double)'
_VGP = "the variational GP needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context"
_SGPR = "SGPR needs a float64 fit: open a GPSO_F64 or GPSO_MIXED context"
_U = np.array([M_._softplus_inv(0.5), M_._softplus_inv(1.2), M_._softplus_inv(0.01)], dtype=np.float64)


def _rng():
    return np.random.default_rng(5)


CALLS = {
    "predict_grad": (lambda e, xs: e.predict_grad(xs),
                     "gpso_predict_grad needs a GPSO_F64 or GPSO_MIXED context (the dense factor in double)"),
    "predict_joint": (lambda e, xs: e.predict_joint(xs), "gpso_predict_joint" + _DENSE),
    "sample_joint": (lambda e, xs: e.sample_joint(xs, _rng().normal(size=(DRAWS, M)), 1.0e-6), "gpso_sample_joint" + _DENSE),
    "paths_draw": (lambda e, xs: e.paths_draw(_rng().normal(size=(FEATURES, D)), _rng().random(FEATURES),
                                              _rng().normal(size=(DRAWS, FEATURES))), "gpso_paths_draw" + _DENSE),
    "paths_draw_q": (lambda e, xs: e.paths_draw_q(_rng().normal(size=(FEATURES, D)), _rng().random(FEATURES),
                                                  _rng().normal(size=(DRAWS, FEATURES))), "gpso_paths_draw_q" + _DENSE),
    "paths_eval": (lambda e, xs: e.paths_eval(xs), "gpso_paths_eval" + _DENSE),
    "cross_cov": (lambda e, xs: e.cross_cov(xs, xs[:2]), "gpso_cross_cov" + _DENSE),
    "best_batch": (lambda e, xs: e.best_batch(xs, A.UCBVar(2.0), 2, 0.01), "gpso_best_batch" + _DENSE),
    "vgp_set_likelihood": (lambda e, xs: e.vgp_set_likelihood("StudentT", 5.0, 20), _VGP),
    "vgp_set_q": (lambda e, xs: e.vgp_set_q(), _VGP),
    "vgp_extend_q": (lambda e, xs: e.vgp_extend_q(), _VGP),
    "vgp_elbo_u": (lambda e, xs: e.vgp_elbo_u(KERNEL, _U, 1, False), _VGP),
    "vgp_natgrad": (lambda e, xs: e.vgp_natgrad(KERNEL, _U, 1, False), _VGP),
    "vgp_posterior": (lambda e, xs: e.vgp_posterior(KERNEL, _U, 1, False), _VGP),
    "sgpr_set_inducing": (lambda e, xs: e.sgpr_set_inducing(xs), _SGPR),
    "sgpr_select_inducing": (lambda e, xs: e.sgpr_select_inducing(KERNEL, _U, 1, M), _SGPR),
    "sgpr_bound_u": (lambda e, xs: e.sgpr_bound_u(KERNEL, _U, 1, False), _SGPR),
    "sgpr_posterior": (lambda e, xs: e.sgpr_posterior(KERNEL, _U, 1, False), _SGPR),
    "svgp_init_q": (lambda e, xs: e.svgp_init_q(), _SGPR),
    "svgp_elbo_u": (lambda e, xs: e.svgp_elbo_u(KERNEL, _U, 1, False), _SGPR),
    "svgp_posterior": (lambda e, xs: e.svgp_posterior(KERNEL, _U, 1, False), _SGPR),
}


@pytest.fixture(scope="module")
def fitted():
    """One float32 context, fitted once; what predict returns on it before any refusal."""
    from pygpso_amd import HipGPEngine

    X, y = synthetic_problem(N, D, seed=7)
    xs = synthetic_leaves(M, D, seed=11)
    eng = HipGPEngine("float32", device=0)
    eng.set_data(X, y)
    eng.fit_eval(KERNEL, [0.5], 1.2, 0.01, 0.0, want_grad=False)
    mean, var = eng.predict(xs)
    yield eng, xs, mean.copy(), var.copy()
    eng.close()


@pytest.mark.parametrize("name", list(CALLS))
def test_a_float32_context_refuses_the_double_only_call(fitted, name):
    eng, xs, _, _ = fitted
    call, message = CALLS[name]
    with pytest.raises(ValueError) as info:  # (HipGPEngine._check: GPSO_E_ARG raises ValueError with gpso_last_error's text)
        call(eng, xs)
    assert type(info.value) is ValueError
    assert str(info.value) == message
    assert eng.last_message() == message


def test_predict_behind_the_refusals_returns_the_bits_it_returned_before(fitted):
    eng, xs, mean0, var0 = fitted
    for name, (call, _) in CALLS.items():  # (every refusal once more, so that this test stands on its own as well)
        with pytest.raises(ValueError):
            call(eng, xs)
    mean, var = eng.predict(xs)
    assert mean.tobytes() == mean0.tobytes() and var.tobytes() == var0.tobytes()
