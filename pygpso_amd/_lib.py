"""
ctypes binding of ``libgpso_hip.so`` (C-ABI: ``include/gpso_hip.h``).

This is the whole Python<->HIP boundary: plain pointers and sizes, no torch types.  The library
is built in-tree by ``__graft_entry__.build()`` / ``make -C pygpso_amd/csrc``.  There is NO CPU
fallback: if the shared library is missing or no HIP device is present, the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPSO_HIP_LIB overrides the path (experimental builds of the same C-ABI)
LIB_PATH = os.environ.get("GPSO_HIP_LIB") or os.path.join(_HERE, "libgpso_hip.so")

# status codes / enums (mirror include/gpso_hip.h)
OK, E_ARG, E_HIP, E_NOTPD, E_OOM, E_STATE, E_RCCL, E_PRECISION = 0, -1, -2, -3, -4, -5, -6, -7
F64, F32, MIXED = 0, 1, 2
MATERN52, MATERN32, MATERN12, SQEXP = 0, 1, 2, 3
MEM_HOST, MEM_DEVICE = 0, 1
UNIQUE_ID_BYTES = 128
MAT_CHOL, MAT_LINV, MAT_KINV, MAT_GRAM = 0, 1, 2, 3
VEC_ALPHA, VEC_WHITE, VEC_NOISE_DIAG = 0, 1, 2
SGPR_KUF, SGPR_LU, SGPR_LB, SGPR_CV = 0, 1, 2, 3
LIK_GAUSSIAN, LIK_STUDENT_T, LIK_GAUSSIAN_GH, LIK_BERNOULLI = 0, 1, 2, 3
LIKELIHOOD_IDS = {"Gaussian": LIK_GAUSSIAN, "StudentT": LIK_STUDENT_T, "GaussianGH": LIK_GAUSSIAN_GH, "Bernoulli": LIK_BERNOULLI}
OPT_PREDICT_MATH = 1
OPT_FIT_SINGLE_LEVEL_MAX = 2
OPT_GENERATION = 3
OPT_PRECISION_CHECK = 4
OPT_FIT_FUSED_SMALL = 5
OPT_FIT_BF16_SYRK = 6
OPT_TIMING = 7
OPT_SPLIT_KERNEL = 8
OPT_SMALL_CALLS = 9
OPT_CONTRACTION = 10
OPT_FUSED_PREP = 11
OPT_FIT_OVERLAP = 12
OPT_ROW_LOOP = 13
OPT_PARK_BYTES = 14
OPT_SCREEN = 15
OPT_SURVIVOR_TILE = 16
SCREEN_NONE, SCREEN_ACCEPTED, SCREEN_REFUSED = 0, 1, 2  # gpso_last_count(ctx, 8)
CONTRACTION_AUTO, CONTRACTION_F32, CONTRACTION_F16 = 0, 1, 2
SPLIT_KERNEL_AUTO, SPLIT_KERNEL_TWO_PHASE, SPLIT_KERNEL_FUSED16, SPLIT_KERNEL_FUSED32 = 0, 1, 2, 3
OPTF_TOL_VAR, OPTF_TOL_MEAN = 100, 101
GEN_F64, GEN_F32, GEN_AUTO = 0, 1, 2
ACQ_UCB_VAR, ACQ_UCB_STD, ACQ_EI, ACQ_LOGEI, ACQ_PI, ACQ_MES = 0, 1, 2, 3, 4, 5
ENSEMBLE_MAX = 32  # members of a hyper-parameter ensemble; gpso_ensemble_info reports ENSEMBLE_THETA doubles per member
ENSEMBLE_THETA = 48 + 3
CONSTRAINTS_MAX = 16  # members of a context's constraint set; gpso_constraint_info reports ENSEMBLE_THETA doubles per member
CON_WEIGHT, CON_GATE, CON_FEASIBILITY = 0, 1, 2  # gpso_cspec.mode
CON_MODES = {"weight": CON_WEIGHT, "gate": CON_GATE, "feasibility": CON_FEASIBILITY}
ACQ_MAX_MAXIMA = 64  # gpso_acq_set_maxima keeps at most this many; gpso_max_logcdf takes at most this many thresholds
FITMATH_NONE, FITMATH_SMALL, FITMATH_F32, FITMATH_F64, FITMATH_BF16X6, FITMATH_F16X3 = 0, 1, 2, 3, 4, 5  # gpso_last_count(ctx, 2)
GEN_IDS = {"float64": GEN_F64, "f64": GEN_F64, "float32": GEN_F32, "f32": GEN_F32, "auto": GEN_AUTO}
DTYPE_IDS = {"float64": F64, "fp64": F64, "f64": F64, "float32": F32, "fp32": F32, "f32": F32, "mixed": MIXED}
MATH_NATIVE, MATH_AUTO, MATH_BF16X3, MATH_BF16X6, MATH_F16X3 = 0, 1, 3, 6, 13
MATH_IDS = {"native": MATH_NATIVE, "f32": MATH_NATIVE, "auto": MATH_AUTO, "bf16x3": MATH_BF16X3, "bf16x6": MATH_BF16X6,
            "f16x3": MATH_F16X3}

KERNEL_IDS = {
    "Matern52": MATERN52,
    "Matern32": MATERN32,
    "Matern12": MATERN12,
    "Exponential": MATERN12,
    "SquaredExponential": SQEXP,
    "RBF": SQEXP,
}

_c_double_p = C.POINTER(C.c_double)
_c_int64_p = C.POINTER(C.c_int64)


class GpsoAcq(C.Structure):
    """``gpso_acq``: what a best-acquisition call ranks by."""
    _fields_ = [("kind", C.c_int), ("latent", C.c_int), ("varsigma", C.c_double), ("incumbent", C.c_double),
                ("xi", C.c_double)]


_c_acq_p = C.POINTER(GpsoAcq)


class GpsoCspec(C.Structure):
    """``gpso_cspec``: how a constrained call combines the acquisition with the probability of feasibility."""
    _fields_ = [("mode", C.c_int), ("log_pof_min", C.c_double)]


_c_cspec_p = C.POINTER(GpsoCspec)

EHVI_FRONT_MAX = 63  # points of the front a gpso_ehvi record may carry


class GpsoEhvi(C.Structure):
    """``gpso_ehvi``: objective 2's member index, the front and the reference point of an EHVI call."""
    _fields_ = [("member", C.c_int), ("latent", C.c_int), ("p", C.c_int), ("front", C.POINTER(C.c_double)), ("ref", C.c_double * 2)]


_c_ehvi_p = C.POINTER(GpsoEhvi)

MC_QEI, MC_QPI = 0, 1  # gpso_mcacq.kind
MC_KINDS = {"qei": MC_QEI, "qnei": MC_QEI, "qpi": MC_QPI}  # (qNoisyEI is QEI under per-draw bars)
MC_MAX_PICKS = MC_MAX_PENDING = 64


class GpsoMcAcq(C.Structure):
    """``gpso_mcacq``: what a Monte-Carlo batch call over the path draws ranks by."""
    _fields_ = [("kind", C.c_int), ("xi", C.c_double), ("incumbent", C.c_double)]


_c_mcacq_p = C.POINTER(GpsoMcAcq)

# every symbol include/gpso_hip.h declares: (restype, argtypes)
SIGNATURES = {
    "gpso_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "gpso_destroy": (None, [C.c_void_p]),
    "gpso_last_error": (C.c_char_p, [C.c_void_p]),
    "gpso_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gpso_synchronize": (C.c_int, [C.c_void_p]),
    "gpso_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "gpso_set_option_f64": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "gpso_wait_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gpso_precision_info": (C.c_int, [C.c_void_p, _c_double_p]),
    "gpso_set_data": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, C.c_int64, C.c_int]),
    "gpso_fit_eval": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_double, C.c_double,
                                C.c_double, _c_double_p, _c_double_p]),
    "gpso_fit_eval_u": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, _c_double_p,
                                  _c_double_p, _c_double_p]),
    "gpso_loo": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_fit_eval_loo": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_double, C.c_double,
                                    C.c_double, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_fit_eval_loo_u": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, _c_double_p,
                                      _c_double_p, _c_double_p, _c_double_p]),
    "gpso_fit_batch_max": (C.c_int, [C.c_void_p]),
    "gpso_fit_eval_u_batch": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                        _c_double_p, _c_double_p, C.POINTER(C.c_int), _c_int64_p]),
    "gpso_set_noise_diag": (C.c_int, [C.c_void_p, _c_double_p, C.c_int64]),
    "gpso_append": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, C.c_int64, _c_double_p]),
    "gpso_append_noise": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, _c_double_p, C.c_int64, _c_double_p]),
    "gpso_set_posterior": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, _c_double_p, C.c_int64,
                                     C.c_int, C.c_int, _c_double_p, C.c_int, C.c_double, C.c_double,
                                     C.c_double]),
    "gpso_vgp_set_likelihood": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, _c_double_p, _c_double_p]),
    "gpso_vgp_set_q": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, C.c_int64]),
    "gpso_vgp_get_q": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p]),
    "gpso_vgp_extend_q": (C.c_int, [C.c_void_p]),
    "gpso_vgp_natgrad": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, C.c_double]),
    "gpso_vgp_elbo_u": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, _c_double_p,
                                  _c_double_p, _c_double_p]),
    "gpso_vgp_posterior": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double]),
    "gpso_sgpr_set_inducing": (C.c_int, [C.c_void_p, _c_double_p, C.c_int64]),
    "gpso_sgpr_select_inducing": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int64, _c_int64_p]),
    "gpso_sgpr_get_inducing": (C.c_int, [C.c_void_p, _c_double_p, _c_int64_p, _c_int64_p]),
    "gpso_sgpr_get_factor": (C.c_int, [C.c_void_p, C.c_int, _c_double_p]),
    "gpso_sgpr_bound_u": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, _c_double_p,
                                    _c_double_p, _c_double_p]),
    "gpso_sgpr_posterior": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, _c_double_p]),
    "gpso_sgpr_move_inducing": (C.c_int, [C.c_void_p, _c_double_p]),
    "gpso_sgpr_bound_uz": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, _c_double_p,
                                     _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_svgp_elbo_uz": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, _c_double_p,
                                    _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_svgp_init_q": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, C.c_double]),
    "gpso_svgp_set_q": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, C.c_int64]),
    "gpso_svgp_get_q": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p]),
    "gpso_svgp_natgrad": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, C.c_double]),
    "gpso_svgp_elbo_u": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, _c_double_p,
                                   _c_double_p, _c_double_p]),
    "gpso_svgp_posterior": (C.c_int, [C.c_void_p, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_double, _c_double_p]),
    "gpso_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                               C.c_void_p, C.c_int]),
    "gpso_predict_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int]),
    "gpso_predict_joint": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_double, C.c_void_p, C.c_void_p,
                                     C.c_int]),
    "gpso_sample_joint": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_double, _c_double_p, C.c_int64,
                                    _c_double_p, _c_int64_p, _c_double_p]),
    "gpso_paths_draw": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, C.c_int64, _c_double_p, _c_double_p, C.c_int64]),
    "gpso_paths_draw_q": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, C.c_int64, _c_double_p, _c_double_p, C.c_int64]),
    "gpso_paths_eval": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_int64_p, C.c_int, C.c_void_p, C.c_int,
                                  _c_int64_p, _c_double_p]),
    "gpso_paths_info": (C.c_int, [C.c_void_p, _c_int64_p, _c_int64_p]),
    "gpso_paths_best_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_mcacq_p, _c_double_p, _c_double_p, C.c_int,
                                        C.c_int, _c_int64_p, _c_double_p, _c_double_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]),
    "gpso_paths_batch_host": (C.c_int, [_c_mcacq_p, _c_double_p, C.c_int64, C.c_int64, C.c_int, _c_double_p, C.c_int, _c_int64_p,
                                        _c_double_p, _c_double_p, C.POINTER(C.c_int), _c_double_p]),
    "gpso_best_ucb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_int64_p,
                                C.c_int, C.c_double, _c_int64_p, _c_double_p, _c_double_p,
                                _c_double_p]),
    "gpso_best_ucb_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_int64_p, C.c_int, C.c_double]),
    "gpso_best_ucb_grow_begin": (C.c_int, [C.c_void_p, _c_double_p, C.c_int, C.c_int, C.c_double]),
    "gpso_best_ucb_end": (C.c_int, [C.c_void_p, C.c_int, _c_int64_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_best_acq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_int64_p, C.c_int, _c_acq_p,
                                _c_int64_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_best_acq_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_int64_p, C.c_int, _c_acq_p]),
    "gpso_best_acq_grow": (C.c_int, [C.c_void_p, _c_double_p, C.c_int, C.c_int, _c_acq_p, _c_int64_p, _c_double_p,
                                     _c_double_p, _c_double_p]),
    "gpso_best_acq_grow_begin": (C.c_int, [C.c_void_p, _c_double_p, C.c_int, C.c_int, _c_acq_p]),
    "gpso_acq_values": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_acq_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int]),
    "gpso_acq_eval_host": (C.c_int, [_c_acq_p, _c_double_p, _c_double_p, C.c_double, C.c_int64, _c_double_p]),
    "gpso_acq_set_maxima": (C.c_int, [C.c_void_p, _c_double_p, C.c_int]),
    "gpso_acq_get_maxima": (C.c_int, [C.c_void_p, _c_double_p, C.POINTER(C.c_int)]),
    "gpso_acq_mes_eval_host": (C.c_int, [_c_double_p, C.c_int, C.c_int, _c_double_p, _c_double_p, C.c_double, C.c_int64,
                                         _c_double_p]),
    "gpso_acq_math_host": (C.c_int, [C.c_int, _c_double_p, C.c_int64, _c_double_p]),
    "gpso_max_logcdf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_double, _c_double_p, C.c_int,
                                  _c_double_p, _c_int64_p]),
    "gpso_max_logcdf_host": (C.c_int, [_c_double_p, _c_double_p, C.c_int64, C.c_double, _c_double_p, C.c_int, _c_double_p,
                                       _c_int64_p]),
    "gpso_cross_cov": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_double_p, C.c_int, C.c_void_p, C.c_int]),
    "gpso_best_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_acq_p, C.c_double, C.c_int, _c_int64_p,
                                  _c_double_p, _c_double_p, _c_double_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]),
    "gpso_batch_greedy_host": (C.c_int, [_c_acq_p, _c_double_p, _c_double_p, _c_double_p, C.c_double, C.c_double, C.c_int64, C.c_int,
                                         _c_int64_p, _c_double_p, _c_double_p, C.POINTER(C.c_int), _c_double_p]),
    "gpso_batch_greedy_mes_host": (C.c_int, [_c_double_p, C.c_int, C.c_int, _c_double_p, _c_double_p, _c_double_p, C.c_double,
                                             C.c_double, C.c_int64, C.c_int, _c_int64_p, _c_double_p, _c_double_p,
                                             C.POINTER(C.c_int), _c_double_p]),
    "gpso_ensemble_max": (C.c_int, [C.c_void_p]),
    "gpso_ensemble_push": (C.c_int, [C.c_void_p]),
    "gpso_ensemble_clear": (C.c_int, [C.c_void_p]),
    "gpso_ensemble_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), _c_double_p]),
    "gpso_ensemble_best_acq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_int64_p, C.c_int, _c_acq_p,
                                         _c_int64_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_ensemble_acq_values": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_acq_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "gpso_ensemble_fold_host": (C.c_int, [_c_acq_p, _c_double_p, _c_double_p, _c_double_p, C.c_int, C.c_int64, _c_double_p,
                                          _c_double_p, _c_double_p]),
    "gpso_constraint_max": (C.c_int, [C.c_void_p]),
    "gpso_constraint_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_int]),
    "gpso_constraint_clear": (C.c_int, [C.c_void_p]),
    "gpso_constraint_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), _c_double_p, _c_double_p, C.POINTER(C.c_int)]),
    "gpso_constrained_best_acq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_int64_p, C.c_int, _c_acq_p,
                                            _c_cspec_p, _c_int64_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_constrained_acq_values": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_acq_p, _c_cspec_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "gpso_constrained_fold_host": (C.c_int, [_c_acq_p, _c_cspec_p, _c_double_p, _c_double_p, C.c_double, _c_double_p, _c_double_p,
                                             _c_double_p, _c_double_p, C.POINTER(C.c_int), C.c_int, C.c_int64, _c_double_p,
                                             _c_double_p]),
    "gpso_constrained_success_fold_host": (C.c_int, [_c_acq_p, _c_cspec_p, _c_double_p, _c_double_p, C.c_double, _c_double_p,
                                                     _c_double_p, _c_double_p, _c_double_p, C.POINTER(C.c_int), C.c_int, C.c_int64,
                                                     _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_ehvi_values": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_ehvi_p, _c_cspec_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_int]),
    "gpso_best_ehvi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, _c_int64_p, C.c_int, _c_ehvi_p, _c_cspec_p,
                                 _c_int64_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_ehvi_fold_host": (C.c_int, [_c_ehvi_p, _c_cspec_p, _c_double_p, _c_double_p, C.c_double, _c_double_p, _c_double_p, C.c_double,
                                      _c_double_p, _c_double_p, _c_double_p, _c_double_p, C.POINTER(C.c_int), C.c_int, C.c_int64,
                                      _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_success_prob_host": (C.c_int, [_c_double_p, _c_double_p, C.c_int64, _c_double_p, _c_double_p]),
    "gpso_predict_prob": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int]),
    "gpso_success_push": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gpso_success_clear": (C.c_int, [C.c_void_p]),
    "gpso_success_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), _c_int64_p, _c_double_p]),
    "gpso_screen_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_double, _c_double_p, _c_double_p,
                                    _c_double_p, _c_double_p]),
    "gpso_screen_eval_host": (C.c_int, [_c_double_p, _c_double_p, C.c_double, C.c_double, C.c_double, C.c_int64, _c_double_p,
                                        _c_double_p]),
    "gpso_screen_threshold_host": (C.c_double, [C.c_double, C.c_double, C.c_double]),
    "gpso_screen_survives_host": (C.c_int, [C.c_double, C.c_double, C.c_double]),
    "gpso_screen_accepts_host": (C.c_int, [C.c_double, C.c_double, C.c_int64, C.c_int64]),
    "gpso_screen_list": (C.c_int, [C.c_void_p, C.c_int64, _c_int64_p, C.POINTER(C.c_float), _c_int64_p]),
    "gpso_screen_partition_host": (C.c_int, [C.c_int64, C.c_int, C.c_int, _c_int64_p, _c_int64_p]),
    "gpso_survivor_narrow_max_host": (C.c_int64, [C.c_int, C.c_int, C.c_int64]),
    "gpso_screen_parts_host": (C.c_int, [C.c_int64]),
    "gpso_grow_rows": (C.c_int64, [C.c_int]),
    "gpso_grow": (C.c_int, [C.c_void_p, _c_double_p, C.c_int, C.c_int, C.c_int, _c_double_p]),
    "gpso_best_ucb_grow": (C.c_int, [C.c_void_p, _c_double_p, C.c_int, C.c_int, C.c_double,
                                     _c_int64_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_padded_n": (C.c_int64, [C.c_void_p]),
    "gpso_problem_shape": (C.c_int, [C.c_void_p, _c_int64_p, C.POINTER(C.c_int)]),
    "gpso_get_matrix": (C.c_int, [C.c_void_p, C.c_int, _c_double_p]),
    "gpso_get_vector": (C.c_int, [C.c_void_p, C.c_int, _c_double_p]),
    "gpso_posterior_buffers": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _c_int64_p, C.c_int]),
    "gpso_posterior_span": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _c_int64_p, _c_int64_p]),
    "gpso_posterior_span_at": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    "gpso_posterior_hash": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "gpso_alloc_posterior": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    "gpso_adopt_posterior": (C.c_int, [C.c_void_p]),
    "gpso_comm_unique_id": (C.c_int, [C.c_void_p]),
    "gpso_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gpso_comm_destroy": (C.c_int, [C.c_void_p]),
    "gpso_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gpso_shard_range": (None, [C.c_int64, C.c_int, C.c_int, _c_int64_p, _c_int64_p]),
    "gpso_broadcast_posterior": (C.c_int, [C.c_void_p, C.c_int]),
    "gpso_broadcast_posterior_rows": (C.c_int, [C.c_void_p, C.c_int]),
    "gpso_posterior_dirty_ranges": (C.c_int, [C.c_void_p, _c_int64_p, _c_int64_p, C.c_int]),
    "gpso_posterior_mark_synced": (C.c_int, [C.c_void_p]),
    "gpso_best_ucb_sharded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                        _c_int64_p, C.c_int, C.c_double, _c_int64_p, _c_double_p,
                                        _c_double_p, _c_double_p]),
    "gpso_best_ucb_grow_sharded": (C.c_int, [C.c_void_p, _c_double_p, C.c_int, C.c_int, C.c_double,
                                             _c_int64_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_comm_abort": (C.c_int, [C.c_void_p]),
    "gpso_group_payload_doubles": (C.c_int, [C.c_int]),
    "gpso_shard_winners": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64,
                                     C.c_int64, _c_int64_p, C.c_int, C.c_double, _c_double_p]),
    "gpso_shard_winners_grow": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _c_double_p, C.c_int, C.c_int,
                                          C.c_double, _c_double_p]),
    "gpso_fold_winners": (C.c_int, [C.c_void_p, _c_double_p, C.c_int, C.c_int64, _c_int64_p, C.c_int,
                                    _c_int64_p, _c_double_p, _c_double_p, _c_double_p]),
    "gpso_last_ms": (C.c_double, [C.c_void_p, C.c_int]),
    "gpso_last_count": (C.c_int64, [C.c_void_p, C.c_int]),
    "gpso_version": (C.c_char_p, []),
}

_lib = None


class GpsoHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libgpso_hip error {code}: {message}")
        self.code = code


class GpsoPrecisionError(GpsoHipError):
    """GPSO_E_PRECISION: the float predict arithmetic fails its self-test on the resident posterior
    (the message carries the measured errors).  Callers open a "mixed" or "float64" engine instead."""


def load():
    """Load libgpso_hip.so (once) and attach prototypes.  Raises if the extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C pygpso_amd/csrc`). "
            "pygpso_amd has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    # (GPSO_HIP_LIB_OLDER=1 -- tools/ab_bits.py, tools/ab_time.py comparing with an EARLIER build of the library: entry points
    # that build does not have yet are skipped instead of failing the load; never set by the product or the tests)
    older = os.environ.get("GPSO_HIP_LIB_OLDER") == "1" and "GPSO_HIP_LIB" in os.environ
    for name, (restype, argtypes) in SIGNATURES.items():
        if older and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def as_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def dptr(a):
    return a.ctypes.data_as(_c_double_p)


def i64ptr(a):
    return a.ctypes.data_as(_c_int64_p)
