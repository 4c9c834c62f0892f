"""
``HipGPEngine``: one GP posterior resident on one MI355X, driven through the C-ABI.

It plays the role the ``gpflow.models.GPR`` object plays for the reference
(``gpso/gp_surrogate.py:488-503``): it owns the training data, the hyper-parameters and the
factorisation, evaluates the training loss (+ gradient) and answers ``predict_y``.  All arithmetic
happens in the hand-written HIP kernels of ``libgpso_hip.so``; this file only marshals pointers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _producer_stream(x):
    """hipStream_t (int) on which the framework that owns the device tensor ``x`` is currently
    queueing work for x's device.  Only torch tensors are recognised -- through the module the CALLER
    has already imported; this package never imports torch itself.  None: unknown (the C-ABI then
    relies on its documented contract: device buffers must be ready before the call)."""
    import sys

    torch = sys.modules.get("torch")
    if torch is None or not isinstance(x, torch.Tensor):
        return None
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # (the pointer without a Stream object: this sits in every call)
    if raw is not None and x.device.index is not None:
        return int(raw(x.device.index))
    return int(torch.cuda.current_stream(x.device).cuda_stream)


class HipGPEngine:
    def __init__(self, dtype="float64", device=0, predict_math=None, generation=None,
                 precision_check=None, tol_var=None, tol_mean=None):
        """``dtype``: "float64" (fit and predict in double: the reference's arithmetic), "float32" (fit
        and predict apply in float) or "mixed" (fit in double, predict apply in float: the
        hyper-parameter path is bit-identical to float64).
        ``predict_math`` (float-predict engines only): "auto" (default: "bf16x6" where the posterior's
        shape allows it and its self-test passes with it, else "native"), "native" f32 MFMA, or the
        split-bf16 modes "bf16x6" (six bf16 MFMAs per f32 product, f32 accumulation: f32-class
        accuracy) / "bf16x3" (|d var| ~ 2e-5 sigma^2) on the bf16 matrix cores.
        ``generation`` (float-predict engines): "auto" (default: float when the posterior's self-test
        passes with it, else double), "float64" (r^2 of the cross-Gram tile formed in double) or
        "float32" (GPflow's GEMM form in float: faster, |d r^2| ~ 1e-5).
        ``precision_check`` / ``tol_var`` / ``tol_mean``: the self-test that guards float predictions
        (include/gpso_hip.h: gpso_precision_info); on by default for float-predict engines."""
        self._lib = L.load()
        if dtype is np.float64:
            dtype = "float64"
        elif dtype is np.float32:
            dtype = "float32"
        self.dtype_name = {L.F64: "float64", L.F32: "float32", L.MIXED: "mixed"}[L.DTYPE_IDS[dtype]]
        self.dtype = L.DTYPE_IDS[dtype]
        self.device = int(device)
        handle = C.c_void_p()
        rc = self._lib.gpso_create(C.byref(handle), self.device, self.dtype)
        if rc != L.OK:
            raise L.GpsoHipError(rc, self._lib.gpso_last_error(None).decode())
        self._h = handle
        self.n = 0
        self.d = 0
        self.rank, self.world = 0, 1
        self._u_bufs = {}
        self._win_bufs = {}
        if predict_math is not None and not (predict_math in ("native", "f32") and self.dtype == L.F64):
            self.set_predict_math(predict_math)
        if generation is not None:
            self.set_generation(generation)
        if precision_check is not None:
            self.set_precision_check(precision_check)
        if tol_var is not None or tol_mean is not None:
            self.set_tolerances(tol_var, tol_mean)

    # -- plumbing ----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpso_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            msg = self._lib.gpso_last_error(self._h).decode()
            if rc == L.E_NOTPD:
                raise np.linalg.LinAlgError(msg)
            if rc == L.E_ARG:
                raise ValueError(msg)
            if rc == L.E_PRECISION:
                raise L.GpsoPrecisionError(rc, msg)
            raise L.GpsoHipError(rc, msg)
        return rc

    def set_predict_math(self, mode):
        self._check(self._lib.gpso_set_option(self._h, L.OPT_PREDICT_MATH, L.MATH_IDS[mode]))

    def set_generation(self, mode):
        """"auto" (default) | "float64" | "float32": arithmetic of the cross-Gram x.x* contraction and r^2."""
        self._check(self._lib.gpso_set_option(self._h, L.OPT_GENERATION, L.GEN_IDS[mode]))

    def set_timing(self, on):
        """GPSO_OPT_TIMING: record the event pairs ``last_ms`` reads (default on); off saves two to four HIP calls per
        entry point -- what a loop of small evaluations wants."""
        self._check(self._lib.gpso_set_option(self._h, L.OPT_TIMING, int(on)))  # (True / 1: every call, k: every k-th)

    def set_split_kernel(self, which):
        """GPSO_OPT_SPLIT_KERNEL: "auto" (the fused step) | "two-phase" (round 3's step): same bits, different speed."""
        self._check(self._lib.gpso_set_option(self._h, L.OPT_SPLIT_KERNEL, {"auto": 0, "two-phase": 1, "fused16": 2, "fused32": 3}[which]))

    def set_contraction(self, which):
        """GPSO_OPT_CONTRACTION: "auto" / "f16" (the x.x* contraction of the fp16-split kernel on the fp16 pipe under
        float generation) | "f32" (the f32 matrix instruction, as in rounds 1-3)."""
        self._check(self._lib.gpso_set_option(self._h, L.OPT_CONTRACTION, {"auto": 0, "f32": 1, "f16": 2}[which]))

    def set_small_calls(self, on):
        """GPSO_OPT_SMALL_CALLS: the short launch sequences for best-UCB calls on small batches (default on; same bits).
        True / 1: three launches, or one where that measures faster; 2: three only; 3: one wherever it applies; 0: general."""
        self._check(self._lib.gpso_set_option(self._h, L.OPT_SMALL_CALLS, int(on)))

    def set_row_loop(self, on):
        """GPSO_OPT_ROW_LOOP (per context): 1 / True = a workgroup of the split predict kernels keeps its leaf tile and loops
        over row blocks, the launcher choosing how many workgroups share a tile (default); 0 = one row block per workgroup
        (rounds 1-5); v >= 2 = exactly min(v, row blocks) workgroups per leaf tile; -1 = exactly one, whatever the batch (a
        test aid: small batches then walk every row block in one workgroup, as C3's 65 536 leaves do).  Same bits."""
        self._check(self._lib.gpso_set_option(self._h, L.OPT_ROW_LOOP, int(on)))

    def set_park_bytes(self, nbytes):
        """GPSO_OPT_PARK_BYTES (per context): 0 = the default split predict kernel regenerates every k-step's cross-Gram pieces in
        every row block; v > 0 = a budget in bytes for parking the lowest even k-steps once per workgroup and reloading them in
        its later row blocks.  Same bits.  ``last_count(5)`` / ``last_count(6)``: k-steps per leaf tile the last launch parked /
        reloaded."""
        self._check(self._lib.gpso_set_option(self._h, L.OPT_PARK_BYTES, int(nbytes)))

    def set_screen(self, mode):
        """GPSO_OPT_SCREEN (per context): 1 = best-UCB calls of more than 16 384 float device leaves, one segment, are screened by
        a mean-only bound before the tile kernel (default); 0 = never; 2 = whatever the batch size (tests).  Same record bits.
        ``last_count(7)``: survivors of the last call; ``last_count(8)``: 0 not screened, 1 accepted, 2 refused and run again."""
        self._check(self._lib.gpso_set_option(self._h, L.OPT_SCREEN, int(mode)))

    def set_survivor_tile(self, mode):
        """GPSO_OPT_SURVIVOR_TILE (per context): 0 = the survivors' launch of a screened best-UCB call runs the narrow tile of the
        split predict kernel (4 waves x 16 leaves: 64 leaves per workgroup) up to the survivor count a makespan model gives it
        (``gpso_survivor_narrow_max_host``), the wide one above, every other launch the wide one (default); 1 = wide everywhere;
        2 = narrow wherever the default float kernels run on float leaves, ``predict`` included (tests).  Same bits.
        ``last_count(9)``: leaves per workgroup of the last split predict launch (256 or 64)."""
        self._check(self._lib.gpso_set_option(self._h, L.OPT_SURVIVOR_TILE, int(mode)))

    def screen_probe(self, xs, varsigma):
        """The mean pass and the screen of a screened best-UCB call alone (``gpso_screen_probe``) -> (my[M], ub[M], survives[M]
        bool, info): every leaf's mean -- ``predict``'s bits --, what its ucb cannot exceed, whether it survives; info =
        {"survivors", "threshold", "cap"}."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        my, ub, flag = (np.empty(m, dtype=np.float64) for _ in range(3))
        info = np.zeros(3, dtype=np.float64)
        self._check(self._lib.gpso_screen_probe(self._h, ptr, dt, mem, m, float(varsigma), L.dptr(my), L.dptr(ub), L.dptr(flag),
                                                L.dptr(info)))
        return my, ub, flag != 0.0, {"survivors": int(info[0]), "threshold": float(info[1]), "cap": int(info[2])}

    def screen_list(self):
        """The compact list the last ``screen_probe`` left for the survivors' launch (``gpso_screen_list``) -> (key[live] int64,
        rows[live, D] float32): the survivors' indices in the probed batch, ascending, and their unscaled rows; live =
        min(survivors, cap)."""
        live = np.zeros(1, dtype=np.int64)
        self._check(self._lib.gpso_screen_list(self._h, 0, None, None, live.ctypes.data_as(C.POINTER(C.c_int64))))
        n = int(live[0])
        key = np.empty(n, dtype=np.int64)
        rows = np.empty((n, self.d), dtype=np.float32)
        self._check(self._lib.gpso_screen_list(self._h, n, key.ctypes.data_as(C.POINTER(C.c_int64)),
                                               rows.ctypes.data_as(C.POINTER(C.c_float)), None))
        return key, rows

    @staticmethod
    def screen_partition_host(m, parts):
        """csrc/screen.hpp's partition of a batch of ``m`` leaves over ``parts`` workgroups of the compaction, on the CPU ->
        [(lo, hi)] * parts."""
        lib = L.load()
        lo, hi = C.c_int64(0), C.c_int64(0)
        out = []
        for w in range(int(parts)):
            rc = lib.gpso_screen_partition_host(int(m), int(parts), w, C.byref(lo), C.byref(hi))
            if rc != L.OK:
                raise L.GpsoHipError(rc, "gpso_screen_partition_host: bad arguments")
            out.append((lo.value, hi.value))
        return out

    @staticmethod
    def screen_parts_host(m):
        """How many workgroups the compaction of a batch of ``m`` leaves runs on (csrc/screen.hpp)."""
        return int(L.load().gpso_screen_parts_host(int(m)))

    @staticmethod
    def screen_eval_host(my, v, variance, noise, varsigma):
        """csrc/screen.hpp on the CPU (no context, no GPU) -> (ucb[n], ub[n]): the finalize stage's ucb of leaves with means
        ``my`` and variance shares ``v``, and the bound a screened call prunes by."""
        my = L.as_f64(np.asarray(my).reshape(-1))
        v = L.as_f64(np.asarray(v).reshape(-1), my.shape)
        ucb, ub = np.empty_like(my), np.empty_like(my)
        rc = L.load().gpso_screen_eval_host(L.dptr(my), L.dptr(v), float(variance), float(noise), float(varsigma),
                                            int(my.shape[0]), L.dptr(ucb), L.dptr(ub))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_screen_eval_host: bad arguments")
        return ucb, ub

    @staticmethod
    def screen_rules_host():
        """(threshold(max_my, noise, varsigma), survives(my, ub, threshold), accepts(u_star, threshold, count, cap)) of
        csrc/screen.hpp on the CPU."""
        lib = L.load()
        return (lambda max_my, noise, vs: float(lib.gpso_screen_threshold_host(float(max_my), float(noise), float(vs))),
                lambda my, ub, t: bool(lib.gpso_screen_survives_host(float(my), float(ub), float(t))),
                lambda u, t, count, cap: bool(lib.gpso_screen_accepts_host(float(u), float(t), int(count), int(cap))))

    def set_precision_check(self, on):
        self._check(self._lib.gpso_set_option(self._h, L.OPT_PRECISION_CHECK, 1 if on else 0))

    def set_tolerances(self, tol_var=None, tol_mean=None):
        """Self-test tolerances: |d var| <= tol_var * sigma^2, |d mean| <= tol_mean * max|y - c|."""
        if tol_var is not None:
            self._check(self._lib.gpso_set_option_f64(self._h, L.OPTF_TOL_VAR, float(tol_var)))
        if tol_mean is not None:
            self._check(self._lib.gpso_set_option_f64(self._h, L.OPTF_TOL_MEAN, float(tol_mean)))

    def precision_info(self, raise_on_fail=False):
        """Self-test of the resident posterior (runs it if needed): measured errors of the predict path
        at the training inputs against their closed form, and the tolerances they are held to."""
        out = np.zeros(12, dtype=np.float64)
        rc = self._lib.gpso_precision_info(self._h, L.dptr(out))
        if rc not in (L.OK, L.E_PRECISION) or (rc == L.E_PRECISION and raise_on_fail):
            self._check(rc)
        keys = ("max_abs_err_mean", "max_abs_err_var", "max_abs_y_minus_c", "min_var", "max_abs_alpha",
                "kernel_variance", "tol_mean_abs", "tol_var_abs", "amplification", "max_kinv_diag")
        info = dict(zip(keys, (float(v) for v in out)))
        info["generation"] = "float32" if out[10] else "float64"
        info["predict_math"] = {L.MATH_NATIVE: "native", L.MATH_BF16X3: "bf16x3", L.MATH_BF16X6: "bf16x6", L.MATH_F16X3: "f16x3"}[int(out[11])]
        info["passed"] = rc == L.OK
        return info

    def wait_stream(self, stream_ptr):
        """Order this engine's stream behind the work queued on another hipStream_t (int pointer;
        0 / None = the legacy default stream)."""
        self._check(self._lib.gpso_wait_stream(self._h, C.c_void_p(stream_ptr or None)))

    def set_fit_single_level_max(self, npad_max):
        """Tuning / test hook (GPSO_OPT_FIT_SINGLE_LEVEL_MAX): 0 forces the two-level Cholesky path."""
        self._check(self._lib.gpso_set_option(self._h, L.OPT_FIT_SINGLE_LEVEL_MAX, int(npad_max)))

    def set_stream(self, stream_ptr):
        """Run on an existing hipStream_t (int pointer, e.g. torch.cuda.Stream().cuda_stream)."""
        self._check(self._lib.gpso_set_stream(self._h, C.c_void_p(stream_ptr or None)))

    def synchronize(self):
        self._check(self._lib.gpso_synchronize(self._h))

    def last_ms(self, what=0):
        return float(self._lib.gpso_last_ms(self._h, int(what)))

    def last_count(self, what=0):
        """0: leaves the kernels scored in the last predict-type call, 1: leaves of the reference's list; 2 .. 6: see
        ``gpso_last_count`` in include/gpso_hip.h (4: bytes of device memory the contexts of this process hold now; 5 / 6:
        k-steps per leaf tile the last split predict launch parked / reloaded under GPSO_OPT_PARK_BYTES; 7 / 8: survivors and
        verdict -- 0 not screened, 1 accepted, 2 refused -- of the last best-UCB call under GPSO_OPT_SCREEN; 9: leaves per
        workgroup of the last split predict launch, 256 or 64 -- GPSO_OPT_SURVIVOR_TILE)."""
        return int(self._lib.gpso_last_count(self._h, int(what)))

    FIT_MATH = {L.FITMATH_NONE: None, L.FITMATH_SMALL: "small", L.FITMATH_F32: "f32", L.FITMATH_F64: "f64",
                L.FITMATH_BF16X6: "bf16x6", L.FITMATH_F16X3: "f16x3"}

    def fit_math(self):
        """Arithmetic the large products of the last ``fit_eval`` ran on (``gpso_last_count(ctx, 2)``, GPSO_FITMATH_*):
        "small" (N <= 128, one launch), "f32" / "f64" (the matrix instruction of the fit type), "bf16x6" / "f16x3" (the
        two-level float fit's 16-bit pieces)."""
        return self.FIT_MATH.get(self.last_count(2))

    @property
    def padded_n(self):
        return int(self._lib.gpso_padded_n(self._h))

    # -- fit ---------------------------------------------------------------------------------
    def set_data(self, X, y):
        X = L.as_f64(X)
        if X.ndim != 2:
            raise ValueError("X must be [N, D]")
        y = L.as_f64(np.asarray(y).reshape(-1), (X.shape[0],))
        self._check(self._lib.gpso_set_data(self._h, L.dptr(X), L.dptr(y), X.shape[0], X.shape[1]))
        self.n, self.d = X.shape

    def set_noise_diag(self, s):
        """``gpso_set_noise_diag``: the known variance s [N] >= 0 of each resident observation (None clears it).  Later fits
        factorise K + diag(noise + s); predictions add the shared noise only.  ``set_data`` clears it; a resident posterior
        is invalidated."""
        if s is None:
            self._check(self._lib.gpso_set_noise_diag(self._h, None, self.n))
            return
        sa = L.as_f64(np.asarray(s).reshape(-1))
        self._check(self._lib.gpso_set_noise_diag(self._h, L.dptr(sa), sa.shape[0]))

    @staticmethod
    def _theta_args(kernel, lengthscales, variance, noise, mean_c):
        kid = L.KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
        ls = L.as_f64(np.atleast_1d(lengthscales))
        return kid, ls, int(ls.shape[0]), float(variance), float(noise), float(mean_c)

    @staticmethod
    def _u_args(kernel, u, n_ls, train_mean, mean_c_fixed, grad=False, theta=False):
        """What every entry point in the optimiser's variables takes: -> (kernel id, u, n_ls, train_mean, mean_c_fixed) as the
        C call wants them, then the ``grad_u`` and ``theta`` output arrays (None where not asked for)."""
        kid = L.KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
        ua = L.as_f64(np.asarray(u).reshape(-1))  # (the returned pointer keeps it alive: ctypes' data_as holds its array)
        ga = np.empty(int(n_ls) + 2 + (1 if train_mean else 0), dtype=np.float64) if grad else None
        ta = np.empty(int(n_ls) + 3, dtype=np.float64) if theta else None
        return (kid, L.dptr(ua), int(n_ls), 1 if train_mean else 0, float(mean_c_fixed)), ga, ta

    def _u_cached(self, fn, kernel, u, n_ls, train_mean, mean_c_fixed, n_loss):
        """``fit_eval_u`` / ``fit_eval_loo_u``: the optimiser's inner loop, so the marshalling buffers are made once per
        entry point and problem shape.  -> the ``n_loss`` scalars the call returns, grad_u, theta."""
        kid = L.KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
        key = (n_loss, int(n_ls), bool(train_mean))  # (n_u alone is ambiguous: theta_out has n_ls + 3 entries whatever train_mean)
        buf = self._u_bufs.get(key)
        if buf is None:
            ua, ga = (np.empty(int(n_ls) + 2 + (1 if train_mean else 0), dtype=np.float64) for _ in range(2))
            ta = np.empty(int(n_ls) + 3, dtype=np.float64)
            out = [C.c_double() for _ in range(n_loss)]
            # (the C argument lists: ..., loss, grad_u, theta and then any further scalar)
            tail = (C.byref(out[0]), L.dptr(ga), L.dptr(ta)) + tuple(C.byref(o) for o in out[1:])
            buf = self._u_bufs[key] = (ua, ga, ta, out, L.dptr(ua), tail)
        ua, ga, ta, out, up, tail = buf
        ua[:] = u
        rc = fn(self._h, kid, up, int(n_ls), 1 if train_mean else 0, float(mean_c_fixed), *tail)
        if rc < 0:
            self._check(rc)
        return [o.value for o in out], ga.copy(), ta.copy()

    def _eval_u(self, fn, kernel, u, n_ls, train_mean, mean_c_fixed, want_grad):
        """A family's loss at fixed q (and Z) in ``u``: -> (loss, grad_u or None, theta)."""
        args, ga, ta = self._u_args(kernel, u, n_ls, train_mean, mean_c_fixed, grad=want_grad, theta=True)
        loss = C.c_double()
        self._check(fn(self._h, *args, C.byref(loss), L.dptr(ga) if want_grad else None, L.dptr(ta)))
        return loss.value, ga, ta

    def fit_eval(self, kernel, lengthscales, variance, noise, mean_c, want_grad=True):
        """One NLML (+ gradient w.r.t. the constrained hyper-parameters) evaluation; leaves the
        posterior resident.  Returns (nlml, grad or None); grad order (ls..., variance, noise, c)."""
        kid, ls, n_ls, var, nz, mc = self._theta_args(kernel, lengthscales, variance, noise, mean_c)
        nlml = C.c_double()
        grad = np.empty(n_ls + 3, dtype=np.float64) if want_grad else None
        self._check(self._lib.gpso_fit_eval(self._h, kid, L.dptr(ls), n_ls, var, nz, mc,
                                            C.byref(nlml), L.dptr(grad) if want_grad else None))
        return nlml.value, grad

    def fit_eval_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        """One loss evaluation in the optimiser's unconstrained variables (``gpso_fit_eval_u``: transforms and chain
        rule inside the library).  Returns (nlml, grad_u, theta): theta = constrained (ls..., variance, noise, mean)."""
        (nlml,), grad_u, theta = self._u_cached(self._lib.gpso_fit_eval_u, kernel, u, n_ls, train_mean, mean_c_fixed, 1)
        return nlml, grad_u, theta

    # -- leave-one-out (include/gpso_hip.h: gpso_loo, gpso_fit_eval_loo*; no counterpart in the reference) -----------------
    def loo(self):
        """``gpso_loo``: the leave-one-out predictive of the resident fitted posterior at its hyper-parameters.  Returns
        (mean [N], var [N], lpd [N], loss): what N refits without point i predict for y_i (its own noise included), the log
        predictive density of each y_i and loss = -sum lpd.  Reads only; GpsoHipError (GPSO_E_STATE) without a posterior
        fitted with targets on this engine."""
        n = C.c_int64()
        d = C.c_int()
        self._check(self._lib.gpso_problem_shape(self._h, C.byref(n), C.byref(d)))
        mean, var, lpd = (np.empty(max(int(n.value), 1), dtype=np.float64) for _ in range(3))
        loss = C.c_double()
        self._check(self._lib.gpso_loo(self._h, L.dptr(mean), L.dptr(var), L.dptr(lpd), C.byref(loss)))
        return mean, var, lpd, loss.value

    def fit_eval_loo(self, kernel, lengthscales, variance, noise, mean_c, want_grad=True):
        """One evaluation of the LOO-CV loss (-sum of the leave-one-out log predictive densities) and its gradient
        (``gpso_fit_eval_loo``); leaves the posterior resident exactly as ``fit_eval`` does.  Returns (loss, grad or None,
        nlml): grad order (ls..., variance, noise, c); nlml is the NLML at the same theta.  "float64" / "mixed" engines."""
        kid, ls, n_ls, var, nz, mc = self._theta_args(kernel, lengthscales, variance, noise, mean_c)
        loss, nlml = C.c_double(), C.c_double()
        grad = np.empty(n_ls + 3, dtype=np.float64) if want_grad else None
        self._check(self._lib.gpso_fit_eval_loo(self._h, kid, L.dptr(ls), n_ls, var, nz, mc, C.byref(loss),
                                                L.dptr(grad) if want_grad else None, C.byref(nlml)))
        return loss.value, grad, nlml.value

    def fit_eval_loo_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        """``fit_eval_u`` for the LOO-CV loss (``gpso_fit_eval_loo_u``).  Returns (loss, grad_u, theta, nlml)."""
        (loss, nlml), grad_u, theta = self._u_cached(self._lib.gpso_fit_eval_loo_u, kernel, u, n_ls, train_mean, mean_c_fixed, 2)
        return loss, grad_u, theta, nlml

    def fit_batch_max(self):
        """Entries one ``gpso_fit_eval_u_batch`` call may hold for the resident data (256 where the one-launch fit applies,
        0 otherwise: N > 128, or N > 64 with a padded D > 32)."""
        return int(self._lib.gpso_fit_batch_max(self._h))

    def fit_eval_u_batch(self, kernel, U, n_ls, train_mean, mean_c_fixed=0.0):
        """``fit_eval_u`` at every row of ``U [B, nu]``: the pending evaluations of a multi-start hyper-parameter search.
        Where the one-launch fit applies they run as launches of up to 256 workgroups, one per row
        (``gpso_fit_eval_u_batch``), bit-identical to the single calls, and the resident posterior is left alone.
        Elsewhere (``fit_batch_max() == 0``) the rows go through ``fit_eval_u`` one after another: correct, no faster, and
        -- as any fit -- the resident posterior is replaced.  Returns (loss [B], grad [B, nu], ok [B]); a row whose matrix
        is not positive definite (or whose theta the library refuses) has ok False and NaN loss and gradient."""
        kid = L.KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
        nu = int(n_ls) + 2 + (1 if train_mean else 0)
        U = L.as_f64(np.atleast_2d(U))
        if U.ndim != 2 or U.shape[1] != nu:
            raise ValueError(f"U must be [B, {nu}]")
        B = U.shape[0]
        loss = np.full(B, np.nan)
        grad = np.full((B, nu), np.nan)
        ok = np.zeros(B, dtype=bool)
        cap = self.fit_batch_max()
        if cap < 0:
            self._check(cap)
        if cap == 0:
            for b in range(B):
                try:
                    loss[b], grad[b], _ = self.fit_eval_u(kid, U[b], n_ls, train_mean, mean_c_fixed)
                    ok[b] = True
                except (np.linalg.LinAlgError, ValueError):
                    pass
            return loss, grad, ok
        for lo in range(0, B, cap):
            hi = min(B, lo + cap)
            u = np.ascontiguousarray(U[lo:hi])
            f = np.empty(hi - lo, dtype=np.float64)
            g = np.empty((hi - lo, nu), dtype=np.float64)
            st = np.empty(hi - lo, dtype=np.intc)
            self._check(self._lib.gpso_fit_eval_u_batch(self._h, kid, L.dptr(u), hi - lo, int(n_ls), 1 if train_mean else 0,
                                                        float(mean_c_fixed), L.dptr(f), L.dptr(g),
                                                        st.ctypes.data_as(C.POINTER(C.c_int)), None))
            loss[lo:hi], grad[lo:hi], ok[lo:hi] = f, g, st == L.OK
        return loss, grad, ok

    def append(self, Xnew, ynew, s=None):
        """``gpso_append``: k new training points extend the resident posterior at its hyper-parameters (two passes over
        L^-1 instead of a factorisation).  Returns (nlml of the N + k points, in_place): ``in_place`` False when the
        library refitted from scratch instead (pad crossing, k > 64, N + k <= 128: ``last_message()`` says which).
        ``s`` [k] (``gpso_append_noise``): the new points' per-point noise; None appends zeros."""
        Xn = L.as_f64(np.atleast_2d(Xnew))
        if Xn.ndim != 2 or Xn.shape[1] != self.d:
            raise ValueError(f"Xnew must be [k, {self.d}]")
        yn = L.as_f64(np.asarray(ynew).reshape(-1), (Xn.shape[0],))
        nlml = C.c_double()
        sn = None if s is None else L.as_f64(np.asarray(s).reshape(-1), (Xn.shape[0],))
        try:
            if sn is None:
                rc = self._check(self._lib.gpso_append(self._h, L.dptr(Xn), L.dptr(yn), Xn.shape[0], C.byref(nlml)))
            else:
                rc = self._check(self._lib.gpso_append_noise(self._h, L.dptr(Xn), L.dptr(yn), L.dptr(sn), Xn.shape[0],
                                                             C.byref(nlml)))
        finally:
            # whatever happened, N is what the library says it holds (a failed append leaves the first N points, in place
            # or refitted: include/gpso_hip.h)
            n, d = C.c_int64(), C.c_int()
            if self._lib.gpso_problem_shape(self._h, C.byref(n), C.byref(d)) == L.OK:
                self.n = int(n.value)
        return nlml.value, rc == L.OK

    def last_message(self):
        return self._lib.gpso_last_error(self._h).decode()

    # -- variational GP (include/gpso_hip.h: gpso_vgp_*) ---------------------------------------------------------------
    def vgp_set_likelihood(self, kind="Gaussian", df=3.0, n_gh=20):
        """The VGP's likelihood: "Gaussian" (closed form, the default), "StudentT" (``df`` > 2, slot n_ls + 1 of u: the
        scale), "GaussianGH" (the Gaussian through the quadrature sequence) or "Bernoulli" (exact probit link; the targets
        are labels, success iff y > 0.5; slot n_ls + 1 of u is read by nothing), with the ``n_gh``-point Gauss-Hermite rule
        of ``numpy.polynomial.hermite.hermgauss`` (GPflow's)."""
        kid = L.LIKELIHOOD_IDS[kind] if isinstance(kind, str) else int(kind)
        x, w = np.polynomial.hermite.hermgauss(int(n_gh))
        x, w = L.as_f64(x), L.as_f64(w)
        if kid == L.LIK_BERNOULLI:
            df = 0.0  # (the kind has no df: the library takes 0 and refuses anything else)
        self._check(self._lib.gpso_vgp_set_likelihood(self._h, kid, float(df), int(n_gh), L.dptr(x), L.dptr(w)))

    def vgp_set_q(self, mu=None, S=None):
        """q(v) = N(mu, S S^T) for the resident data; None, None: the prior (mu = 0, S = I)."""
        if mu is None and S is None:
            self._check(self._lib.gpso_vgp_set_q(self._h, None, None, self.n))
            return
        m = L.as_f64(np.asarray(mu).reshape(-1), (self.n,))
        Sa = L.as_f64(S, (self.n, self.n))
        self._check(self._lib.gpso_vgp_set_q(self._h, L.dptr(m), L.dptr(Sa), self.n))

    def vgp_extend_q(self):
        """After ``set_data`` with the rows q was made for first, in the same order: q keeps its leading block and the
        new rows get the prior (on the device)."""
        self._check(self._lib.gpso_vgp_extend_q(self._h))

    def vgp_get_q(self):
        """(mu [N], S [N, N]) of the variational state on the device."""
        m = np.empty(self.n, dtype=np.float64)
        Sa = np.empty((self.n, self.n), dtype=np.float64)
        self._check(self._lib.gpso_vgp_get_q(self._h, L.dptr(m), L.dptr(Sa)))
        return m, Sa

    def vgp_natgrad(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, gamma=1.0):
        """One natural-gradient step of length ``gamma`` on q at the theta of ``u``."""
        args, _, _ = self._u_args(kernel, u, n_ls, train_mean, mean_c_fixed)
        self._check(self._lib.gpso_vgp_natgrad(self._h, *args, float(gamma)))

    def vgp_elbo_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, want_grad=True):
        """-ELBO at fixed q and its gradient in ``u``.  Returns (loss, grad_u or None, theta)."""
        return self._eval_u(self._lib.gpso_vgp_elbo_u, kernel, u, n_ls, train_mean, mean_c_fixed, want_grad)

    def vgp_posterior(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        """Install the VGP predictive at the theta of ``u`` as the resident posterior."""
        args, _, _ = self._u_args(kernel, u, n_ls, train_mean, mean_c_fixed)
        self._check(self._lib.gpso_vgp_posterior(self._h, *args))

    # -- sparse GP regression on inducing points (include/gpso_hip.h: gpso_sgpr_*) ----------------
    def sgpr_set_inducing(self, Z):
        """Z [M, D] summarises the resident training data; afterwards the engine's resident rows are Z (``n`` = M)."""
        Z = L.as_f64(Z)
        if Z.ndim != 2 or Z.shape[1] != self.d:
            raise ValueError(f"Z must be [M, {self.d}]")
        self._check(self._lib.gpso_sgpr_set_inducing(self._h, L.dptr(Z), Z.shape[0]))
        self.n = int(Z.shape[0])

    def sgpr_select_inducing(self, kernel, u, n_ls, m):
        """Greedy conditional-variance selection of ``m`` training rows on the device at the kernel hyper-parameters of
        ``u``; they become Z.  Returns their indices in pick order."""
        (kid, up, n_ls, _, _), _, _ = self._u_args(kernel, u, n_ls, False, 0.0)
        idx = np.empty(int(m), dtype=np.int64)
        self._check(self._lib.gpso_sgpr_select_inducing(self._h, kid, up, n_ls, int(m), L.i64ptr(idx)))
        self.n = int(m)
        return idx

    def sgpr_get_inducing(self):
        """(Z [M, D], N of the training data held beside it)."""
        m, n = C.c_int64(), C.c_int64()
        self._check(self._lib.gpso_sgpr_get_inducing(self._h, None, C.byref(m), C.byref(n)))
        Z = np.empty((m.value, self.d), dtype=np.float64)
        self._check(self._lib.gpso_sgpr_get_inducing(self._h, L.dptr(Z), None, None))
        return Z, int(n.value)

    def sgpr_get_factor(self, which):
        """An intermediate of the last ``sgpr_bound_u``: "Kuf" [M, N], "Lu" [M, M], "LB" [M, M] or "cv" [M] (for checks)."""
        ids = {"Kuf": L.SGPR_KUF, "Lu": L.SGPR_LU, "LB": L.SGPR_LB, "cv": L.SGPR_CV}
        if which == "Kuf":
            n = C.c_int64()
            self._check(self._lib.gpso_sgpr_get_inducing(self._h, None, None, C.byref(n)))
            out = np.empty((self.n, n.value), dtype=np.float64)
        else:
            out = np.empty(self.n if which == "cv" else (self.n, self.n), dtype=np.float64)
        self._check(self._lib.gpso_sgpr_get_factor(self._h, ids[which], L.dptr(out)))
        return out

    def sgpr_bound_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, want_grad=True):
        """-bound (Titsias) and its gradient in ``u``, Z fixed.  Returns (loss, grad_u or None, theta)."""
        return self._eval_u(self._lib.gpso_sgpr_bound_u, kernel, u, n_ls, train_mean, mean_c_fixed, want_grad)

    def sgpr_posterior(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        """Install the SGPR predictive at the theta of ``u`` over the rows Z.  Returns the shift delta (0: exact)."""
        args, _, _ = self._u_args(kernel, u, n_ls, train_mean, mean_c_fixed)
        delta = C.c_double()
        self._check(self._lib.gpso_sgpr_posterior(self._h, *args, C.byref(delta)))
        return delta.value

    # -- sparse variational GP on inducing points (include/gpso_hip.h: gpso_svgp_*; Z from sgpr_set / select_inducing) -----
    def svgp_init_q(self, kernel=None, u=None, n_ls=1, train_mean=False, mean_c_fixed=0.0, noise_variance=0.0):
        """Start q: the prior (``noise_variance`` <= 0), or one Gaussian natural-gradient step of length 1 at that noise
        variance and the theta of ``u`` (the conjugate start)."""
        if not noise_variance > 0.0:
            self._check(self._lib.gpso_svgp_init_q(self._h, 0, None, 0, 0, 0.0, 0.0))
            return
        args, _, _ = self._u_args(kernel, u, n_ls, train_mean, mean_c_fixed)
        self._check(self._lib.gpso_svgp_init_q(self._h, *args, float(noise_variance)))

    def svgp_set_q(self, mu=None, S=None):
        """q(v) = N(mu, S S^T) over the M inducing values; None, None: the prior."""
        if mu is None and S is None:
            self._check(self._lib.gpso_svgp_set_q(self._h, None, None, self.n))
            return
        m = L.as_f64(np.asarray(mu).reshape(-1), (self.n,))
        Sa = L.as_f64(np.asarray(S).reshape(self.n, self.n), (self.n, self.n))
        self._check(self._lib.gpso_svgp_set_q(self._h, L.dptr(m), L.dptr(Sa), self.n))

    def svgp_get_q(self):
        """(mu [M], S [M, M]) of the SVGP's variational state on the device."""
        m = np.empty(self.n, dtype=np.float64)
        Sa = np.empty((self.n, self.n), dtype=np.float64)
        self._check(self._lib.gpso_svgp_get_q(self._h, L.dptr(m), L.dptr(Sa)))
        return m, Sa

    def svgp_natgrad(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, gamma=1.0):
        """One natural-gradient step of length ``gamma`` on the SVGP's q at the theta of ``u``."""
        args, _, _ = self._u_args(kernel, u, n_ls, train_mean, mean_c_fixed)
        self._check(self._lib.gpso_svgp_natgrad(self._h, *args, float(gamma)))

    def svgp_elbo_u(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, want_grad=True):
        """-ELBO of the SVGP at fixed q and Z and its gradient in ``u``.  Returns (loss, grad_u or None, theta)."""
        return self._eval_u(self._lib.gpso_svgp_elbo_u, kernel, u, n_ls, train_mean, mean_c_fixed, want_grad)

    def svgp_posterior(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0):
        """Install the SVGP predictive at the theta of ``u`` over the rows Z.  Returns the shift delta (0: exact)."""
        args, _, _ = self._u_args(kernel, u, n_ls, train_mean, mean_c_fixed)
        delta = C.c_double()
        self._check(self._lib.gpso_svgp_posterior(self._h, *args, C.byref(delta)))
        return delta.value

    # -- the sparse models at a moving Z (include/gpso_hip.h: gpso_sgpr_move_inducing, gpso_sgpr_bound_uz, gpso_svgp_elbo_uz) --
    def _z_arg(self, Z):
        if Z is None:
            return None
        Z = L.as_f64(np.asarray(Z).reshape(-1, self.d))
        if Z.shape[0] != self.n:
            raise ValueError(f"Z must be [{self.n}, {self.d}]: the resident inducing rows are replaced in place")
        return Z

    def sgpr_move_inducing(self, Z):
        """Replace the resident inducing rows by Z [M, D] in place (same M; the data, and the SVGP's q, stay)."""
        Z = self._z_arg(Z)
        self._check(self._lib.gpso_sgpr_move_inducing(self._h, L.dptr(Z) if Z is not None else None))

    def _eval_uz(self, fn, kernel, u, n_ls, train_mean, mean_c_fixed, Z, want_grad):
        args, ga, ta = self._u_args(kernel, u, n_ls, train_mean, mean_c_fixed, grad=want_grad, theta=True)
        Z = self._z_arg(Z)
        gz = np.empty((self.n, self.d), dtype=np.float64) if want_grad else None
        loss = C.c_double()
        self._check(fn(self._h, *args, L.dptr(Z) if Z is not None else None, C.byref(loss), L.dptr(ga) if want_grad else None,
                       L.dptr(gz) if want_grad else None, L.dptr(ta)))
        return loss.value, ga, gz, ta

    def sgpr_bound_uz(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, Z=None, want_grad=True):
        """-bound at the inducing points Z [M, D] (None: the resident ones), which replace the resident rows in place,
        and its gradient in ``u`` and in Z.  Returns (loss, grad_u or None, grad_z [M, D] or None, theta)."""
        return self._eval_uz(self._lib.gpso_sgpr_bound_uz, kernel, u, n_ls, train_mean, mean_c_fixed, Z, want_grad)

    def svgp_elbo_uz(self, kernel, u, n_ls, train_mean, mean_c_fixed=0.0, Z=None, want_grad=True):
        """-ELBO at fixed q and the inducing points Z [M, D] (None: the resident ones; q is kept), and its gradient in
        ``u`` and in Z.  Returns (loss, grad_u or None, grad_z [M, D] or None, theta)."""
        return self._eval_uz(self._lib.gpso_svgp_elbo_uz, kernel, u, n_ls, train_mean, mean_c_fixed, Z, want_grad)

    def set_posterior(self, X, Lchol, alpha, kernel, lengthscales, variance, noise, mean_c):
        X = L.as_f64(X)
        n, d = X.shape
        Lc = L.as_f64(Lchol, (n, n))
        al = L.as_f64(np.asarray(alpha).reshape(-1), (n,))
        kid, ls, n_ls, var, nz, mc = self._theta_args(kernel, lengthscales, variance, noise, mean_c)
        self._check(self._lib.gpso_set_posterior(self._h, L.dptr(X), L.dptr(Lc), L.dptr(al), n, d,
                                                 kid, L.dptr(ls), n_ls, var, nz, mc))
        self.n, self.d = n, d

    # -- predict -----------------------------------------------------------------------------
    def _winner_bufs(self, nseg):
        """Output arrays of a best-UCB call and their ctypes pointers, made once per segment count: these calls are the
        optimiser's inner loop (the arrays are copied out, so callers may keep what they get)."""
        bufs = self._win_bufs.get(nseg)
        if bufs is None:
            idx = np.empty(nseg, dtype=np.int64)
            mean = np.empty(nseg, dtype=np.float64)
            var = np.empty(nseg, dtype=np.float64)
            ucb = np.empty(nseg, dtype=np.float64)
            bufs = self._win_bufs[nseg] = (idx, mean, var, ucb, L.i64ptr(idx), L.dptr(mean), L.dptr(var), L.dptr(ucb))
        return bufs

    def _leaf_args(self, xs):
        """-> (pointer, xs_dtype, xs_mem, M, keepalive)"""
        if _is_device_tensor(xs):
            if xs.dim() != 2 or not xs.is_contiguous():
                raise ValueError("device leaves must be a contiguous [M, D] tensor")
            name = str(xs.dtype)
            if name.endswith("float64"):
                dt = L.F64
            elif name.endswith("float32"):
                dt = L.F32
            else:
                raise ValueError(f"unsupported leaf dtype {xs.dtype}")
            if self.d and xs.shape[1] != self.d:
                raise ValueError(f"leaves have D={xs.shape[1]}, model has D={self.d}")
            self._order_after(xs)
            return C.c_void_p(xs.data_ptr()), dt, L.MEM_DEVICE, int(xs.shape[0]), xs
        a = np.asarray(xs)
        if a.ndim != 2:
            raise ValueError("leaves must be [M, D]")
        if self.d and a.shape[0] and a.shape[1] != self.d:
            raise ValueError(f"leaves have D={a.shape[1]}, model has D={self.d}")
        if a.dtype == np.float32:
            a = np.ascontiguousarray(a)
            dt = L.F32
        else:
            a = np.ascontiguousarray(a, dtype=np.float64)
            dt = L.F64
        return C.c_void_p(a.ctypes.data), dt, L.MEM_HOST, int(a.shape[0]), a

    def _order_after(self, tensor):
        """The engine runs on its own stream: queue it behind whatever the tensor's framework has
        pending on its current stream (reads of leaves still being written / writes into outputs still
        being read would otherwise race)."""
        ps = _producer_stream(tensor)
        if ps is not None:
            self.wait_stream(ps)

    def predict(self, xs, out=None):
        """predict_y: (mean[M], var[M]) float64; var includes the noise variance.  ``out`` may be a
        pair of float64 CUDA tensors of length M to keep the results on the device."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        if out is not None:
            mean_t, var_t = out
            self._order_after(mean_t)
            self._order_after(var_t)
            self._check(self._lib.gpso_predict(self._h, ptr, dt, mem, m, C.c_void_p(mean_t.data_ptr()),
                                               C.c_void_p(var_t.data_ptr()), L.MEM_DEVICE))
            return mean_t, var_t
        mean = np.empty(m, dtype=np.float64)
        var = np.empty(m, dtype=np.float64)
        self._check(self._lib.gpso_predict(self._h, ptr, dt, mem, m, C.c_void_p(mean.ctypes.data),
                                           C.c_void_p(var.ctypes.data), L.MEM_HOST))
        return mean, var

    def predict_grad(self, xs, out=None):
        """predict_y and its gradients in the test points: (mean[M], var[M], dmean[M, D], dvar[M, D]) float64, var with
        the noise variance, gradients in the coordinates as passed.  float64 and mixed engines (the dense factor in
        double); any resident posterior but an adopted one.  ``out`` may be four float64 CUDA tensors of those shapes to
        keep the results on the device; an entry may be None for an output that is not wanted (not all four)."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        if out is not None:
            if len(out) != 4:
                raise ValueError("out must hold four entries: mean, var, dmean, dvar (tensors or None)")
            for t in out:
                if t is not None:
                    self._order_after(t)
            self._check(self._lib.gpso_predict_grad(self._h, ptr, dt, mem, m,
                                                    *[None if t is None else C.c_void_p(t.data_ptr()) for t in out], L.MEM_DEVICE))
            return tuple(out)
        d = int(keep.shape[1])
        mean, var = np.empty(m, dtype=np.float64), np.empty(m, dtype=np.float64)
        dmean, dvar = np.empty((m, d), dtype=np.float64), np.empty((m, d), dtype=np.float64)
        self._check(self._lib.gpso_predict_grad(self._h, ptr, dt, mem, m, *[C.c_void_p(a.ctypes.data) for a in (mean, var, dmean, dvar)],
                                                L.MEM_HOST))
        return mean, var, dmean, dvar

    def predict_joint(self, xs, diag_add=0.0, out=None):
        """The joint predictive at the M <= 1024 rows of ``xs``: (mean [M], cov [M, M]) float64, cov = K** - V^T V +
        diag_add I, exactly symmetric (``gpso_predict_joint``; GPflow's ``predict_f(full_cov=True)``).  ``diag_add``: 0 for
        the latent f, the predictive noise for y.  float64 and mixed engines; any resident posterior but an adopted one.
        ``out`` may be a pair (mean [M] or None, cov [M, M]) of contiguous float64 CUDA tensors to keep the results on the
        device."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        if out is not None:
            mean_t, cov_t = out
            if cov_t is None or tuple(cov_t.shape) != (m, m) or not cov_t.is_contiguous():
                raise ValueError(f"out[1] must be a contiguous [{m}, {m}] tensor")
            for t in out:
                if t is not None:
                    self._order_after(t)
            self._check(self._lib.gpso_predict_joint(self._h, ptr, dt, mem, m, float(diag_add),
                                                     None if mean_t is None else C.c_void_p(mean_t.data_ptr()),
                                                     C.c_void_p(cov_t.data_ptr()), L.MEM_DEVICE))
            return mean_t, cov_t
        mean, cov = np.empty(m, dtype=np.float64), np.empty((m, m), dtype=np.float64)
        self._check(self._lib.gpso_predict_joint(self._h, ptr, dt, mem, m, float(diag_add), C.c_void_p(mean.ctypes.data),
                                                 C.c_void_p(cov.ctypes.data), L.MEM_HOST))
        return mean, cov

    def sample_joint(self, xs, z, diag_add, want_samples=True):
        """S draws of the joint predictive at the M <= 1024 rows of ``xs`` from the standard normals ``z`` [S, M]:
        mean + chol(cov + diag_add I) z per draw (``gpso_sample_joint``; GPflow's ``predict_f_samples``).  Returns
        (samples [S, M] or None, best_idx [S], best_val [S]): the draws, and per draw the index (the lowest on ties) and
        the value of its highest entry.  ``want_samples=False`` leaves the draws on the device.  A cov + diag_add I that is
        not positive definite raises ``numpy.linalg.LinAlgError``: pass a larger ``diag_add`` (jitter)."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        z = np.ascontiguousarray(z, dtype=np.float64)
        if z.ndim != 2 or z.shape[1] != m:
            raise ValueError(f"z must be [S, M] with M={m}, got {z.shape}")
        s = int(z.shape[0])
        samples = np.empty((s, m), dtype=np.float64) if want_samples else None
        best_idx, best_val = np.empty(s, dtype=np.int64), np.empty(s, dtype=np.float64)
        self._check(self._lib.gpso_sample_joint(self._h, ptr, dt, mem, m, float(diag_add), L.dptr(z), s,
                                                None if samples is None else L.dptr(samples), L.i64ptr(best_idx),
                                                L.dptr(best_val)))
        return samples, best_idx, best_val

    def paths_draw(self, omega, phase, w, eps=None):
        """Draw S posterior functions of the resident fitted exact GP and keep them on the context (``gpso_paths_draw``):
        ``omega`` [F, D] frequencies in scaled coordinates, ``phase`` [F], ``w`` [S, F] feature weights, ``eps`` [S, N]
        standard normals of the observation noise (None: zeros).  ``pygpso_amd.paths`` draws them from a seed.  The set
        lives until the posterior changes; ``paths_eval`` evaluates it."""
        self._paths_draw(self._lib.gpso_paths_draw, omega, phase, w, eps)

    def paths_draw_q(self, omega, phase, w, eps=None):
        """``paths_draw`` for the variational posterior that ``vgp_posterior`` / ``sgpr_posterior`` / ``svgp_posterior``
        installed (``gpso_paths_draw_q``): ``eps`` [S, n] are the whitened normals over the n RESIDENT rows -- the
        training rows of a VGP, the M inducing points of the sparse two."""
        self._paths_draw(self._lib.gpso_paths_draw_q, omega, phase, w, eps)

    def _paths_draw(self, entry, omega, phase, w, eps):
        omega = L.as_f64(omega)
        if omega.ndim != 2 or (self.d and omega.shape[1] != self.d):
            raise ValueError(f"omega must be [F, D] with D={self.d}, got {omega.shape}")
        f = int(omega.shape[0])
        phase = L.as_f64(np.asarray(phase).reshape(-1))
        w = L.as_f64(w)
        if phase.shape != (f,) or w.ndim != 2 or w.shape[1] != f:
            raise ValueError(f"phase must be [F] and w [S, F] with F={f}, got {phase.shape} and {w.shape}")
        s = int(w.shape[0])
        if eps is not None:
            eps = L.as_f64(eps)
            if eps.shape != (s, self.n):
                raise ValueError(f"eps must be [S, N] = [{s}, {self.n}], got {eps.shape}")
        self._check(entry(self._h, L.dptr(omega), L.dptr(phase), f, L.dptr(w), None if eps is None else L.dptr(eps), s))

    def paths_info(self):
        """(S, F) of the valid path set, (0, 0) when none is resident."""
        s, f = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        self._check(self._lib.gpso_paths_info(self._h, L.i64ptr(s), L.i64ptr(f)))
        return int(s[0]), int(f[0])

    def paths_eval(self, xs, seg_off=None, want_values=True, out=None):
        """Evaluate the resident path set at the M rows of ``xs`` (``gpso_paths_eval``; any M).  Returns (values [S, M] or
        None, best_idx [S, nseg], best_val [S, nseg]): per draw and segment the index relative to the segment start (the
        lowest on ties) and the value of its highest entry.  ``want_values=False`` leaves the values on the device;
        ``out``: a contiguous float64 CUDA tensor [S, M] that receives them instead of a host array."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        s, _ = self.paths_info()
        if seg_off is None:
            nseg, so_ptr = 1, None
        else:
            so = np.ascontiguousarray(seg_off, dtype=np.int64)
            nseg, so_ptr = int(so.shape[0] - 1), L.i64ptr(so)
        rows = max(s, 1)
        best_idx, best_val = np.empty((rows, nseg), dtype=np.int64), np.empty((rows, nseg), dtype=np.float64)
        if out is not None:
            if tuple(out.shape) != (s, m) or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous [{s}, {m}] tensor")
            self._order_after(out)
            values, vptr, vmem = out, C.c_void_p(out.data_ptr()), L.MEM_DEVICE
        elif want_values:
            values = np.empty((rows, m), dtype=np.float64)
            vptr, vmem = C.c_void_p(values.ctypes.data), L.MEM_HOST
        else:
            values, vptr, vmem = None, None, L.MEM_HOST
        self._check(self._lib.gpso_paths_eval(self._h, ptr, dt, mem, m, so_ptr, nseg, vptr, vmem, L.i64ptr(best_idx),
                                              L.dptr(best_val)))
        return values, best_idx, best_val

    # -- Monte-Carlo batch acquisition over the path draws (csrc/mcbatch.hip, csrc/mcbatch.hpp) ------------------------
    @staticmethod
    def _mc_rec(kind, xi, incumbent, incumbent_s):
        if kind not in L.MC_KINDS:
            raise ValueError(f"kind={kind!r}: one of {sorted(L.MC_KINDS)}")
        if incumbent_s is None and incumbent is None:
            raise ValueError("one of incumbent and incumbent_s is needed")
        bars = None if incumbent_s is None else L.as_f64(np.asarray(incumbent_s, dtype=np.float64).reshape(-1))
        return L.GpsoMcAcq(L.MC_KINDS[kind], float(xi), 0.0 if incumbent is None else float(incumbent)), bars

    def paths_best_batch(self, xs, q, kind="qei", incumbent=None, incumbent_s=None, pending=None, xi=0.0, want_gain0=False):
        """``q`` rows of ``xs`` picked greedily by the sample-average batch acquisition over the resident path set
        (``gpso_paths_best_batch``): ``kind`` "qei" (or "qnei", the same arithmetic -- pass the per-draw bars) or "qpi".
        The bars: ``incumbent_s`` [S], or the scalar ``incumbent`` for every draw.  ``pending`` [B, D], B <= 64: points
        still being evaluated, folded into the bars and never returned.  Returns (idx, gain, batch_value) of the picks
        made -- at most ``q`` -- and with ``want_gain0`` every row's round-0 gain [M] as a fourth entry.  The values
        never leave the device."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        rec, bars = self._mc_rec(kind, xi, incumbent, incumbent_s)
        s, _ = self.paths_info()
        if bars is not None and s and bars.shape != (s,):
            raise ValueError(f"incumbent_s must be [S] with S={s}, got {bars.shape}")
        if pending is None:
            pend, b = None, 0
        else:
            pend = L.as_f64(np.atleast_2d(np.asarray(pending, dtype=np.float64)))
            if pend.ndim != 2 or pend.shape[1] != self.d:
                raise ValueError(f"pending must be [B, D] with D={self.d}, got {pend.shape}")
            b = int(pend.shape[0])
        q = int(q)
        cap = max(q, 1)
        idx = np.full(cap, -1, dtype=np.int64)
        gain, value = (np.full(cap, np.nan, dtype=np.float64) for _ in range(2))
        n_picked = C.c_int(0)
        gain0 = np.empty(m, dtype=np.float64) if want_gain0 else None
        self._check(self._lib.gpso_paths_best_batch(self._h, ptr, dt, mem, m, C.byref(rec), None if bars is None else L.dptr(bars),
                                                    None if b == 0 else L.dptr(pend), b, q, L.i64ptr(idx), L.dptr(gain), L.dptr(value),
                                                    C.byref(n_picked), None if gain0 is None else C.c_void_p(gain0.ctypes.data),
                                                    L.MEM_HOST))
        k = int(n_picked.value)
        res = (idx[:k].copy(), gain[:k].copy(), value[:k].copy())
        return res + (gain0,) if want_gain0 else res

    @staticmethod
    def paths_batch_host(values, q, kind="qei", incumbent=None, incumbent_s=None, n_pending=0, xi=0.0):
        """The rounds of ``paths_best_batch`` on the CPU from given ``values`` [S, M + B] -- the M candidates, then the
        ``n_pending`` = B pending columns -- (``gpso_paths_batch_host``: no context, no GPU) -> (idx, gain, batch_value,
        gain0)."""
        values = L.as_f64(np.asarray(values, dtype=np.float64))
        if values.ndim != 2:
            raise ValueError(f"values must be [S, M + B], got {values.shape}")
        s, b = int(values.shape[0]), int(n_pending)
        m = int(values.shape[1]) - b
        rec, bars = HipGPEngine._mc_rec(kind, xi, incumbent, incumbent_s)
        if bars is not None and bars.shape != (s,):
            raise ValueError(f"incumbent_s must be [S] with S={s}, got {bars.shape}")
        q = int(q)
        cap = max(q, 1)
        idx = np.full(cap, -1, dtype=np.int64)
        gain, value = (np.full(cap, np.nan, dtype=np.float64) for _ in range(2))
        gain0 = np.empty(max(m, 1), dtype=np.float64)
        n_picked = C.c_int(0)
        rc = L.load().gpso_paths_batch_host(C.byref(rec), L.dptr(values), s, m, b, None if bars is None else L.dptr(bars), q,
                                            L.i64ptr(idx), L.dptr(gain), L.dptr(value), C.byref(n_picked), L.dptr(gain0))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_paths_batch_host: bad record, bars or arguments")
        k = int(n_picked.value)
        return idx[:k].copy(), gain[:k].copy(), value[:k].copy(), gain0[:max(m, 0)]

    def best_ucb(self, xs, varsigma, seg_off=None):
        """gp_eval_best_ucb per segment -> (idx, mean, var, ucb) arrays of length nseg."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        if seg_off is None:
            nseg, so_ptr = 1, None
        else:
            so = np.ascontiguousarray(seg_off, dtype=np.int64)
            nseg, so_ptr = int(so.shape[0] - 1), L.i64ptr(so)
        idx, mean, var, ucb, pi, pm, pv, pu = self._winner_bufs(nseg)
        rc = self._lib.gpso_best_ucb(self._h, ptr, dt, mem, m, so_ptr, nseg, float(varsigma), pi, pm, pv, pu)
        if rc < 0:
            self._check(rc)
        return idx.copy(), mean.copy(), var.copy(), ucb.copy()

    def best_ucb_begin(self, xs, varsigma, seg_off=None):
        """Non-blocking ``best_ucb``: enqueues the call and returns a ticket for ``best_ucb_end``; two calls may be in
        flight (``gpso_best_ucb_begin``).  The leaves must stay untouched until the call is ended."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        if seg_off is None:
            nseg, so_ptr = 1, None
        else:
            so = np.ascontiguousarray(seg_off, dtype=np.int64)
            nseg, so_ptr = int(so.shape[0] - 1), L.i64ptr(so)
        ticket = self._check(self._lib.gpso_best_ucb_begin(self._h, ptr, dt, mem, m, so_ptr, nseg, float(varsigma)))
        self._open_tickets = getattr(self, "_open_tickets", {})
        self._open_tickets[ticket] = (nseg, keep)
        return ticket

    def best_ucb_grow_begin(self, bounds, depth, varsigma):
        b = L.as_f64(bounds)
        if b.ndim == 2:
            b = b[None]
        nseg, d, _ = b.shape
        if d != self.d:
            raise ValueError(f"bounds have D={d}, model has D={self.d}")
        ticket = self._check(self._lib.gpso_best_ucb_grow_begin(self._h, L.dptr(b), nseg, int(depth), float(varsigma)))
        self._open_tickets = getattr(self, "_open_tickets", {})
        self._open_tickets[ticket] = (nseg, None)
        return ticket

    def best_ucb_end(self, ticket):
        """Wait for the call behind ``ticket`` -> (idx, mean, var, ucb) arrays of length nseg."""
        nseg, _keep = self._open_tickets.pop(ticket)
        idx = np.empty(nseg, dtype=np.int64)
        mean = np.empty(nseg, dtype=np.float64)
        var = np.empty(nseg, dtype=np.float64)
        ucb = np.empty(nseg, dtype=np.float64)
        self._check(self._lib.gpso_best_ucb_end(self._h, int(ticket), L.i64ptr(idx), L.dptr(mean), L.dptr(var), L.dptr(ucb)))
        return idx, mean, var, ucb

    # -- acquisition functions (pygpso_amd/acquisition.py; csrc/acq.hpp) ---------------------------------------------
    def _seg_args(self, seg_off):
        if seg_off is None:
            return 1, None, None
        so = np.ascontiguousarray(seg_off, dtype=np.int64)
        return int(so.shape[0] - 1), L.i64ptr(so), so

    def _bounds_arg(self, bounds):
        b = L.as_f64(bounds)
        if b.ndim == 2:
            b = b[None]
        nseg, d, _ = b.shape
        if d != self.d:
            raise ValueError(f"bounds have D={d}, model has D={self.d}")
        return b, nseg

    def _acq_rec(self, acq, incumbent):
        """The ``gpso_acq`` record of a call on this context; a spec that carries maxima (``acquisition.MES``) has them
        installed first, unless they are the resident ones already."""
        maxima = getattr(acq, "maxima", None)
        if maxima is not None and not np.array_equal(np.asarray(maxima, dtype=np.float64).reshape(-1), self.acq_get_maxima()):
            self.acq_set_maxima(maxima)
        return acq.c_struct(incumbent)

    def best_acq(self, xs, acq, seg_off=None, incumbent=None):
        """``best_ucb`` ranked by the acquisition spec ``acq`` -> (idx, mean, var, value) arrays of length nseg."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        nseg, so_ptr, _so = self._seg_args(seg_off)
        rec = self._acq_rec(acq, incumbent)
        idx, mean, var, val, pi, pm, pv, pu = self._winner_bufs(nseg)
        rc = self._lib.gpso_best_acq(self._h, ptr, dt, mem, m, so_ptr, nseg, C.byref(rec), pi, pm, pv, pu)
        if rc < 0:
            self._check(rc)
        return idx.copy(), mean.copy(), var.copy(), val.copy()

    def best_acq_begin(self, xs, acq, seg_off=None, incumbent=None):
        """Non-blocking ``best_acq``: a ticket for ``best_ucb_end`` (the two slots of ``best_ucb_begin``)."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        nseg, so_ptr, _so = self._seg_args(seg_off)
        rec = self._acq_rec(acq, incumbent)
        ticket = self._check(self._lib.gpso_best_acq_begin(self._h, ptr, dt, mem, m, so_ptr, nseg, C.byref(rec)))
        self._open_tickets = getattr(self, "_open_tickets", {})
        self._open_tickets[ticket] = (nseg, keep)
        return ticket

    def best_acq_grow(self, bounds, depth, acq, incumbent=None):
        """``best_ucb_grow`` ranked by the acquisition spec ``acq``."""
        b, nseg = self._bounds_arg(bounds)
        rec = self._acq_rec(acq, incumbent)
        idx, mean, var, val, pi, pm, pv, pu = self._winner_bufs(nseg)
        rc = self._lib.gpso_best_acq_grow(self._h, L.dptr(b), nseg, int(depth), C.byref(rec), pi, pm, pv, pu)
        if rc < 0:
            self._check(rc)
        return idx.copy(), mean.copy(), var.copy(), val.copy()

    def best_acq_grow_begin(self, bounds, depth, acq, incumbent=None):
        b, nseg = self._bounds_arg(bounds)
        rec = self._acq_rec(acq, incumbent)
        ticket = self._check(self._lib.gpso_best_acq_grow_begin(self._h, L.dptr(b), nseg, int(depth), C.byref(rec)))
        self._open_tickets = getattr(self, "_open_tickets", {})
        self._open_tickets[ticket] = (nseg, None)
        return ticket

    def acq_values(self, xs, acq, incumbent=None):
        """``predict`` with the acquisition column: (mean[M], var[M], value[M]) float64 on the host."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        rec = self._acq_rec(acq, incumbent)
        mean, var, val = (np.empty(m, dtype=np.float64) for _ in range(3))
        self._check(self._lib.gpso_acq_values(self._h, ptr, dt, mem, m, C.byref(rec), C.c_void_p(mean.ctypes.data),
                                              C.c_void_p(var.ctypes.data), C.c_void_p(val.ctypes.data), L.MEM_HOST))
        return mean, var, val

    # -- the hyper-parameter ensemble (csrc/ensemble.hpp) -------------------------------------
    def ensemble_max(self):
        """Members an ensemble on the resident data may hold (32), or 0 where it does not apply."""
        return int(self._lib.gpso_ensemble_max(self._h))

    def ensemble_push(self):
        """The resident posterior becomes the next member of the ensemble -> its index."""
        return self._check(self._lib.gpso_ensemble_push(self._h))

    def ensemble_clear(self):
        self._check(self._lib.gpso_ensemble_clear(self._h))

    def ensemble_info(self):
        """-> (k, theta[k, 51]): per member 48 lengthscales, kernel variance, noise variance, constant mean."""
        k = C.c_int(0)
        theta = np.zeros((L.ENSEMBLE_MAX, L.ENSEMBLE_THETA), dtype=np.float64)
        self._check(self._lib.gpso_ensemble_info(self._h, C.byref(k), L.dptr(theta)))
        return int(k.value), theta[:k.value].copy()

    def ensemble_best_acq(self, xs, acq, seg_off=None, incumbent=None):
        """``best_acq`` under the integrated acquisition of the resident ensemble -> (idx, mean_mix, var_mix, value)
        arrays of length nseg."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        nseg, so_ptr, _so = self._seg_args(seg_off)
        rec = acq.c_struct(incumbent)
        idx = np.empty(nseg, dtype=np.int64)
        mean, var, val = (np.empty(nseg, dtype=np.float64) for _ in range(3))
        self._check(self._lib.gpso_ensemble_best_acq(self._h, ptr, dt, mem, m, so_ptr, nseg, C.byref(rec), L.i64ptr(idx),
                                                     L.dptr(mean), L.dptr(var), L.dptr(val)))
        return idx, mean, var, val

    def ensemble_acq_values(self, xs, acq, incumbent=None, want_members=False):
        """-> (mean_mix[M], var_mix[M], value[M]) float64 on the host; with ``want_members`` also the members' columns
        (member_mean[K, M], member_var[K, M])."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        rec = acq.c_struct(incumbent)
        mean, var, val = (np.empty(m, dtype=np.float64) for _ in range(3))
        k = self.ensemble_info()[0] if want_members else 0
        mm, mv = (np.empty((k, m), dtype=np.float64) for _ in range(2))
        pm, pv = (C.c_void_p(a.ctypes.data) if want_members and k > 0 else None for a in (mm, mv))
        self._check(self._lib.gpso_ensemble_acq_values(self._h, ptr, dt, mem, m, C.byref(rec), C.c_void_p(mean.ctypes.data),
                                                       C.c_void_p(var.ctypes.data), C.c_void_p(val.ctypes.data), pm, pv, L.MEM_HOST))
        return (mean, var, val, mm, mv) if want_members else (mean, var, val)

    @staticmethod
    def ensemble_fold_host(acq, member_mean, member_var, noise=None, incumbent=None):
        """The device's fold on the CPU (``gpso_ensemble_fold_host``: no context, no GPU): member columns [K, M] and the
        members' noise variances [K] -> (mean_mix[M], var_mix[M], value[M])."""
        mm = L.as_f64(np.atleast_2d(member_mean))
        mv = L.as_f64(np.atleast_2d(member_var), mm.shape)
        k, m = mm.shape
        nz = None if noise is None else L.as_f64(np.asarray(noise).reshape(-1), (k,))
        mean, var, val = (np.empty(m, dtype=np.float64) for _ in range(3))
        rec = acq.c_struct(incumbent)
        rc = L.load().gpso_ensemble_fold_host(C.byref(rec), L.dptr(mm), L.dptr(mv), None if nz is None else L.dptr(nz), int(k), int(m),
                                              L.dptr(mean), L.dptr(var), L.dptr(val))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_ensemble_fold_host: bad acquisition record (GPSO_ACQ_MES is not integrated) or arguments")
        return mean, var, val

    # -- outcome constraints (csrc/constraints.hpp) ------------------------------------------
    def constraint_max(self):
        """Members a constraint set on this context may hold (16), or 0 where a push does not apply."""
        return int(self._lib.gpso_constraint_max(self._h))

    def constraint_push(self, src, threshold, sense):
        """The exact-GP posterior resident on ``src`` (another engine on this device, or ``self``) becomes the next
        member of this context's constraint set -> its index.  ``sense`` +1: feasible where c <= threshold; -1: where
        c >= threshold."""
        return self._check(self._lib.gpso_constraint_push(self._h, src._h, float(threshold), int(sense)))

    def constraint_clear(self):
        self._check(self._lib.gpso_constraint_clear(self._h))

    def constraint_info(self):
        """-> (k, theta[k, 51], threshold[k], sense[k]); theta as ``ensemble_info``."""
        k = C.c_int(0)
        theta = np.zeros((L.CONSTRAINTS_MAX, L.ENSEMBLE_THETA), dtype=np.float64)
        thr = np.zeros(L.CONSTRAINTS_MAX, dtype=np.float64)
        sense = np.zeros(L.CONSTRAINTS_MAX, dtype=np.intc)
        self._check(self._lib.gpso_constraint_info(self._h, C.byref(k), L.dptr(theta), L.dptr(thr),
                                                   sense.ctypes.data_as(C.POINTER(C.c_int))))
        return int(k.value), theta[:k.value].copy(), thr[:k.value].copy(), sense[:k.value].astype(np.int64)

    @staticmethod
    def _cspec(mode, log_pof_min):
        return L.GpsoCspec(L.CON_MODES[mode] if isinstance(mode, str) else int(mode), float(log_pof_min))

    def constrained_best_acq(self, xs, acq, mode="gate", log_pof_min=-np.inf, seg_off=None, incumbent=None):
        """``best_acq`` under the resident constraint set -> (idx, mean, var, value, logpof) arrays of length nseg."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        nseg, so_ptr, _so = self._seg_args(seg_off)
        rec, cs = acq.c_struct(incumbent), self._cspec(mode, log_pof_min)
        idx = np.empty(nseg, dtype=np.int64)
        mean, var, val, lp = (np.empty(nseg, dtype=np.float64) for _ in range(4))
        self._check(self._lib.gpso_constrained_best_acq(self._h, ptr, dt, mem, m, so_ptr, nseg, C.byref(rec), C.byref(cs), L.i64ptr(idx),
                                                        L.dptr(mean), L.dptr(var), L.dptr(val), L.dptr(lp)))
        return idx, mean, var, val, lp

    def constrained_acq_values(self, xs, acq, mode="gate", log_pof_min=-np.inf, incumbent=None, want_members=False):
        """-> (mean[M], var[M], value[M], logpof[M]) float64 on the host: the objective's predictive columns, the ranked
        value and the log probability of feasibility; with ``want_members`` also the constraint models' columns
        (member_mean[J, M], member_var[J, M])."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        rec, cs = acq.c_struct(incumbent), self._cspec(mode, log_pof_min)
        mean, var, val, lp = (np.empty(m, dtype=np.float64) for _ in range(4))
        # (while a success member is resident its latent columns follow the constraint models' as one more row)
        k = self.constraint_info()[0] + (1 if self.success_info()[0] else 0) if want_members else 0
        mm, mv = (np.empty((k, m), dtype=np.float64) for _ in range(2))
        pm, pv = (C.c_void_p(a.ctypes.data) if want_members and k > 0 else None for a in (mm, mv))
        self._check(self._lib.gpso_constrained_acq_values(self._h, ptr, dt, mem, m, C.byref(rec), C.byref(cs), C.c_void_p(mean.ctypes.data),
                                                          C.c_void_p(var.ctypes.data), C.c_void_p(val.ctypes.data),
                                                          C.c_void_p(lp.ctypes.data), pm, pv, L.MEM_HOST))
        return (mean, var, val, lp, mm, mv) if want_members else (mean, var, val, lp)

    @staticmethod
    def constrained_fold_host(acq, mean, var, noise, member_mean, member_var, member_noise, threshold, sense, mode="gate",
                              log_pof_min=-np.inf, incumbent=None):
        """The device's constrained fold on the CPU (``gpso_constrained_fold_host``: no context, no GPU): the objective's
        columns [M] and noise variance, the members' columns [J, M], noise variances, thresholds and senses [J] ->
        (value[M], logpof[M])."""
        mm = L.as_f64(np.atleast_2d(member_mean))
        mv = L.as_f64(np.atleast_2d(member_var), mm.shape)
        k, m = mm.shape
        om, ov = L.as_f64(np.asarray(mean).reshape(-1), (m,)), L.as_f64(np.asarray(var).reshape(-1), (m,))
        nz = L.as_f64(np.asarray(member_noise, dtype=np.float64).reshape(-1), (k,))
        thr = L.as_f64(np.asarray(threshold, dtype=np.float64).reshape(-1), (k,))
        sn = np.ascontiguousarray(np.asarray(sense).reshape(-1), dtype=np.intc)
        if sn.shape != (k,):
            raise ValueError(f"sense must have {k} entries")
        val, lp = (np.empty(m, dtype=np.float64) for _ in range(2))
        rec, cs = acq.c_struct(incumbent), HipGPEngine._cspec(mode, log_pof_min)
        rc = L.load().gpso_constrained_fold_host(C.byref(rec), C.byref(cs), L.dptr(om), L.dptr(ov), float(noise), L.dptr(mm), L.dptr(mv),
                                                 L.dptr(nz), L.dptr(thr), sn.ctypes.data_as(C.POINTER(C.c_int)), int(k), int(m),
                                                 L.dptr(val), L.dptr(lp))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_constrained_fold_host: bad acquisition record (GPSO_ACQ_MES is not served, a UCB kind "
                                     "cannot be weighted), constraint record or arguments")
        return val, lp

    @staticmethod
    def constrained_success_fold_host(acq, mean, var, noise, member_mean, member_var, member_noise, threshold, sense, success_mean,
                                      success_var, mode="gate", log_pof_min=-np.inf, incumbent=None):
        """``constrained_fold_host`` with a success member (``gpso_constrained_success_fold_host``): its latent columns
        ``success_mean`` / ``success_var`` [M] add ``success_log_prob`` to logpof as the last term.  J = 0 (``member_mean``
        None or of zero rows) is served: the success term then is logpof.  -> (value[M], logpof[M])."""
        sm = L.as_f64(np.asarray(success_mean).reshape(-1))
        m = sm.shape[0]
        sv = L.as_f64(np.asarray(success_var).reshape(-1), (m,))
        mm = np.zeros((0, m)) if member_mean is None else L.as_f64(np.asarray(member_mean, dtype=np.float64).reshape(-1, m))
        k = mm.shape[0]
        mv = np.zeros((0, m)) if member_var is None else L.as_f64(np.asarray(member_var, dtype=np.float64).reshape(-1, m), (k, m))
        om, ov = L.as_f64(np.asarray(mean).reshape(-1), (m,)), L.as_f64(np.asarray(var).reshape(-1), (m,))
        nz = L.as_f64(np.asarray([] if member_noise is None else member_noise, dtype=np.float64).reshape(-1), (k,))
        thr = L.as_f64(np.asarray([] if threshold is None else threshold, dtype=np.float64).reshape(-1), (k,))
        sn = np.ascontiguousarray(np.asarray([] if sense is None else sense).reshape(-1), dtype=np.intc)
        if sn.shape != (k,):
            raise ValueError(f"sense must have {k} entries")
        val, lp = (np.empty(m, dtype=np.float64) for _ in range(2))
        rec, cs = acq.c_struct(incumbent), HipGPEngine._cspec(mode, log_pof_min)
        some = k > 0
        rc = L.load().gpso_constrained_success_fold_host(
            C.byref(rec), C.byref(cs), L.dptr(om), L.dptr(ov), float(noise), L.dptr(mm) if some else None, L.dptr(mv) if some else None,
            L.dptr(nz) if some else None, L.dptr(thr) if some else None, sn.ctypes.data_as(C.POINTER(C.c_int)) if some else None, int(k),
            int(m), L.dptr(sm), L.dptr(sv), L.dptr(val), L.dptr(lp))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_constrained_success_fold_host: bad acquisition record (GPSO_ACQ_MES is not served, a UCB "
                                     "kind cannot be weighted), constraint record or arguments")
        return val, lp

    # -- bi-objective search (csrc/ehvi.hpp) ---------------------------------------------------
    @staticmethod
    def _ehvi_rec(member, front, ref, latent):
        """The ``gpso_ehvi`` record and the array its ``front`` points into (keep it alive over the call)."""
        f = L.as_f64(np.zeros((0, 2)) if front is None else np.asarray(front, dtype=np.float64).reshape(-1, 2))
        r = L.as_f64(np.asarray(ref, dtype=np.float64).reshape(-1), (2,))
        rec = L.GpsoEhvi(int(member), 1 if latent else 0, int(f.shape[0]), L.dptr(f) if f.shape[0] else None, (C.c_double * 2)(r[0], r[1]))
        return rec, f

    @staticmethod
    def _ehvi_cspec(mode, log_pof_min):
        """``None``: no cspec (value = EHVI); else the ``gpso_cspec`` of ``mode``."""
        return None if mode is None else HipGPEngine._cspec(mode, log_pof_min)

    def ehvi_values(self, xs, member, front, ref, latent=True, mode=None, log_pof_min=-np.inf):
        """The exact EHVI of (the objective, constraint-set member ``member``) over ``front`` [P, 2] (rows (f1, f2), f1
        ascending) and the reference point ``ref`` at the points ``xs`` -> (value[M], logpof[M], mean[2, M], var[2, M]):
        the ranked value (``mode`` None: the EHVI; "weight" / "gate": under the other members' logpof), logpof, and the two
        objectives' predictive columns (row 0: the objective, row 1: the member)."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        rec, _front = self._ehvi_rec(member, front, ref, latent)
        cs = self._ehvi_cspec(mode, log_pof_min)
        val, lp = (np.empty(m, dtype=np.float64) for _ in range(2))
        mean, var = (np.empty((2, m), dtype=np.float64) for _ in range(2))
        self._check(self._lib.gpso_ehvi_values(self._h, ptr, dt, mem, m, C.byref(rec), None if cs is None else C.byref(cs),
                                               C.c_void_p(val.ctypes.data), C.c_void_p(lp.ctypes.data), C.c_void_p(mean.ctypes.data),
                                               C.c_void_p(var.ctypes.data), L.MEM_HOST))
        return val, lp, mean, var

    def best_ehvi(self, xs, member, front, ref, latent=True, mode=None, log_pof_min=-np.inf, seg_off=None):
        """Per segment the arg-max of ``ehvi_values``' value -> (idx[nseg], value[nseg], logpof[nseg], mean[2, nseg],
        var[2, nseg])."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        nseg, so_ptr, _so = self._seg_args(seg_off)
        rec, _front = self._ehvi_rec(member, front, ref, latent)
        cs = self._ehvi_cspec(mode, log_pof_min)
        idx = np.empty(nseg, dtype=np.int64)
        val, lp = (np.empty(nseg, dtype=np.float64) for _ in range(2))
        mean, var = (np.empty((2, nseg), dtype=np.float64) for _ in range(2))
        self._check(self._lib.gpso_best_ehvi(self._h, ptr, dt, mem, m, so_ptr, nseg, C.byref(rec), None if cs is None else C.byref(cs),
                                             L.i64ptr(idx), L.dptr(val), L.dptr(lp), L.dptr(mean), L.dptr(var)))
        return idx, val, lp, mean, var

    @staticmethod
    def ehvi_fold_host(front, ref, mean1, var1, noise1, mean2, var2, noise2, other_mean=None, other_var=None, other_noise=None,
                       threshold=None, sense=None, success_mean=None, success_var=None, latent=True, mode=None, log_pof_min=-np.inf):
        """The device's EHVI fold on the CPU (``gpso_ehvi_fold_host``: no context, no GPU): the two objectives' columns [M]
        and noise variances, the OTHER members' columns [K, M] (objective 2 left out; K >= 0) with their noise variances,
        thresholds and senses [K], the success member's latent columns [M] or None -> (value[M], logpof[M])."""
        m1 = L.as_f64(np.asarray(mean1, dtype=np.float64).reshape(-1))
        m = m1.shape[0]
        v1, m2, v2 = (L.as_f64(np.asarray(a, dtype=np.float64).reshape(-1), (m,)) for a in (var1, mean2, var2))
        om = np.zeros((0, m)) if other_mean is None else L.as_f64(np.asarray(other_mean, dtype=np.float64).reshape(-1, m))
        k = om.shape[0]
        ov = np.zeros((0, m)) if other_var is None else L.as_f64(np.asarray(other_var, dtype=np.float64).reshape(-1, m), (k, m))
        nz = L.as_f64(np.asarray([] if other_noise is None else other_noise, dtype=np.float64).reshape(-1), (k,))
        thr = L.as_f64(np.asarray([] if threshold is None else threshold, dtype=np.float64).reshape(-1), (k,))
        sn = np.ascontiguousarray(np.asarray([] if sense is None else sense).reshape(-1), dtype=np.intc)
        if sn.shape != (k,):
            raise ValueError(f"sense must have {k} entries")
        sm = None if success_mean is None else L.as_f64(np.asarray(success_mean, dtype=np.float64).reshape(-1), (m,))
        sv = None if success_var is None else L.as_f64(np.asarray(success_var, dtype=np.float64).reshape(-1), (m,))
        val, lp = (np.empty(m, dtype=np.float64) for _ in range(2))
        rec, _front = HipGPEngine._ehvi_rec(0, front, ref, latent)
        cs = HipGPEngine._ehvi_cspec(mode, log_pof_min)
        some = k > 0
        rc = L.load().gpso_ehvi_fold_host(
            C.byref(rec), None if cs is None else C.byref(cs), L.dptr(m1), L.dptr(v1), float(noise1), L.dptr(m2), L.dptr(v2), float(noise2),
            L.dptr(om) if some else None, L.dptr(ov) if some else None, L.dptr(nz) if some else None, L.dptr(thr) if some else None,
            sn.ctypes.data_as(C.POINTER(C.c_int)) if some else None, int(k), int(m), None if sm is None else L.dptr(sm),
            None if sv is None else L.dptr(sv), L.dptr(val), L.dptr(lp))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_ehvi_fold_host: bad front (at most 63 finite points, f1 strictly ascending, f2 strictly "
                                     "descending, every point strictly above the finite reference point), constraint record "
                                     "(feasibility mode is not served) or arguments")
        return val, lp

    # -- failed evaluations (csrc/success.hpp) ------------------------------------------------
    @staticmethod
    def success_prob_host(mean, var):
        """The device's probit map on the CPU (``gpso_success_prob_host``: no context, no GPU): latent (mean, var) [n] ->
        (prob[n], logprob[n]) with logprob = log Phi(mean / sqrt(1 + max(var, 0)))."""
        mean = L.as_f64(np.asarray(mean, dtype=np.float64).reshape(-1))
        var = L.as_f64(np.asarray(var, dtype=np.float64).reshape(-1), mean.shape)
        lp, pr = np.empty_like(mean), np.empty_like(mean)
        rc = L.load().gpso_success_prob_host(L.dptr(mean), L.dptr(var), int(mean.shape[0]), L.dptr(lp), L.dptr(pr))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_success_prob_host: bad arguments")
        return pr, lp

    def predict_prob(self, xs, want_latent=False):
        """P(success) at the points ``xs`` of the Bernoulli-installed VGP resident here (``gpso_predict_prob``) ->
        (prob[M], logprob[M]); with ``want_latent`` also the latent (mean[M], var[M]) the map read."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        pr, lp, mean, var = (np.empty(m, dtype=np.float64) for _ in range(4))
        lat = (C.c_void_p(mean.ctypes.data), C.c_void_p(var.ctypes.data)) if want_latent else (None, None)
        self._check(self._lib.gpso_predict_prob(self._h, ptr, dt, mem, m, C.c_void_p(pr.ctypes.data), C.c_void_p(lp.ctypes.data),
                                                lat[0], lat[1], L.MEM_HOST))
        return (pr, lp, mean, var) if want_latent else (pr, lp)

    def success_push(self, src):
        """The Bernoulli-installed classifier posterior resident on ``src`` (another engine on this device) becomes this
        context's success member: the constrained calls then add its log-probability to logpof, and serve J = 0."""
        self._check(self._lib.gpso_success_push(self._h, src._h))

    def success_clear(self):
        self._check(self._lib.gpso_success_clear(self._h))

    def success_info(self):
        """-> (present, n, theta[51]); theta as a row of ``ensemble_info`` (zeros while no member is resident)."""
        present, n = C.c_int(0), C.c_int64(0)
        theta = np.zeros(L.ENSEMBLE_THETA, dtype=np.float64)
        self._check(self._lib.gpso_success_info(self._h, C.byref(present), C.byref(n), L.dptr(theta)))
        return bool(present.value), int(n.value), theta

    @staticmethod
    def acq_eval_host(acq, mean, var, noise=0.0, incumbent=None):
        """The device's acquisition maps on the CPU (``gpso_acq_eval_host``: no context, no GPU) -> value[n]."""
        mean = L.as_f64(np.asarray(mean).reshape(-1))
        var = L.as_f64(np.asarray(var).reshape(-1), mean.shape)
        out = np.empty_like(mean)
        rec = acq.c_struct(incumbent)
        rc = L.load().gpso_acq_eval_host(C.byref(rec), L.dptr(mean), L.dptr(var), float(noise), int(mean.shape[0]), L.dptr(out))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_acq_eval_host: bad acquisition record or arguments")
        return out

    # -- max-value entropy search (csrc/acq.hpp: GPSO_ACQ_MES; csrc/maxcdf.hip) ---------------------------------------
    def acq_set_maxima(self, ystar):
        """Install the sampled maxima y* that ``acquisition.MES`` calls on this context read (``gpso_acq_set_maxima``): at
        most 64 finite values; ``None`` or an empty list clears them.  They are the caller's numbers: fits, appends and
        installs keep them.  Refused (E_STATE) while an asynchronous best-UCB ticket is open."""
        ys = np.zeros(0) if ystar is None else L.as_f64(np.asarray(ystar, dtype=np.float64).reshape(-1))
        self._check(self._lib.gpso_acq_set_maxima(self._h, L.dptr(ys) if ys.size else None, int(ys.size)))

    def acq_get_maxima(self):
        """The resident maxima -> float64 [k] (k = 0: none)."""
        buf = np.empty(L.ACQ_MAX_MAXIMA, dtype=np.float64)
        k = C.c_int(0)
        self._check(self._lib.gpso_acq_get_maxima(self._h, L.dptr(buf), C.byref(k)))
        return buf[:int(k.value)].copy()

    @staticmethod
    def acq_mes_eval_host(ystar, mean, var, noise=0.0, latent=True):
        """The device's MES map on the CPU (``gpso_acq_mes_eval_host``: no context, no GPU) -> value[n].  With ``latent``
        the map reads ``var - noise``."""
        ys = L.as_f64(np.asarray(ystar, dtype=np.float64).reshape(-1))
        mean = L.as_f64(np.asarray(mean).reshape(-1))
        var = L.as_f64(np.asarray(var).reshape(-1), mean.shape)
        out = np.empty_like(mean)
        rc = L.load().gpso_acq_mes_eval_host(L.dptr(ys) if ys.size else None, int(ys.size), int(bool(latent)), L.dptr(mean), L.dptr(var),
                                             float(noise), int(mean.shape[0]), L.dptr(out))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_acq_mes_eval_host: 1..64 finite maxima, a noise that is no NaN")
        return out

    ACQ_MATH = {"exp": 0, "log": 1, "log1p": 2, "erfc": 3, "mills_p": 4}

    @staticmethod
    def acq_math_host(name, x):
        """One of the functions the MES map is made of (``gpso_acq_math_host``; csrc/acq.hpp) at the float64 array ``x``."""
        x = L.as_f64(np.asarray(x, dtype=np.float64).reshape(-1))
        out = np.empty_like(x)
        rc = L.load().gpso_acq_math_host(HipGPEngine.ACQ_MATH[name], L.dptr(x), int(x.size), L.dptr(out))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_acq_math_host: bad arguments")
        return out

    def max_logcdf(self, mean, var, y, var_sub=0.0, want_used=False):
        """log P(max_j f_j < y_i) under independent leaves: sum_j log Phi((y_i - mean_j) / sqrt(max(var_j - var_sub, 0)))
        for at most 64 thresholds ``y`` (``gpso_max_logcdf``).  ``mean`` / ``var`` [M]: float64 numpy arrays or contiguous
        float64 tensors on the engine's device.  Rows with a NaN are skipped; ``want_used`` adds their complement's count."""
        y = L.as_f64(np.asarray(y, dtype=np.float64).reshape(-1))
        out = np.empty_like(y)
        used = C.c_int64(0)
        if hasattr(mean, "data_ptr"):
            if str(mean.dtype) != "torch.float64" or str(var.dtype) != "torch.float64" or not mean.is_contiguous() \
                    or not var.is_contiguous() or mean.numel() != var.numel():
                raise ValueError("mean / var must be contiguous float64 tensors of one length")
            self._order_after(mean)
            self._order_after(var)
            pm, pv, mem, m = C.c_void_p(mean.data_ptr()), C.c_void_p(var.data_ptr()), L.MEM_DEVICE, int(mean.numel())
        else:
            mean = L.as_f64(np.asarray(mean).reshape(-1))
            var = L.as_f64(np.asarray(var).reshape(-1), mean.shape)
            pm, pv, mem, m = C.c_void_p(mean.ctypes.data), C.c_void_p(var.ctypes.data), L.MEM_HOST, int(mean.shape[0])
        self._check(self._lib.gpso_max_logcdf(self._h, pm, pv, mem, m, float(var_sub), L.dptr(y), int(y.size), L.dptr(out),
                                              C.byref(used)))
        return (out, int(used.value)) if want_used else out

    @staticmethod
    def max_logcdf_host(mean, var, y, var_sub=0.0, want_used=False):
        """``max_logcdf`` on the CPU (``gpso_max_logcdf_host``: no context, no GPU; the rows are added in index order)."""
        mean = L.as_f64(np.asarray(mean).reshape(-1))
        var = L.as_f64(np.asarray(var).reshape(-1), mean.shape)
        y = L.as_f64(np.asarray(y, dtype=np.float64).reshape(-1))
        out = np.empty_like(y)
        used = C.c_int64(0)
        rc = L.load().gpso_max_logcdf_host(L.dptr(mean), L.dptr(var), int(mean.shape[0]), float(var_sub), L.dptr(y), int(y.size),
                                           L.dptr(out), C.byref(used))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_max_logcdf_host: M >= 1, 1..64 thresholds, no NaN among them")
        return (out, int(used.value)) if want_used else out

    @staticmethod
    def batch_greedy_mes_host(ystar, mean, s2, cov, noise, obs_noise, q, latent=True):
        """``batch_greedy_host`` under MES with the maxima ``ystar`` (``gpso_batch_greedy_mes_host``)."""
        ys = L.as_f64(np.asarray(ystar, dtype=np.float64).reshape(-1))
        mean = L.as_f64(np.asarray(mean).reshape(-1))
        m = int(mean.shape[0])
        s2 = L.as_f64(np.asarray(s2).reshape(-1), mean.shape)
        cov = L.as_f64(np.asarray(cov), (m, m))
        q = int(q)
        cap = max(q, 1)
        idx = np.full(cap, -1, dtype=np.int64)
        var, val = (np.full(cap, np.nan, dtype=np.float64) for _ in range(2))
        after = np.empty(m, dtype=np.float64)
        n_picked = C.c_int(0)
        rc = L.load().gpso_batch_greedy_mes_host(L.dptr(ys) if ys.size else None, int(ys.size), int(bool(latent)), L.dptr(mean), L.dptr(s2),
                                                 L.dptr(cov), float(noise), float(obs_noise), m, q, L.i64ptr(idx), L.dptr(var),
                                                 L.dptr(val), C.byref(n_picked), L.dptr(after))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_batch_greedy_mes_host: bad maxima or arguments")
        k = int(n_picked.value)
        return idx[:k].copy(), var[:k].copy(), val[:k].copy(), after

    # -- latent cross-covariance and greedy batch selection (csrc/batch.hip, csrc/batch.hpp) --------------------------
    def cross_cov(self, xa, xb, out=None):
        """The latent posterior covariance between the M rows of ``xa`` and the B <= 64 rows of ``xb``: cov [B, M]
        float64, cov[c, j] = Cov(f(xa_j), f(xb_c)) (``gpso_cross_cov``).  float64 and mixed engines; any resident posterior
        but an adopted one.  ``out`` may be a contiguous [B, M] float64 CUDA tensor to keep the result on the device."""
        ptr, dt, mem, m, keep = self._leaf_args(xa)
        xb = L.as_f64(np.atleast_2d(np.asarray(xb, dtype=np.float64)))
        if xb.ndim != 2 or xb.shape[1] != self.d:
            raise ValueError(f"xb must be [B, D] with D={self.d}, got {xb.shape}")
        b = int(xb.shape[0])
        if out is not None:
            if tuple(out.shape) != (b, m) or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous [{b}, {m}] tensor")
            self._order_after(out)
            self._check(self._lib.gpso_cross_cov(self._h, ptr, dt, mem, m, L.dptr(xb), b, C.c_void_p(out.data_ptr()), L.MEM_DEVICE))
            return out
        cov = np.empty((b, m), dtype=np.float64)
        self._check(self._lib.gpso_cross_cov(self._h, ptr, dt, mem, m, L.dptr(xb), b, C.c_void_p(cov.ctypes.data), L.MEM_HOST))
        return cov

    def best_batch(self, xs, spec, q, obs_noise, incumbent=None, want_var_after=False):
        """``q`` rows of ``xs`` picked greedily under hallucinated updates (``gpso_best_batch``; GP-BUCB): the best row by
        the acquisition spec ``spec``, then the best once that row counts as observed at its mean with noise variance
        ``obs_noise``, and so on.  Returns (idx, mean, var, value) of the picks made -- at most ``q``: a NaN value, a
        fantasy variance that is not positive, or no distinct row left end the batch -- and, with ``want_var_after``, the
        predictive variance [M] of every row after them as a fifth entry."""
        ptr, dt, mem, m, keep = self._leaf_args(xs)
        rec = self._acq_rec(spec, incumbent)
        q = int(q)
        cap = max(q, 1)
        idx = np.full(cap, -1, dtype=np.int64)
        mean, var, val = (np.full(cap, np.nan, dtype=np.float64) for _ in range(3))
        n_picked = C.c_int(0)
        after = np.empty(m, dtype=np.float64) if want_var_after else None
        self._check(self._lib.gpso_best_batch(self._h, ptr, dt, mem, m, C.byref(rec), float(obs_noise), q, L.i64ptr(idx), L.dptr(mean),
                                              L.dptr(var), L.dptr(val), C.byref(n_picked),
                                              None if after is None else C.c_void_p(after.ctypes.data), L.MEM_HOST))
        k = int(n_picked.value)
        res = (idx[:k].copy(), mean[:k].copy(), var[:k].copy(), val[:k].copy())
        return res + (after,) if want_var_after else res

    @staticmethod
    def batch_greedy_host(spec, mean, s2, cov, noise, obs_noise, q, incumbent=None):
        """The greedy rounds of ``best_batch`` on the CPU from a given mean [M], predictive variance [M] and latent
        covariance [M, M] (``gpso_batch_greedy_host``: no context, no GPU) -> (idx, var, value, var_after)."""
        mean = L.as_f64(np.asarray(mean).reshape(-1))
        m = int(mean.shape[0])
        s2 = L.as_f64(np.asarray(s2).reshape(-1), mean.shape)
        cov = L.as_f64(np.asarray(cov), (m, m))
        q = int(q)
        cap = max(q, 1)
        idx = np.full(cap, -1, dtype=np.int64)
        var, val = (np.full(cap, np.nan, dtype=np.float64) for _ in range(2))
        after = np.empty(m, dtype=np.float64)
        n_picked = C.c_int(0)
        rec = spec.c_struct(incumbent)
        rc = L.load().gpso_batch_greedy_host(C.byref(rec), L.dptr(mean), L.dptr(s2), L.dptr(cov), float(noise), float(obs_noise), m, q,
                                             L.i64ptr(idx), L.dptr(var), L.dptr(val), C.byref(n_picked), L.dptr(after))
        if rc != L.OK:
            raise L.GpsoHipError(rc, "gpso_batch_greedy_host: bad acquisition record or arguments")
        k = int(n_picked.value)
        return idx[:k].copy(), var[:k].copy(), val[:k].copy(), after

    # -- ternary geometry ------------------------------------------------------------------------
    def grow_rows(self, depth):
        return int(self._lib.gpso_grow_rows(int(depth)))

    def grow(self, bounds, depth):
        """bounds [nseg, D, 2] (or [D, 2]) -> centres [nseg, rows, D] (or [rows, D]) float64."""
        b = L.as_f64(bounds)
        single = b.ndim == 2
        if single:
            b = b[None]
        nseg, d, two = b.shape
        assert two == 2
        rows = self.grow_rows(depth)
        out = np.empty((nseg, rows, d), dtype=np.float64)
        self._check(self._lib.gpso_grow(self._h, L.dptr(b), nseg, d, int(depth), L.dptr(out)))
        return out[0] if single else out

    def best_ucb_grow(self, bounds, depth, varsigma):
        b = L.as_f64(bounds)
        if b.ndim == 2:
            b = b[None]
        nseg, d, _ = b.shape
        if d != self.d:
            raise ValueError(f"bounds have D={d}, model has D={self.d}")
        idx, mean, var, ucb, pi, pm, pv, pu = self._winner_bufs(nseg)
        rc = self._lib.gpso_best_ucb_grow(self._h, L.dptr(b), nseg, int(depth), float(varsigma), pi, pm, pv, pu)
        if rc < 0:
            self._check(rc)
        return idx.copy(), mean.copy(), var.copy(), ucb.copy()

    # -- multi-GPU group (RCCL behind the C-ABI; see pygpso_amd/distributed.py) ------------------
    def comm_init(self, rank, world, unique_id):
        """Join a group (collective: every rank calls it with the same 128-byte id of
        ``distributed.unique_id()``)."""
        buf = C.create_string_buffer(bytes(unique_id), L.UNIQUE_ID_BYTES)
        self._check(self._lib.gpso_comm_init(self._h, int(rank), int(world), buf))
        self.rank, self.world = int(rank), int(world)

    def comm_destroy(self):
        self._check(self._lib.gpso_comm_destroy(self._h))
        self.rank, self.world = 0, 1

    def broadcast_posterior(self, root=0):
        """Collective: the posterior resident on ``root`` becomes resident here (RCCL broadcast)."""
        self._check(self._lib.gpso_broadcast_posterior(self._h, int(root)))
        n, d = C.c_int64(), C.c_int()
        self._check(self._lib.gpso_problem_shape(self._h, C.byref(n), C.byref(d)))
        self.n, self.d = int(n.value), int(d.value)

    def broadcast_posterior_rows(self, root=0):
        """Collective: after ``append`` on ``root`` only what the appends wrote travels (``gpso_broadcast_posterior_rows``);
        any rank that cannot take rows makes every rank take the whole range.  Returns True when rows sufficed;
        ``last_count(0)`` = the bytes that travelled."""
        rc = self._check(self._lib.gpso_broadcast_posterior_rows(self._h, int(root)))
        n, d = C.c_int64(), C.c_int()
        self._check(self._lib.gpso_problem_shape(self._h, C.byref(n), C.byref(d)))
        self.n, self.d = int(n.value), int(d.value)
        return rc == L.OK

    def posterior_dirty_ranges(self):
        """[(offset, nbytes), ...] of the posterior arena that a peer holding the posterior of the last hand-off lacks
        (``gpso_posterior_dirty_ranges``): [] = up to date; one range = the whole span when rows do not apply."""
        off = np.zeros(12, dtype=np.int64)
        nb = np.zeros(12, dtype=np.int64)
        cnt = self._check(self._lib.gpso_posterior_dirty_ranges(self._h, L.i64ptr(off), L.i64ptr(nb), 12))
        return [(int(off[i]), int(nb[i])) for i in range(cnt)]

    def posterior_mark_synced(self):
        """The peers now hold this posterior (after a hand-off by plain copies): the next ``posterior_dirty_ranges`` counts from here."""
        self._check(self._lib.gpso_posterior_mark_synced(self._h))

    def best_ucb_sharded(self, local_leaves, m_global, varsigma, seg_off=None):
        """Collective ``best_ucb``: ``local_leaves`` are this rank's rows
        ``distributed.shard_range(m_global, rank, world)`` of the batch; ``seg_off`` is global.
        Returns the global (idx, mean, var, ucb) per segment, identical on every rank."""
        ptr, dt, mem, m, keep = self._leaf_args(local_leaves)
        if seg_off is None:
            nseg, so_ptr = 1, None
        else:
            so = np.ascontiguousarray(seg_off, dtype=np.int64)
            nseg, so_ptr = int(so.shape[0] - 1), L.i64ptr(so)
        idx = np.empty(nseg, dtype=np.int64)
        mean = np.empty(nseg, dtype=np.float64)
        var = np.empty(nseg, dtype=np.float64)
        ucb = np.empty(nseg, dtype=np.float64)
        self._check(self._lib.gpso_best_ucb_sharded(self._h, ptr, dt, mem, m, int(m_global), so_ptr, nseg,
                                                    float(varsigma), L.i64ptr(idx), L.dptr(mean), L.dptr(var),
                                                    L.dptr(ucb)))
        return idx, mean, var, ucb

    def best_ucb_grow_sharded(self, bounds, depth, varsigma):
        """Collective ``best_ucb_grow``: every rank grows and scores its share of the reference rows."""
        b = L.as_f64(bounds)
        if b.ndim == 2:
            b = b[None]
        nseg, d, _ = b.shape
        if d != self.d:
            raise ValueError(f"bounds have D={d}, model has D={self.d}")
        idx = np.empty(nseg, dtype=np.int64)
        mean = np.empty(nseg, dtype=np.float64)
        var = np.empty(nseg, dtype=np.float64)
        ucb = np.empty(nseg, dtype=np.float64)
        self._check(self._lib.gpso_best_ucb_grow_sharded(self._h, L.dptr(b), nseg, int(depth), float(varsigma),
                                                         L.i64ptr(idx), L.dptr(mean), L.dptr(var), L.dptr(ucb)))
        return idx, mean, var, ucb

    def comm_abort(self):
        """Abort this engine's communicator (``ncclCommAbort``).  The one call that may come from ANOTHER thread
        than the one blocked inside a group call of this engine: that call then returns an error."""
        self._lib.gpso_comm_abort(self._h)

    # -- the two halves of the sharded calls, for an arbitrary (rank, world), no communicator needed ----
    def shard_winners(self, rank, world, local_leaves, m_global, varsigma, seg_off=None):
        """Rank ``rank``'s local half of ``best_ucb_sharded`` in a group of ``world``: its payload
        (``gpso_group_payload_doubles(nseg)`` float64: nseg x (mean, var, ucb, bit-cast index), spare, status)."""
        ptr, dt, mem, m, keep = self._leaf_args(local_leaves)
        if seg_off is None:
            nseg, so_ptr = 1, None
        else:
            so = np.ascontiguousarray(seg_off, dtype=np.int64)
            nseg, so_ptr = int(so.shape[0] - 1), L.i64ptr(so)
        payload = np.empty(self._lib.gpso_group_payload_doubles(nseg), dtype=np.float64)
        self._check(self._lib.gpso_shard_winners(self._h, int(rank), int(world), ptr, dt, mem, m, int(m_global),
                                                 so_ptr, nseg, float(varsigma), L.dptr(payload)))
        return payload

    def shard_winners_grow(self, rank, world, bounds, depth, varsigma):
        b = L.as_f64(bounds)
        if b.ndim == 2:
            b = b[None]
        nseg = b.shape[0]
        payload = np.empty(self._lib.gpso_group_payload_doubles(nseg), dtype=np.float64)
        self._check(self._lib.gpso_shard_winners_grow(self._h, int(rank), int(world), L.dptr(b), nseg, int(depth),
                                                      float(varsigma), L.dptr(payload)))
        return payload

    def fold_winners(self, payloads, nseg, m_global=-1, seg_off=None):
        """Payloads of all ranks (rank order) -> (idx, mean, var, ucb) per segment, as the group call returns
        them.  ``m_global`` >= 0 (with the global ``seg_off``): payloads of ``shard_winners``; < 0: of
        ``shard_winners_grow``."""
        g = np.ascontiguousarray(np.stack([np.asarray(q, dtype=np.float64) for q in payloads]))
        so_ptr = None
        if seg_off is not None:
            so = np.ascontiguousarray(seg_off, dtype=np.int64)
            so_ptr = L.i64ptr(so)
        idx = np.empty(nseg, dtype=np.int64)
        mean = np.empty(nseg, dtype=np.float64)
        var = np.empty(nseg, dtype=np.float64)
        ucb = np.empty(nseg, dtype=np.float64)
        self._check(self._lib.gpso_fold_winners(self._h, L.dptr(g), int(g.shape[0]), int(m_global), so_ptr, int(nseg),
                                                L.i64ptr(idx), L.dptr(mean), L.dptr(var), L.dptr(ucb)))
        return idx, mean, var, ucb

    # -- introspection -----------------------------------------------------------------------
    def get_matrix(self, which):
        out = np.empty((self.n, self.n), dtype=np.float64)
        self._check(self._lib.gpso_get_matrix(self._h, int(which), L.dptr(out)))
        return out

    def get_vector(self, which):
        out = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.gpso_get_vector(self._h, int(which), L.dptr(out)))
        return out

    def posterior_buffers(self):
        """[(device_ptr, nbytes), ...] of what a peer rank needs to predict."""
        ptrs = (C.c_void_p * 8)()
        nb = (C.c_int64 * 8)()
        cnt = self._check(self._lib.gpso_posterior_buffers(self._h, ptrs, nb, 8))
        return [(int(ptrs[i] or 0), int(nb[i])) for i in range(cnt)]

    def posterior_span(self):
        """(device_ptr, offset, nbytes): the ONE contiguous range of this context's posterior arena the resident
        posterior uses -- what ``broadcast_posterior`` moves with a single ncclBroadcast."""
        ptr, off, nb = C.c_void_p(), C.c_int64(), C.c_int64()
        self._check(self._lib.gpso_posterior_span(self._h, C.byref(ptr), C.byref(off), C.byref(nb)))
        return int(ptr.value or 0), int(off.value), int(nb.value)

    def posterior_span_at(self, offset, nbytes):
        """Device pointer of (offset, nbytes) -- a peer's ``posterior_span`` -- inside THIS context's arena."""
        ptr = C.c_void_p()
        self._check(self._lib.gpso_posterior_span_at(self._h, int(offset), int(nbytes), C.byref(ptr)))
        return int(ptr.value or 0)

    def posterior_hash(self):
        """64-bit fingerprint of the resident predict-ready posterior (``gpso_posterior_hash``)."""
        out = C.c_uint64()
        self._check(self._lib.gpso_posterior_hash(self._h, C.byref(out)))
        return int(out.value)

    def alloc_posterior(self, n, d):
        self._check(self._lib.gpso_alloc_posterior(self._h, int(n), int(d)))
        self.n, self.d = int(n), int(d)

    def adopt_posterior(self):
        self._check(self._lib.gpso_adopt_posterior(self._h))
        n, d = C.c_int64(), C.c_int()  # (a posterior extended by gpso_append on the sender arrives with more rows)
        self._check(self._lib.gpso_problem_shape(self._h, C.byref(n), C.byref(d)))
        self.n, self.d = int(n.value), int(d.value)
