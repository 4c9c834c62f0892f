/*
 * gpso_hip.h -- C-ABI of libgpso_hip.so: the MI355X (gfx950) GP-surrogate + leaf-UCB engine.
 *
 * The reference (jajcayn/pygpso v0.6.1) is pure Python and has NO native interface: its numerics
 * are GPflow/TensorFlow calls.  Every entry point below therefore cites the reference call site
 * it replaces (paths relative to the reference repo) instead of an existing FFI symbol.  The
 * Python binding a maintainer adds is the ctypes stub in INTEGRATION.md (shipped as
 * pygpso_amd/_lib.py).
 *
 * Conventions
 *   - plain pointers and sizes only; all host matrices are C-contiguous row-major float64;
 *   - every call returns GPSO_OK (0) or a negative GPSO_E_* code; the message is available from
 *     gpso_last_error(ctx) (ctx == NULL: the message of the last failed gpso_create on this thread);
 *   - the library owns its device memory; the caller owns every buffer it passes in;
 *   - calls are synchronous at the boundary: host outputs are valid on return;
 *   - a context is bound to one device and one HIP stream, is NOT thread-safe and NOT fork-safe
 *     (the reference drives this path from a single Python thread, gpso/optimisation.py:594-622);
 *   - "mem" arguments say where a caller buffer lives: GPSO_MEM_HOST or GPSO_MEM_DEVICE
 *     (a device pointer valid on the context's device, e.g. torch.Tensor.data_ptr()).
 */
#ifndef GPSO_HIP_H
#define GPSO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpso_ctx gpso_ctx;

/* status codes */
#define GPSO_OK 0
#define GPSO_E_ARG (-1)   /* bad argument / shape                                             */
#define GPSO_E_HIP (-2)   /* a HIP runtime call failed                                        */
#define GPSO_E_NOTPD (-3) /* K + noise*I not positive definite (message names the pivot);     */
                          /* the reference lets TF's InvalidArgumentError escape here         */
#define GPSO_E_OOM (-4)   /* device allocation failed                                         */
#define GPSO_E_STATE (-5) /* call order: no training data / no posterior resident yet         */
#define GPSO_E_RCCL (-6)  /* an RCCL call of the multi-GPU group failed (or librccl could not be loaded) */
#define GPSO_E_PRECISION (-7) /* float predict arithmetic cannot meet the stated tolerance on this */
                          /* posterior (measured by the self-test, see gpso_precision_info): open a   */
                          /* GPSO_MIXED or GPSO_F64 context instead                                   */

/* arithmetic type of a context (what the kernels compute in).  Also the type tag of leaf buffers
 * (xs_dtype: GPSO_F64 | GPSO_F32 only). */
#define GPSO_F64 0   /* fit and predict in float64 (the reference's dtype: gpflow.default_float)      */
#define GPSO_F32 1   /* fit (Gram, Cholesky, L^-1, alpha) and predict apply in float32                */
#define GPSO_MIXED 2 /* fit in float64, predict apply in float32 (or split bf16): the hyper-parameter */
                     /* path is bit-identical to GPSO_F64, only predictions carry float rounding      */

/* stationary kernels, [gpflow.kernels]: the objects passed as gp_kernel at gpso/gp_surrogate.py:393-434 */
#define GPSO_MATERN52 0 /* default, gpso/gp_surrogate.py:424 */
#define GPSO_MATERN32 1
#define GPSO_MATERN12 2
#define GPSO_SQEXP 3 /* SquaredExponential / RBF */

#define GPSO_MEM_HOST 0
#define GPSO_MEM_DEVICE 1

/* options (gpso_set_option) */
#define GPSO_OPT_PREDICT_MATH 1 /* arithmetic of the L^-1 apply in predict/best_ucb, float-predict contexts: */
#define GPSO_MATH_NATIVE 0      /*   f32 MFMA (what GPSO_F64 contexts always use, in double)             */
#define GPSO_MATH_AUTO 1        /*   default: a ladder walked per posterior -- F16X3 where the posterior */
                                /*   allows it (padded N a multiple of 256, leaf fragments fit LDS) and   */
                                /*   its self-test passes with it, else BF16X6, else the f32 MFMA kernel  */
#define GPSO_MATH_BF16X3 3      /*   2-way bf16 split, 3 bf16 MFMAs per product: |d var| ~ 2e-5 sigma^2  */
#define GPSO_MATH_BF16X6 6      /*   3-way bf16 split, 6 bf16 MFMAs per f32 product, f32 accumulation:   */
                                /*   f32-class accuracy (measured beside native f32 in bench.py)         */
#define GPSO_MATH_F16X3 13      /*   2-way fp16 split (2 x 11 bits), 3 fp16 MFMAs per product, operands   */
                                /*   scaled by powers of two into fp16's range, f32 accumulation: each    */
                                /*   operand carried to 2^-22, the dropped low x low product 2^-22        */
#define GPSO_OPT_FIT_SINGLE_LEVEL_MAX 2 /* tuning / test hook: largest padded N whose Cholesky runs single-level */
                                        /* with L^-1 built beside it (default 3584, double 2560); 0 = always two-level +     */
                                        /* level-doubling triangular inverse.  Results agree to rounding.       */
#define GPSO_OPT_GENERATION 3   /* float-predict contexts: arithmetic of the cross-Gram x.x* contraction / r^2 */
#define GPSO_GEN_F64 0          /*   double: r^2 free of float cancellation error                              */
#define GPSO_GEN_F32 1          /*   float: GPflow's GEMM form evaluated in float (|d r^2| ~ 1e-5 at l ~ 0.1) */
#define GPSO_GEN_AUTO 2         /*   (default) float when the precision self-test of the posterior at hand     */
                                /*   passes with it by a margin of 8x, double otherwise; double when no self-test can run and    */
                                /*   for Matern-1/2 (its sqrt at r -> 0 is blind to the test)                  */
#define GPSO_OPT_PRECISION_CHECK 4 /* 1: the first predict after every fit runs the self-test and returns       */
                                   /* GPSO_E_PRECISION when it fails (default in GPSO_F32 / GPSO_MIXED); 0: off  */
                                   /* (default in GPSO_F64)                                                     */
#define GPSO_OPT_FIT_FUSED_SMALL 5 /* 1 (default): N <= 128 is fitted by the single-launch, single-workgroup     */
                                   /* kernel; 0: the general multi-launch path (test hook: results agree to     */
                                   /* rounding)                                                                 */
#define GPSO_OPT_FIT_BF16_SYRK 6   /* GPSO_F32 contexts, N above the single-level limit: the large products of the fit     */
                                   /* (rank-W trailing updates, level-doubling inverse, K^-1) run on the 16-bit matrix     */
                                   /* cores as split products with f32 accumulation.  2 (default): TWO fp16 pieces of the  */
                                   /* power-of-two scaled operands, three MFMAs per product (the dropped low x low term is */
                                   /* 2^-22 relative) -- where the hyper-parameters keep every operand in fp16's range      */
                                   /* (noise / variance above ~1e-9), else as 1; 1: THREE bf16 pieces, six MFMAs per       */
                                   /* product (round 3-4; f32-class entry by entry); 0: f32 MFMA                            */
#define GPSO_OPT_TIMING 7          /* 1 (default): every fit / predict-type entry point records the event pairs           */
                                   /* gpso_last_ms reads (two to four HIP calls + an elapsed-time query: 10-25 us of a     */
                                   /* call); 0: none, gpso_last_ms returns 0 -- for callers in a loop of small evaluations */
                                   /* (the drop-in surrogate switches it off); k > 1: every k-th call is timed, the others */
                                   /* leave gpso_last_ms at the last sample (bench.py: sampled kernel times inside its     */
                                   /* timed region)                                                                        */
#define GPSO_OPT_SPLIT_KERNEL 8    /* which step the split predict kernels (F16X3, BF16X6, BF16X3) run: 0 (default) the  */
#define GPSO_SPLIT_KERNEL_AUTO 0   /*   FUSED step of round 4 (every wave applies step q with the generation of step q+1  */
#define GPSO_SPLIT_KERNEL_TWO_PHASE 1 /* dealt into its MFMA shadows), 1 round 3's two-phase step.  Both give the SAME    */
                                   /*   BITS (tests/test_gpu_parity.py); the option exists for that comparison            */
#define GPSO_SPLIT_KERNEL_FUSED16 2 /* the fused step by name (= AUTO)                                                     */
#define GPSO_SPLIT_KERNEL_FUSED32 3 /* the fused step on the 32x32x16 matrix instruction: fewer issue slots, 4.9 % fewer  */
                                   /*   clocks, an 11 % lower clock -- 7 % slower; only in builds with -DGPSO_STEP32=1,    */
                                   /*   GPSO_E_ARG otherwise.  Same tolerances, not the same bits.                         */
#define GPSO_OPT_SMALL_CALLS 9     /* best-UCB calls on small batches (<= 16384 rows) are launch-bound.  1 (default): a   */
                                   /* short sequence -- THREE launches (growth + input scaling with the boxes by value,    */
                                   /* tiles, one-workgroup finalize + arg-max writing pinned host memory), or ONE where   */
                                   /* that measures faster (native tile kernel, N_pad = 256: rows made in the kernel's     */
                                   /* prologue, leaves finalised and reduced in its epilogue, the last workgroup to arrive */
                                   /* writes the records); no copy operation either way.  2: three launches only; 3: one   */
                                   /* launch wherever it applies (N_pad = 128 too); 0: always the general sequence (2      */
                                   /* copies in, 5 launches, a copy back).  Same bits in all (tests/test_gpu_parity.py)    */
#define GPSO_OPT_CONTRACTION 10    /* the x.x* contraction of the fp16-split kernel (GPSO_MATH_F16X3) under float         */
#define GPSO_CONTRACTION_AUTO 0    /*   generation: 0 (default) on the fp16 pipe -- the scaled inputs split into fp16      */
#define GPSO_CONTRACTION_F32 1     /*   piece pairs like L^-1, three products, the training input's norm riding in a spare */
#define GPSO_CONTRACTION_F16 2     /*   slot; 1: the f32 matrix instruction (rounds 1-3); 2: same as 0 today.  Different  */
                                   /*   roundings of r^2, both inside the float class: the self-test rules on whichever    */
                                   /*   runs                                                                                */
#define GPSO_OPT_FUSED_PREP 11     /* 1 (default): float leaves (GPSO_F32) of a one-chunk batch are scaled by the lengthscales in  */
                                   /* the fp16-contraction kernel's own prologue -- no prep launch in front of it; 0: the separate */
                                   /* prep kernel.  Same bits (tests/test_gpu_parity.py); the option exists for that comparison     */
#define GPSO_OPT_FIT_OVERLAP 12    /* float64 fits above the single-level limit (N_pad > 2560; the fit of GPSO_F64 and GPSO_MIXED      */
                                   /* contexts).  Bit 1 (value 2, default): the level-doubling inverse runs on a second stream, pair   */
                                   /* by pair, as soon as the panels a product reads are final -- beside the rest of the factorisation */
                                   /* instead of behind it.  Bit 0: the next diagonal block is factored on a side stream beside the    */
                                   /* trailing update (as the float fit does; measured not to pay in double: the chain's launches need */
                                   /* whole free CUs and starve behind the update's tiles).  0: round 5's sequential schedule.  The    */
                                   /* same products in the same order on the same tiles: the same bits whatever the value.             */
#define GPSO_OPT_ROW_LOOP 13       /* 1 (default): a workgroup of the split predict kernels keeps its 256 leaves and loops over row     */
                                   /* blocks of L^-1, the row blocks of a leaf tile shared by as many workgroups as gives the shortest  */
                                   /* modelled makespan (C3: one -- 256 workgroups of 288 k-steps instead of 2 048 of 8 .. 64; ragged   */
                                   /* batches and batches whose live count only the device knows: one row block per workgroup);        */
                                   /* 0: one row block per workgroup always (rounds 1-5); v >= 2: exactly min(v, row blocks)            */
                                   /* workgroups per leaf tile, -1: exactly one, whatever the batch (tests).  Per context.  Same bits   */
                                   /* whatever the value.                                                                               */
#define GPSO_OPT_PARK_BYTES 14     /* the default split predict kernel (fp16 split, fused step, one chunk of the fp16 contraction:      */
                                   /* D <= 28) regenerates every k-step's cross-Gram pieces in every row block a workgroup loops over.  */
                                   /* v > 0: a budget in bytes for PARKING the lowest even k-steps instead -- stored once by a          */
                                   /* workgroup's first row block (32 KB per step and workgroup, in a buffer of the context that is     */
                                   /* allocated by the first launch that parks and reused from then on) and reloaded by its later row   */
                                   /* blocks, odd steps and diagonal steps generated as ever; as many steps as the budget pays for,     */
                                   /* none where a workgroup has fewer than three row blocks or the kernel's LDS has no room for the    */
                                   /* reload windows.  0: off -- exactly the kernel without it.  Per context.  Same bits whatever the   */
                                   /* value.  gpso_last_count(ctx, 5) and (ctx, 6) say what the last launch did.                        */
                                   /* Default 256 MB (268435456): the best of 0 / 64 / 128 / 256 MB at C3 -- +3.6 / +3.7 % predictions/s */
                                   /* on two boxes, level with off on a third; C4 share +2.4 % | level (profiles/park_reload_ab_*.txt). */
                                   /* The buffer (201 MB at C3) is held until the context is destroyed.                                 */
#define GPSO_OPT_SCREEN 15         /* gpso_best_ucb / _begin on float leaves on the device, one segment, the default float kernels (fp16 */
                                   /* split, fp16 contraction, fused step), a finite varsigma >= 0.  1 (default): calls of more than    */
                                   /* 16384 rows are SCREENED -- every leaf's mean is computed alone (the bits the tile kernel gives    */
                                   /* it), a leaf whose ucb at zero variance share lies below that of the largest mean is dropped, and  */
                                   /* the tile kernel scores the survivors only; the call's last kernel accepts the record or asks for  */
                                   /* the general sequence, which the call then runs.  After one refusal the posterior is not screened  */
                                   /* again until it changes.  0: today's launches exactly.  2: any batch size (tests).  Per context.   */
                                   /* Same record bits whatever the value; gpso_last_count(ctx, 7) and (ctx, 8) say what happened.      */
#define GPSO_OPT_SURVIVOR_TILE 16  /* the tile of the split predict kernels' default family (fp16 split, fp16 contraction, fused step,  */
                                   /* float generation).  WIDE: a workgroup of 8 waves owns 256 leaves, two column tiles of 16 per      */
                                   /* wave -- the batch kernel.  NARROW: a workgroup of 4 waves owns 64 leaves, one column tile per     */
                                   /* wave, one wave per SIMD: the few hundred survivors of a screened call (GPSO_OPT_SCREEN) spread    */
                                   /* over four times as many compute units, and a wave's k-step is half as long.  0 (default): the     */
                                   /* survivors' launch of a screened call takes the narrow tile up to the survivor count a makespan    */
                                   /* model gives it (gpso_survivor_narrow_max_host) and the wide one above -- chosen on the device:    */
                                   /* both launches are enqueued and one leaves at once --, every other launch is wide.  1: wide        */
                                   /* everywhere.  2:                                                                                   */
                                   /* narrow wherever the default family runs on float leaves, gpso_predict included (tests: every      */
                                   /* leaf's bits, not only a winner's).  Per context.  Same bits whatever the value: a leaf's          */
                                   /* arithmetic depends neither on its lane nor on its wave nor on its workgroup.                      */
                                   /* gpso_last_count(ctx, 9) says which tile the last launch used.                                     */
/* floating-point options (gpso_set_option_f64): tolerances of the self-test */
#define GPSO_OPTF_TOL_VAR 100  /* max |d var| at the training inputs, relative to the kernel variance (default 1e-4; GPSO_F32: 1e-3) */
#define GPSO_OPTF_TOL_MEAN 101 /* max |d mean| at the training inputs, relative to max |y - c|   (default 1e-4; GPSO_F32: 1e-3) */

/* which device-resident matrix / vector the debug getters copy out (as float64) */
#define GPSO_MAT_CHOL 0  /* L, lower Cholesky factor of K + noise*I (upper triangle returned as 0) */
#define GPSO_MAT_LINV 1  /* L^-1 (lower)                                                        */
#define GPSO_MAT_KINV 2  /* (K + noise*I)^-1, valid after a gpso_fit_eval with grad != NULL      */
#define GPSO_MAT_GRAM 3  /* K + noise*I as assembled (only valid before factorisation: debug)    */
#define GPSO_VEC_ALPHA 0 /* alpha = (K + noise*I)^-1 (y - c)                                     */
#define GPSO_VEC_WHITE 1 /* a = L^-1 (y - c)                                                     */
#define GPSO_VEC_NOISE_DIAG 2 /* s, the per-point noise of gpso_set_noise_diag (zeros when none is set); needs data only */

/* ---- lifetime ---------------------------------------------------------------------------- */

/* Replaces: constructing gpflow.models.GPR (gpso/gp_surrogate.py:488-495) -- the model object
 * that owns data, hyper-parameters and cached factorisation.  dtype: GPSO_F64 | GPSO_F32. */
int gpso_create(gpso_ctx** out, int device, int dtype);
void gpso_destroy(gpso_ctx* ctx);
const char* gpso_last_error(const gpso_ctx* ctx);

/* Run all work on an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) instead
 * of the context's own stream; NULL restores the private stream. */
int gpso_set_stream(gpso_ctx* ctx, void* hip_stream);
int gpso_synchronize(gpso_ctx* ctx);
/* No counterpart in the reference (GPflow computes in float64 throughout): selects how the
 * predict path multiplies by L^-1.  The split modes work on row blocks of 256: GPSO_F32 / GPSO_MIXED
 * contexts pad N > 128 to a multiple of 256 for them (GPSO_F64 contexts and N <= 128 pad to 128
 * and run the native kernel), and keep an extra nsplit * N_pad^2 16-bit copy of L^-1. */
int gpso_set_option(gpso_ctx* ctx, int option, int value);
int gpso_set_option_f64(gpso_ctx* ctx, int option, double value);
/* Order the context's stream behind everything already queued on producer_stream (a hipStream_t, e.g.
 * torch.cuda.current_stream().cuda_stream; NULL = the legacy default stream): call it before handing
 * the library device buffers that another stream is still writing (GPSO_MEM_DEVICE leaves / outputs).
 * The library itself is synchronous at the boundary, so no ordering is needed after a call returns. */
int gpso_wait_stream(gpso_ctx* ctx, void* producer_stream);

/* ---- fit (GPSurrogate.gp_update -> GPRSurrogate._gp_train) --------------------------------- */

/* Replaces: GPSurrogate.current_training_data hand-off + `model.data = (x, y)`
 * (gpso/gp_surrogate.py:232-244, :498).  X[N*D], y[N] float64 host. */
int gpso_set_data(gpso_ctx* ctx, const double* X, const double* y, int64_t n, int d);

/* No counterpart in the reference (its pinned GPflow has one likelihood variance for all points; newer GPflow takes a
 * per-point one): replaces nothing, adds the known variance of each observation -- e.g. of the mean of eval_repeats scores,
 * which gpso/optimisation.py:220-241 reduces to that mean alone.  s[N] (host float64, s_i >= 0) is fixed, not trained:
 * every later fit on this data factorises K_y = k(X, X) + diag(noise + s_i), noise being the trained shared variance of
 * gpso_fit_eval / gpso_fit_eval_u / gpso_fit_eval_u_batch, whose NLML, alpha, L^-1 and gradient keep their formulas with
 * that K_y (d K_y / d noise is still I).  Predictions add the shared noise only: s is not known at a new point.
 * Call it after gpso_set_data with the same n.  s = NULL clears the vector; every gpso_set_data (and gpso_set_posterior)
 * clears it too.  A resident posterior is invalidated as by new data: fit again before predicting.  The vector itself stays
 * resident (N_pad doubles on the device, a host mirror for GPSO_VEC_NOISE_DIAG and the refits of gpso_append).
 * GPSO_E_ARG: n is not the resident N, or some s_i is negative or not finite.  GPSO_E_STATE: no training data, or an
 * asynchronous best-UCB call in flight.
 * The VGP, SGPR, SVGP and inducing-point entry points return GPSO_E_ARG on a context with a vector set. */
int gpso_set_noise_diag(gpso_ctx* ctx, const double* s /* [n] host, nullable */, int64_t n);

/* Replaces: ONE evaluation of gpflow GPR.training_loss (+ its reverse-mode gradient) inside
 * optimiser.minimize (gpso/gp_surrogate.py:500-503).  Hyper-parameters are the CONSTRAINED values:
 * lengthscales[n_ls] (n_ls = 1 isotropic, or = D for ARD), kernel variance, noise variance,
 * constant mean.  Outputs: *nlml = 1/2 |L^-1(y-c)|^2 + sum log L_ii + N/2 log 2pi;
 * grad (nullable) = d nlml / d (lengthscales..., variance, noise, mean_c), n_ls + 3 values.
 * Leaves L, L^-1, alpha resident (the posterior is predict-ready afterwards). */
int gpso_fit_eval(gpso_ctx* ctx, int kernel, const double* lengthscales, int n_ls, double variance,
                  double noise, double mean_c, double* nlml, double* grad);

/* The same evaluation in the OPTIMISER's variables -- what one call of the closure SciPy's L-BFGS-B drives costs in
 * the reference: GPflow's parameter transforms, training_loss and its reverse-mode gradient
 * (gpso/gp_surrogate.py:500-503; transforms: SURVEY.md Appendix A.1).  u = the unconstrained vector in tf.Module's
 * order: lengthscales[n_ls], kernel variance, likelihood variance [, constant mean when train_mean != 0; otherwise the
 * mean is mean_c_fixed].  lengthscale = softplus(u), variance = softplus(u), noise = 1e-6 + softplus(u), mean = u; the
 * transforms and the chain rule d/du = d/dtheta * sigmoid(u) run on the host side of the library with numpy's own
 * formulas (bit-identical to evaluating them in Python and calling gpso_fit_eval).  Outputs: *nlml; grad_u (nullable)
 * [n_ls + 2 + (train_mean != 0)]; theta_out (nullable) [n_ls + 3]: the constrained values used (lengthscales...,
 * variance, noise, mean). */
int gpso_fit_eval_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                    double* nlml, double* grad_u, double* theta_out);

/* ---- leave-one-out (no counterpart in the reference: GPflow's GPR has no LOO predictive and no LOO-CV objective) -------
 * With alpha = K_y^-1 (y - c) and kappa_i = (K_y^-1)_ii, K_y = k(X, X) + diag(noise + s_i) (s: gpso_set_noise_diag, else 0):
 *   mean_i = y_i - alpha_i / kappa_i,  var_i = 1 / kappa_i  (the predictive variance of the OBSERVATION y_i: its own
 *   noise + s_i included, as gpso_predict includes the noise),  lpd_i = (log kappa_i - alpha_i^2 / kappa_i - log 2pi) / 2:
 * what N refits without point i would predict for it at the resident hyper-parameters, in O(N) from what a fit leaves
 * (Rasmussen & Williams, section 5.4.2). */

/* The LOO predictive of the resident fitted posterior: mean[N], var[N], lpd[N] (host float64, each nullable), *loss
 * (nullable) = -sum lpd.  Every context type (GPSO_F32 reads its float factor's alpha and diagonal); after gpso_append /
 * gpso_append_noise it covers the appended points.  Reads only: the posterior stays resident, bit for bit, and the same
 * call gives the same bits.  GPSO_E_STATE when no posterior fitted WITH TARGETS on this context is resident (the condition
 * of gpso_precision_info: a posterior from gpso_set_posterior, gpso_vgp_posterior, gpso_sgpr_posterior, gpso_svgp_posterior
 * or a hand-off has none), or while an asynchronous best-UCB ticket is open; GPSO_E_ARG for N < 2. */
int gpso_loo(gpso_ctx* ctx, double* mean, double* var, double* lpd, double* loss);

/* ONE evaluation of the LOO-CV loss F = -sum lpd_i and its gradient: arguments, the order of grad (n_ls + 3 values,
 * nullable) and the statuses as gpso_fit_eval; *nlml (nullable) receives the NLML at the same theta, which the
 * factorisation gives for free.  dF/dtheta = sum_ab W_ab dK_y,ab/dtheta with W = K_y^-1 diag(c) K_y^-1 - (h alpha^T +
 * alpha h^T) / 2, c_i = (1 + alpha_i^2 / kappa_i) / (2 kappa_i), h = K_y^-1 (alpha / kappa); dF/dnoise = tr W, dF/dc =
 * -sum h: one N^3 product more than the NLML's gradient, then the same tile contraction.
 * GPSO_F64 and GPSO_MIXED contexts (the fit is in double); GPSO_F32: GPSO_E_ARG.  GPSO_E_ARG for N < 2; GPSO_E_NOTPD as
 * gpso_fit_eval.  Runs the factorisation of gpso_fit_eval with a gradient and leaves THE SAME L, L^-1, alpha, packed
 * copies and hyper block, bit for bit: the posterior is predict-ready afterwards.  GPSO_MAT_KINV is still K_y^-1 (the
 * weights are built in scratch the fit has finished with).  N <= 128 with GPSO_OPT_FIT_FUSED_SMALL on: two launches (the
 * one-launch fit, one workgroup for everything else) and no copy operation; otherwise the general sequence -- results
 * agree to rounding.  gpso_last_ms(ctx, 2) covers the whole call.  The same call gives the same bits. */
int gpso_fit_eval_loo(gpso_ctx* ctx, int kernel, const double* lengthscales, int n_ls, double variance, double noise,
                      double mean_c, double* loss, double* grad, double* nlml);
/* The same evaluation in the optimiser's variables: u, train_mean, mean_c_fixed, grad_u, theta_out, the host-side
 * transforms and the chain rule exactly as gpso_fit_eval_u. */
int gpso_fit_eval_loo_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                        double* loss, double* grad_u, double* theta_out, double* nlml);

/* Multi-start hyper-parameter search: the pending evaluations of several L-BFGS-B searches in one launch, one workgroup
 * per theta (fit.hip: small_fit_batch_kernel -- the one-launch fit's arithmetic, bit for bit).
 * gpso_fit_batch_max: how many entries one gpso_fit_eval_u_batch call may hold for the resident data: 256 when the
 * one-launch fit applies (N <= 64, or N <= 128 with a padded D <= 32, and GPSO_OPT_FIT_FUSED_SMALL on), else 0. */
int gpso_fit_batch_max(gpso_ctx* ctx);

/* B evaluations of gpso_fit_eval_u at U[b*nu .. ], nu = n_ls + 2 + (train_mean != 0), in one launch.
 * loss[B]; grad_u[B*nu] (nullable); status[B]: what gpso_fit_eval_u returns for that entry alone -- GPSO_OK,
 * GPSO_E_NOTPD (pivot[B], nullable, gets the failing pivot; -1 otherwise), or GPSO_E_ARG for an entry whose lengthscale
 * or kernel variance does not come out positive (NaN included; such an entry is not launched).
 * Returns GPSO_OK when the launch ran, whatever the entries' verdicts; a failed entry has loss = NaN (and a NaN
 * gradient), and gpso_last_error names the first one.  Refused before anything is done: no data or an asynchronous
 * call in flight (GPSO_E_STATE); b < 1, b > gpso_fit_batch_max, a NULL U / loss / status (GPSO_E_ARG).
 * Leaves the context as it found it: a resident posterior stays resident and predict-ready, bit for bit.
 * gpso_last_ms(ctx, 2) is the launch's device time, as for a fit. */
int gpso_fit_eval_u_batch(gpso_ctx* ctx, int kernel, const double* U, int b, int n_ls, int train_mean,
                          double mean_c_fixed, double* loss, double* grad_u, int* status, int64_t* pivot);

/* Replaces: `model.data = (x, y)` at gpso/gp_surrogate.py:496-498 for an update that KEEPS the hyper-parameters (the
 * reference always re-optimises right after, :500-503, and so refactorises from scratch although N grew by 1-7 points
 * per iteration, gpso/optimisation.py:324-329).  With the posterior of the N points resident at theta
 * (after gpso_fit_eval), the k new points Xnew[k*D], ynew[k] (host float64) extend L, L^-1, alpha, the NLML and the
 * predict-ready copies of L^-1 IN PLACE: L21 = K21 L11^-T from one pass over the resident L^-1, L22 = chol(K22 + noise I -
 * L21 L21^T) in one workgroup, the new rows of L^-1 = -L22^-1 L21 L11^-1 from a second pass -- O(N^2 k) and N^2 s bytes
 * instead of O(N^3); arithmetic in double whatever the context's matrix type.  *nlml (nullable) receives the NLML of
 * the N + k points at theta.
 * Returns GPSO_OK (extended in place); 1 when the posterior of the N + k points was instead REFITTED from scratch at
 * theta -- k > 64 (k > 32 below a padded size of 4096, where the refit is as fast), N + k above the padded size
 * (gpso_padded_n: every buffer's layout changes), or N + k <= 128 (the one-launch fit is the shorter exact update
 * there) -- gpso_last_error then says which; GPSO_E_NOTPD with the failing
 * pivot (N + p) when the appended block is not positive definite: the posterior of the N points then stays resident
 * unchanged; GPSO_E_STATE without a posterior fitted on this context.  The gradient-side K^-1 (GPSO_MAT_KINV) is not
 * extended.  The precision self-test runs again before the next prediction of a float-predict context. */
int gpso_append(gpso_ctx* ctx, const double* Xnew, const double* ynew, int64_t k, double* nlml);

/* gpso_append for points that carry per-point noise (gpso_set_noise_diag): snew[k] (host float64, >= 0; NULL = zeros) is
 * filed behind the resident vector and the appended block is K22 + diag(noise + snew_j) - L21 L21^T.  Statuses, the
 * in-place / refit rule (a refit carries the whole vector along) and what stays resident are gpso_append's; additionally
 * GPSO_E_ARG for a negative or non-finite snew_j.  On a context without a vector, a non-zero snew creates one with zeros
 * for the resident points.  gpso_append itself, on a context with a vector set, appends zeros. */
int gpso_append_noise(gpso_ctx* ctx, const double* Xnew, const double* ynew, const double* snew /* [k], nullable */,
                      int64_t k, double* nlml);

/* Interop / debug: install a posterior computed elsewhere (host float64: X[N*D], L[N*N] row-major
 * lower, alpha[N]) -- the device still derives L^-1 and its tile packing itself.  Mirrors loading
 * saved GPflow parameters into a placeholder model (gpso/gp_surrogate.py:463-473). */
int gpso_set_posterior(gpso_ctx* ctx, const double* X, const double* L, const double* alpha,
                       int64_t n, int d, int kernel, const double* lengthscales, int n_ls,
                       double variance, double noise, double mean_c);

/* ---- variational GP (VGPSurrogate._gp_train, gpso/gp_surrogate.py:536-699) ------------------------------------------
 * GPflow 2's whitened VGP (Gaussian likelihood unless gpso_vgp_set_likelihood says otherwise) on the resident training data (gpso_set_data): q(v) = N(mu, S S^T),
 * f = L v + c, L = chol(k(X, X) + 1e-6 I) (GPflow's default jitter).  u, n_ls, train_mean, mean_c_fixed: the optimiser's
 * vector and transforms exactly as gpso_fit_eval_u (the likelihood variance s2 = 1e-6 + softplus(u[n_ls + 1])).  float64
 * arithmetic throughout: GPSO_F64 and GPSO_MIXED contexts (GPSO_F32: GPSO_E_ARG).  Every call replaces whatever posterior
 * was resident.  q starts at the prior (mu = 0, S = I) whenever the shape of the data changes. */

/* The VGP's likelihood (gpso_vgp_set_likelihood).  GPSO_LIK_GAUSSIAN (the default of every context): the closed-form
 * Gaussian sequence; u[n_ls + 1] is softplus^-1(s2 - 1e-6).  GPSO_LIK_STUDENT_T: gpflow.likelihoods.StudentT(scale, df),
 * df fixed, through GPflow's Gauss-Hermite variational expectations; u[n_ls + 1] is softplus^-1(scale) (GPflow's
 * positive(), no shift), theta_out[n_ls + 1] the scale, grad_u[n_ls + 1] d(-ELBO)/du of it, and gpso_vgp_posterior
 * installs the predictive variance var_f + scale^2 df / (df - 2).  Under either quadrature kind S S^T can exceed I in a
 * direction; the install then serves var_f + delta (k** - |L^-1 k*|^2), delta the first of 0, 1e-8, 2e-8, ... for which
 * I - S S^T / (1 + delta) factorises: never below var_f, at most delta k** above it.  GPSO_LIK_GAUSSIAN_GH: the Gaussian through the
 * same quadrature sequence as the Student-t (u as GPSO_LIK_GAUSSIAN): a check of that sequence against the closed form.
 * GPSO_LIK_BERNOULLI: a GP classifier.  The targets of gpso_set_data are labels: a point is a success
 * (s = +1) iff y > 0.5, otherwise s = -1, and log p(y | f) = log Phi(s f), the EXACT probit -- not GPflow's inv_probit, which
 * mixes a 1e-3 jitter in; the exact one is log-concave.  It has no parameter: slot n_ls + 1 of u stays in the vector (one
 * layout), is decoded as GPSO_LIK_GAUSSIAN's and read by nothing; grad_u[n_ls + 1] is exactly 0.0.  Every gpso_vgp_* call
 * serves it through the quadrature sequence.  gpso_vgp_posterior installs noise 0: gpso_predict and every leaf call on the
 * context then return the LATENT mean and variance of f, and gpso_predict_prob (below) maps them to P(success).  With a
 * log-concave likelihood S S^T stays below I and the shift delta is 0.  The sparse family does not serve it: every gpso_svgp_*
 * call returns GPSO_E_ARG while it is set.  The kind has no df: gpso_vgp_set_likelihood takes df = 0 with it and answers
 * GPSO_E_ARG to any other value (kind 3 with a df was refused before the kind existed, a test of the Student-t's arguments
 * holds the library to that, and so it stays refused: DESIGN.md section 7s). */
#define GPSO_LIK_GAUSSIAN 0
#define GPSO_LIK_STUDENT_T 1
#define GPSO_LIK_GAUSSIAN_GH 2
#define GPSO_LIK_BERNOULLI 3

/* Replaces: choosing the likelihood of gpflow.models.VGP(likelihood=...) (gpso/gp_surrogate.py:536-541).  kind:
 * GPSO_LIK_*; df: the Student-t's degrees of freedom (> 2; 0 under GPSO_LIK_BERNOULLI; ignored otherwise); gh_x[n_gh], gh_w[n_gh]: the Gauss-Hermite
 * nodes and weights of numpy.polynomial.hermite.hermgauss(n_gh) (GPflow's 20 points), 1 <= n_gh <= 64 (both ignored
 * for GPSO_LIK_GAUSSIAN).  Anything else: GPSO_E_ARG.  Takes effect at the next gpso_vgp_* call; q is kept.  The
 * same setting is the likelihood of the sparse variational GP (gpso_svgp_*, below).
 * Under a quadrature likelihood gpso_vgp_natgrad forms the step at the current q (Lambda* = I + L^T diag(a) L,
 * h* = L^T (g_m + a (m - c))); when a factorisation fails -- an indefinite step, e.g. at gross outliers with gamma = 1 --
 * it returns GPSO_E_NOTPD and leaves q exactly as it was (as GPflow), where the Gaussian restarts q at the prior. */
int gpso_vgp_set_likelihood(gpso_ctx* ctx, int kind, double df, int n_gh, const double* gh_x, const double* gh_w);

/* Replaces: assigning q_mu / q_sqrt of a GPflow VGP (gpflow.utilities.multiple_assign, gpso/gp_surrogate.py:667-671).
 * Host float64 mu[n], S[n*n] (row-major, lower triangle read); n must equal the resident N; both NULL: the prior. */
int gpso_vgp_set_q(gpso_ctx* ctx, const double* mu, const double* S, int64_t n);
/* Reading q_mu / q_sqrt back (gpflow.utilities.parameter_dict, gpso/gp_surrogate.py:690-692): mu[N], S[N*N] (nullable). */
int gpso_vgp_get_q(gpso_ctx* ctx, double* mu, double* S);
/* Replaces: assigning grown data to a VGP whose q keeps its old size (gpso/gp_surrogate.py:630-633; GPflow's
 * update_vgp_data).  After gpso_set_data with the rows q was made for FIRST, in the same order: q keeps its leading block
 * and the new rows get the prior (mu = 0, an identity block of S), on the device. */
int gpso_vgp_extend_q(gpso_ctx* ctx);
/* Replaces: natgrad_optimiser.minimize(training_loss, [(q_mu, q_sqrt)]) (gpso/gp_surrogate.py:639-642): one natural-gradient
 * step of length gamma in (0, 1] on q at theta.  GPSO_E_NOTPD (q then restarts at the prior) when a factorisation fails. */
int gpso_vgp_natgrad(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                     double gamma);
/* Replaces: ONE evaluation of the VGP training_loss (-ELBO) and its reverse-mode gradient in the trainable variables inside
 * optimiser.minimize (gpso/gp_surrogate.py:643-646), at fixed q.  *loss; grad_u (nullable) [n_ls + 2 + (train_mean != 0)];
 * theta_out (nullable) [n_ls + 3] = (lengthscales..., variance, s2, mean). */
int gpso_vgp_elbo_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                    double* loss, double* grad_u, double* theta_out);
/* Replaces: the predict_y / predict_f of the trained VGP (gpso/gp_surrogate.py:298, 325).  Installs the predictive at theta
 * as the resident posterior: mean = k*^T L^-T mu + c, var = k** - |C k*|^2 + s2 with C = R L^-1, I - S S^T = R^T R -- the
 * form every predict path evaluates, so gpso_predict, gpso_best_ucb (+ _begin / _end, _grow), the sharded and hand-off
 * calls serve it unchanged.  Like gpso_set_posterior the installed posterior carries no GPR targets: the float-predict
 * self-test is skipped (generation in double) and gpso_append returns GPSO_E_STATE.  The getters follow the installed form:
 * GPSO_MAT_LINV returns C and GPSO_VEC_ALPHA returns L^-T mu; GPSO_MAT_CHOL and GPSO_VEC_WHITE return GPSO_E_STATE. */
int gpso_vgp_posterior(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed);

/* ---- sparse GP regression on inducing points (no counterpart in the reference: gpflow.models.SGPR, Titsias 2009) -------
 * GPflow 2's SGPR, Gaussian likelihood, with M inducing points Z summarising the N resident training rows (fixed in the
 * calls of this block; the block "at a moving Z" below trains them):
 * Kuu = k(Z, Z) + 1e-6 I, Lu = chol Kuu, A = Lu^-1 k(Z, X) / sigma, B = I + A A^T, LB = chol B, cv = LB^-1 A (y - c) / sigma;
 * training costs O(N M^2), a prediction O(M^2) whatever N.  u, n_ls, train_mean, mean_c_fixed: as
 * gpso_fit_eval_u (s2 = 1e-6 + softplus(u[n_ls + 1])).  float64 throughout: GPSO_F64 and GPSO_MIXED contexts (GPSO_F32:
 * GPSO_E_ARG).  Sequence: gpso_set_data (X, y), then gpso_sgpr_set_inducing or gpso_sgpr_select_inducing, then any number
 * of gpso_sgpr_bound_u, then gpso_sgpr_posterior; a call out of that order returns GPSO_E_STATE.
 * WHAT THE CONTEXT DESCRIBES AFTERWARDS: setting the inducing points moves the training data into SGPR buffers of its own and
 * makes Z the context's resident rows.  From then on gpso_problem_shape reports (M, D), gpso_padded_n the padding of M, and
 * after gpso_sgpr_posterior the getters return the installed form over the rows Z: GPSO_MAT_LINV the M x M matrix C,
 * GPSO_VEC_ALPHA beta (M values); GPSO_MAT_CHOL / GPSO_VEC_WHITE return GPSO_E_STATE and gpso_append returns GPSO_E_STATE
 * (set the grown data and train again).  The next gpso_set_data replaces the data and drops Z; a gpso_fit_eval or
 * gpso_set_posterior on the context ends the SGPR sequence too (the resident rows are then no inducing points). */

/* Z[m * D] row-major, used as given (1 <= m <= 65536; m > N is allowed).  May be called again to replace Z for the same
 * data.  A call rejected for its arguments or its place in the sequence (GPSO_E_ARG / GPSO_E_STATE) leaves the context as it
 * was; a HIP or allocation failure inside it leaves the context without data (gpso_set_data again). */
int gpso_sgpr_set_inducing(gpso_ctx* ctx, const double* Z, int64_t m);
/* Greedy conditional-variance selection of m <= N training rows ON THE DEVICE (pivoted partial Cholesky of k(X, X) at the
 * kernel hyper-parameters of u; only u[0 .. n_ls] are read): d_i = variance; m times: p = arg-max d over the unpicked rows,
 * the lowest index on exact ties; l = (k(X, x_p) - L L[p]^T) / sqrt(d_p); d -= l^2.  O(N m^2).  The picked rows become Z;
 * idx_out (nullable) [m] receives their indices in pick order.  Arguments are checked first (a rejected call leaves the
 * context as it was); after that the call replaces whatever posterior was resident.  When the largest remaining d falls to
 * 1e-12 variance or below before m rows are picked -- k(X, X) numerically of rank < m: duplicated rows, very long
 * lengthscales, m close to N -- the call returns GPSO_E_NOTPD with the rank reached in gpso_last_error and sets no Z. */
int gpso_sgpr_select_inducing(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int64_t m, int64_t* idx_out);
/* Z (nullable) [M * D], *m (nullable) = M, *n_data (nullable) = N of the training data held beside it. */
int gpso_sgpr_get_inducing(gpso_ctx* ctx, double* Z, int64_t* m, int64_t* n_data);
/* The intermediates of the last successful gpso_sgpr_bound_u, for checks against a reference (tests): out receives
 * GPSO_SGPR_KUF: k(Z, X) [M * N] row-major; GPSO_SGPR_LU: Lu [M * M]; GPSO_SGPR_LB: LB [M * M] (lower, zero above);
 * GPSO_SGPR_CV: cv [M].  GPSO_E_STATE once any call other than a getter has followed that evaluation. */
#define GPSO_SGPR_KUF 0
#define GPSO_SGPR_LU 1
#define GPSO_SGPR_LB 2
#define GPSO_SGPR_CV 3
int gpso_sgpr_get_factor(gpso_ctx* ctx, int which, double* out);
/* ONE evaluation of SGPR.training_loss (-bound of Titsias) and its gradient in the trainable variables, Z fixed.  *loss;
 * grad_u (nullable) [n_ls + 2 + (train_mean != 0)]; theta_out (nullable) [n_ls + 3] = (lengthscales..., variance, s2, mean).
 * GPSO_E_NOTPD names the matrix (Kuu or B) and the pivot.  Replaces whatever posterior was resident. */
int gpso_sgpr_bound_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                      double* loss, double* grad_u, double* theta_out);
/* SGPR.predict_y at theta, installed as the resident posterior over the rows Z: mean = k*u^T beta + c with
 * beta = Lu^-T LB^-T cv, var = k** - |C k*u|^2 + s2 with C = R Lu^-1, I - B^-1 = R^T R -- the form every predict path
 * evaluates, so gpso_predict, gpso_best_ucb (+ _begin / _end, _grow), the sharded and hand-off calls serve it unchanged.
 * Where I - B^-1 does not factor (N < M, duplicated rows of Z) the install serves var + delta (k** - |Lu^-1 k*u|^2) with
 * delta the first of 0, 1e-8, 2e-8, ... for which I - B^-1 / (1 + delta) factors: never below the exact variance, at most
 * delta k** above it, exact when delta = 0 (DESIGN.md sections 7a.1, 7b).  *delta_out (nullable) = delta. */
int gpso_sgpr_posterior(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                        double* delta_out);

/* ---- sparse variational GP on inducing points (GPflow 2 SVGP, whitened, full q_sqrt, full batch) ---------------------
 * q(v) = N(mu, S S^T) over the M inducing values, f(x) = k(x, Z) Lu^-T v + c, Lu = chol(k(Z, Z) + 1e-6 I), trained against
 * the likelihood of gpso_vgp_set_likelihood (that call sets the likelihood of the VGP AND of the SVGP: Gaussian in closed
 * form, Student-t or the Gaussian through 20-point Gauss-Hermite quadrature).  Training costs O(N M^2), a prediction
 * O(M^2).  Z and the training data are the SGPR's: gpso_set_data, then gpso_sgpr_set_inducing or
 * gpso_sgpr_select_inducing; Z is then the context's resident rows (see the SGPR block above).  Setting Z starts q at the
 * prior (mu = 0, S = I); the next gpso_set_data drops Z and q.  A call before Z is set returns GPSO_E_STATE, a
 * GPSO_F32 context GPSO_E_ARG.  u, n_ls, train_mean, mean_c_fixed: the optimiser's vector and transforms exactly as
 * gpso_vgp_elbo_u, the likelihood slot u[n_ls + 1] included (the Student-t scale, or 1e-6 + softplus for the Gaussian
 * variance).  The SGPR's and the VGP's own state and entry points are untouched by these calls. */

/* Start q: noise_variance <= 0: the prior (u may be NULL); else the conjugate start -- one natural-gradient step of
 * length 1 with a Gaussian likelihood of variance noise_variance, at the theta of u, whatever the context's likelihood
 * (SVGPSurrogate passes the Student-t's predictive variance scale^2 df / (df - 2)).  GPSO_E_NOTPD: q unchanged. */
int gpso_svgp_init_q(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                     double noise_variance);
/* Host float64 mu[m], S[m*m] (row-major, lower triangle read) of the resident Z (m must equal M); both NULL: the prior.
 * gpso_svgp_get_q copies q out (either pointer nullable). */
int gpso_svgp_set_q(gpso_ctx* ctx, const double* mu, const double* S, int64_t m);
int gpso_svgp_get_q(gpso_ctx* ctx, double* mu /* [M] */, double* S /* [M*M] */);
/* One natural-gradient step of length gamma in (0, 1] on q at theta (GPflow's NaturalGradient): with A = Lu^-1 Kuf and
 * the per-point g_m = dVE/dm, a = -2 dVE/dv at the current q, Lambda* = I + A diag(a) A^T, h* = A (g_m + a (m - c)), mixed
 * with q's natural parameters by gamma.  When a factorisation fails (an indefinite step: gross outliers under the
 * Student-t) it returns GPSO_E_NOTPD and leaves q exactly as it was, for every likelihood. */
int gpso_svgp_natgrad(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                      double gamma);
/* -ELBO = -sum_i VE_i(m_i, v_i) + KL(q || N(0, I)) at fixed q and Z, m_i = A_i^T mu + c, v_i = variance - |A_i|^2 +
 * |S^T A_i|^2; grad_u (nullable) d(-ELBO)/du; theta_out[n_ls + 3] (nullable) (lengthscales..., variance, likelihood
 * parameter, c).  Deterministic: the same call gives the same bits. */
int gpso_svgp_elbo_u(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                     double* loss, double* grad_u, double* theta_out);
/* Install the SVGP predictive over the rows Z: mean = k*u^T Lu^-T mu + c, var = k** - k*u^T Lu^-T (I - S S^T) Lu^-1 k*u
 * + the likelihood's variance (s2, or scale^2 df / (df - 2) for the Student-t) -- the VGP's install with L := Lu, delta
 * shift included (where I - S S^T does not factor: var + delta (k** - |Lu^-1 k*u|^2), delta the first of 0, 1e-8, 2e-8, ...
 * for which I - S S^T / (1 + delta) does; *delta_out, nullable).  Every predict path then serves it; the getters return
 * the installed form as after gpso_sgpr_posterior, and gpso_append returns GPSO_E_STATE. */
int gpso_svgp_posterior(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                        double* delta_out);

/* ---- the sparse models at a moving Z: training the inducing points (GPflow's default: inducing_variable.Z trainable) -----
 * The entry points above keep Z fixed; these evaluate at a Z the optimiser moves, and return the gradient in it (DESIGN.md
 * section 7d).  Z[M * D] (row-major; nullable: keep the resident Z) REPLACES THE RESIDENT INDUCING ROWS IN PLACE: same M, the
 * training data buffers untouched, no allocation, no upload of X or y, and the SVGP's q kept (it is whitened: valid at any
 * Z).  WHAT STAYS RESIDENT: the new Z -- gpso_sgpr_get_inducing returns it (n_data unchanged) and gpso_sgpr_bound_u,
 * gpso_sgpr_posterior, gpso_svgp_natgrad, gpso_svgp_elbo_u and gpso_svgp_posterior then work at it; whatever posterior was
 * resident is replaced, as by the fixed-Z evaluations.  With Z = NULL, or Z equal to the resident rows, *loss and grad_u are
 * bit for bit those of the fixed-Z entry point; the same call gives the same bits (fixed-order reductions, no atomics).
 * grad_z (nullable) [M * D] = d loss / d Z:  with zs = Z / l, xs = X / l, k' = dk/dr^2, Vc = dF/dKuf (.) k'(Z, X) and
 * Vu = 2 dF/dKuu (.) k'(Z, Z) (diagonal 0),  dF/dZ[m, d] = (2 / l_d) (zs[m, d] (rowsum Vc + rowsum Vu)[m] - (Vc xs + Vu zs)[m, d]).
 * COINCIDENT PAIRS: a pair with r^2 <= 1e-36 (a row of Z equal to a row of X, or to another row of Z) contributes zero, as
 * in GPflow; that is the exact derivative for the Matern-3/2, -5/2 and the squared exponential, and the convention at the
 * Matern-1/2's kink.
 * ERRORS: a call rejected for its arguments or its place in the sequence -- before Z is set: GPSO_E_STATE; a GPSO_F32
 * context, a non-finite value in Z, a non-positive hyper-parameter: GPSO_E_ARG -- leaves the context as it was, the
 * resident Z included.  GPSO_E_NOTPD names the matrix and the pivot as the fixed-Z calls do (two rows of Z collapsing onto
 * each other can make Kuu singular beyond the 1e-6 jitter); the new Z is resident then. */

/* Replace the resident inducing rows by Z[M * D] and evaluate nothing. */
int gpso_sgpr_move_inducing(gpso_ctx* ctx, const double* Z);
/* gpso_sgpr_bound_u at Z, and the gradient of the loss in Z. */
int gpso_sgpr_bound_uz(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                       const double* Z /* [M*D], nullable */, double* loss, double* grad_u,
                       double* grad_z /* [M*D], nullable */, double* theta_out);
/* gpso_svgp_elbo_u at Z (q fixed), and the gradient of the loss in Z. */
int gpso_svgp_elbo_uz(gpso_ctx* ctx, int kernel, const double* u, int n_ls, int train_mean, double mean_c_fixed,
                      const double* Z /* [M*D], nullable */, double* loss, double* grad_u,
                      double* grad_z /* [M*D], nullable */, double* theta_out);

/* ---- predict (gpflow_model.predict_y users) ----------------------------------------------- */

/* Replaces: gpflow_model.predict_y(coords) at gpso/gp_surrogate.py:298 (gp_predict) and
 * gpso/plotting.py:351-353.  Xs[M*D] in xs_dtype (GPSO_F64|GPSO_F32) living in xs_mem;
 * mean[M], var[M] float64 living in out_mem; var INCLUDES the noise variance. */
int gpso_predict(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double* mean,
                 double* var, int out_mem);

/* No counterpart in the reference (a GPflow user differentiates predict_f / predict_y by tf.GradientTape).
 * gpso_predict's mean and var at the m test points AND their gradients in the test points' coordinates, as passed (not
 * scaled by the lengthscales): with xs = x / l, r2_i = |xs* - xs_i|^2 formed from direct differences in double, k_i =
 * k(r2_i), k'_i = dk/dr2, v = C k*, w = C^T v,
 *   mean = alpha^T k* + c,  var = variance - |v|^2 + noise (noise INCLUDED, as gpso_predict),
 *   dmean/dx*_d = sum_i alpha_i g_id,  dvar/dx*_d = -2 sum_i w_i g_id,  g_id = 2 k'_i (xs*_d - xs_i,d) / l_d
 * (DESIGN.md section 7h).  A pair with r2 <= 1e-36 contributes zero to the gradients: exact for the squared exponential and
 * the Matern-3/2 and -5/2, the convention at the Matern-1/2's kink (as gpso_sgpr_bound_uz).
 * xs, xs_dtype, xs_mem, out_mem as gpso_predict; mean[m], var[m], dmean[m * D], dvar[m * D] (row-major) float64 living in
 * out_mem, each nullable.  Reads the dense fit-type factor (GPSO_MAT_LINV), so every output is double-class on GPSO_F64 AND
 * GPSO_MIXED contexts, also where gpso_predict is float-class; GPSO_F32: GPSO_E_ARG.  Serves every resident posterior that
 * has its dense factor: fitted (after gpso_append / gpso_append_noise too), gpso_set_posterior, gpso_vgp_posterior,
 * gpso_sgpr_posterior and gpso_svgp_posterior (the sparse ones over the rows Z, a shift delta included as installed).
 * GPSO_E_STATE: no posterior, a posterior from a hand-off (the dense factor may not have travelled), or an asynchronous
 * best-UCB ticket open.  GPSO_E_ARG: a GPSO_F32 context, m < 1, xs NULL, or all four outputs NULL.
 * Reads only: the posterior, its packed copies and the hyper block stay bit for bit; the precision self-test is neither run
 * nor consumed; the same call gives the same bits, and a test point's bits do not depend on the rest of the batch.
 * gpso_last_ms(ctx, 1) covers the call when timing is on; gpso_last_count(ctx, 0) and (ctx, 1) are m, as after gpso_predict. */
int gpso_predict_grad(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m,
                      double* mean /* [m], nullable */, double* var /* [m], nullable */,
                      double* dmean /* [m*D] row-major, nullable */, double* dvar /* [m*D], nullable */, int out_mem);

/* Replaces: gpflow_model.predict_f(Xnew, full_cov=True) -- and predict_y's, by way of diag_add -- for the reference's users
 * (gpso/gp_surrogate.py hands them the GPflow model).  The JOINT predictive at the m test points: with V = C K* (N x m,
 * K*[i, a] = k(x_i, t_a)) and K**[a, b] = k(t_a, t_b) from direct differences in double,
 *   mean = K*^T alpha + c,   cov = K** - V^T V + diag_add I   (m x m row-major, EXACTLY symmetric)
 * (DESIGN.md section 7i).  diag_add is an absolute term the caller chooses: 0 for the latent f, the family's predictive noise
 * for y, plus a jitter where a factorisation follows; the library adds no noise of its own here.
 * xs, xs_dtype, xs_mem, out_mem as gpso_predict; mean[m] (nullable) and cov[m * m] float64 living in out_mem.  Contexts,
 * posteriors and statuses as gpso_predict_grad: GPSO_F64 and GPSO_MIXED contexts (GPSO_F32: GPSO_E_ARG); every resident
 * posterior that has its dense factor; GPSO_E_STATE without a posterior, for a posterior from a hand-off and while an
 * asynchronous best-UCB ticket is open.  GPSO_E_ARG also for m < 1, m > 1024 (the joint covariance of more test points is out
 * of scope: the workspace and the factorisation are sized for one chunk), xs or cov NULL, a diag_add that is not finite.
 * Reads only: the posterior, its packed copies, the hyper block, the self-test's verdicts and gpso_posterior_hash stay as
 * they are; the same call gives the same bits.  gpso_last_ms(ctx, 1) and gpso_last_count as after gpso_predict_grad. */
int gpso_predict_joint(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add,
                       double* mean /* [m], nullable */, double* cov /* [m*m] row-major */, int out_mem);

/* Replaces: gpflow_model.predict_f_samples(Xnew, num_samples) for the reference's users, and the arg-max of every draw over
 * the m test points (Thompson sampling over a set of candidates).  With gpso_predict_joint's mean and cov (diag_add
 * included: the jitter, and the predictive noise for draws of y), L = chol(cov):
 *   samples[q, :] = mean + L z[q, :]   for the s rows of z,
 *   best_idx[q] = the index of the highest entry of draw q (the lowest index on ties), best_val[q] that entry.
 * z[s * m]: standard normals from the CALLER, host memory (there is no random generator on the device: draws are
 * reproducible from a seed on the host).  samples[s * m], best_idx[s], best_val[s]: host memory, each nullable, not all
 * three -- with samples NULL the draws never leave the device.  Conditions and statuses as gpso_predict_joint; GPSO_E_ARG
 * also for s < 1, s > 2^20 (draw in several calls), s * m > 2^31 and z NULL.  GPSO_E_NOTPD: the Cholesky of cov met a pivot that is not positive --
 * gpso_last_error names it, the outputs then hold nothing of use and a larger diag_add (jitter) is the remedy; the posterior
 * is untouched and serves the next call.  Reads only, as gpso_predict_joint. */
int gpso_sample_joint(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double diag_add,
                      const double* z /* [s*m] host */, int64_t s, double* samples /* [s*m] host, nullable */,
                      int64_t* best_idx /* [s], nullable */, double* best_val /* [s], nullable */);

/* Pathwise posterior draws (no counterpart in the reference): s posterior FUNCTIONS of the resident
 * fitted exact GP, kept on the context (the "path set") and evaluated by gpso_paths_eval at any number of points -- Matheron's
 * rule over a random-Fourier-feature prior, no m x m object anywhere.  With phi_j(x) = sqrt(2 variance / f) cos(omega_j . x/l
 * + phase_j),
 *   value[q, a] = c + sum_{j < f} phi_j(t_a) w[q, j] + sum_{i < N} k(x_i, t_a) v[i, q],   v = L^-T L^-1 R,
 *   R[i, q] = (y_i - c) - sum_j phi_j(x_i) w[q, j] - sqrt(noise + s_i) eps[q, i]
 * (k from direct differences in double, s_i the gpso_set_noise_diag vector or 0).  With w = 0 and eps = 0 a path is the
 * posterior mean.  omega[f * D]: frequencies in SCALED coordinates, drawn from the kernel's spectral density (standard normal
 * for the squared exponential; Student-t with 2 nu degrees of freedom for the Matern-nu); phase[f] uniform on [0, 2 pi);
 * w[s * f] feature weights and eps[s * N] (nullable = zeros) standard normals -- all host float64, all from the CALLER (no
 * generator on the device, as gpso_sample_joint).
 * Posteriors: one fitted with targets on this context (gpso_loo's condition; after gpso_append / gpso_append_noise too), on
 * GPSO_F64 and GPSO_MIXED contexts.  GPSO_E_ARG: a GPSO_F32 context, s outside [1, 256], f outside [1, 65536], a NULL omega /
 * phase / w, an input that is not finite.  GPSO_E_STATE: no posterior, an installed, adopted or variational one (no targets;
 * gpso_paths_draw_q draws from a variational one), or an asynchronous best-UCB ticket open.  A call that fails or is refused
 * leaves the previous path set as it was.
 * The set lives until the posterior changes: every fit, append, gpso_set_data, gpso_set_noise_diag, install and hand-off ends
 * it.  Reads only: the posterior, its packed copies, the hyper block, the self-test's verdicts and gpso_posterior_hash stay
 * bit for bit; the same call gives the same set, and a draw's bits do not depend on s.  gpso_last_ms(ctx, 1) covers the call. */
int gpso_paths_draw(gpso_ctx* ctx, const double* omega /* [f*D] host */, const double* phase /* [f] host */, int64_t f,
                    const double* w /* [s*f] host */, const double* eps /* [s*N] host, nullable */, int64_t s);

/* Pathwise draws of the VARIATIONAL posteriors (Wilson et al. 2020, section 3.2, in GPflow's whitened
 * form): the path set of the posterior that gpso_vgp_posterior, gpso_sgpr_posterior or gpso_svgp_posterior installed, over
 * its n resident rows Zr (the training rows of a VGP, the inducing points Z of the sparse two).  With Lu = chol(k(Zr, Zr) +
 * 1e-6 I), the whitened q(v) = N(mu, Q Q^T) and beta = Lu^-T mu,
 *   value[q, a] = c + sum_{j < f} phi_j(t_a) w[q, j] + sum_{i < n} k(Zr_i, t_a) v[i, q],
 *   v[:, q] = beta + Lu^-T (Q eps[q, :] - Lu^-1 P[:, q]),   P[i, q] = sum_j phi_j(Zr_i) w[q, j]
 * (Q: the lower root of q for the VGP and the SVGP, LB^-T for the SGPR).  With w = 0 and eps = 0 a path is the family's
 * predictive mean; the draws come from q itself: the shift delta of a Student-t or singular-B install is in the served
 * variance only, never in a path.  omega, phase, w as gpso_paths_draw; eps[s * n] (nullable = zeros) the whitened normals, n
 * the RESIDENT row count (gpso_problem_shape).  The set replaces whatever set is resident and is served by gpso_paths_eval /
 * gpso_paths_info; it costs O(n + f) a point whatever the size of the training set behind a sparse posterior.
 * GPSO_E_ARG: as gpso_paths_draw.  GPSO_E_STATE: no posterior, a fitted one (gpso_paths_draw's), an installed or adopted one,
 * the install's factors no longer resident, or an asynchronous best-UCB ticket open.  A call that fails or is refused leaves
 * the previous path set as it was.  The set lives until the posterior changes: every variational evaluation, natural-gradient
 * step, install, gpso_vgp_set_q / gpso_svgp_set_q, move of Z, gpso_set_data and hand-off ends it (and the factors' residency
 * with it); gpso_predict, gpso_predict_grad, gpso_predict_joint and gpso_sample_joint touch none of the factors, so a draw after
 * them gives the bits of a draw right after the install.  Reads only, as gpso_paths_draw (it writes scratch of the
 * install's -- vA, vB, the factorisation's work matrix -- to rebuild Lu^-1); a draw's bits do not depend on s.
 * gpso_last_ms(ctx, 1) covers the call. */
int gpso_paths_draw_q(gpso_ctx* ctx, const double* omega /* [f*D] host */, const double* phase /* [f] host */, int64_t f,
                      const double* w /* [s*f] host */, const double* eps /* [s*n] host, nullable */, int64_t s);

/* Evaluates the resident path set at m points (xs, xs_dtype, xs_mem as gpso_predict; any m >= 1, worked off in chunks of
 * 16384 points inside, so the workspace does not grow with m): values[s * m] (draw-major, float64 living in out_mem, nullable);
 * best_idx / best_val [s * nseg] (host, nullable; not all three NULL): per draw and segment the highest value and its index
 * relative to the segment start, the lowest index on ties; an empty segment gives -1 and a NaN.  seg_off / nseg as
 * gpso_best_ucb (nseg <= 1024).  With values NULL the values never leave the device.
 * GPSO_E_STATE: no valid path set (none drawn, or the posterior changed since), or an asynchronous best-UCB ticket open.
 * GPSO_E_ARG: a GPSO_F32 context, m < 1, xs NULL, all three outputs NULL, a bad seg_off / nseg.
 * Reads only, as gpso_paths_draw.  The same call gives the same bits; a point's value bits depend neither on the rest of the
 * batch, nor on its place in it, nor on how m is chunked.  gpso_last_ms(ctx, 1) covers the call; gpso_last_count(ctx, 0) and
 * (ctx, 1) are m. */
int gpso_paths_eval(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
                    double* values /* [s*m], nullable */, int out_mem, int64_t* best_idx /* [s*nseg] host, nullable */,
                    double* best_val /* [s*nseg] host, nullable */);

/* Draws and features of the valid path set; 0, 0 when none is resident. */
int gpso_paths_info(gpso_ctx* ctx, int64_t* s, int64_t* f);

/* Monte-Carlo batch acquisition over the resident path set (no counterpart in the reference): q rows
 * of a batch picked by sequential greedy selection of the sample-average qEI / qNoisyEI / qPI over the S draws, which are
 * the fixed base samples.  With V[s][j] the value of draw s at row j (gpso_paths_eval's bits) and t[s] the draw's bar:
 *   GPSO_MC_QEI: gain(j) = (1/S) sum_s max(V[s][j] - t[s] - x[s], 0) -- draw order, double, nothing fused, one division.
 *     x[s] is xi until a pick (or a pending point) has cleared the draw's bar by more than xi, and 0 from then on.  After
 *     pick p the bar of every cleared draw moves: t[s] = max(t[s], V[s][p]); a draw the picks have not cleared keeps its
 *     bar.  At xi = 0 that is max(V - t, 0) and t = max(t, V[p]) in every draw.  The margin is charged once per draw, so
 *     the gains add up to the batch's value (below) whatever xi is.  The pick's fantasy therefore moves the means: a draw
 *     in which the pick is high has a higher bar from then on.
 *   GPSO_MC_QPI: gain(j) = (1/S) #{ s : not yet improved, V[s][j] > t[s] + xi } -- an integer count, one division.  The bars
 *     stay; a draw is improved once a pick (or a pending point) has cleared its original bar.
 *   Initial bars: incumbent_s[s] (host, [S]) when given, else acq->incumbent for every draw.  qNoisyEI is GPSO_MC_QEI with
 *     incumbent_s[s] = the maximum of draw s over the evaluated points (gpso_paths_eval's best_val over them).
 *   pending [b * D] (host float64, nullable with b = 0): points still being evaluated.  They are evaluated by the same
 *     kernel as b more columns and folded into the bars (QEI) or the flags (QPI) before round 0, in their order, as picks
 *     are; they are never candidates.
 *   Arg-max: the first maximum wins a tie and a NaN beats every number (gpso_best_batch's rule).  A row with a NaN among
 *     its terms (QPI: anywhere in its column) has a NaN gain.
 *   A picked row is retired.  A row whose column equals the pick's in every draw has gain 0 from then on, so it is not
 *     picked again (no coordinate comparison is made).
 *   Ending: round 0's pick is always reported; a later round whose best gain is not > 0 ends the batch without reporting
 *     that pick; a NaN gain is reported and ends the batch; no live row left ends it.  *n_picked <= q says how many entries
 *     are valid; the rest of idx / gain / batch_value is not written.
 *   idx / gain / batch_value [q] (host; the last two nullable): the pick, the gain it was ranked by, and the running sum of
 *     the gains in pick order -- for QEI the batch's sample-average value (1/S) sum_s max over the picks of the improvement.
 *   gain0 [m] (float64 living in out_mem, nullable): every row's round-0 gain -- at q = 1 the plain sample-average EI / PI.
 * gpso_paths_batch_host: the same rounds on the host from given values [s * (m + b)] (draw-major: row s holds the m
 *   candidates, then the b pending columns) -- the same header, the same roundings, the same end rules; no context and no
 *   GPU.  A device gain has its bits on the same values.  incumbent_s as above; gain / batch_value / gain0 nullable.
 *   Returns GPSO_OK or GPSO_E_ARG (a NULL acq / values / idx / n_picked, s outside [1, 256], and the bounds below).
 * GPSO_E_STATE (gpso_paths_eval's conditions): no valid path set, or an asynchronous best-UCB ticket open.
 * GPSO_E_ARG: a GPSO_F32 context; m < 1; q outside [1, 64]; b outside [0, 64], or b > 0 with pending NULL; S * (m + b) >
 *   2^26; NULL xs / acq / idx / n_picked; an unknown kind; a xi, incumbent (where it is read) or incumbent_s entry that is
 *   NaN.  +-inf bars are allowed: -inf makes round 0 rank by +inf ties, and the first row wins.
 * Reads only: the posterior, its packed copies, the hyper block, the self-test's verdicts, gpso_posterior_hash and the path
 * set stay bit for bit (a gpso_paths_eval after the call returns the bits of one before it); the workspace -- S * (m + b)
 * doubles, padded -- is the call's own and grows only.  The same call gives the same bits; a row's gain0 bits depend neither
 * on the rest of the batch nor on its place in it.  gpso_last_ms(ctx, 1) covers the call and (ctx, 0) its rounds alone --
 * the fold of the pending columns, the q round and fold launches, the read-back of the picks; the rest is stage A --;
 * gpso_last_count(ctx, 0) and (ctx, 1) are m.
 * Out of scope: segments, grown leaves (_grow), the asynchronous _begin / _end pair, sharded groups. */
#define GPSO_MC_QEI 0
#define GPSO_MC_QPI 1
typedef struct {
  int kind;         /* GPSO_MC_QEI, GPSO_MC_QPI */
  double xi;        /* improvement margin, in the paths' (latent) units */
  double incumbent; /* the bar of every draw when incumbent_s is NULL */
} gpso_mcacq;
int gpso_paths_best_batch(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_mcacq* acq,
                          const double* incumbent_s /* [S] host, nullable */, const double* pending /* [b*D] host, nullable */,
                          int b, int q, int64_t* idx, double* gain, double* batch_value /* [q] host, last two nullable */,
                          int* n_picked, double* gain0 /* [m], nullable */, int out_mem);
int gpso_paths_batch_host(const gpso_mcacq* acq, const double* values /* [s*(m+b)] draw-major */, int64_t s, int64_t m, int b,
                          const double* incumbent_s, int q, int64_t* idx, double* gain, double* batch_value, int* n_picked,
                          double* gain0);

/* Replaces: GPSurrogate.gp_eval_best_ucb (gpso/gp_surrogate.py:313-328): predict_y, then
 * ucb = mean + varsigma * VAR, then first arg-max -- per segment.  seg_off[nseg+1] (host) delimits
 * independent leaf batches (NULL with nseg = 1 means one segment [0, M)); outputs (host, nseg each):
 * idx = winner's row index relative to its segment start, and its mean / var / ucb. */
int gpso_best_ucb(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m,
                  const int64_t* seg_off, int nseg, double varsigma, int64_t* idx, double* mean,
                  double* var, double* ucb);

/* The same calls as a non-blocking pair (round 5).  _begin checks and enqueues the call on the context's stream and
 * returns a ticket (0 or 1) without waiting, or a negative status; gpso_best_ucb_end(ticket) waits for THAT call and fills
 * the outputs (nseg each, nullable).  Two calls may be in flight on a context: the device work of the second queues up
 * behind the first while the host still reads the first's result, so the GPU does not idle over the host's round trip.
 * The reference's loop (gpso/optimisation.py:366-382) is synchronous -- the blocking calls above are _begin + _end --;
 * callers with several independent batches (conditional grids, one batch per tree level of several trees) overlap them.
 * Between a _begin and its _end the leaves buffer (GPSO_MEM_DEVICE) must stay untouched; host leaves are copied before
 * _begin returns.  nseg <= 1024.  Calls that replace or change the posterior (gpso_set_data, gpso_fit_eval, gpso_append,
 * gpso_set_posterior, gpso_alloc_posterior) return GPSO_E_STATE while a ticket is open.  gpso_last_ms is not updated by
 * asynchronous calls. */
int gpso_best_ucb_begin(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off,
                        int nseg, double varsigma);
int gpso_best_ucb_grow_begin(gpso_ctx* ctx, const double* bounds, int nseg, int depth, double varsigma);
int gpso_best_ucb_end(gpso_ctx* ctx, int ticket, int64_t* idx, double* mean, double* var, double* ucb);

/* Diagnostic: the mean pass and the screen of a screened call (GPSO_OPT_SCREEN) alone, whatever the option and the batch
 * size say.  Per leaf (host, m each, nullable): my -- the mean, bit for bit gpso_predict's --, ub -- what the leaf's ucb cannot
 * exceed: my + varsigma * (variance + noise) in the finalize stage's roundings --, flag -- 1.0: the leaf survives.
 * info (3 doubles, nullable): the survivors' count, the threshold T', and how many survivors a call has room for.
 * GPSO_E_STATE where no call on this context, batch and varsigma could be screened. */
int gpso_screen_probe(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double varsigma, double* my,
                      double* ub, double* flag, double* info);
/* Diagnostic: the compact list the last gpso_screen_probe on this context left for the survivors' launch, as it stood behind
 * the probe.  *live (nullable): its rows, min(survivors, room).  key[0 .. min(live, max_rows)): the survivors' indices in the
 * probed batch, ascending; rows[..][D]: their unscaled float rows.  GPSO_E_STATE before the first probe. */
int gpso_screen_list(gpso_ctx* ctx, int64_t max_rows, int64_t* key, float* rows, int64_t* live);
/* The screen's arithmetic on the host (csrc/screen.hpp, the header the device code includes; no context, no GPU):
 * ucb[i] = the finalize stage's ucb of a leaf with mean my[i] and variance share v[i] (NULL: zeros), ub[i] = its bound;
 * the threshold from the largest finite mean; the survive test; the acceptance test of the survivors' winner. */
int gpso_screen_eval_host(const double* my, const double* v, double variance, double noise, double varsigma, int64_t n,
                          double* ucb /* nullable */, double* ub /* nullable */);
double gpso_screen_threshold_host(double max_my, double noise, double varsigma);
int gpso_screen_survives_host(double my, double ub, double threshold);
int gpso_screen_accepts_host(double u_star, double threshold, int64_t count, int64_t cap);
/* The compaction's partition of a batch of m leaves: part w of `parts` owns the leaves [*lo, *hi) -- ascending, every leaf
 * in exactly one part, every range but the last non-empty one a multiple of 64 long; and how many parts a batch is given. */
int gpso_screen_partition_host(int64_t m, int parts, int w, int64_t* lo, int64_t* hi);
int gpso_screen_parts_host(int64_t m);
/* GPSO_OPT_SURVIVOR_TILE = 0: up to how many survivors the survivors' launch of a screened call takes the narrow tile (a multiple of
 * 64, at most room; 0: none) -- the makespan model of csrc/screen.hpp for a posterior of row_blocks = N_pad / 256 row blocks of
 * L^-1 on a device of `cus` compute units, in a launch with room for `room` rows.  Above it the wide tile runs.  Negative
 * (GPSO_E_ARG) on bad arguments.  No context, no GPU. */
int64_t gpso_survivor_narrow_max_host(int row_blocks, int cus, int64_t room);

/* ---- acquisition functions (no counterpart in the reference: it ranks by mean + varsigma * VAR only) ----------------
 *
 * What a leaf is ranked by, as a map of the (mean, var) the predict path produces -- maximisation throughout:
 *   d = mean - incumbent - xi,   s = sqrt(max(s2, 0)),   z = d / s
 *   GPSO_ACQ_UCB_VAR   mean + varsigma * var      the reference's rule: the bits of gpso_best_ucb
 *   GPSO_ACQ_UCB_STD   mean + varsigma * s        GP-UCB, in score units; numpy's bits of  m + vs * np.sqrt(v)
 *   GPSO_ACQ_EI        s * (phi(z) + z * Phi(z))  expected improvement over the incumbent
 *   GPSO_ACQ_LOGEI     log EI                     finite and accurate where float64 EI is 0.0 (z below about -38)
 *   GPSO_ACQ_PI        Phi(z)                     probability of improvement
 * s2 is the predictive variance the call returns (noise included, as the reference's UCB reads it); with latent != 0
 * it is the latent one, variance - sum before the noise is added.  UCB_VAR reads var as it is; the other kinds clamp s2
 * at 0 from below.  s == 0: EI = max(d, 0), LOGEI = log max(d, 0) (-inf for d <= 0), PI = 1, 1/2 or 0 by the sign of d.
 * A leaf with a NaN coordinate gets a NaN value (and wins its segment, as under gpso_best_ucb).
 * GPSO_E_ARG: acq NULL, an unknown kind, a non-finite varsigma (the UCB kinds) or incumbent / xi (EI, LOGEI, PI). */
#define GPSO_ACQ_UCB_VAR 0
#define GPSO_ACQ_UCB_STD 1
#define GPSO_ACQ_EI 2
#define GPSO_ACQ_LOGEI 3
#define GPSO_ACQ_PI 4
typedef struct {
  int kind;   /* GPSO_ACQ_* */
  int latent; /* != 0: EI / LOGEI / PI / UCB_STD read the latent variance */
  double varsigma, incumbent, xi;
} gpso_acq;

/* gpso_best_ucb, gpso_best_ucb_begin, gpso_best_ucb_grow and gpso_best_ucb_grow_begin with the acquisition in place of
 * varsigma: the same arguments, state rules, routes (small-call kernels, two-stage and keyed arg-max, one-launch calls),
 * first-maximum and NaN rules; `value` receives the winner's acquisition value.  Every posterior the predict path serves
 * is served (fitted, appended, installed, VGP, SGPR, SVGP).  Tickets of the _begin calls are ended with
 * gpso_best_ucb_end, and share its two slots.  With kind GPSO_ACQ_UCB_VAR every output has the bits of the gpso_best_ucb*
 * call.  (No sharded variants: the group fold is acquisition-agnostic, the local halves take varsigma only.) */
int gpso_best_acq(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
                  const gpso_acq* acq, int64_t* idx, double* mean, double* var, double* value);
int gpso_best_acq_begin(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off,
                        int nseg, const gpso_acq* acq);
int gpso_best_acq_grow(gpso_ctx* ctx, const double* bounds, int nseg, int depth, const gpso_acq* acq, int64_t* idx,
                       double* mean, double* var, double* value);
int gpso_best_acq_grow_begin(gpso_ctx* ctx, const double* bounds, int nseg, int depth, const gpso_acq* acq);

/* gpso_predict with the acquisition column: mean / var / value [m] (float64 living in out_mem, each nullable, not all
 * three).  mean and var have the bits of gpso_predict on the same batch; value[j] is what gpso_best_acq ranks leaf j by
 * (np.argmax of it is gpso_best_acq's idx).  State rules and errors as gpso_predict. */
int gpso_acq_values(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_acq* acq, double* mean,
                    double* var, double* value, int out_mem);

/* The same maps on the host: out[i] from (mean[i], var[i]), n each; with latent != 0 the kinds that read it use
 * var[i] - noise.  No context and no GPU (as gpso_shard_range); returns GPSO_OK or GPSO_E_ARG. */
int gpso_acq_eval_host(const gpso_acq* acq, const double* mean, const double* var, double noise, int64_t n, double* out);

/* ---- max-value entropy search (Wang & Jegelka 2017; no counterpart in the reference) ---------------------------------
 *
 * GPSO_ACQ_MES ranks a leaf by the expected reduction of the entropy of the optimum's VALUE y*, from K samples of y*:
 *   value = (1/K) sum_k t(g_k),   g_k = (y*_k - mean) / s,   t(g) = g phi(g) / (2 Phi(g)) - log Phi(g)
 * terms added in index order, one division by K; s2 as for the other kinds (latent != 0: the latent variance).  s == 0: 0
 * (a point without uncertainty tells nothing); a NaN mean or s2: NaN, which wins its segment; otherwise the value is >= 0
 * and finite.  t is evaluated in three pieces that join at g = -1 and g = -10 (csrc/acq.hpp): for g -> -inf both halves grow
 * like g^2 / 2 and cancel down to log |g|, Phi underflows at g = -38, and for g -> +inf the term needs log1p.
 * varsigma, incumbent and xi are not read.
 *
 * The K maxima are state of the context, not of the gpso_acq record (its layout stays), and they are the caller's numbers:
 * fits, appends and installs keep them, only the next gpso_acq_set_maxima changes them; they are no part of the posterior
 * (gpso_posterior_hash, the packed copies and a resident path set do not see them).
 *   gpso_acq_set_maxima: k in 0..64, k = 0 clears; GPSO_E_ARG for another k, a NULL ystar with k > 0 or an entry that is
 *     not finite; GPSO_E_STATE while an asynchronous best-UCB ticket is open (its kernels may be reading the set).
 *   gpso_acq_get_maxima: *k and, where ystar is not NULL, the k values (room for 64).
 * Every call that takes a gpso_acq serves the kind -- gpso_best_acq, _begin, _grow, _grow_begin, gpso_acq_values,
 * gpso_best_batch (the maxima stay fixed over the q rounds) -- on every posterior and context type, and returns
 * GPSO_E_STATE for it while no set is resident.  The kind is never screened.  gpso_acq_eval_host cannot see the maxima and
 * returns GPSO_E_ARG for it; gpso_acq_mes_eval_host and gpso_batch_greedy_mes_host are the host twins that take them as
 * arguments (k in 1..64, every value finite; no context and no GPU).  No sharded variants. */
#define GPSO_ACQ_MES 5
#define GPSO_ACQ_MAX_MAXIMA 64
int gpso_acq_set_maxima(gpso_ctx* ctx, const double* ystar /* [k] host; k = 0 clears */, int k);
int gpso_acq_get_maxima(gpso_ctx* ctx, double* ystar /* [64], nullable */, int* k);
int gpso_acq_mes_eval_host(const double* ystar, int k, int latent, const double* mean, const double* var, double noise,
                           int64_t n, double* out);

/* The functions the MES map and gpso_max_logcdf are made of, on their own (csrc/acq.hpp: written out so that host and
 * device agree to the bit; this entry exists so that a test can hold them to an extended-precision reference):
 * fn 0: exp(x); 1: log(x); 2: log1p(x), x > -1; 3: erfc(x); 4: T^2 (1 - T R(T)) for 1 <= T <= 10, R Mills' ratio.
 * No context and no GPU; GPSO_E_ARG for another fn or a NULL pointer. */
int gpso_acq_math_host(int fn, const double* x, int64_t n, double* out);

/* The law of the maximum over m leaves taken as independent, at g thresholds:
 *   logcdf[i] = sum_j log Phi((y_i - mean_j) / sqrt(max(var_j - var_sub, 0)))
 * -- what a Gumbel law is fitted to when y* is sampled without a path set.  mean / var [m]: float64 living in `mem`, the
 * columns gpso_acq_values writes; var_sub: the noise for the latent law, or 0.  y / logcdf [g]: host, g in 1..64; m >= 1.
 * A row with a NaN mean or var is skipped, *n_used (nullable) counts the others.  A row with s = 0 adds 0, log 1/2 or
 * -inf by the sign of y - mean.  log Phi has a tail form, so a threshold far below a leaf's mean gives a large finite
 * negative number.  One pass: a workgroup of four waves owns 512 consecutive leaves, a thread two of them in registers; the
 * thresholds are walked in order, and for each the wave folds its 64 lanes' terms in a fixed butterfly and the four waves'
 * sums are added in wave order -- one partial per workgroup and threshold (a thread's g sums pass through one register in
 * turn, they do not lie side by side: csrc/maxcdf.hip says why).  A single workgroup then adds the workgroups' partials in
 * index order, one thread per threshold: m / 512 dependent additions, 137 at m = 70 001 and 2 * 10^5 at m = 10^8, where that
 * stage is what the call costs.  No floating-point atomics, a grid that depends on m only, the same bits for the same
 * call.  Reads nothing of the posterior and changes nothing of the context but a
 * workspace of its own.  GPSO_E_ARG: a NULL pointer, a bad mem, m < 1, g outside 1..64, a var_sub or a y that is NaN;
 * GPSO_E_STATE while an asynchronous best-UCB ticket is open.  The host twin adds the rows in index order. */
int gpso_max_logcdf(gpso_ctx* ctx, const double* mean, const double* var, int mem, int64_t m, double var_sub,
                    const double* y /* [g] host */, int g, double* logcdf /* [g] host */, int64_t* n_used /* nullable */);
int gpso_max_logcdf_host(const double* mean, const double* var, int64_t m, double var_sub, const double* y, int g,
                         double* logcdf, int64_t* n_used /* nullable */);

/* ---- latent cross-covariance and greedy batch selection (no counterpart in the reference) ----------------------------
 *
 * Every posterior the predict path serves installs mean = k*^T alpha + c, var = variance - |C k*|^2 + noise over its
 * resident rows, C the dense double factor.  The LATENT posterior covariance between two points is then
 *     Cov(a, b) = k(t_a, t_b) - k_a^T w_b,   w_b = C^T (C k_b):
 * one vector of length N per point b (two passes over C), then O(N D) per pair.
 *
 * gpso_cross_cov: cov[c * m + j] = Cov(f(xa_j), f(xb_c)) for m points xa (dtype / memory as the leaves of gpso_predict)
 * and b points xb (host float64, [b * D]); cov is float64 [b * m] living in out_mem.  A row with a NaN coordinate gives
 * NaNs.  m is worked off in chunks; the bits of an entry depend neither on the chunking nor on the rest of either batch.
 *
 * gpso_best_batch: q leaves of one batch, picked greedily under hallucinated updates (GP-BUCB, "kriging believer"): pick
 * the best leaf, pretend it was observed at its posterior mean with noise variance obs_noise, re-rank, repeat.  The
 * fantasy observation leaves every mean as it is and lowers the variances near the pick.
 *   Round 0 reads the (mean, var, value) of gpso_acq_values on the same batch: it goes through the context's predict
 *     path and has that call's bits.  The first pick with its mean, var and value therefore has the bits of gpso_best_acq
 *     with one segment.
 *   Later rounds are double arithmetic on top of that (csrc/batch.hpp): with G[s][.] the columns of the earlier rounds,
 *     c[j] = Cov(j, p_t) - sum_{s<t} G[s][j] G[s][p_t],  d_t = c[p_t] + obs_noise,  G[t][j] = c[j] / sqrt(d_t),
 *     s2[j] -= G[t][j]^2.
 *   idx / mean / var / value [q] (host; mean, var and value nullable): var[t] is the predictive variance pick t was ranked
 *     by, conditional on the earlier picks; mean[t] is its round-0 mean (the bits of gpso_predict at that row); value[t]
 *     what it was ranked by.  With acq->latent set the kinds read s2 - noise, as they do today (UCB_VAR never does).  The
 *     incumbent and xi do not move between rounds.
 *   obs_noise is the variance of the fantasy observation: absolute, >= 0, the caller's decision as diag_add is (the Python
 *     layer passes the family's predictive noise).
 *   Retiring: a picked row is retired, and with it every row whose scaled coordinates equal the pick's exactly (r^2 == 0
 *     in the column pass: grown leaves repeat rows).  Retired rows never win; their var_after is still updated.
 *   Ending early: a pick whose value is NaN is still reported and the batch ends after it; the same holds if its d_t is
 *     not finite or <= 0 (that pick changes no variance); if no live row is left the batch ends.  *n_picked <= q says how
 *     many entries are valid; the rest of idx / mean / var / value is not written.
 *   var_after (float64 [m] living in out_mem, nullable): the predictive variance of every row after the n_picked picks.
 *   The first maximum wins a tie and a NaN beats every number (np.argmax's rule, and gpso_best_ucb's).
 * GPSO_E_ARG: a GPSO_F32 context (either call); m < 1; q or b outside [1, 64]; q * m > 2^27; NULL xs / xa, xb, cov, acq, idx
 *   or n_picked; a bad acq (the checks of gpso_best_acq); an obs_noise that is negative or not finite.
 * GPSO_E_STATE as gpso_predict_grad: no posterior, an adopted one that travelled without the dense factor, an asynchronous
 *   best-UCB call open.
 * Both calls are stateless: the posterior, its packed copies, the hyper block, the self-test's verdicts,
 * gpso_posterior_hash and a resident path set stay bit for bit; the workspaces are the calls' own and grow only.
 * gpso_last_ms(ctx, 1) covers the call, gpso_last_count(ctx, 0) and (ctx, 1) are m.  gpso_best_batch keeps the scaled
 * leaves (m * D_pad doubles) and G (q * m doubles) on the device for the length of the call.
 * Out of scope: segments, grown leaves (_grow), the asynchronous _begin / _end pair, sharded groups, and the screen. */
int gpso_cross_cov(gpso_ctx* ctx, const void* xa, int xs_dtype, int xs_mem, int64_t m, const double* xb /* [b*D] host */,
                   int b, double* cov /* [b*m] */, int out_mem);
int gpso_best_batch(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_acq* acq,
                    double obs_noise, int q, int64_t* idx, double* mean, double* var, double* value /* [q] host */,
                    int* n_picked, double* var_after /* [m], nullable */, int out_mem);
/* The greedy rounds on the host from a given mean[m], predictive s2[m] and LATENT cov[m*m] (noise: what a latent kind
 * subtracts from s2): the same header, the same roundings, the same end rules; no context and no GPU.  The host sees no
 * coordinates: a row is retired with the pick when cov cannot tell them apart (Cov(j,j), Cov(j,p) and Cov(p,p) are the
 * same number).  var / value / var_after nullable.  Returns GPSO_OK or GPSO_E_ARG. */
int gpso_batch_greedy_host(const gpso_acq* acq, const double* mean, const double* s2, const double* cov, double noise,
                           double obs_noise, int64_t m, int q, int64_t* idx, double* var, double* value,
                           int* n_picked, double* var_after /* nullable */);
/* ... with GPSO_ACQ_MES under the k maxima ystar (latent as in gpso_acq) */
int gpso_batch_greedy_mes_host(const double* ystar, int k, int latent, const double* mean, const double* s2, const double* cov,
                               double noise, double obs_noise, int64_t m, int q, int64_t* idx, double* var, double* value,
                               int* n_picked, double* var_after /* nullable */);

/* ---- the hyper-parameter ensemble: K posteriors of the same data, the integrated acquisition ----
 * No counterpart in the reference, which ranks every leaf under one hyper-parameter vector.  An ensemble holds up to
 * GPSO_ENSEMBLE_MAX posteriors of the RESIDENT DATA at different theta -- samples of p(theta | y), as
 * pygpso_amd/hyper_sampler.py draws them -- and the integrated calls score every leaf under all of them and rank by the
 * average (Snoek, Larochelle & Adams 2012).
 *
 * Where it applies: an exact-GP posterior fitted on this context (gpso_fit_eval*, with or without a noise vector, after
 * gpso_append too), N <= 128, D <= 48, a GPSO_F64 or GPSO_MIXED context (the rule of gpso_predict_grad).  gpso_ensemble_max
 * is 32 where a push can apply to the resident data, else 0.
 *
 * gpso_ensemble_push: the resident posterior becomes the next member; returns its index (>= 0) or a status (< 0).  A
 * member is a device-to-device copy, on the context's stream, of what a point call reads -- the hyper block, the scaled
 * rows, the dense double L^-1, alpha, the kernel kind -- into buffers of the ensemble's own (32 x (128 KB + the rows)).
 * Nothing is computed: a member holds the bits the context's fit at its theta left.  All members share N, D and the kernel.
 *   GPSO_E_ARG: a GPSO_F32 context; N > 128.   GPSO_E_STATE: no posterior, or a variational, installed (gpso_set_posterior)
 *   or adopted one; a 33rd member; a posterior whose N, D or kernel disagrees with the members'; an asynchronous call open.
 * gpso_ensemble_clear: no members.  GPSO_E_STATE while an asynchronous call is open.
 * gpso_ensemble_info: *k members; theta (nullable) [k * 51]: per member 48 lengthscales (as the hyper block expands
 * them), kernel variance, noise variance, constant mean.
 * Lifetime: the members describe the data.  gpso_set_data, gpso_append*, gpso_set_noise_diag, gpso_set_posterior, every
 * variational and sparse call that replaces the posterior or its rows, gpso_alloc_posterior and gpso_adopt_posterior end
 * the ensemble (k = 0).  A refit at another theta does not, and changes no bit of a later integrated call.  The ensemble is
 * no part of gpso_posterior_hash, the packed copies, a broadcast or a path set; pushing, clearing and the integrated
 * calls leave all of those, the hyper block and the posterior bit for bit.
 *
 * The integrated calls.  Per member k and leaf j (one launch, a workgroup per 64 leaves and member): the leaf scaled by
 * member k's lengthscales, k* from direct differences in double, V = L_k^-1 k* on the f64 MFMA,
 *     mean_kj = alpha_k^T k* + c_k,   var_kj = (variance_k - sum_i V_i^2) + noise_k        (predictive)
 * then, per leaf (a second launch), with a_kj acq's map (gpso_acq_values' per-member value; a latent kind reads
 * var_kj - noise_k; incumbent, xi and varsigma are the caller's single numbers):
 *     UCB_VAR, UCB_STD, EI, PI:  value_j = (sum_k a_kj) / K          index order, one division
 *     LOGEI:  value_j = mx + log(sum_k exp(l_kj - mx)) - log K,  mx = max_k l_kj     (the log of the mean EI; -inf if all are)
 *     mean_mix_j = (sum_k mean_kj) / K,   var_mix_j = (sum_k (var_kj + (mean_kj - mean_mix_j)^2)) / K
 * A NaN member gives a NaN value; a leaf with a NaN coordinate is NaN in every member.  K = 1 returns the member's own
 * three numbers.  The same call gives the same bits: no atomics, every sum in a fixed order.  A member's columns agree
 * with gpso_predict on a context fitted at its theta to the float64 row of DESIGN.md 2.1, not bit for bit.
 * gpso_ensemble_best_acq: per segment (seg_off / nseg as gpso_best_ucb) the arg-max of value -- the first maximum wins, a
 *   NaN beats every number -- with idx relative to the segment (-1 and NaNs for an empty one); mean_mix / var_mix / value
 *   [nseg] host, nullable: the winner's entries of gpso_ensemble_acq_values' columns, bit for bit.
 * gpso_ensemble_acq_values: mean_mix / var_mix / value [m] and member_mean / member_var [k * m] (member-major), each
 *   nullable, in out_mem.
 * gpso_ensemble_fold_host: the fold alone on the host from given member columns [k * m] and noise [k] (nullable unless a
 *   latent kind reads it): the same header, the same roundings; no context and no GPU.  GPSO_OK or GPSO_E_ARG.
 * GPSO_E_ARG: a GPSO_F32 context; GPSO_ACQ_MES (its maxima belong to one theta) or another bad acq; m < 1; k * m > 2^28;
 *   bad dtype / memory; nseg outside [1, 1024] or bad seg_off; NULL xs, idx, or every output.
 * GPSO_E_STATE: no ensemble resident; an asynchronous best-UCB call open.
 * gpso_last_ms(ctx, 1) covers a call; gpso_last_count(ctx, 0) and (ctx, 1) are m.
 * Out of scope: grown leaves (_grow), the _begin / _end pair, sharded groups, the screen, gpso_best_batch on an ensemble,
 * the variational families, GPSO_F32. */
#define GPSO_ENSEMBLE_MAX 32
int gpso_ensemble_max(gpso_ctx* ctx);
int gpso_ensemble_push(gpso_ctx* ctx);
int gpso_ensemble_clear(gpso_ctx* ctx);
int gpso_ensemble_info(gpso_ctx* ctx, int* k, double* theta /* [k*(48+3)], nullable */);
int gpso_ensemble_best_acq(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off,
                           int nseg, const gpso_acq* acq, int64_t* idx, double* mean_mix, double* var_mix, double* value);
int gpso_ensemble_acq_values(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_acq* acq,
                             double* mean_mix, double* var_mix, double* value /* [m], each nullable */,
                             double* member_mean, double* member_var /* [k*m], nullable */, int out_mem);
int gpso_ensemble_fold_host(const gpso_acq* acq, const double* member_mean, const double* member_var,
                            const double* noise /* [k] */, int k, int64_t m, double* mean_mix, double* var_mix,
                            double* value);

/* ---- outcome constraints: J GP feasibility models and the constrained acquisition ------------
 * No counterpart in the reference.  Gardner et al. (2014), Gelbart, Snoek & Adams (2014): every constrained output c_i(x)
 * has an exact GP of its own, and a leaf is ranked by the objective's acquisition weighted or gated by the probability
 * that the latent constraint functions are satisfied.
 *
 * The constraint set.  A context holds up to GPSO_CONSTRAINTS_MAX posteriors of OTHER targets in buffers of the set's own.
 * gpso_constraint_push: the exact-GP posterior resident on `src` -- another context on the same device, or ctx itself --
 *   becomes the next member; returns its index (>= 0) or a status (< 0).  The copy is gpso_ensemble_push's (hyper block,
 *   scaled rows, dense double L^-1, alpha, kernel kind), device to device; src's stream is waited for; nothing is
 *   computed.  sense = +1: feasible where c(x) <= threshold; sense = -1: feasible where c(x) >= threshold.
 *   Where it applies is gpso_ensemble_push's rule, on src: an exact GP fitted there (with or without a noise vector, after
 *   gpso_append too), N <= 128, D <= 48, GPSO_F64 or GPSO_MIXED on both contexts; all members share N, D and the kernel.
 *   GPSO_E_ARG: a GPSO_F32 context (either); N > 128; different devices; NULL src; a sense other than +1 / -1; a threshold
 *     that is not finite.
 *   GPSO_E_STATE: no posterior on src, or a variational, sparse, installed or adopted one; a 17th member; a posterior whose
 *     N, D or kernel disagrees with the members'; an asynchronous call open on either context.
 * gpso_constraint_clear: no members.  GPSO_E_STATE while an asynchronous call is open.
 * gpso_constraint_info: *k members; theta (nullable) [k * 51] as gpso_ensemble_info; threshold [k], sense [k] (nullable).
 * gpso_constraint_max: GPSO_CONSTRAINTS_MAX where ctx can hold a set -- a GPSO_F64 or GPSO_MIXED context whose resident data,
 *   if it has any yet, has N <= 128 (a push itself depends on src, and may come before ctx has data) --, else 0.
 * Lifetime: the set belongs to the CONTEXT, not to its data -- a constraint model has its own targets.  gpso_set_data,
 * gpso_append, a noise vector and a refit on ctx keep it; gpso_constraint_clear, gpso_alloc_posterior and gpso_destroy end
 * it.  A constrained call whose objective's N, D or kernel differs from the members' is refused (GPSO_E_STATE): the set is
 * stale.  The set is no part of gpso_posterior_hash, the packed copies, a broadcast, a path set or the ensemble; push, clear
 * and the constrained calls leave all of those and the posterior bit for bit.
 *
 * The constrained calls.  The objective is the posterior resident on ctx (the same rule as a member: exact GP fitted here,
 * N <= 128); its predictive columns (mean_j, var_j) and the members' (mean_ij, var_ij) come from the ensemble's stage 1
 * (one launch on the context's own buffers, one over the set: nothing of size N^2 is copied per call).  Then per leaf j:
 *     s2_i = max(var_ij - noise_i, 0);  z_i = sense_i (t_i - mean_ij) / sqrt(s2_i);  lp_i = log Phi(z_i)
 *     (s2_i = 0: lp_i = 0 where sense_i (t_i - mean_ij) >= 0, else -inf)
 *     logpof_j = sum_i lp_i          index order, from its first term; a NaN anywhere: NaN
 *     a0 = acq's map on the objective (gpso_acq_values' value; a latent kind reads var_j - noise)
 *   cspec.mode GPSO_CON_WEIGHT: EI, PI: value = a0 exp(logpof); LOGEI: value = l0 + logpof; -inf where logpof <
 *     log_pof_min.  The UCB kinds are refused (GPSO_E_ARG): a signed value cannot be weighted.
 *   GPSO_CON_GATE: value = a0 where logpof >= log_pof_min, else -inf; a0's own bits, in score units.  log_pof_min = -inf
 *     (no gate) returns the unconstrained values of the same columns.
 *   GPSO_CON_FEASIBILITY: value = logpof (the rule while no feasible point is known).
 * log Phi is accurate far into the tail (finite to z = -1e150).  The same call gives the same bits: no atomics.
 * gpso_constrained_best_acq: per segment (seg_off / nseg as gpso_best_ucb) the arg-max of value -- the first maximum wins,
 *   a NaN beats every number -- with idx relative to the segment (-1 and NaNs for an empty one); mean / var / value /
 *   logpof [nseg] host, nullable: the winner's entries of gpso_constrained_acq_values' columns, bit for bit.
 * gpso_constrained_acq_values: mean / var / value / logpof [m] and member_mean / member_var [k * m] (member-major), each
 *   nullable, in out_mem.
 * gpso_constrained_fold_host: the fold alone on the host from given columns -- objective mean / var [m] and its noise
 *   variance, member columns [k * m], member_noise / threshold / sense [k]: the same header, the same roundings; no
 *   context and no GPU.  mean / var may be NULL in GPSO_CON_FEASIBILITY.  GPSO_OK or GPSO_E_ARG.
 * GPSO_E_ARG: GPSO_ACQ_MES or another bad acq; a bad cspec (mode; log_pof_min NaN or > 0); a UCB kind in weight mode; a
 *   GPSO_F32 context; N > 128; m < 1; (k + 1) * m > 2^28; bad dtype / memory; nseg outside [1, 1024] or bad seg_off; NULL xs,
 *   idx, or every output.
 * GPSO_E_STATE: no set; a stale set; no exact-GP posterior fitted on ctx; an ensemble resident on ctx; an asynchronous
 *   best-UCB call open.
 * gpso_last_ms(ctx, 1) covers a call; gpso_last_count(ctx, 0) and (ctx, 1) are m.
 * Out of scope: N > 128, GPSO_F32, variational and sparse members, _begin / _end, grown leaves on the device, sharded and
 * screened variants, gpso_best_batch under constraints, MES, the ensemble together with constraints. */
#define GPSO_CONSTRAINTS_MAX 16
#define GPSO_CON_WEIGHT 0
#define GPSO_CON_GATE 1
#define GPSO_CON_FEASIBILITY 2
typedef struct {
  int mode;           /* GPSO_CON_* */
  double log_pof_min; /* <= 0; -INFINITY: no gate */
} gpso_cspec;
int gpso_constraint_max(gpso_ctx* ctx);
int gpso_constraint_push(gpso_ctx* ctx, gpso_ctx* src, double threshold, int sense);
int gpso_constraint_clear(gpso_ctx* ctx);
int gpso_constraint_info(gpso_ctx* ctx, int* k, double* theta /* [k*(48+3)] */, double* threshold /* [k] */,
                         int* sense /* [k], each nullable */);
int gpso_constrained_best_acq(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off,
                              int nseg, const gpso_acq* acq, const gpso_cspec* cspec, int64_t* idx, double* mean,
                              double* var, double* value, double* logpof);
int gpso_constrained_acq_values(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_acq* acq,
                                const gpso_cspec* cspec, double* mean, double* var, double* value,
                                double* logpof /* [m], each nullable */, double* member_mean,
                                double* member_var /* [k*m], nullable */, int out_mem);
int gpso_constrained_fold_host(const gpso_acq* acq, const gpso_cspec* cspec, const double* mean, const double* var,
                               double noise, const double* member_mean, const double* member_var,
                               const double* member_noise, const double* threshold, const int* sense, int k, int64_t m,
                               double* value, double* logpof);

/* ---- failed evaluations: the success probability and the success member ------------------------
 * No counterpart in the reference.  Gelbart, Snoek & Adams (2014), the constraint that is only observed as "it worked / it
 * did not": a GP classifier (a VGP under GPSO_LIK_BERNOULLI, installed by gpso_vgp_posterior) of whether an evaluation
 * returns a finite score, and its probability of success weighting or gating the acquisition.
 *
 * gpso_success_prob_host: the probit map alone on the host, no context and no GPU: for n latent (mean, var) pairs
 *   logprob = log Phi(mean / sqrt(1 + max(var, 0))) and prob = exp(logprob), the device's text and roundings; a NaN in gives
 *   a NaN out.  logprob / prob nullable, not both.  GPSO_OK or GPSO_E_ARG.
 * gpso_predict_prob: P(success) at m points of the Bernoulli install resident on ctx.  Stage 1 is the ensemble's member
 *   kernel with K = 1 on the context's own buffers (the latent mean and variance), then one thread per point of the map above.
 *   prob / logprob / mean / var [m] in out_mem, each nullable, not all.  Where it applies is gpso_ensemble_push's rule: N <= 128,
 *   D <= 48, GPSO_F64 or GPSO_MIXED.
 *   GPSO_E_ARG: a GPSO_F32 context; N > 128; m < 1 or > 2^28; bad dtype / memory; NULL xs; every output NULL.
 *   GPSO_E_STATE: no posterior, or any other than a Bernoulli install (a Gaussian or Student-t VGP, an exact GP, a sparse,
 *     installed or adopted one); an asynchronous best-UCB call open.
 * gpso_success_push: the Bernoulli install resident on `src` (a context on the same device) is copied into the ONE slot of the
 *   success member on ctx: the four device-to-device copies of gpso_constraint_push (hyper block, scaled rows, dense double C,
 *   beta), nothing computed; a member already there is replaced.  The member's N and kernel may differ from the objective's --
 *   the classifier is trained on failed points the objective never sees --, D must agree, N <= 128.
 *   GPSO_E_ARG: a GPSO_F32 context (either); N > 128; different devices; NULL src; D on src differing from the data on ctx.
 *   GPSO_E_STATE: src holds no Bernoulli install; an asynchronous call open on either context.
 * gpso_success_clear: no member.  GPSO_E_STATE while an asynchronous call is open.
 * gpso_success_info: *present 0 / 1; *n (nullable) the member's N; theta (nullable) [51] as a row of gpso_ensemble_info.
 * Lifetime: the constraint set's.  The member belongs to the CONTEXT: gpso_set_data, gpso_append and refits of the objective
 * keep it; gpso_success_clear, gpso_alloc_posterior and gpso_destroy end it.  It is no part of gpso_posterior_hash, the packed
 * copies, a broadcast, a path set, the ensemble, the constraint set's count or gpso_constraint_info; push and clear leave both
 * posteriors bit for bit.
 *
 * While a member is resident gpso_constrained_acq_values and gpso_constrained_best_acq take it in: one more K = 1 stage-1
 * launch with the member's own N and kernel writes row 1 + J of the [1 + J + 1][m] workspace, and the fold adds
 * log Phi(mean_s / sqrt(1 + var_s)) to logpof as its LAST term, behind the J constraints in index order; the sum still starts
 * at its first term, so with J = 0 the success term IS logpof.  J = 0 is served when, and only when, a member is resident.
 * Modes, kinds, the gate, the NaN rules, the arg-max and the gather are unchanged.  gpso_constrained_acq_values' member_mean /
 * member_var then hold [(J + 1) * m]: the member's latent columns follow the constraints'.  A member whose D differs from the
 * objective's: GPSO_E_STATE.
 * gpso_constrained_success_fold_host: that fold on the host, as gpso_constrained_fold_host with success_mean / success_var
 *   [m]; k may be 0 (the member arrays are then not read).
 * Out of scope: the sparse families as classifier, N > 128, GPSO_F32, _begin / _end, grown leaves, sharded and screened
 * variants, gpso_best_batch, MES, the ensemble. */
int gpso_success_prob_host(const double* mean, const double* var, int64_t n, double* logprob, double* prob);
int gpso_predict_prob(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, double* prob, double* logprob,
                      double* mean, double* var /* [m], each nullable */, int out_mem);
int gpso_success_push(gpso_ctx* ctx, gpso_ctx* src);
int gpso_success_clear(gpso_ctx* ctx);
int gpso_success_info(gpso_ctx* ctx, int* present, int64_t* n, double* theta /* [48+3], nullable */);
int gpso_constrained_success_fold_host(const gpso_acq* acq, const gpso_cspec* cspec, const double* mean, const double* var,
                                       double noise, const double* member_mean, const double* member_var,
                                       const double* member_noise, const double* threshold, const int* sense, int k,
                                       int64_t m, const double* success_mean, const double* success_var, double* value,
                                       double* logpof);

/* ---- bi-objective search: a Pareto front and the exact expected hypervolume improvement ---------
 * No counterpart in the reference.  Emmerich, Giannakoglou & Naujoks (2006); Emmerich, Yang, Deutz et al. (2016): with two
 * objectives to MAXIMISE, a leaf is ranked by the expected growth of the hypervolume its outcome adds to the front found so
 * far.  The first objective is the posterior resident on ctx.  The second is ONE MEMBER of the constraint set -- an output
 * declared as a constraint already has its exact GP there --, named by gpso_ehvi.member; nothing new is made resident, and
 * gpso_constraint_push, the set's lifetime and the constrained calls are what they were.  The REMAINING members, and the
 * success member where one is resident, stay constraints: their logpof weights or gates the EHVI.
 *
 * gpso_ehvi: member -- objective 2's index in the set; latent -- non-zero: s^2 = max(var - noise, 0) for both objectives,
 *   noise being slot 5 of each model's own hyper block, zero: the predictive variance clamped at 0; p and front -- the front
 *   as p pairs (f1, f2), host memory, f1 strictly ascending, f2 strictly descending, every point strictly above ref in both
 *   coordinates, p <= GPSO_EHVI_FRONT_MAX (p = 0: no front yet, front may be NULL); ref -- the reference point (r1, r2).
 * Per leaf, with a_0 = r1, a_k = f1 of point k, a_{p+1} = +inf, strip heights h_k = f2 of point k + 1 (k < p), h_p = r2,
 * Y1 ~ N(mean1, s1^2) and Y2 ~ N(mean2, s2^2) independent, g(x) = E[(Y1 - x)+] = s1 H((mean1 - x) / s1), e_k = E[(Y2 - h_k)+],
 * H(z) = phi(z) + z Phi(z) (s = 0: max(mean - x, 0)):
 *     EHVI = sum_{k=0..p} (g(a_k) - g(a_{k+1})) e_k,     g(+inf) = 0          (exact; p = 0: g(r1) e_0)
 * The p + 1 terms occupy slots 0 .. p of 64, the rest are +0.0, and are added as slot[i] += slot[i + w] for w = 32, 16, 8,
 * 4, 2, 1: an order that is the same on the device (a wave a leaf, a strip a lane, six shuffle steps) and on the host, so a
 * device value has the bits of gpso_ehvi_fold_host on the same columns; exp and erfc are the library's own, not libm's.
 * A NaN mean or variance of either objective: NaN (the arg-max then picks it); a mean of -inf: 0; else a mean of +inf: +inf.
 *     logpof = sum of the constrained calls' log Phi terms over the members OTHER than `member`, index order, from its
 *              first term; the success member's term last; no term at all: +0.0
 *   cspec NULL: value = EHVI (logpof is still reported).
 *   GPSO_CON_WEIGHT: value = EHVI exp(logpof); -inf where logpof < log_pof_min.
 *   GPSO_CON_GATE: value = EHVI's own bits where logpof >= log_pof_min, else -inf; log_pof_min = -inf: no gate.
 *   A NaN logpof gives a NaN value in both modes but the open gate.
 * gpso_ehvi_values: value / logpof [m] and mean / var [2 m] -- the objective's column, then the member's --, each nullable,
 *   in out_mem.  The columns are gpso_constrained_acq_values' (the same stage 1), bit for bit.
 * gpso_best_ehvi: per segment (seg_off / nseg as gpso_constrained_best_acq) the arg-max of value: the first maximum wins, a
 *   NaN beats every number, idx is relative to the segment (-1 and NaNs for an empty one); value / logpof [nseg] and mean /
 *   var [2 nseg] host, nullable: the winner's entries of gpso_ehvi_values' columns, bit for bit.
 * gpso_ehvi_fold_host: the fold alone on the host, no context and no GPU (ehvi->member is ignored): the two objectives'
 *   columns [m] and noise variances, the OTHER members' columns [k m] (objective 2 already left out; k >= 0, at most 15) with
 *   other_noise / threshold / sense [k], success_mean / success_var [m] (both NULL: no success member).  GPSO_OK or GPSO_E_ARG.
 * GPSO_E_ARG: NULL ehvi; member outside [0, J); p outside [0, 63]; p > 0 with a NULL front; a front or reference entry that
 *   is not finite; f1 not strictly ascending; f2 not strictly descending; a front point not strictly above ref in both
 *   coordinates; cspec with GPSO_CON_FEASIBILITY (gpso_constrained_* serve it), an unknown mode, or log_pof_min NaN or > 0;
 *   a GPSO_F32 context; N > 128; m < 1; (J + 1) * m > 2^28; bad dtype / memory / out_mem; nseg outside [1, 1024] or bad
 *   seg_off; NULL xs, idx, or every output.
 * GPSO_E_STATE: no constraint set (a success member alone is no objective); a stale set or success member; no exact-GP
 *   posterior fitted on ctx; an ensemble resident on ctx; an asynchronous best-UCB call open.
 * Every refusal comes before anything is allocated or enqueued.  The calls leave both posteriors, gpso_posterior_hash, the
 * set and the success member as they are.  gpso_last_ms(ctx, 1) covers a call; gpso_last_count(ctx, 0) and (ctx, 1) are m.
 * A front of more than 63 points is the caller's to thin (pygpso_amd.pareto.truncate_front: the EHVI over a subset of the
 * front is an upper bound).
 * Out of scope: more than two objectives; log-EHVI (float64 EHVI is exactly 0 far behind the front, such leaves tie and the
 * first wins: the follow-up, as log-EI was to EI); correlated objectives; N > 128 and GPSO_F32; _begin / _end, grown
 * leaves, sharded and screened variants; gpso_best_batch; the ensemble; the optimiser's loop (EHVI is not in score units). */
#define GPSO_EHVI_FRONT_MAX 63
typedef struct {
  int member;          /* objective 2: its index in the constraint set */
  int latent;          /* non-zero: both objectives without their noise variance */
  int p;               /* points of the front, 0 .. GPSO_EHVI_FRONT_MAX */
  const double* front; /* host [2 p]: (f1, f2) pairs, f1 ascending; NULL where p = 0 */
  double ref[2];       /* the reference point (r1, r2) */
} gpso_ehvi;
int gpso_ehvi_values(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const gpso_ehvi* ehvi,
                     const gpso_cspec* cspec /* nullable */, double* value, double* logpof /* [m] */, double* mean,
                     double* var /* [2 m]: objective, then member; each nullable */, int out_mem);
int gpso_best_ehvi(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m, const int64_t* seg_off, int nseg,
                   const gpso_ehvi* ehvi, const gpso_cspec* cspec /* nullable */, int64_t* idx, double* value,
                   double* logpof /* [nseg] */, double* mean, double* var /* [2 nseg], each nullable */);
int gpso_ehvi_fold_host(const gpso_ehvi* ehvi /* member ignored */, const gpso_cspec* cspec /* nullable */,
                        const double* mean1, const double* var1, double noise1, const double* mean2, const double* var2,
                        double noise2, const double* other_mean, const double* other_var /* [k m] */,
                        const double* other_noise, const double* threshold, const int* sense /* [k] */, int k /* >= 0 */,
                        int64_t m, const double* success_mean, const double* success_var /* [m], nullable */,
                        double* value, double* logpof);

/* ---- ternary geometry on device (LeafNode.grow, gpso/param_space.py:175-200,257-307) -------- */

/* Centres of levels 0..depth-1 of the ternary subtree under each of nseg boxes, generated on the
 * device with the reference's float64 recurrence (bit-for-bit), level-major; rows per box =
 * (3^depth - 1) / 2.  bounds[nseg*D*2] = (lo, hi) per dimension, host float64.
 * gpso_grow copies the centres out (host float64 [nseg*rows*D]);
 * gpso_best_ucb_grow scores them without leaving the device: one call = one exploration level
 * of GPSOptimiser._tree_explore (gpso/optimisation.py:366-403).  Rows that repeat an earlier row bit for
 * bit are scored once; idx is the REFERENCE row index (first maximum over the full duplicated list), so
 * the result equals gpso_best_ucb on the rows gpso_grow returns. */
int64_t gpso_grow_rows(int depth);
int gpso_grow(gpso_ctx* ctx, const double* bounds, int nseg, int d, int depth, double* out_coords);
int gpso_best_ucb_grow(gpso_ctx* ctx, const double* bounds, int nseg, int depth, double varsigma,
                       int64_t* idx, double* mean, double* var, double* ucb);

/* ---- multi-GPU group (no counterpart in the reference: it has no distributed path) --------------- */

/* One context per GPU -- in one process per GPU (torchrun / MPI style) or on several threads of one
 * process -- joined into a group through RCCL.  The predict path shards (leaves are independent given
 * the posterior): the GP is fitted on ONE rank, its predict-ready state is broadcast over xGMI, every
 * rank scores a contiguous share of the leaves with no data-path collective, and the per-segment
 * winners (4 doubles each) are all-gathered and folded on the device with np.argmax's order on
 * (ucb, global index) -- so every rank returns the same result, bit-identical to the single-GPU call.
 * librccl is loaded (dlopen) by the first of these calls; failures return GPSO_E_RCCL.
 * Every rank of a group must make the same sequence of group calls with the same arguments (as for any
 * collective); the arithmetic options (dtype, predict math, generation) must match across the group. */
#define GPSO_UNIQUE_ID_BYTES 128
/* rank 0 creates the group id (ncclGetUniqueId) and hands the 128 bytes to every rank by any means
 * (the launcher's rendezvous, MPI, a file); ctx-less: the message of a failure is gpso_last_error(NULL) */
int gpso_comm_unique_id(void* out_id /* [GPSO_UNIQUE_ID_BYTES] */);
/* collective over the group: ncclCommInitRank on the context's device */
int gpso_comm_init(gpso_ctx* ctx, int rank, int world, const void* unique_id);
int gpso_comm_destroy(gpso_ctx* ctx);
/* returns 1 when the context belongs to a group, 0 otherwise; rank / world are filled either way */
int gpso_comm_info(const gpso_ctx* ctx, int* rank, int* world);
/* the contiguous share [lo, hi) of m leaves (or reference rows) that `rank` of `world` handles */
void gpso_shard_range(int64_t m, int rank, int world, int64_t* lo, int64_t* hi);
/* collective: the posterior resident on `root` (after gpso_fit_eval / gpso_set_posterior) becomes
 * resident on every rank -- one RCCL broadcast per buffer of gpso_posterior_buffers, device to device */
int gpso_broadcast_posterior(gpso_ctx* ctx, int root);
/* After gpso_append on the root: bring the peers up to date moving ONLY what the appends wrote -- the new rows of the scaled
 * inputs and of each predict-ready copy of L^-1 (whole 16-row tile rows), alpha, the hyper block: ~1.1 MB instead of the 1.07
 * GB of gpso_broadcast_posterior for 7 new points at N = 16 384 (the reference re-creates its model on every update,
 * gpso/gp_surrogate.py:496-498; there is no hand-off to replace).  Collective, same header / verdict protocol: the root
 * offers rows when its posterior is the one of the last hand-off extended in place (same predict math, same fp16 scale);
 * every rank says whether it holds that base; if all do, the ranges travel (one ncclBroadcast each, grouped) and the call
 * returns GPSO_OK -- otherwise EVERY rank takes the whole range as gpso_broadcast_posterior does and the call returns 1.
 * gpso_last_count(ctx, 0) = the bytes that travelled. */
int gpso_broadcast_posterior_rows(gpso_ctx* ctx, int root);
/* The same decision without a communicator (hand-offs by plain device copies: several contexts of one process, tests): the
 * ranges [offsets[i], offsets[i] + nbytes[i]) of the posterior arena -- offsets as gpso_posterior_span reports them, valid on
 * every context of the same shape and type (gpso_posterior_span_at) -- that a peer holding the posterior of the last
 * hand-off lacks.  Returns their number (<= 9; cap >= 10): 0 = the peer is up to date; when rows do not apply, ONE range: the
 * whole span.  After copying them the receiver calls gpso_adopt_posterior, the sender gpso_posterior_mark_synced (which
 * gpso_broadcast_posterior / _rows do themselves on every rank, and a receiver's gpso_adopt_posterior does not: a receiver
 * that becomes a sender marks explicitly). */
int gpso_posterior_dirty_ranges(gpso_ctx* ctx, int64_t* offsets, int64_t* nbytes, int cap);
int gpso_posterior_mark_synced(gpso_ctx* ctx);

/* collective gpso_best_ucb: xs holds THIS rank's rows gpso_shard_range(m_global, rank, world) of the
 * batch (m_local of them); seg_off[nseg+1] (host, NULL = one segment) is in GLOBAL rows; idx is relative
 * to the global segment start.  Outputs are identical on every rank. */
int gpso_best_ucb_sharded(gpso_ctx* ctx, const void* xs, int xs_dtype, int xs_mem, int64_t m_local,
                          int64_t m_global, const int64_t* seg_off, int nseg, double varsigma,
                          int64_t* idx, double* mean, double* var, double* ucb);
/* collective gpso_best_ucb_grow: every rank generates and scores the reference rows
 * gpso_shard_range(gpso_grow_rows(depth), rank, world) of every box on its own device (O(D) bytes in) */
int gpso_best_ucb_grow_sharded(gpso_ctx* ctx, const double* bounds, int nseg, int depth, double varsigma,
                               int64_t* idx, double* mean, double* var, double* ucb);

/* Collective safety: every rank takes part in every collective of a group call whatever happened in its own half
 * of it (bad arguments, no posterior, GPSO_E_PRECISION from the self-test, a failed allocation): a failing rank
 * sends an empty payload carrying its status, the fold takes the worst status over the ranks, and EVERY rank
 * returns that code (its own message on the rank that failed, "rank r failed ..." on the others).  In particular a
 * posterior that fails the precision self-test on the fitting rank makes gpso_broadcast_posterior return
 * GPSO_E_PRECISION on every rank.  What cannot be agreed on is a failure of HIP or RCCL itself in the middle of
 * a call; gpso_comm_abort (ncclCommAbort), called from another thread for the context whose call is blocked, is
 * the way out of that one -- the blocked call then returns GPSO_E_RCCL / GPSO_E_HIP and the context must leave the
 * group (gpso_comm_destroy) before it joins another. */
int gpso_comm_abort(gpso_ctx* ctx);

/* The two halves of the sharded calls on their own, for an arbitrary (rank, world) and WITHOUT a communicator: what
 * a group of `world` ranks computes can be replayed on one device (tests, debugging; also a transport other than
 * RCCL): gpso_shard_winners / gpso_shard_winners_grow run rank `rank`'s local half of gpso_best_ucb_sharded /
 * gpso_best_ucb_grow_sharded and copy out its payload -- gpso_group_payload_doubles(nseg) doubles: nseg x (mean, var,
 * ucb, bit-cast int64 index), a spare slot, the status of the half (also the return value); gpso_fold_winners takes
 * the payloads of all ranks concatenated in rank order (m_global >= 0 with seg_off: payloads of gpso_shard_winners,
 * whose indices are relative to the local piece of each segment; m_global < 0: of gpso_shard_winners_grow) and
 * returns what the group call returns, the worst status included.  These run the very kernels and index arithmetic
 * of the group calls; only ncclAllGather is replaced by the caller's concatenation. */
int gpso_group_payload_doubles(int nseg);
int gpso_shard_winners(gpso_ctx* ctx, int rank, int world, const void* xs, int xs_dtype, int xs_mem,
                       int64_t m_local, int64_t m_global, const int64_t* seg_off, int nseg, double varsigma,
                       double* payload);
int gpso_shard_winners_grow(gpso_ctx* ctx, int rank, int world, const double* bounds, int nseg, int depth,
                            double varsigma, double* payload);
int gpso_fold_winners(gpso_ctx* ctx, const double* gathered, int world, int64_t m_global, const int64_t* seg_off,
                      int nseg, int64_t* idx, double* mean, double* var, double* ucb);

/* ---- introspection ------------------------------------------------------------------------- */

/* padded problem size the device works with (a multiple of 128; of 256 in float-predict contexts above
 * N = 128), 0 before gpso_set_data */
int64_t gpso_padded_n(const gpso_ctx* ctx);
/* N and D of the problem the context currently holds (0, 0 before any data / posterior arrived) */
int gpso_problem_shape(const gpso_ctx* ctx, int64_t* n, int* d);
int gpso_get_matrix(gpso_ctx* ctx, int which, double* out /* [N*N] host */);
int gpso_get_vector(gpso_ctx* ctx, int which, double* out /* [N] host */);

/* Device pointers + byte sizes of everything a peer GPU needs to predict: hyper-parameter block, packed
 * lower tiles of L^-1, scaled X (double: plain, as MFMA fragments, norms), alpha [, the bf16 pieces of
 * L^-1 when a split-bf16 predict math is on]: fills up to cap (>= 7) entries, returns the count (or a
 * negative status).  On a context that holds a posterior the call first lets GPSO_GEN_AUTO rule (it may
 * run the self-test) and records the choice in the hyper block, so that the receiver generates alike. */
int gpso_posterior_buffers(gpso_ctx* ctx, void** ptrs, int64_t* nbytes, int cap);
/* Round 4: all of those buffers are slices of ONE device allocation per context (the "posterior arena"), laid out as
 * [packed L^-1 | hyper | X / l | its fragments | norms | alpha | scale slot + 16-bit planes of L^-1] -- a function of
 * (padded N, padded D, dtype) only -- so that what the resident posterior USES is one contiguous range whichever predict
 * math it runs (f32 MFMA kernel: [packed L^-1 .. alpha]; split math: [hyper .. the planes in use], the packed L^-1 then
 * stays home).  gpso_posterior_span returns that range: device pointer, its offset inside the arena (the same on every
 * context of the same shape / dtype) and its length; gpso_posterior_span_at maps an (offset, length) announced by a
 * peer onto this context's arena after gpso_alloc_posterior.  gpso_broadcast_posterior moves exactly this range with a
 * single ncclBroadcast.  Replaces (as does gpso_posterior_buffers) nothing in the reference: it has no second device
 * (gpso/gp_surrogate.py:313-328 runs where the GPflow model lives). */
int gpso_posterior_span(gpso_ctx* ctx, void** ptr /* nullable */, int64_t* offset /* nullable */, int64_t* nbytes /* nullable */);
int gpso_posterior_span_at(gpso_ctx* ctx, int64_t offset, int64_t nbytes, void** ptr);
/* 64-bit fingerprint of the predict-ready posterior resident on the context (a position-salted wrap-around sum over the
 * words of the buffers in use; deterministic).  The fit is bit-deterministic, so contexts that ran the same
 * gpso_set_data + gpso_fit_eval hold the same value: a group may REPLICATE the fit on every rank and compare
 * fingerprints instead of broadcasting the factor (SURVEY 8e "measure both"; pygpso_amd.distributed: posterior=
 * "replicate").  Stands where gpso/gp_surrogate.py:500-503 leaves its one GPflow model. */
int gpso_posterior_hash(gpso_ctx* ctx, uint64_t* out);
/* Allocate the same buffers for n, d on a receiving rank so they can be broadcast into. */
int gpso_alloc_posterior(gpso_ctx* ctx, int64_t n, int d);
/* After the buffers were filled by a broadcast: mark the posterior resident (reads the
 * hyper-parameter block back from the device). */
int gpso_adopt_posterior(gpso_ctx* ctx);

/* Precision self-test of the resident posterior (runs it if it has not run since the last fit; needs
 * the training targets, i.e. a posterior produced by gpso_fit_eval on this context): the predict path
 * is evaluated at the training inputs, where mean and variance have the closed form
 * mean_i = y_i - noise alpha_i, var_i = 2 noise - noise^2 (K_y^-1)_ii.  out[12]:
 *   [0] max |d mean|   [1] max |d var|   [2] max |y - c|   [3] min predicted var (incl. noise)
 *   [4] max |alpha|    [5] kernel variance   [6] tolerance on [0] (absolute)   [7] tolerance on [1]
 *   [8] amplification a: 1 for a float64 factor (GPSO_MIXED / GPSO_F64); for a float factor (GPSO_F32)
 *       max(1, sqrt(sigma^2 max_i (K_y^-1)_ii)) -- the training inputs see the factor's backward error
 *       unamplified, a general leaf amplified by the solve weights (calibrated heuristic)
 *   [9] max_i (K_y^-1)_ii
 *   [10] generation arithmetic in use on this posterior: 0 double, 1 float (GPSO_GEN_AUTO's choice)
 *   [11] predict math in use on this posterior (GPSO_MATH_NATIVE / BF16X3 / BF16X6 / F16X3)
 * Returns GPSO_OK, GPSO_E_PRECISION when sqrt(a) [0] > [6] or a [1] > [7] (or a value is not finite), or
 * GPSO_E_STATE when no fitted posterior with targets is resident. */
int gpso_precision_info(gpso_ctx* ctx, double* out);

/* last-call device timings in milliseconds measured with HIP events on the context's stream:
 * what = 0: dominant predict kernel (leaf tiles) of the last predict/best_ucb call,
 *        1: whole last predict/best_ucb call, 2: whole last gpso_fit_eval / gpso_append call,
 *        3: the collective of the last gpso_best_ucb*_sharded call (ncclAllGather of the winners + the fold kernel).
 * After a SCREENED call (GPSO_OPT_SCREEN) what = 0 spans from the start of the mean pass to the end of the survivors' tile
 * kernel: a figure that prices the batch's algorithmic flops against it prices work the call no longer does. */
double gpso_last_ms(gpso_ctx* ctx, int what);

/* leaf counts of the last predict / best_ucb / best_ucb_grow call: what = 0: rows the predict kernels
 * actually scored, 1: rows of the reference's list.  They differ for gpso_best_ucb_grow, which drops the
 * rows of LeafNode.grow that repeat an earlier row bit for bit (a centre child's centre is its parent's,
 * gpso/param_space.py:186-200: (3^depth - 1) / 2 rows per box, 3^(depth-1) distinct).
 * what = 2: the arithmetic the LARGE PRODUCTS of the last gpso_fit_eval ran on (GPSO_FITMATH_*: what a roofline figure of
 * the fit is priced against -- the f32 / f64 matrix instruction, or the two-level float fit's 16-bit pieces: six bf16 or
 * three fp16 MFMAs per f32 product).
 * what = 3: how many workgroups shared a leaf tile's row blocks in the last launch of a split predict kernel (GPSO_OPT_ROW_LOOP;
 * per context: the last launch THIS context made; for tests and tools).
 * what = 5, 6: k-steps per leaf tile that the last launch of a split predict kernel parked (5) and reloaded instead of generating
 * them (6) under GPSO_OPT_PARK_BYTES; 0 where it parked nothing.  Per context, like what = 3.  A screened call reports its
 * batch-sized launch -- the mean pass -- under 3, 5 and 6, not the survivors' launch.
 * what = 7, 8: the last gpso_best_ucb / gpso_best_ucb_end call under GPSO_OPT_SCREEN: how many leaves survived the screen (7; 0
 * where the call was not screened), and 8: 0 not screened, 1 screened and accepted, 2 screened, refused and run again by the
 * general sequence.
 * what = 9: leaves per workgroup of the last launch of a split predict kernel this context made: 256 (the wide tile) or 64 (the
 * narrow one, GPSO_OPT_SURVIVOR_TILE) -- after a screened call the survivors' launch, unlike 3, 5 and 6.  For tests and tools.
 * what = 4: bytes of device memory the buffers of ALL contexts of this process hold now (process-wide, whichever ctx asks;
 * back where it stood once a context is destroyed; for tests and tools). */
#define GPSO_FITMATH_NONE 0
#define GPSO_FITMATH_SMALL 1   /* N <= 128: one launch, vector arithmetic in double */
#define GPSO_FITMATH_F32 2     /* v_mfma_f32_16x16x4_f32 (float fits up to N_pad = 3584, or GPSO_OPT_FIT_BF16_SYRK = 0) */
#define GPSO_FITMATH_F64 3     /* v_mfma_f64_16x16x4_f64 (float64 / mixed contexts) */
#define GPSO_FITMATH_BF16X6 4  /* two-level float fit: three bf16 pieces per operand, six MFMAs per product */
#define GPSO_FITMATH_F16X3 5   /* two-level float fit: two scaled fp16 pieces per operand, three MFMAs per product */
int64_t gpso_last_count(gpso_ctx* ctx, int what);

const char* gpso_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GPSO_HIP_H */
