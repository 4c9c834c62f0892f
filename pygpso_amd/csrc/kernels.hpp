// Host-callable launchers of the gfx950 kernels (definitions in predict.hip / fit.hip / grow.hip).
//
// Type roles:  TF = fit type (Gram, Cholesky, L^-1, alpha: float | double)
//              T / TP = predict ("apply") type (packed L^-1, alpha, accumulators: float | double)
//              TG = generation type of the cross-Gram tile's x.x* contraction and r^2 (float | double;
//                   double by default also in float contexts, see predict.hip)
#pragma once
#include "acq.hpp"
#include "common.hpp"

namespace gpso {

// ---- runtime helpers (api.hip) ------------------------------------------------------------------
// Opt a kernel into `bytes` of dynamic LDS (> 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize)
// on the CURRENT device; remembered per (function, device), thread-safe.  Returns 0 or a negative
// GPSO_E_* code (also recorded with note_launch_error).
int ensure_dyn_lds(const void* fn, int bytes);
// Remember the first launcher-side error of the call in flight (thread-local); the C-ABI entry
// points turn it into GPSO_E_HIP with this message.
void note_launch_error(const char* msg);

// tile shape of the dominant predict kernel: BM rows of L^-1 x (4 waves * CT * 16) leaves per workgroup
constexpr int kLeafPad = 256;  // leaf batches are padded to a multiple of this
// rows of L^-1 per workgroup for a given padded N and D / 4, and the resulting number of row blocks
template <typename T>
int leaf_tiles_bm(int64_t npad, int dp4);
template <typename T>
inline int leaf_tiles_nbi(int64_t npad, int dp4) { return (int)(npad / leaf_tiles_bm<T>(npad, dp4)); }

// ---- predict.hip ----------------------------------------------------------------------------------
// m_live (nullable, device): number of live leaves; rows at or beyond it are padding
template <typename TG, typename TIN>
void launch_prep_leaves(hipStream_t st, const TIN* xs, int64_t m, int64_t mpad, int d, int dp,
                        const double* ls, const int64_t* m_live, TG* out, TG* norm);
// partial sums per row block of L^-1: part_var / part_mean [nbi][mpad] double
template <typename T, typename TG>
int launch_leaf_tiles(hipStream_t st, const T* linv_p, const TG* xs_p, const TG* xnorm,
                      const T* alpha, const TG* leaves_s, const TG* lnorm, double* part_var,
                      double* part_mean, int64_t npad, int dp4, int64_t mpad, const KernParams& kp,
                      const int64_t* m_live);
// split-bf16 apply (float contexts): nsplit = 2 -> bf16x3, 3 -> bf16x6; needs npad % 256 == 0.
// linv_b = nsplit * npad * npad bf16, produced by launch_pack_linv_bf16 from the fit-type L^-1
// rt0 > 0: only the 16-row tiles from rt0 on are (re)packed -- the rows a gpso_append wrote
template <typename TF>
void launch_pack_linv_bf16(hipStream_t st, int nsplit, const TF* linv, int64_t n, int64_t npad,
                           void* linv_b, int64_t rt0 = 0);
// dynamic LDS of the split-bf16 kernel: A pieces (2 buffers x nsplit x 16 KiB) + 3 X buffers + the 8 waves' leaf
// fragments, for a generation type of tg_bytes
// c16: the contraction runs on the fp16 pipe (float generation only): the X fragments of a k-step and the leaf fragments
// of a wave are fp16 piece pairs of 32-dimension chunks instead of float groups of four dimensions
bool leaf_step32_built();  // predict_split_f32.hip: was the library built with -DGPSO_STEP32=1 (leaf_split.hpp)
inline int leaf_c16_chunks(int dp4) { return (dp4 + 8) / 8; }  // D_pad inputs + the norm slot, 32 slots per chunk
// nw, ct: waves per workgroup and column tiles per wave (8 x 2; the narrow kernel: 4 x 1) -- a wave's leaf fragments are ct
// halves of a k-step's X fragments
inline size_t leaf_bf16_lds_bytes(int nsplit, int dp4, int tg_bytes, bool c16 = false, int nw = 8, int ct = 2) {
  const size_t xfrag = c16 ? (size_t)leaf_c16_chunks(dp4) * 4096 : (size_t)2 * dp4 * 64 * tg_bytes;
  return (size_t)2 * nsplit * 16 * 64 * 16 + (size_t)3 * (xfrag + 64 * tg_bytes + 256) + (size_t)nw * (xfrag / 2 * ct);
}
// fp16 piece pairs of the float scaled inputs in the fragment order of the fp16 contraction (predict.hip); scal: 4 device
// floats ([0] max |x / l|, [1] := 2^sx, [2] := 2^-2sx); xs_h16: npad / 16 * leaf_c16_chunks * 2 KB
void launch_gen_inputs_f16(hipStream_t st, const float* xs32, const float* xnorm32, int64_t npad, int dp, float* scal,
                           void* xs_h16);
// the caller's unscaled float leaves for the fp16-contraction kernels, whose prologue can scale them itself (round 5: the
// prep launch and the dependency gap behind it are 12 us of a 740 us step at C3); x == nullptr: leaves_s / lnorm are read
struct RawLeaves {
  const float* x = nullptr;
  const double* ls = nullptr;  // lengthscale per input dimension (device)
  int64_t m = 0;
  int d = 0;
};
// the leaves a workgroup of the split kernels owns: 256 (8 waves x 2 column tiles of 16) or 64 (4 waves x 1)
enum class LeafTile : int { Wide = 0, Narrow = 1 };
// What one launch of the split leaf-tile kernels reads and reports (launch_leaf_tiles_bf16): the posterior's operands,
// the leaf batch, and the launching context's own settings -- nothing about a launch lives outside this struct
template <typename TG>
struct SplitLeafLaunch {
  int nsplit = 2;                // pieces of L^-1: 2 -> bf16x3 (or f16x3: f16_inv_scale_a), 3 -> bf16x6
  const void* linv_b = nullptr;  // nsplit * npad * npad 16-bit pieces (launch_pack_linv_bf16 / _f16)
  const TG* xs_p = nullptr;
  const TG* xnorm = nullptr;
  const float* alpha = nullptr;
  const TG* leaves_s = nullptr;
  const TG* lnorm = nullptr;
  double* part_var = nullptr;  // partial sums per row block of L^-1: [npad / 256][mpad] double
  double* part_mean = nullptr;
  int64_t npad = 0;  // a multiple of 256
  int dp4 = 0;
  int64_t mpad = 0;
  const int64_t* m_live = nullptr;  // (nullable, device): number of live leaves; rows at or beyond it are padding
  // != nullptr: the fp16 split (two pieces, three products; predict.hip) -- linv_b and the scale (device, 2 floats:
  // max |L^-1|, 2^-sa) come from launch_pack_linv_f16
  const float* f16_inv_scale_a = nullptr;
  // both set: the contraction on the fp16 pipe as well (fp16 split, float generation; launch_gen_inputs_f16)
  const void* xs_h16 = nullptr;
  const float* c16_scale = nullptr;
  int64_t n_rows = 0;  // N (0: unknown) -- the fused step stops at the k-steps that hold padding points only
  RawLeaves raw;       // (fp16 contraction only)
  bool step32 = false;  // GPSO_SPLIT_KERNEL_FUSED32 -- the fused step on the 32x32x16 instruction, where built
  // Narrow: 64 leaves per workgroup (4 waves x 1 column tile) where the default family runs -- fp16 split, fp16 contraction,
  // fused step, float generation (leaf_narrow_applies); every other launch is the wide kernel whatever this says.  Same bits.
  LeafTile tile = LeafTile::Wide;
  int row_loop = 1;     // GPSO_OPT_ROW_LOOP of the launching context (leaf_split.hpp: leaf_row_splits)
  int cu_count = 256;   // compute units of the launching context's device
  int64_t* splits_out = nullptr;  // (nullable) receives the workgroups per leaf tile the launcher chose
  int64_t* tile_out = nullptr;    // (nullable) receives the leaves per workgroup of the kernel launched: 256 wide, 64 narrow
  // GPSO_OPT_PARK_BYTES of the launching context (leaf_split.hpp, PARK): the budget (0: off), and who grants a device buffer of
  // at least `bytes` for the parked pieces (nullptr to decline: the launch then parks nothing); owner: the launching context
  int64_t park_bytes = 0;
  void* (*park_scratch)(void* owner, size_t bytes) = nullptr;
  void* park_owner = nullptr;
  int64_t* park_out = nullptr;  // (nullable) receives, per leaf tile: [0] k-steps parked, [1] k-steps reloaded instead of generated
};
// FUSED: the fused step (round 4) or round 3's two-phase step -- same bits; one explicit instantiation per slice
// (TG, FUSED, KS) in predict_split_*.hip
template <typename TG, bool FUSED, int KS /* kernel families 0-1 | 2-3 */>
int launch_leaf_tiles_bf16_v(hipStream_t st, const KernParams& kp, const SplitLeafLaunch<TG>& a);
// the narrow kernels (predict_split_f32_narrow.hip: all four kernel families in one translation unit), and where they exist
int launch_leaf_tiles_narrow(hipStream_t st, const KernParams& kp, const SplitLeafLaunch<float>& a);
template <typename TG>
inline bool leaf_narrow_applies(const SplitLeafLaunch<TG>& a, bool fused) {
  return sizeof(TG) == 4 && fused && a.nsplit == 2 && a.f16_inv_scale_a != nullptr && a.xs_h16 != nullptr && a.c16_scale != nullptr &&
         !a.step32 && leaf_c16_chunks(a.dp4) <= 2;
}
// variant: GPSO_OPT_SPLIT_KERNEL (0 the fused step, 1 the two-phase step)
template <typename TG>
inline int launch_leaf_tiles_bf16(hipStream_t st, const KernParams& kp, const SplitLeafLaunch<TG>& a, int variant = 0) {
  const bool low = kp.kernel == 0 || kp.kernel == 1;
  auto* fn = variant != 1 ? (low ? launch_leaf_tiles_bf16_v<TG, true, 0> : launch_leaf_tiles_bf16_v<TG, true, 1>)
                          : (low ? launch_leaf_tiles_bf16_v<TG, false, 0> : launch_leaf_tiles_bf16_v<TG, false, 1>);
  return fn(st, kp, a);
}
// scal: 2 device floats -- [0] max |L^-1|, [1] := 2^-sa.  have_max false: the maximum is computed here first (memset +
// absmax_kernel); true: the fit left it in scal[0] (launch_solve_alpha: its own pass over L^-1).
// rt0 > 0 (after a gpso_append; scal[0] already holds the new maximum, scal[3] the 2^-sa the resident pieces were packed
// with): only the 16-row tiles from rt0 on are repacked -- unless the maximum crossed a power of two, which the kernel
// sees on the device and then repacks everything
template <typename TF>
void launch_pack_linv_f16(hipStream_t st, const TF* linv, int64_t n, int64_t npad, float* scal, void* linv_b,
                          bool have_max = false, int64_t rt0 = 0);
// what finalising a leaf needs (leaf_finalize_kernel, or fused into the arg-max's first stage: launch_seg_argmax)
struct LeafFinalize {
  const double* part_var = nullptr;
  const double* part_mean = nullptr;
  int nbi = 0;
  int64_t mpad = 0;
  double variance = 0, noise = 0, mean_c = 0, varsigma = 0;
  double* mean = nullptr;
  double* var = nullptr;
  double* ucb = nullptr;
  // nullable: the leaves' squared norms (generation type: float | double).  A leaf with a NaN coordinate has a NaN norm
  // and gets NaN mean / var / ucb -- what GPflow returns for it (and np.argmax then picks it); the kernel map's clamp
  // max(r^2, 1e-36) would otherwise turn its r^2 into 0 against every training point (finite garbage, negative variance)
  const void* lnorm = nullptr;
  int lnorm_f64 = 0;
  // what the `ucb` column holds and the arg-max ranks by (acq.hpp); uniform over a launch.  GPSO_ACQ_UCB_VAR reads
  // varsigma only and keeps the arithmetic above; the other kinds read the latent variance (variance - sum) when
  // `latent` is set, the predictive one otherwise
  int kind = GPSO_ACQ_UCB_VAR, latent = 0;
  double incumbent = 0, xi = 0;
  // GPSO_ACQ_MES: the context's sampled maxima (device memory) and their count
  const double* ystar = nullptr;
  int nystar = 0;
  LeafFinalize& with(const AcqSpec& a) {
    ystar = a.ystar;
    nystar = a.nystar;
    varsigma = a.varsigma;
    kind = a.kind;
    latent = a.latent;
    incumbent = a.incumbent;
    xi = a.xi;
    return *this;
  }
};
void launch_leaf_finalize(hipStream_t st, const double* part_var, const double* part_mean, int nbi,
                          int64_t mpad, int64_t m, const KernParams& kp, const AcqSpec& acq,
                          double* mean, double* var, double* ucb, const void* lnorm = nullptr, int lnorm_f64 = 0);
void launch_seg_argmax(hipStream_t st, const double* mean, const double* var, const double* ucb,
                       const int64_t* seg_off_dev, int nseg, int nblk, void* partial_dev,
                       double* out_vals_dev /* [nseg*4 + 2]: per segment mean, var, ucb, bit-cast int64 index; spare; 0.0 (status slot) */,
                       const LeafFinalize* fin = nullptr /* the leaves are still partial sums: finalise them in stage 1 */,
                       double* host_vals = nullptr /* pinned host copy of out_vals, written by the kernel itself */,
                       double done_token = 0.0 /* nseg == 1 only: host_vals[nseg * 4 + 2] := token behind the records */);
// arg-max over a de-duplicated, keyed leaf list (grow.hip: launch_grow_unique); out_vals_dev[nseg*4 + 2]:
// per segment mean, var, ucb, bit-cast reference row index; then the bit-cast live row count; then 0.0 (status slot)
void launch_keyed_argmax(hipStream_t st, const double* mean, const double* var, const double* ucb,
                         const int64_t* key_dev, int64_t rows, int64_t uniq, int nseg, const int64_t* live_dev,
                         int nblk, void* partial_dev, int64_t* pos_dev, double* out_vals_dev,
                         const LeafFinalize* fin = nullptr, double* host_vals = nullptr, double done_token = 0.0,
                         const int64_t* screen_ctl = nullptr /* the list holds a screened call's survivors (launch_screen's ctl): the
                         last kernel judges the record (screen.hpp: screen_accepts) -- status slot 1.0: refused; the slot in front of
                         it: the survivors' count */, int64_t screen_cap = 0);

// ---- maxcdf.hip: the law of the maximum at g thresholds (gpso_max_logcdf) ------------------------------------------------
// mean / var [m] and y_dev [g] on the device; partial: max_logcdf_blocks(m) * kMaxCdfSlots doubles; out [g + 1] on the
// device: the g sums, then the number of rows without a NaN.  Two launches, no atomics, a grid that depends on m only
constexpr int kMaxCdfThresholds = 64, kMaxCdfSlots = kMaxCdfThresholds + 1, kMaxCdfLeaves = 512;
inline int64_t max_logcdf_blocks(int64_t m) { return (m + kMaxCdfLeaves - 1) / kMaxCdfLeaves; }
void launch_max_logcdf(hipStream_t st, const double* mean, const double* var, int64_t m, double var_sub, const double* y_dev, int g,
                       double* partial, double* out);

// ---- screen.hip: screened best-UCB calls (screen.hpp) ------------------------------------------------------------------
// The mean pass of a batch of m float leaves: my[m], every leaf's mean -- the bits the split tile kernel with the fp16 split and
// the fp16 contraction, and the finalize stage behind it, give it -- from the generation of the diagonal k-steps alone, and
// block_max[*nblk_out], the largest FINITE mean of every block of leaves (-inf: none).  Float generation; leaves: raw.x
// (unscaled, the kernel scales them as the tile kernel's prologue does) or leaves_s (scaled).  A workgroup owns 128 leaves.
// Where the batch fills the chip (two leaf tiles per CU or more) it walks all their row blocks in ascending order and keeps
// the f64 sum of the shares in registers: one launch, part_mean untouched.  A smaller batch splits a tile's row blocks over
// gridDim.y workgroups; their shares go through part_mean[npad / 256][mpad] and a second launch sums them.
// *splits_out: leaf_row_splits' value for a batch of this size -- what the tile kernel's launch of the same batch would
// report --, whatever grid the mean pass itself uses.
struct LeafMeanLaunch {
  const void* xs_h16 = nullptr;
  const float* alpha = nullptr;
  const float* c16_scale = nullptr;
  const float* leaves_s = nullptr;
  RawLeaves raw;
  double* part_mean = nullptr;  // scratch, [npad / 256][mpad]
  int64_t npad = 0, mpad = 0, m = 0, n_rows = 0;
  int dp4 = 0;
  double mean_c = 0;
  double* my = nullptr;         // [m]
  double* block_max = nullptr;  // [mpad / 128]
  int* nblk_out = nullptr;
  int row_loop = 1, cu_count = 256;
  int64_t* splits_out = nullptr;
};
int launch_leaf_mean(hipStream_t st, const KernParams& kp, const LeafMeanLaunch& a);
// The screen and the ordered compaction of the mean pass's my / block_max (two launches over screen_parts(m) workgroups, none
// of which waits for another: every part counts its survivors, then every part sums the counts in front of it and writes its
// own): key[cap] the survivors' indices, ascending; rows_out[cap][d] their raw rows, and zero rows from the live count up to the
// next multiple of 256; ctl (3 x int64): live rows = min(count, cap), count, T' (bit-cast); counts[kScreenMaxParts] scratch;
// probe (nullable, [2][m]): every leaf's ub and survive flag
struct ScreenLaunch {
  const double* my = nullptr;
  const double* block_max = nullptr;
  int nblk = 0;
  int64_t m = 0;
  double variance = 0, noise = 0, varsigma = 0;
  const float* raw = nullptr;
  int d = 0;
  int64_t cap = 0;  // a multiple of 256
  int64_t narrow_max = 0;  // counts up to this take the narrow tile of the survivors' launch (screen.hpp: survivor_narrow_max)
  int64_t* counts = nullptr;
  int64_t* key = nullptr;
  float* rows_out = nullptr;
  int64_t* ctl = nullptr;
  double* probe = nullptr;
};
void launch_screen(hipStream_t st, const ScreenLaunch& a);
// screen.hpp on the host (gpso_screen_*_host: the CPU tests)
void screen_eval_host(const double* my, const double* v, double variance, double noise, double varsigma, long long n,
                      double* ucb, double* ub);
double screen_threshold_host(double max_my, double noise, double varsigma);
int screen_survives_host(double my, double ub, double threshold);
int screen_accepts_host(double u_star, double threshold, long long count, long long cap);
void screen_partition_host(long long m, int parts, int w, long long* lo, long long* hi);
int screen_parts_host(long long m);
// out_dev[c] = number of live leaves inside chunk c of a batch whose total live count is *live_dev
void launch_chunk_live(hipStream_t st, const int64_t* live_dev, int64_t chunk, int nchunk, int64_t* out_dev);
// *acc += sum_i mix(words[i], i, salt)  (64-bit wrap-around sum of a per-word mix: order-independent, so the parallel
// reduction is deterministic) -- the posterior fingerprint of gpso_posterior_hash
void launch_hash_words(hipStream_t st, const void* words, size_t nwords, uint64_t salt, unsigned long long* acc);
constexpr int kArgmaxBlocks = 256;     // stage-1 blocks per segment, at most (argmax_blocks picks: one pass of 256 leaves per block)
inline int argmax_blocks(int64_t m, int nseg) {
  const int64_t per_seg = (m / (nseg > 0 ? nseg : 1) + 255) / 256;
  return (int)(per_seg < 1 ? 1 : per_seg > kArgmaxBlocks ? kArgmaxBlocks : per_seg);
}
constexpr size_t kArgmaxPartialBytes = 16;  // sizeof(Best)

// ---- fit.hip --------------------------------------------------------------------------------------
// scaled inputs: xs[npad*dp] = X/ls (zero padded), xnorm[npad], xs_p (nullable) = MFMA-fragment packing
template <typename T>
void launch_scale_x(hipStream_t st, const double* x64, int64_t n, int64_t npad, int d, int dp,
                    const double* ls, T* xs, T* xnorm, T* xs_p);
// float generation inputs (xs, xnorm, fragment packing) derived from the double scaled inputs
void launch_gen_inputs_f32(hipStream_t st, const double* xs64, int64_t npad, int dp, float* xs, float* xnorm,
                           float* xs_p);
// K = k(X, X) + noise * I on rows < n (lower 64x64 tiles only); identity on the padding.  r^2 is
// always formed in double from the double scaled inputs.  sdiag (device [npad], nullable): per-point noise s, the
// diagonal then receives noise + s_i (one double addition, rounded to T where noise is).
template <typename T>
void launch_gram(hipStream_t st, const double* xs, const double* xnorm, int64_t n, int64_t npad, int dp,
                 const KernParams& kp, T* K, int* info = nullptr /* device: set to INT_MAX ("no failing pivot") */,
                 const double* sdiag = nullptr);
// blocked right-looking Cholesky, K (destroyed) -> Lf (lower); also writes the inverted 64x64 diagonal
// blocks into linv, the unrounded diagonal of L to diag64[npad], and the first failing pivot (or
// INT_MAX) to info
// Returns bit flags.  Bit 0: linv already holds the COMPLETE inverse (small sizes: it is built beside
// the factorisation, using work as scratch) and launch_trtri must be skipped.  Bit 1: kinv (nullable:
// only wanted with the gradient) already holds K^-1 = L^-T L^-1 (lower tiles).
// Float fits above the single-level limit can run their large products on the bf16 matrix cores (3-way split,
// six bf16 MFMAs per product: float-class accuracy).  The operands then live as bf16 planes of N_pad x N_pad
// matrices (fit_plane_set_bytes(npad) each): L, X = L^-1, XT = X^T, WT = scratch (fit.hip: gemm_bf16_kernel).
struct FitPlanes {
  unsigned short *L, *X, *XT, *WT;
  int64_t stride;  // 16-bit elements between the planes of a set
  int nkb;         // npad / 32
  // Round 5: the planes hold either three bf16 pieces per value (np = 3: six MFMAs per product) or TWO fp16 pieces of the
  // value times a power of two (np = 2: three MFMAs per product -- the split that carries the predict path): fp16 has 5
  // exponent bits, so every plane set is scaled into its range by a bound known on the host -- |L| <= sqrt(s2 + noise),
  // |L^-1| <= 1 / sqrt(noise), |L[B,A] L^-1[A,A]| <= sqrt((s2 + noise) / noise) -- with 2^13 as the scaled bound (a factor
  // of 8 below fp16's largest number); fit_plane_scales() fills them
  int np = 3;
  float sL = 1.0f, sX = 1.0f, sW = 1.0f;
  // look-ahead (all three set, or none): the next diagonal block is factored on `side` while the rest of the
  // current rank-W update runs on the caller's stream; ev_col / ev_chain order the two streams
  hipStream_t side = nullptr;
  hipEvent_t ev_col = nullptr, ev_chain = nullptr;
  // Round 6 (double fits; L == nullptr): `side` also carries the look-ahead of the float64 two-level fit, and `inv` (nullable)
  // the level-doubling inverse, issued pair by pair as soon as the panels it reads are final -- the first product of the last
  // level starts when HALF of the factorisation is done (launch_potrf); ev_panel / ev_inv order the streams
  hipStream_t inv = nullptr;
  hipEvent_t ev_panel = nullptr, ev_inv = nullptr;
  int overlap = 0;  // double fits: bit 0 look-ahead on `side`, bit 1 the inverse on `inv` (GPSO_OPT_FIT_OVERLAP)
  int cu_count = 256;  // compute units of the fitting context's device: the grid of the persistent bf16 GEMMs
};
inline size_t fit_plane_set_bytes(int64_t npad) { return (size_t)3 * (size_t)npad * (size_t)npad * 2; }
// power-of-two scales of the fp16 planes for hyper-parameters (variance, noise); false: a scale leaves the range in which
// the second piece of a typical entry is still a normal fp16 number (noise / variance below ~1e-9): keep bf16 pieces
// s_max: the largest per-point noise term on the diagonal (0 without one) -- |L| <= sqrt(s2 + noise + s_max)
bool fit_plane_scales(double variance, double noise, FitPlanes& pl, double s_max = 0.0);
// planes (float fits, nullable): with them the TRSM GEMMs also emit L into planes->L and the rank-W trailing
// updates run on the bf16 matrix cores
// does launch_potrf take the single-level path at this size?  (It then writes every entry of L^-1 that anything reads --
// the lower 64-tiles, diagonal tiles whole -- and linv needs no zero fill; the two-level path's GEMMs read whole panels.)
template <typename T>
bool potrf_is_single_level(int64_t npad, int64_t single_level_max /* < 0: default */);
template <typename T>
int launch_potrf(hipStream_t st, T* K, T* Lf, T* linv, T* work, T* kinv, int64_t n, int64_t npad,
                 double* diag64, int* info, int64_t single_level_max /* < 0: default */, const FitPlanes* planes);
// the level-doubling inverse on the bf16 matrix cores (after a launch_potrf with the same planes)
void launch_trtri_bf16(hipStream_t st, float* linv, const FitPlanes& planes, int64_t npad, int64_t first_level,
                       bool keep_xt /* also emit the planes of L^-T at the last level (K^-1 for the gradient) */);
bool trtri_bf16_applies(int64_t npad, int64_t first_level);
// L^-1 by level-doubling from level first_level (64 or the factorisation's outer panel width): needs the
// inverses of the first_level-wide diagonal blocks already in linv; work = npad x npad scratch
// width of the diagonal blocks of the two-level factorisation (and first level of the level-doubling
// inverse).  Measured (posterior fit, float, ms, 512 | 1024): N 4096 1.78 | 1.66, 8192 6.16 | 5.91,
// 16384 29.95 | 30.18 -- the wider panel halves the passes over the trailing matrix, which pays while
// the SYRKs are short.
inline int fit_outer_panel(int64_t npad) { return (npad >= 4096) ? 1024 : 512; }
template <typename T>
void launch_trtri(hipStream_t st, const T* L, T* linv, T* work, int64_t npad, int64_t first_level);
// zero rows/cols >= n and re-tile the lower 16x16 tiles of L^-1 into the MFMA fragment-major layout
// the predict kernel reads: npad16 (npad16 + 1) / 2 tiles of 256 elements
template <typename TF, typename TP>
void launch_pack_linv(hipStream_t st, const TF* linv, int64_t n, int64_t npad, TP* linv_p, int64_t rt0 = 0 /* first 16-row tile row to pack */);
inline size_t packed_linv_elems(int64_t npad) { return (size_t)(npad / 16) * (size_t)(npad / 16 + 1) / 2 * 256; }
// a = L^-1 (y - c), alpha = L^-T a, nlml = 1/2 a.a + sum log diag64 + n/2 log 2pi  (double accumulators);
// kinv_diag[npad] = squared column norms of L^-1 = diag((K + noise I)^-1)
constexpr int kAlphaChunk = 64;
inline size_t alpha_part_doubles(int64_t npad) { return (size_t)2 * ((npad + kAlphaChunk - 1) / kAlphaChunk) * npad; }
template <typename T>
void launch_solve_alpha(hipStream_t st, const T* linv, const double* y64, int64_t n, int64_t npad,
                        double mean_c, const double* diag64, T* white, T* alpha,
                        double* alpha_part /* alpha_part_doubles(npad) scratch */, double* kinv_diag,
                        double* nlml_out, void* alpha_p = nullptr /* predict-type copy of alpha */, int alpha_p_f64 = 0,
                        float* amax_rows = nullptr /* [npad] scratch */, float* linv_absmax = nullptr /* receives max |L^-1| */);
// Kinv = L^-T L^-1 (lower tiles; skipped when kinv_ready), then the gradient reductions of SURVEY.md A.3;
// grad_out[n_ls + 3] = d nlml / d (ls..., variance, noise, c)
template <typename T>
void launch_gradient(hipStream_t st, const T* linv, const T* alpha, const double* xs, const double* xnorm,
                     int64_t n, int64_t npad, int d, int dp, int n_ls, const double* ls,
                     const KernParams& kp, T* kinv, bool kinv_ready, double* partial, double* grad_out,
                     const FitPlanes* xt_planes = nullptr /* float: planes of L^-T left by launch_trtri_bf16(keep_xt) */);
constexpr int kGradMaxLs = 64;
// fused single-launch fit for N <= 128 (one workgroup, matrices in LDS): everything launch_scale_x<double>
// .. launch_pack_linv / launch_convert_vec produce, in one kernel (definition + field docs: fit.hip)
struct SmallFitArgs {
  const double* x64;
  const double* y64;
  double ls[48];     // lengthscale per input dimension (isotropic: repeated), by value: the kernel also
                     // writes the hyper-parameter block the predict path reads, so the evaluation needs no
                     // host-to-device copy of its own
  double* hyper;     // [8 + 48] hyper-parameter block (device, output)
  int n, d, dp, kernel, n_ls, want_grad;
  int zero_tile_rows;  // 16-row tile rows of linv_p an earlier fit may have left non-zero (8 = unknown)
  double variance, noise, mean_c;
  const double* sdiag;  // [128] per-point noise s (device, nullable): the diagonal receives noise + s_i
  // outputs
  double* xs64;    // [128 * dp] scaled inputs
  double* xnorm64; // [128]
  double* xs_p64;  // [128 * dp] MFMA A fragments (double layout)
  void* Lf;        // [128 * 128] T
  void* linv;      // [128 * 128] T
  void* kinv;      // [128 * 128] T, nullable
  void* white;     // [128] T
  void* alpha_f;   // [128] T
  void* alpha_p;   // [128] TP
  void* linv_p;    // packed lower tiles, TP
  double* diag64;  // [128]
  double* kinv_diag;  // [128]
  double* scal;    // [0] nlml, [1] info (int), [8 ..] gradient (ls..., variance, noise, c)
  double* scal_host;  // nullable: pinned host memory (device-visible) that receives the same scalars straight from the
                      // kernel -- the evaluation then needs no device-to-host copy operation behind it either
  double done_token;  // != 0: scal_host[7] := token behind the scalars (system-scope release; the host spins on it)
};

bool small_fit_eligible(int64_t n, int dp);
template <typename T, typename TP>
int launch_small_fit(hipStream_t st, const SmallFitArgs& args);

// the same evaluation at B values of theta in ONE launch, one workgroup per theta (multi-start hyper-parameter search):
// loss, gradient and the factorisation's verdict per entry and nothing else -- no buffer a predict or a later fit reads
// is written, so a resident posterior stays as it is
constexpr int kSmallBatchMax = 256;   // workgroups per launch: one per CU (the LDS of one fills a CU's)
constexpr int kSmallBatchTheta = 56;  // doubles per theta record: [0] variance, [1] noise, [2] mean c, [8 + k] lengthscale of
                                      // padded dimension k < 48 (isotropic: repeated) -- the hyper block's layout
struct SmallBatchArgs {
  const double* x64;
  const double* y64;
  const double* theta;  // [B][kSmallBatchTheta], device memory
  double* loss;         // [B]
  double* grad;         // [B][n_ls + 3]: d nlml / d (ls..., variance, noise, c)
  int* info;            // [B]: failing pivot, INT_MAX = positive definite
  int n, d, dp, kernel, n_ls, want_grad;
  const double* sdiag;  // [128] per-point noise s shared by every entry (device, nullable)
};
template <typename T, typename TP>
int launch_small_fit_batch(hipStream_t st, const SmallBatchArgs& args, int b);

// precision self-test: predictions at the training inputs vs the closed form the fit implies;
// out[6] = max |d mean|, max |d var|, max |y - c|, min predicted var, max |alpha|, max_i (K_y^-1)_ii
template <typename T>
void launch_selftest(hipStream_t st, const double* mean, const double* var, const double* y64,
                     const T* alpha, const double* kinv_diag, int64_t n, double noise, double mean_c,
                     double* out, const double* sdiag = nullptr /* device [n], per-point noise: the closed forms use noise + s_i */);

// conversions and getters
template <typename TS, typename TD>
void launch_convert_vec(hipStream_t st, const TS* src, TD* dst, int64_t len);
template <typename T>
void launch_convert_in(hipStream_t st, const double* src, T* dst, int64_t rows, int64_t cols,
                       int64_t ld_dst);
template <typename T>
void launch_convert_out(hipStream_t st, const T* src, int64_t ld_src, double* dst, int64_t rows,
                        int64_t cols, int lower_only);
// install L (row-major lower, n x n float64 on device) into the padded T buffer + invert diagonal blocks
template <typename T>
void launch_install_chol(hipStream_t st, const double* L64, int64_t n, int64_t npad, T* K, T* linv);
// linv = L^-1 of a padded lower factor already on the device (its lower triangle is read; a non-zero diagonal on the padding
// too): linv is zeroed, the 64-wide diagonal blocks are inverted, then launch_trtri doubles the levels; work = npad x npad
template <typename T>
void launch_trinv(hipStream_t st, const T* L, T* linv, T* work, int64_t npad);

// C = alpha op(A) op(B) + beta C, whole N_pad x N_pad float64 matrices (fit.hip; N_pad a multiple of 64)
void launch_dgemm(hipStream_t st, const double* A, bool trans_a, const double* B, bool trans_b, double* C, int64_t npad,
                  double alpha, double beta);
// ---- vgp.hip: variational GP (dense N_pad x N_pad float64 buffers, rows / columns >= n are padding) --------------------
void launch_vgp_clean_lower(hipStream_t st, const double* src, double* dst, int64_t n, int64_t npad, double pad_diag);
void launch_vgp_pad_identity(hipStream_t st, double* m, int64_t n, int64_t npad, int* info /* nullable: := INT_MAX */);
void launch_vgp_axpby(hipStream_t st, const double* x, double* y, int64_t len, double a, double b);
// out = (sub ? sub - v : v), v = alpha op(A) (x - xshift) + add on rows < n (trans: add ignored, sub must be NULL)
void launch_vgp_gemv(hipStream_t st, const double* A, bool trans, const double* x, double xshift, double alpha, double add,
                     const double* sub, double* out, int64_t n, int64_t npad);
void launch_vgp_rownorm(hipStream_t st, const double* A, double* out, int64_t n, int64_t npad);
void launch_vgp_lbar(hipStream_t st, double* lsig, const double* r, const double* mu, int64_t n, int64_t npad, double inv_s2);
void launch_vgp_phi_sym(hipStream_t st, const double* p, double* m, int64_t n, int64_t npad);
void launch_vgp_reverse(hipStream_t st, const double* src, double* out, int64_t n, int64_t npad, int mode, int* info);
void launch_vgp_elbo_sums(hipStream_t st, const double* r, const double* fvar, const double* mu, const double* srow,
                          const double* S, int64_t n, int64_t npad, double* out);
// general scalar likelihoods (kind: GPSO_LIK_STUDENT_T or GPSO_LIK_GAUSSIAN_GH; p: its parameter; gh: [0, 64) nodes,
// [64, 128) weights, scaled as GPflow's): per point gm, a, t = gm + a (m - c), VE and dVE/dp
void launch_vgp_quad(hipStream_t st, const double* y, const double* m, const double* v, const double* gh, int n_gh, int kind,
                     double p, double nu, double cst, double c, double* gm, double* a, double* t, double* ve, double* dve,
                     int64_t n, int64_t npad);
void launch_vgp_lik_sums(hipStream_t st, const double* ve, const double* dve, const double* gm, const double* mu,
                         const double* srow, const double* S, int64_t n, int64_t npad, double* out);
void launch_vgp_lbar_w(hipStream_t st, double* lsig, const double* a, const double* gm, const double* mu, int64_t n,
                       int64_t npad);
void launch_vgp_rowscale(hipStream_t st, const double* A, const double* a, double* B, int64_t n, int64_t npad);
// ---- loo.hip: leave-one-out predictive and LOO-CV objective of the exact GP ---------------------
// vec: kLooVecs vectors of N_pad doubles, zero on the padding -- the predictive (mean, var, lpd), sqrt c, g / sqrt c, h and
// a vector of zeros (the alpha the weight contraction is called with)
enum { kLooMean = 0, kLooVar = 1, kLooLpd = 2, kLooSc = 3, kLooT = 4, kLooH = 5, kLooZero = 6, kLooVecs = 7 };
// the per-point pass from the resident alpha (fit type) and kinv_diag; loss_out[0] = -sum lpd (one workgroup, fixed order)
template <typename T>
void launch_loo_points(hipStream_t st, const T* alpha, const double* kinv_diag, const double* y64, int64_t n, int64_t npad,
                       double* vec, double* loss_out);
// after launch_loo_points: S := diag(sqrt c) K_y^-1 (kinv: lower triangle read), M := S^T S, h := K_y^-1 g into vec, then
// S := 2 W = 2 M - (h alpha^T + alpha h^T) on the lower 64-tiles, zero on the padding -- what launch_gradient takes as its
// kinv with kinv_ready and the zero vector for alpha.  S, M: N_pad^2 doubles each
void launch_loo_weights(hipStream_t st, const double* kinv, const double* alpha, double* vec, double* S, double* M, int64_t n,
                        int64_t npad);
// out[0] = dF/dc = -sum h
void launch_loo_mean_grad(hipStream_t st, const double* vec, int64_t n, int64_t npad, double* out);
// N <= 128, behind the one-launch fit with want_grad: the point pass, M, h and the contraction with dK in ONE workgroup
struct LooSmallArgs {
  const double* kinv;       // [npad * npad] K_y^-1, lower triangle read
  const double* alpha;      // [npad]
  const double* kinv_diag;  // [npad]
  const double* y64;        // [n]
  const double* xs;         // [npad * dp] scaled inputs
  const double* ls;         // lengthscale per padded dimension (device: the hyper block)
  int n, npad, dp, kernel, n_ls;
  double variance;
  double* vec;        // nullable: mean, var, lpd at kLooMean / kLooVar / kLooLpd
  double* scal;       // [0] loss, [8 ..] gradient (ls..., variance, noise, c)
  double* scal_host;  // nullable: pinned host memory that receives the same scalars
  double done_token;  // != 0: scal_host[7] := token behind the scalars
};
int launch_loo_small(hipStream_t st, const LooSmallArgs& args);
// ---- predict_grad.hip: mean, variance and their gradients in the test points ---------------------
constexpr int64_t kJointMaxDraws = (int64_t)1 << 20;  // draws per gpso_sample_joint call (a workgroup of pj_argmax_kernel each)
constexpr int64_t kPredictGradChunk = 1024;  // test points per launch sequence: the workspace does not grow with M
struct PredictGradLaunch {
  const double* C = nullptr;      // [npad * npad] dense fit-type factor; read only where column <= row < n
  const double* alpha = nullptr;  // [npad]
  const double* xs = nullptr;     // [npad * dp] scaled rows
  const double* ls = nullptr;     // lengthscale per padded dimension (device: the hyper block)
  const double* ts = nullptr;     // [roundup(m, 64) * dp] scaled test points, zero rows behind the m live ones
  int64_t n = 0, npad = 0, m = 0; // m <= kPredictGradChunk
  int d = 0, dp = 0;
  KernParams kp{0, 1.0, 0.0, 0.0};
  double* work = nullptr;         // predict_grad_workspace_doubles(npad, dp, roundup(m, 64)) doubles
  double *mean = nullptr, *var = nullptr, *dmean = nullptr, *dvar = nullptr;  // device, [m], [m], [m * d], [m * d]; each nullable
};
size_t predict_grad_workspace_doubles(int64_t npad, int dp, int64_t mc);
int launch_predict_grad(hipStream_t st, const PredictGradLaunch& g);
// the apply stage alone: V = C k* in the layout [roundup(m, 64) / 64][npad][64] at g.work, whose rows are written up to
// ceil(n / 128) * 128 only, followed by the partial |v|^2 (g.alpha, g.ls and the outputs are not read); g.work holds
// predict_grad_apply_workspace_doubles(npad, roundup(m, 64)) doubles
size_t predict_grad_apply_workspace_doubles(int64_t npad, int64_t mc);
int launch_predict_grad_apply(hipStream_t st, const PredictGradLaunch& g);
// ---- joint.hip: the joint predictive at m <= kPredictGradChunk test points -----------------------
struct JointLaunch {
  const double* V = nullptr;      // launch_predict_grad_apply's V for the same n, npad, m, ts
  const double* ts = nullptr;     // [roundup(m, 64) * dp] scaled test points, zero rows behind the m live ones
  const double* alpha = nullptr;  // [npad]
  const double* xs = nullptr;     // [npad * dp] scaled rows
  int64_t n = 0, npad = 0, m = 0;
  int dp = 0;
  KernParams kp{0, 1.0, 0.0, 0.0};
  double diag_add = 0.0;          // added to the diagonal of Sigma
  double* part = nullptr;         // joint_partial_doubles(n, m) doubles
  double* mean = nullptr;         // [m], nullable
  double* cov = nullptr;          // Sigma = K** - V^T V + diag_add I with leading dimension ldc, nullable
  int64_t ldc = 0;
  // true: ldc >= roundup(m, 64) and the rows / columns m .. roundup(m, 64) - 1 receive the identity's entries (a matrix
  // handed to launch_potrf); false: ldc >= m and nothing beyond the m x m block is written
  bool pad_identity = false;
};
// the contraction over the training rows is split into this many pieces of *chunk_rows rows (a multiple of 128) each: a
// function of (n, m) alone, so a call's bits are too
int joint_splits(int64_t n, int64_t m, int64_t* chunk_rows);
size_t joint_partial_doubles(int64_t n, int64_t m);
int launch_joint(hipStream_t st, const JointLaunch& g);
// f[s][c] = mu[c] + sum_{j <= c} L[c][j] z[s][j] (L lower with leading dimension ldl; z, f [s][m] row-major)
void launch_joint_draw(hipStream_t st, const double* L, int64_t ldl, const double* z, const double* mu, int64_t m, int64_t s,
                       double* f);
// per row of f [s][m]: the highest value and its index, the lowest on ties (idx, val [s], each nullable)
void launch_joint_argmax(hipStream_t st, const double* f, int64_t m, int64_t s, int64_t* idx, double* val);
// ---- paths.hip: pathwise posterior draws of the exact GP ---------------------------------------------
constexpr int64_t kPathsMaxDraws = 256;       // draws of a path set
constexpr int64_t kPathsMaxFeatures = 65536;  // random Fourier features of a path set
constexpr int64_t kPathsChunk = 16384;        // points per launch sequence of gpso_paths_eval: the workspace does not grow with M
struct PathsEvalLaunch {
  const double* ts = nullptr;     // [roundup(m, 64) * dp] scaled points, finite rows behind the m live ones
  const double* xs = nullptr;     // [npad * dp] scaled training rows
  const double* omega = nullptr;  // [roundup(f, 16) * dp] frequencies in scaled coordinates, zero padding
  const double* phase = nullptr;  // [roundup(f, 16)]
  const double* W = nullptr;      // [s][ldw] feature weights, ldw >= f
  const double* VT = nullptr;     // [roundup(s, 64)][npad] v^T; nullptr: features only, and no constant mean
  int64_t n = 0, npad = 0, m = 0, s = 0, f = 0, ldw = 0;
  int dp = 0;
  KernParams kp{0, 1.0, 0.0, 0.0};
  double* out = nullptr;          // [s][ldo] values, draw-major; columns up to roundup(m, 64) are written
  int64_t ldo = 0;
};
int launch_paths_eval(hipStream_t st, const PathsEvalLaunch& g);
// R = (y - c) - P^T - sqrt(noise + s_i) eps^T, U = L^-1 R, VT = (L^-T U)^T for s draws padded to spad = roundup(s, 64):
// C the dense fit-type L^-1 (read where column <= row < n), P [s][ldp] = Phi(X) w^T, eps [s * n] (nullable), sdiag [npad]
// (nullable); R, U: roundup(n, 64) * spad doubles each, VT: spad * npad
void launch_paths_solve(hipStream_t st, const double* C, const double* y, const double* P, int64_t ldp, const double* eps,
                        const double* sdiag, const KernParams& kp, int64_t n, int64_t npad, int64_t s, double* R, double* U,
                        double* VT);
// The draw of a whitened variational posterior over n resident rows: VT = (beta + Lu^-T (Q eps^T -
// Lu^-1 P^T))^T for s draws padded to spad = roundup(s, 64).  Lui the dense Lu^-1, Q the lower root of the whitened
// covariance -- q_transposed: Q is the TRANSPOSE of the lower matrix given (the SGPR's LB^-1) --, both npad x npad and read
// where column <= row < n only; beta [>= n]; P [s][ldp] = Phi(Zr) w^T; eps [s * n] (nullable: zeros).  Pt, E, X:
// roundup(n, 64) * spad doubles each (Pt ends as the residual, zero on the padding draws); VT: spad * npad
void launch_paths_solve_q(hipStream_t st, const double* Lui, const double* Q, bool q_transposed, const double* beta, const double* P,
                          int64_t ldp, const double* eps, int64_t n, int64_t npad, int64_t s, double* Pt, double* E, double* X,
                          double* VT);
// vals [s][ldv] hold the points [off, off + mc) of the batch: per (draw, segment) their highest value against the running
// winner in best_i / best_v [s * nseg] (best_i < 0: none yet; indices count from the start of the batch)
void launch_paths_argmax(hipStream_t st, const double* vals, int64_t ldv, int64_t off, int64_t mc, const int64_t* seg_off_dev, int nseg,
                         int64_t s, int64_t* best_i, double* best_v);
// ---- batch.hip: latent cross-covariance and the greedy batch rounds built on it ---------------------------
constexpr int64_t kBatchChunk = 16384;  // points per launch sequence of gpso_cross_cov / per scaling launch of gpso_best_batch
// the device words of one gpso_best_batch call (zeroed when it starts)
struct BatchState {
  int stop;      // != 0: the batch has ended; the launches still queued do nothing
  int n_picked;
  double d, root_d;  // d_t of the round in flight and its square root
  double gp[64];     // G[s][p_t], s < t
  int64_t idx[64];
  double mean[64], var[64], value[64];
};
// K_b = k(Xr, t_b), U = C K_b (each [b][npad], rows below n written), W = C^T U as batch_w_slabs(n) partial sums over slabs
// of rows ([slabs][b][npad]: the column launches add them in their order) and lv[c] = variance - |u_c|^2 for the b scaled
// points tb [b][dp].  Kb, U and W together: batch_pick_workspace_doubles(n, npad, b) doubles.  C the dense fit-type L^-1, read where column <= row < n.  st (nullable; b == 1): a round of
// gpso_best_batch -- nothing runs once st->stop is set, and d_t = lv - sum_{s < t} gp[s]^2 + obs_noise, its root and the stop
// test go to st
struct BatchPickLaunch {
  const double* C = nullptr;
  const double* xs = nullptr;  // [npad * dp] scaled rows
  const double* tb = nullptr;
  int64_t n = 0, npad = 0;
  int b = 0, dp = 0;
  KernParams kp{0, 1.0, 0.0, 0.0};
  double *Kb = nullptr, *U = nullptr, *W = nullptr, *lv = nullptr;
  BatchState* st = nullptr;
  int t = 0;
  double obs_noise = 0.0;
};
int batch_w_slabs(int64_t n);  // a function of n alone: so are the bits of w
size_t batch_pick_workspace_doubles(int64_t n, int64_t npad, int b);
int launch_batch_pick_vectors(hipStream_t st, const BatchPickLaunch& g);
struct BatchColLaunch {
  const double* ts = nullptr;     // [roundup(m, 64) * dp] scaled leaves, zero rows behind the m live ones
  const double* tnorm = nullptr;  // [roundup(m, 64)] their squared norms: a NaN marks a row with a NaN coordinate
  const double* xs = nullptr;     // [npad * dp] scaled rows
  const double* W = nullptr;      // launch_batch_pick_vectors' W for the points tb
  const double* tb = nullptr;     // [b][dp]
  const double* bnorm = nullptr;  // [b] (launch_batch_cross; nullable)
  int64_t n = 0, npad = 0, m = 0;
  int b = 1, dp = 0;
  KernParams kp{0, 1.0, 0.0, 0.0};
  double* cov = nullptr;          // launch_batch_cross: cov[c * ldc + j] = Cov(f(t_j), f(tb_c)), ldc >= m
  int64_t ldc = 0;
  // launch_batch_round (b == 1: the pick of round t): G [q][m], s2 / mean / live [m], the tiles' maxima [batch_round_blocks(m)]
  BatchState* st = nullptr;
  int t = 0;
  bool rank = true;               // false: G and the downdate only
  double* G = nullptr;
  double* s2 = nullptr;
  const double* mean = nullptr;
  unsigned char* live = nullptr;
  AcqSpec acq;
  double* bmax_v = nullptr;
  int64_t* bmax_i = nullptr;
};
int launch_batch_cross(hipStream_t st, const BatchColLaunch& g);
int launch_batch_round(hipStream_t st, const BatchColLaunch& g);
int64_t batch_init_blocks(int64_t m);
int64_t batch_round_blocks(int64_t m);
// round 0: live := 1 and the blocks' first maxima of value [m] (bmax_* [batch_init_blocks(m)])
void launch_batch_init(hipStream_t st, const double* value, int64_t m, unsigned char* live, double* bmax_v, int64_t* bmax_i);
// the pick of round t from nblocks maxima: its record into st, its scaled row into tp [dp], its history into st->gp
void launch_batch_finish(hipStream_t st, BatchState* state, int t, const double* bmax_v, const int64_t* bmax_i, int64_t nblocks,
                         const double* ts, int dp, const double* mean, const double* s2, const double* G, int64_t m, unsigned char* live,
                         double* tp);
// ---- mcbatch.hip: Monte-Carlo batch acquisition over the path draws (mcbatch.hpp) --------------------------
// the device words of one gpso_paths_best_batch call (zeroed when it starts, then bar := the initial bars); the host reads
// back the part in front of bar
struct McState {
  int stop;      // != 0: the batch has ended; the launches still queued do nothing
  int n_picked;
  int64_t idx[64];
  double gain[64], value[64];
  double bar[256];   // QEI: the draws' current bars; QPI: their original ones
  double thr[256];   // QPI: bar + xi
  int cleared[256];  // a pick or a pending point has cleared the draw's bar by more than xi
};
struct McLaunch {
  McState* st = nullptr;
  const double* V = nullptr;  // [s][ld] draw-major values: candidates in columns 0 .. m - 1, pending points in pcol .. pcol + b - 1
  int64_t ld = 0, m = 0, pcol = 0;
  int s = 0, b = 0, kind = 0;
  double xi = 0.0;
  unsigned char* live = nullptr;  // [m], 1 on entry
  double* bmax_v = nullptr;       // [mc_round_blocks(m)]
  int64_t* bmax_i = nullptr;
};
int64_t mc_round_blocks(int64_t m);
// the pending columns folded into st->bar / st->cleared, st->thr set
int launch_mc_init(hipStream_t st, const McLaunch& g);
// round t: every live row's gain (round 0 also into gain0 [m], nullable), the blocks' first maxima, then the one-workgroup fold
// that makes the pick, writes its record, retires the row and applies it to the bars or flags
void launch_mc_round(hipStream_t st, const McLaunch& g, int t, double* gain0);
// ---- sgpr.hip: sparse GP regression on inducing points (rectangular [M_pad x N_pad] float64 buffers, zero padding) -------
// C (m x n, leading dimension ldc) = alpha opA opB + beta C with opA(i, k) = A[i * sai + k * sak], opB(k, j) = B[k * sbk +
// j * sbj] (fit.hip: the LDS-DMA tile GEMM behind launch_dgemm; m, n multiples of 64, each operand unit-stride in one index).
// nsplit > 1: split-K -- k is cut into nsplit equal chunks (each a multiple of 128) and chunk s goes to C + s * m * ldc
// (beta ignored); the caller sums the partial products in their fixed order (launch_sgpr_splitk_sum).
void launch_dgemm_rect(hipStream_t st, const double* A, int64_t sai, int64_t sak, const double* B, int64_t sbk, int64_t sbj,
                       double* C, int64_t ldc, int64_t m, int64_t n, int64_t k, double alpha, double beta, int nsplit = 1);
void launch_sgpr_cross_gram(hipStream_t st, const double* zs, const double* xs, int64_t m, int64_t mpad, int64_t n,
                            int64_t npad, int dp, const KernParams& kp, double* kuf);
// out[n_ls + 1] = sum_ij (g_ij + a_i t_j) dKuf_ij / d(lengthscales..., variance); partial: (mpad / 64) (npad / 64) (n_ls + 1)
void launch_sgpr_cross_grad(hipStream_t st, const double* g, const double* a, const double* t, const double* zs,
                            const double* xs, int64_t m, int64_t mpad, int64_t n, int64_t npad, int dp, int n_ls,
                            const double* ls, const KernParams& kp, double* partial, double* out);
void launch_sgpr_splitk_sum(hipStream_t st, const double* part, int nsplit, int64_t m, int64_t mpad, double* aat, double* bm,
                            int* info);
// out = alpha op(A) x over the real block of a [mpad x npad] matrix (trans: out has n entries, x has m)
void launch_sgpr_gemv(hipStream_t st, const double* A, bool trans, const double* x, double alpha, double* out, int64_t m,
                      int64_t mpad, int64_t n, int64_t npad);
void launch_sgpr_resid(hipStream_t st, const double* y, double c, double* e, int64_t n, int64_t npad);
void launch_sgpr_tvec(hipStream_t st, const double* e, const double* w, double p, double q, double* t, int64_t n, int64_t npad);
void launch_sgpr_wuu(hipStream_t st, const double* g1, const double* p, const double* a, double b, double* kin, int64_t m,
                     int64_t mpad);
constexpr int kSgprSums = 9;
void launch_sgpr_sums(hipStream_t st, const double* lb, const double* aat, const double* cv, const double* e, const double* w,
                      const double* lbinv_rows, int64_t m, int64_t mpad, int64_t n, double* out);
// greedy conditional-variance selection of m rows of xs (scaled inputs, n rows): idx[m]; lg: m * npad doubles of scratch
void launch_sgpr_greedy(hipStream_t st, const double* xs, int64_t n, int64_t npad, int dp, const KernParams& kp, int m,
                        double* lg, double* dvec, double* pivot, int64_t* idx);
// ---- svgp.hip: sparse variational GP on inducing points (the [M_pad x N_pad] layout of sgpr.hip) -----------------------
// fm = A^T mu + c, fv = variance - colnorm(A) + colnorm(B) (B nullable) over the n columns of an [m x npad] A, B
void launch_svgp_moments(hipStream_t st, const double* A, const double* B, const double* mu, double variance, double c,
                         double* fm, double* fv, int64_t m, int64_t n, int64_t npad);
void launch_svgp_colscale(hipStream_t st, const double* A, const double* a, double* D, int64_t m, int64_t mpad, int64_t n,
                          int64_t npad);
void launch_svgp_gauss(hipStream_t st, const double* y, const double* fm, const double* fv, double s2, double c, double* gm,
                       double* a, double* t, double* ve, double* dve, int64_t n, int64_t npad);
constexpr int kSvgpSums = 7;
void launch_svgp_sums(hipStream_t st, const double* ve, const double* dve, const double* gm, const double* a, int64_t n,
                      const double* mu, const double* srow, const double* S, int64_t m, int64_t mpad, double* out);
// ---- inducing.hip: the gradient of the sparse objectives in the inducing points -----------------
// grad_z[m * d] = cc dFc/dZ + cu dFu/dZ: Fc's weights dF/dKuf = wc + a t^T ([mpad x npad], [mpad], [npad], the operands of
// launch_sgpr_cross_grad), Fu's weights dF/dKuu = kin / 2 (lower triangle read, as launch_gradient reads its K^-1).
// part: (inducing_slices(mpad, npad) + 1) * mpad * (dp + 1) doubles of scratch.  0, or a negative GPSO_E_* code.
constexpr int kInducingSlicesLargeM = 16;  // slices of the N direction from M_pad = 1024 on
constexpr int kInducingSlicesMax = 64;     // ... and at most, for a smaller M_pad (inducing_slices)
int inducing_slices(int64_t mpad, int64_t npad);
int launch_inducing_grad(hipStream_t st, const double* wc, const double* a, const double* t, const double* kin,
                         const double* zs, const double* xs, int64_t m, int64_t mpad, int64_t n, int64_t npad, int d, int dp,
                         const double* ls, const KernParams& kp, double cc, double cu, double* part, double* grad_z);
// ---- append.hip: rank-k append at fixed hyper-parameters ----------------------------------------------------------------
// The posterior of the first n points is resident; k <= kAppendMax new points (already copied behind the old ones in
// x64 / y64) extend L, L^-1, a, alpha, diag(K_y^-1), the NLML and the scaled inputs in place: two passes over L^-1
// (append.hip).  Everything below lives on the device; scratch = append_scratch_doubles(npad, append_kp(k)) doubles.
constexpr int kAppendMax = 64;
struct AppendArgs {
  double* x64;         // [npad * d] raw inputs: rows n .. n + k - 1 are filed by the cross kernel
  double* y64;         // [npad]
  const double *xnew, *ynew;  // the k new points [k * d], [k] in pinned HOST memory (read by the cross kernel itself: no copies)
  const double* snew;  // [k] their per-point noise, pinned host (nullable = zeros)
  double* sdiag;       // [npad] per-point noise of the resident rows (device, nullable: none set); rows n .. n + k - 1 are filed

  const double* ls;    // lengthscale per input dimension (device)
  int64_t n, npad;
  int k, kp, d, dp, kernel;
  double variance, noise, mean_c;
  double *xs64, *xnorm64, *xs_p64;  // scaled inputs (rows n .. n + k - 1 are written)
  double *Kc, *Bm, *part, *sm;      // scratch (carved by launch_append)
  int* info;                        // scratch: INT_MAX, or the first failing pivot (n + p)
  double* diag64;                   // [npad] diagonal of L
  double* nlml;                     // device scalar: the resident NLML, updated in place
  double* kinv_diag;                // [npad] squared column norms of L^-1
  void* alpha_p;                    // [npad] predict-type copy of alpha
  double* hyper;                    // hyper block: slot 0 (n) is updated
  float* f16_scal;                  // nullable: scale slot of the fp16 split ([0] max |L^-1| grows by atomicMax, [3] := [1])
  double* host_out;                 // pinned host: [0] the new NLML, [1] 1.0 = extended / 2.0 = not positive definite, [2] pivot
};
int append_kp(int k);
size_t append_scratch_doubles(int64_t npad, int kp);
template <typename TF, typename TP>
void launch_append(hipStream_t st, AppendArgs a, void* scratch, TF* linv, TF* Lf, TF* white, TF* alpha_f);

// ---- grow.hip -------------------------------------------------------------------------------------
// centres of the ternary subtree (levels 0..depth-1) under each box; out[nseg*rows*d] float64
void launch_grow(hipStream_t st, const double* bounds_dev, int nseg, int d, int depth,
                 double* out_dev);
// the same centres WITHOUT the rows that repeat an earlier row bit for bit (a centre child repeats its
// parent): grow_unique_rows(depth) = 3^(depth-1) analytic slots per box, then the centre children whose
// centre differs from the parent's in the last bit; key_dev[slot] = seg * rows + reference row index;
// *count_dev must hold nseg * grow_unique_rows(depth) on entry and holds the live row count on exit
// Only the reference rows [row_lo, row_hi) of every box (a rank's share of a sharded call; the whole list
// is [0, rows)): analytic slots per box = grow_unique_before(row_hi) - grow_unique_before(row_lo).
int64_t grow_unique_rows(int depth);
int64_t grow_unique_before(int64_t row);
void launch_grow_unique(hipStream_t st, const double* bounds_dev, int nseg, int d, int depth, int64_t row_lo,
                        int64_t row_hi, double* out_dev, int64_t* key_dev, int64_t* count_dev);
// Small calls (round 4, launch-bound: the optimiser's exploration levels): growth and input scaling in ONE launch with
// the boxes passed by value -- rows land scaled (x / l in TG, norms) where the tile kernel reads them, keys as above; a
// row that does not repeat its parent goes to nseg * uniq + atomicAdd(extra); *extra_dev is zero between calls
constexpr int kGrowBoxDoubles = 96;  // nseg * d * 2 doubles of boxes fit the kernel-argument struct
struct GrowBoxes {
  double b[kGrowBoxDoubles];
};
template <typename TG>
void launch_grow_unique_prep(hipStream_t st, const GrowBoxes& boxes, int nseg, int d, int dp, int depth, int64_t row_lo,
                             int64_t row_hi, const double* ls_dev, TG* leaves_s, TG* lnorm, int64_t* key_dev,
                             unsigned long long* extra_dev);
// ... and the whole arg-max of a small batch in ONE launch of one workgroup: finalises every live leaf (LeafFinalize),
// reduces per segment with np.argmax's rule, writes the records (device and pinned host) and resets *extra_dev
struct SmallBest {
  LeafFinalize fin;
  const int64_t* key = nullptr;       // keyed (grown) batches: reference keys, rows per box, analytic slots per box
  int64_t rows = 0, uniq = 0, base = 0;
  unsigned long long* extra = nullptr;
  const int64_t* seg_off = nullptr;   // plain batches: segment offsets (device), total leaves m
  int64_t m = 0;
  int nseg = 0;
  double* out_vals = nullptr;         // [nseg * 4 + 2]
  double* host_vals = nullptr;        // nullable pinned host copy
  double done_token = 0.0;            // != 0: written to host_vals[nseg * 4 + 2] behind the records (system-scope release):
                                      // the host spins on it instead of polling an event (round 5)
};
// ... and, where ONE row block covers L^-1 (N_pad = 128 or 256) and the native tile kernel runs, the whole call in ONE
// launch (predict.hip: leaf_tiles_v2_one_kernel): rows made in the prologue, leaves finalised and reduced in the epilogue,
// the last workgroup to arrive writes the records
struct OneLaunch {
  int mode = 0;  // 1: rows grown from `boxes` (all reference rows of every box), 2: raw rows at `raw`
  GrowBoxes boxes;
  int nseg = 0, d = 0, depth = 0, raw_f64 = 0;
  int64_t rows = 0, uniq = 0;  // grown: reference rows and analytic slots per box
  int64_t total = 0;           // live rows: nseg * uniq (grown) or m (raw)
  const void* raw = nullptr;
  const int64_t* seg_off = nullptr;  // raw: segment offsets (device)
  const double* ls = nullptr;        // lengthscale per dimension (device)
  void* leaves_s = nullptr;          // [mpad * dp] TG: the scaled rows (written by the prologue, read by the tile code)
  void* lnorm = nullptr;             // [mpad] TG
  int64_t* key = nullptr;            // [mpad]: reference keys of grown rows
  LeafFinalize fin;
  void* partial = nullptr;           // [grid * nseg] winners per workgroup (ucb, id)
  int64_t* ppos = nullptr;           // [grid * nseg] their rows
  unsigned* ticket = nullptr;        // arrival counter, zero between calls
  unsigned* fallback = nullptr;      // raised when a centre child does not repeat its parent; zero between calls
  double* out_vals = nullptr;        // [nseg * 4 + 2]: records, live rows (bit-cast), status (1.0 = fallback wanted)
  double* host_vals = nullptr;       // nullable pinned host copy
  double done_token = 0.0;           // as SmallBest::done_token
};
template <typename T, typename TG>
int launch_leaf_tiles_one(hipStream_t st, const T* linv_p, const TG* xs_p, const TG* xnorm, const T* alpha,
                          double* part_var, double* part_mean, int64_t npad, int dp4, int64_t mpad, const KernParams& kp,
                          const OneLaunch& one);
constexpr int64_t kSmallBestMaxRows = 16384;
void launch_small_best(hipStream_t st, const SmallBest& a, bool keyed);
// winners of several ranks -> the global winner per segment, np.argmax order on (ucb, global index):
// gathered[world][stride], a rank's payload = nseg x (mean, var, ucb, bit-cast index) [, spare, status: stride ==
// kGroupPayload(nseg)]; base[world][nseg] (nullable) is added to a rank's indices first; out[nseg][4] [, bit-cast rank
// of the worst status, worst status]
void launch_reduce_winners(hipStream_t st, const double* gathered, const int64_t* base, int world, int nseg,
                           int stride, double* out, double* host_out = nullptr /* pinned host copy of out, written by the kernel */,
                           double done_token = 0.0 /* nseg <= 64 (one workgroup): host_out[nseg * 4 + 2] := token behind the records */);
// doubles of one rank's group payload: the winners, the live row count of a growth call (bit-cast), the status
inline int group_payload_doubles(int nseg) { return nseg * 4 + 2; }

}  // namespace gpso
