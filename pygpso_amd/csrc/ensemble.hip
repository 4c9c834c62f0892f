// The hyper-parameter ensemble's two kernels (ensemble.hpp holds the fold and the launch records).
//
// ens_members_kernel, grid (ceil(m / 64), K), 256 threads: a workgroup takes 64 raw leaves and ONE member k, i.e. that
// member's copies of the hyper block, the scaled rows, the dense double L^-1 and alpha (N <= 128: one row block).  It scales
// the leaves by the member's lengthscales (x / l, prep_leaves_kernel's division), regenerates the cross-Gram tile from direct
// differences in double (predict_grad.hip's pair_r2 form, never the norm expansion), forms V = L^-1 k* on
// v_mfma_f64_16x16x4_f64 with predict_grad.hip's staging (16 columns of L^-1 and 16 scaled rows a step, at an odd LDS
// stride; tiles above the diagonal and tiles of padding rows are skipped) and, beside it, alpha^T k*.  Then
//     mean = alpha^T k* + c,   var = (variance - sum_i V_i^2) + noise         (gpso_predict's association)
// with both sums in a fixed order: a lane adds its rows in ascending order, the four lane groups that share a column are
// folded by two xor-shuffles.  No atomics; the bits of a (member, leaf) pair depend neither on the leaf's column slot nor on
// the rest of the batch nor on K.  A leaf with a NaN coordinate gets a NaN mean and var (the kernel map's clamp
// max(r^2, 1e-36) would otherwise give it finite garbage): the arg-max then picks it, as gpso_best_acq does.
// LDS: (128 x 17 + 16 x (D_pad + 1) + 64 x (D_pad + 1)) doubles -- 48.8 KB at D_pad = 48, three workgroups a CU.
//
// ens_fold_kernel: one thread per leaf, ensemble_fold_leaf (ensemble.hpp) over the K members in index order.
// Compiled with -ffp-contract=off; every fused multiply-add is written out.
#include "ensemble.hpp"
#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;
constexpr int kCols = 64;    // leaves per workgroup: 4 waves x 16 MFMA columns
constexpr int kRows = 128;   // rows of L^-1: 8 accumulator tiles a wave
constexpr int kStage = 16;   // columns of L^-1 staged in LDS per step
constexpr int kStageLd = kStage + 1;

__device__ __forceinline__ double ens_pair_r2(const double* __restrict__ t /* LDS */, const double* __restrict__ xj /* LDS */, int dp) {
  double r2 = 0.0;
  for (int k = 0; k < dp; k += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double df = t[k + q] - xj[k + q];
      r2 = fma(df, df, r2);
    }
  }
  return r2;
}

template <typename TIN>
__global__ __launch_bounds__(kThreads) void ens_members_kernel(EnsembleMembersLaunch a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double* Al = reinterpret_cast<double*>(lds_raw);  // [kRows][kStageLd]: the step's columns of L^-1
  double* Xl = Al + kRows * kStageLd;               // [kStage][dp + 1]: the step's scaled rows
  double* tl = Xl + kStage * (a.dp + 1);            // [kCols][dp + 1]: the scaled leaves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t mt = blockIdx.x;
  const int member = blockIdx.y;
  const int n = a.n, npad = a.npad, d = a.d, dp = a.dp, ldt = dp + 1;
  const double* hy = a.hyper + (int64_t)member * a.hyper_stride;
  const double* C = a.linv + (int64_t)member * npad * npad;
  const double* xs = a.xs + (int64_t)member * npad * dp;
  const double* al = a.alpha + (int64_t)member * npad;
  const double variance = hy[4], noise = hy[5], mean_c = hy[6];
  const double* ls = hy + 8;
  const int col = 16 * wave + (lane & 15), kq = lane >> 4;
  // the 64 leaves of this tile, scaled; rows at or beyond m and the padding dimensions are zeros
  const TIN* raw = static_cast<const TIN*>(a.leaves);
  for (int e = tid; e < kCols * dp; e += kThreads) {
    const int c = e / dp, k = e - c * dp;
    const int64_t j = mt * kCols + c;
    double v = 0.0;
    if (j < a.m && k < d) v = (double)raw[j * d + k] / ls[k];
    tl[c * ldt + k] = v;
  }
  const double* tcol = tl + col * ldt;
  f64x4 acc[kRows / 16];
#pragma unroll
  for (int t = 0; t < kRows / 16; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int steps = (n + kStage - 1) / kStage;
  // thread -> row tid / 2, 8 consecutive columns of the staged 16; and up to three of the step's kStage * dp scaled inputs
  // (rows j0 .. j0 + 15 < N_pad: one contiguous piece)
  const int lr = tid >> 1, lc = (tid & 1) * 8;
  constexpr int kXPer = (kStage * 48 + kThreads - 1) / kThreads;
  const int xcount = kStage * dp;
  double pre[8], prex[kXPer];
  auto fetch = [&](int j0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int j = j0 + lc + q;
      pre[q] = (lr < n && j <= lr) ? C[lr * npad + j] : 0.0;  // (j <= lr < n: inside the member's factor)
    }
#pragma unroll
    for (int u = 0; u < kXPer; ++u) {
      const int e = tid + u * kThreads;
      prex[u] = e < xcount ? xs[j0 * dp + e] : 0.0;
    }
  };
  fetch(0);
  double pm = 0.0;
  for (int s = 0; s < steps; ++s) {
    const int j0 = s * kStage;
    __syncthreads();  // the previous step's reads of Al / Xl are done (first step: nothing to wait for)
#pragma unroll
    for (int q = 0; q < 8; ++q) Al[lr * kStageLd + lc + q] = pre[q];
#pragma unroll
    for (int u = 0; u < kXPer; ++u) {
      const int e = tid + u * kThreads;
      if (e < xcount) Xl[(e / dp) * ldt + e % dp] = prex[u];
    }
    __syncthreads();  // (first step: the leaf tile is complete too)
    if (s + 1 < steps) fetch(j0 + kStage);
    // B operand: lane l holds k(xs_j, t_col) for j = j0 + 4 q + (l >> 4), col = l & 15 of the wave's 16
    double kv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + 4 * q + kq;
      kv[q] = 0.0;
      if (j < n) {
        double k, dk;
        kern_and_dkern_same(a.kernel, ens_pair_r2(tcol, Xl + (4 * q + kq) * ldt, dp), variance, k, dk);
        kv[q] = k;
        pm = fma(al[j], k, pm);
      }
    }
#pragma unroll
    for (int t = 0; t < kRows / 16; ++t) {
      if (j0 > 16 * t + 15 || 16 * t >= n) continue;  // (wave-uniform: above the diagonal, or padding rows only)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double af = Al[(16 * t + (lane & 15)) * kStageLd + 4 * q + kq];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, kv[q], acc[t], 0, 0, 0);
      }
    }
  }
  // register r of tile t: row 16 t + (l >> 4) + 4 r, column l & 15
  double ss = 0.0;
#pragma unroll
  for (int t = 0; t < kRows / 16; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ss = fma(acc[t][r], acc[t][r], ss);
  }
  ss += __shfl_xor(ss, 16);
  ss += __shfl_xor(ss, 32);
  pm += __shfl_xor(pm, 16);
  pm += __shfl_xor(pm, 32);
  const int64_t j = mt * kCols + col;
  if (kq == 0 && j < a.m) {
    bool bad = false;
    for (int k = 0; k < d; ++k) bad = bad || tcol[k] != tcol[k];
    const double nan = __builtin_nan("");
    a.mean[(int64_t)member * a.ld + j] = bad ? nan : pm + mean_c;
    a.var[(int64_t)member * a.ld + j] = bad ? nan : (variance - ss) + noise;
  }
}

__global__ __launch_bounds__(kThreads) void ens_fold_kernel(AcqSpec a, const double* __restrict__ mean, const double* __restrict__ var,
                                                            const double* __restrict__ hyper, int64_t hyper_stride, int k, int64_t ld,
                                                            int64_t m, double* __restrict__ mean_mix, double* __restrict__ var_mix,
                                                            double* __restrict__ value) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  double noise[kEnsembleMax];
  for (int i = 0; i < k; ++i) noise[i] = hyper[(int64_t)i * hyper_stride + 5];
  double mm, vm, val;
  ensemble_fold_leaf(a, mean, var, noise, k, ld, j, &mm, &vm, &val);
  if (mean_mix != nullptr) mean_mix[j] = mm;
  if (var_mix != nullptr) var_mix[j] = vm;
  if (value != nullptr) value[j] = val;
}

}  // namespace

void ensemble_fold_host(const AcqSpec& a, const double* member_mean, const double* member_var, const double* noise, int k, long long m,
                        double* mean_mix, double* var_mix, double* value) {
  for (long long j = 0; j < m; ++j) {
    double mm, vm, val;
    ensemble_fold_leaf(a, member_mean, member_var, noise, k, (int64_t)m, (int64_t)j, &mm, &vm, &val);
    if (mean_mix) mean_mix[j] = mm;
    if (var_mix) var_mix[j] = vm;
    if (value) value[j] = val;
  }
}

int launch_ensemble_members(hipStream_t st, const EnsembleMembersLaunch& g) {
  if (g.n < 1 || g.n > kEnsembleMaxN || g.npad != kRows || g.dp < 4 || g.dp % 4 != 0 || g.dp > 48 || g.d < 1 || g.d > g.dp || g.m < 1 ||
      g.ld < g.m || g.k < 1 || g.k > kEnsembleMax || g.hyper_stride < 8 + g.dp) {
    note_launch_error("launch_ensemble_members: shape outside the kernel's");
    return -1;
  }
  const dim3 grid((unsigned)((g.m + kCols - 1) / kCols), (unsigned)g.k);
  const size_t lds = (size_t)(kRows * kStageLd + (kStage + kCols) * (g.dp + 1)) * 8;
  if (g.leaves_f64) hipLaunchKernelGGL(ens_members_kernel<double>, grid, dim3(kThreads), lds, st, g);
  else hipLaunchKernelGGL(ens_members_kernel<float>, grid, dim3(kThreads), lds, st, g);
  return 0;
}

void launch_ensemble_fold(hipStream_t st, const AcqSpec& a, const double* mean, const double* var, const double* hyper, int64_t hyper_stride,
                          int k, int64_t ld, int64_t m, double* mean_mix, double* var_mix, double* value) {
  hipLaunchKernelGGL(ens_fold_kernel, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a, mean, var, hyper,
                     hyper_stride, k, ld, m, mean_mix, var_mix, value);
}

}  // namespace gpso
