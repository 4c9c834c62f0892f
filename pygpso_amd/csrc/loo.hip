// Leave-one-out predictive of the exact GP and the LOO-CV log pseudo-likelihood with its gradient (Rasmussen & Williams
// 5.4.2).  No counterpart in the reference: GPflow's GPR has neither.  With alpha = K_y^-1 (y - c)
// and kappa_i = (K_y^-1)_ii, both resident after a fit:
//     mean_-i = y_i - alpha_i / kappa_i,  var_-i = 1 / kappa_i,  lpd_i = (log kappa_i - alpha_i^2 / kappa_i - log 2pi) / 2,
//     F = -sum lpd_i;   dF/dtheta = sum_ab W_ab dK_y,ab / dtheta  with
//     c_i = (1 + alpha_i^2 / kappa_i) / (2 kappa_i),  g_i = alpha_i / kappa_i,  h = K_y^-1 g,
//     W = K_y^-1 diag(c) K_y^-1 - (h alpha^T + alpha h^T) / 2,   dF/dnoise = tr W,   dF/dc = -sum h.
// The contraction with dK is the NLML gradient's own (fit.hip: grad_tile_kernel reads W' = (kinv - a a^T) / 2 over the
// lower tiles): it is called with kinv := 2 W and a := 0.  Every reduction here runs in a fixed order, no atomics: the
// same call gives the same bits.  api.hip (EngineT::loo, EngineT::fit_eval_impl) sequences the launches.
#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;
constexpr double kLog2Pi = 1.83787706640934548356;

inline unsigned blocks_for(int64_t total) { return total < kThreads ? 1u : (unsigned)((total + kThreads - 1) / kThreads); }

// sum over the workgroup's 256 threads in a fixed order (wave butterflies, then the four waves); every thread gets it
__device__ __forceinline__ double block_sum256(double v, double* red /* [4] LDS */) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// the per-point pass.  vec: the seven vectors of kernels.hpp (kLoo*), zero on the padding; one workgroup
template <typename T>
__global__ __launch_bounds__(kThreads) void loo_point_kernel(const T* __restrict__ alpha, const double* __restrict__ kinv_diag,
                                                             const double* __restrict__ y64, int64_t n, int64_t npad,
                                                             double* __restrict__ vec, double* __restrict__ loss_out) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < npad; i += kThreads) {
    double mean = 0.0, var = 0.0, lpd = 0.0, sc = 0.0, t = 0.0, g = 0.0;
    if (i < n) {
      const double a = (double)alpha[i], kap = kinv_diag[i];
      var = 1.0 / kap;
      g = a * var;
      mean = y64[i] - g;
      const double q = a * g;  // alpha_i^2 / kappa_i
      lpd = 0.5 * (log(kap) - q - kLog2Pi);
      const double c = 0.5 * (1.0 + q) * var;
      sc = sqrt(c);
      t = g / sc;  // h = K_y^-1 g = S^T (g / sqrt c) with S = diag(sqrt c) K_y^-1
      acc -= lpd;
    }
    vec[kLooMean * npad + i] = mean;
    vec[kLooVar * npad + i] = var;
    vec[kLooLpd * npad + i] = lpd;
    vec[kLooSc * npad + i] = sc;
    vec[kLooT * npad + i] = t;
    vec[kLooH * npad + i] = 0.0;
    vec[kLooZero * npad + i] = 0.0;
  }
  const double loss = block_sum256(acc, red);
  if (threadIdx.x == 0) loss_out[0] = loss;
}

// S = diag(sc) K_y^-1 on the real block, K_y^-1 read from its LOWER triangle (all the fit leaves); zero on the padding
__global__ __launch_bounds__(kThreads) void loo_rowscale_sym_kernel(const double* __restrict__ kinv, const double* __restrict__ sc,
                                                                    double* __restrict__ S, int64_t n, int64_t npad) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npad * npad) return;
  const int64_t i = idx / npad, j = idx - i * npad;
  double v = 0.0;
  if (i < n && j < n) v = sc[i] * (j <= i ? kinv[idx] : kinv[j * npad + i]);
  S[idx] = v;
}

// out = 2 W = 2 M - (h alpha^T + alpha h^T) on the lower 64-tiles (what grad_tile_kernel reads), zero on the padding;
// tiles above the diagonal are not touched
__global__ __launch_bounds__(kThreads) void loo_weights_kernel(const double* __restrict__ M, const double* __restrict__ h,
                                                               const double* __restrict__ alpha, double* __restrict__ out,
                                                               int64_t n, int64_t npad) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npad * npad) return;
  const int64_t i = idx / npad, j = idx - i * npad;
  if ((j >> 6) > (i >> 6)) return;
  out[idx] = (i < n && j < n) ? 2.0 * M[idx] - (h[i] * alpha[j] + alpha[i] * h[j]) : 0.0;
}

// out[0] = -sum_i h_i (dF/dc); one workgroup
__global__ __launch_bounds__(kThreads) void loo_mean_grad_kernel(const double* __restrict__ h, int64_t n, double* __restrict__ out) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) acc -= h[i];
  const double s = block_sum256(acc, red);
  if (threadIdx.x == 0) out[0] = s;
}

// ---- N <= 128: the whole LOO evaluation behind the one-launch fit, in ONE workgroup ---------------------------------------
// K_y^-1 (symmetric, from the lower triangle the fit wrote; zero beyond N) lives in LDS at an odd row stride; a wave owns
// 16 x 16 tiles of the lower triangle as the fused fit's gradient does: M_ij = sum_k c_k Kinv_ki Kinv_kj on the f64 MFMA
// (16x16x4: lane l feeds A[i = l & 15][k = l >> 4] = c_k Kinv[k][16 ti + i] and B[k][j = l & 15] = Kinv[k][16 tj + j], and
// holds M[(l >> 4) + 4 r][l & 15] in register r), turned into W_ij in registers and contracted with dK regenerated from
// the scaled inputs at once.  M is never stored.  The scaled inputs ride in the rest of the CU's LDS where they fit
// (N_pad D_pad <= kLsXs doubles: D_pad <= 24), else they are read from global memory.
constexpr int kLsN = 128, kLsStride = kLsN + 1;
constexpr int kLsGacc = kGradMaxLs + 2;
// Kf | c, g, h, alpha | per-wave gradient partials | reduction slots | scaled inputs
constexpr int kLsFixed = kLsN * kLsStride + 4 * kLsN + 4 * kLsGacc + 16;
constexpr int kLooSmallLdsDoubles = 160 * 1024 / 8;
constexpr int kLsXs = kLooSmallLdsDoubles - kLsFixed;

// XS_LDS: the scaled inputs fit the LDS behind the fixed part (the launcher's choice; a template parameter so that their reads
// are LDS reads, not flat ones)
template <bool XS_LDS>
__global__ __launch_bounds__(kThreads) void loo_small_kernel(LooSmallArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double* Kf = reinterpret_cast<double*>(lds_raw);
  double* cv = Kf + kLsN * kLsStride;
  double* gv = cv + kLsN;
  double* hv = gv + kLsN;
  double* al = hv + kLsN;
  double* gacc = al + kLsN;
  double* red = gacc + 4 * kLsGacc;
  double* xl = red + 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n, dp = a.dp;
  // 1. K_y^-1 into LDS, both triangles from the lower one (rows of it read along j: coalesced), zero beyond N; the point pass
  // (a fixed trip count and two phases -- sixteen predicated loads issued, then their stores: with its loads one behind the
  // other this loop took longer than everything else in the kernel)
  for (int it0 = 0; it0 < kLsN * kLsN / kThreads; it0 += 16) {
    double v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = (it0 + q) * kThreads + tid, i = e >> 7, j = e & (kLsN - 1);
      v[q] = (j <= i && i < n) ? a.kinv[i * a.npad + j] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = (it0 + q) * kThreads + tid, i = e >> 7, j = e & (kLsN - 1);
      if (j <= i) {
        Kf[i * kLsStride + j] = v[q];
        Kf[j * kLsStride + i] = v[q];
      }
    }
  }
  if constexpr (XS_LDS) {
#pragma unroll 4
    for (int e = tid; e < kLsN * dp; e += kThreads) xl[e] = a.xs[e];
  }
  auto xs_at = [&](int e) -> double {
    if constexpr (XS_LDS) return xl[e];
    else return a.xs[e];
  };
  for (int h = tid; h < 4 * kLsGacc; h += kThreads) gacc[h] = 0.0;
  double nlpd = 0.0;
  if (tid < kLsN) {
    double mean = 0.0, var = 0.0, lpd = 0.0, c = 0.0, g = 0.0, alpha = 0.0;
    if (tid < n) {
      alpha = a.alpha[tid];
      const double kap = a.kinv_diag[tid];
      var = 1.0 / kap;
      g = alpha * var;
      mean = a.y64[tid] - g;
      const double q = alpha * g;
      lpd = 0.5 * (log(kap) - q - kLog2Pi);
      c = 0.5 * (1.0 + q) * var;
      nlpd = -lpd;
    }
    cv[tid] = c;
    gv[tid] = g;
    al[tid] = alpha;
    if (a.vec != nullptr) {
      a.vec[kLooMean * a.npad + tid] = mean;
      a.vec[kLooVar * a.npad + tid] = var;
      a.vec[kLooLpd * a.npad + tid] = lpd;
    }
  }
  const double loss = block_sum256(nlpd, red);  // (its barriers also publish Kf and the vectors)
  // 2. h = K_y^-1 g (a thread per row, k in order); dF/dc = -sum h
  double hi = 0.0;
  if (tid < n) {
    double p[4] = {0.0, 0.0, 0.0, 0.0};  // (four chains: rows and g are zero beyond n)
    for (int k = 0; k < 16 * ((n + 15) / 16); k += 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) p[q] = fma(Kf[tid * kLsStride + k + q], gv[k + q], p[q]);
    }
    hi = (p[0] + p[1]) + (p[2] + p[3]);
    hv[tid] = hi;
  } else if (tid < kLsN) {
    hv[tid] = 0.0;
  }
  const double gc = -block_sum256(tid < n ? hi : 0.0, red);
  // 3. the lower 16 x 16 tiles, dealt over the waves
  const int nt16 = (n + 15) / 16;
  const double variance = a.variance;
  double g_var = 0.0, g_noise = 0.0, g_iso = 0.0;
  for (int t = wave; t < nt16 * (nt16 + 1) / 2; t += 4) {
    int ti = 0, tj = t;
    while (tj > ti) {
      tj -= ti + 1;
      ++ti;
    }
    const int jcol = 16 * tj + (lane & 15), irow0 = 16 * ti + (lane >> 4);
    f64x4 m{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < 16 * nt16; k0 += 16) {  // (rows and columns >= n of Kf are zero, c there too)
      double fa[4], fb[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + 4 * q + (lane >> 4);
        fa[q] = cv[k] * Kf[k * kLsStride + 16 * ti + (lane & 15)];
        fb[q] = Kf[k * kLsStride + 16 * tj + (lane & 15)];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) m = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[q], fb[q], m, 0, 0, 0);
    }
    double base[4], r2d[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < dp; c += 4) {  // (D_pad is a multiple of 4: twenty independent reads per step)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double xj = xs_at(jcol * dp + c + q);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double df = xs_at((irow0 + 4 * r) * dp + c + q) - xj;
          r2d[r] = fma(df, df, r2d[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = irow0 + 4 * r, j = jcol;
      base[r] = 0.0;
      if (i >= n || j >= n || j > i) continue;
      const double w = (i == j) ? 1.0 : 2.0;
      const double Wij = m[r] - 0.5 * (hv[i] * al[j] + al[i] * hv[j]);
      double kv, dk;
      kern_and_dkern_same(a.kernel, r2d[r], variance, kv, dk);
      g_var += w * Wij * kv / variance;
      if (i == j) g_noise += Wij;
      base[r] = w * Wij * dk;
      g_iso += base[r] * (-2.0 * r2d[r]);
    }
    if (a.n_ls > 1) {
      for (int dd = 0; dd < a.n_ls; ++dd) {
        double a2 = 0.0;
        const double xj = xs_at(jcol * dp + dd);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double df = xs_at((irow0 + 4 * r) * dp + dd) - xj;
          a2 += base[r] * (-2.0 * df * df);
        }
        a2 = wave_sum(a2);
        if (lane == 0) gacc[wave * kLsGacc + dd] += a2;
      }
    }
  }
  g_var = wave_sum(g_var);
  g_noise = wave_sum(g_noise);
  g_iso = wave_sum(g_iso);
  if (lane == 0) {
    gacc[wave * kLsGacc + a.n_ls] = g_var;
    gacc[wave * kLsGacc + a.n_ls + 1] = g_noise;
    if (a.n_ls == 1) gacc[wave * kLsGacc] = g_iso;
  }
  __syncthreads();
  const int H = a.n_ls + 2;
  if (tid < H) {
    double v = (gacc[tid] + gacc[kLsGacc + tid]) + (gacc[2 * kLsGacc + tid] + gacc[3 * kLsGacc + tid]);
    if (tid < a.n_ls) v /= a.ls[a.n_ls == 1 ? 0 : tid];
    a.scal[8 + tid] = v;
    if (a.scal_host != nullptr) a.scal_host[8 + tid] = v;
  }
  if (tid == 0) {
    a.scal[0] = loss;
    a.scal[8 + H] = gc;
    if (a.scal_host != nullptr) {
      a.scal_host[0] = loss;
      a.scal_host[8 + H] = gc;
    }
  }
  if (a.scal_host != nullptr && a.done_token != 0.0) {  // every writer releases at system scope, then the token
    __threadfence_system();
    __syncthreads();
    if (tid == 0) *reinterpret_cast<volatile double*>(a.scal_host + 7) = a.done_token;
  }
}

}  // namespace

template <typename T>
void launch_loo_points(hipStream_t st, const T* alpha, const double* kinv_diag, const double* y64, int64_t n, int64_t npad,
                       double* vec, double* loss_out) {
  hipLaunchKernelGGL((loo_point_kernel<T>), dim3(1), dim3(kThreads), 0, st, alpha, kinv_diag, y64, n, npad, vec, loss_out);
}
template void launch_loo_points<float>(hipStream_t, const float*, const double*, const double*, int64_t, int64_t, double*, double*);
template void launch_loo_points<double>(hipStream_t, const double*, const double*, const double*, int64_t, int64_t, double*, double*);

void launch_loo_weights(hipStream_t st, const double* kinv, const double* alpha, double* vec, double* S, double* M, int64_t n,
                        int64_t npad) {
  double* h = vec + kLooH * npad;
  hipLaunchKernelGGL(loo_rowscale_sym_kernel, dim3(blocks_for(npad * npad)), dim3(kThreads), 0, st, kinv, vec + kLooSc * npad, S, n,
                     npad);
  launch_dgemm(st, S, true, S, false, M, npad, 1.0, 0.0);                                  // M = S^T S
  launch_vgp_gemv(st, S, true, vec + kLooT * npad, 0.0, 1.0, 0.0, nullptr, h, n, npad);    // h = S^T (g / sqrt c)
  hipLaunchKernelGGL(loo_weights_kernel, dim3(blocks_for(npad * npad)), dim3(kThreads), 0, st, M, h, alpha, S, n, npad);  // S := 2 W
}

void launch_loo_mean_grad(hipStream_t st, const double* vec, int64_t n, int64_t npad, double* out) {
  hipLaunchKernelGGL(loo_mean_grad_kernel, dim3(1), dim3(kThreads), 0, st, vec + kLooH * npad, n, out);
}

int launch_loo_small(hipStream_t st, const LooSmallArgs& args) {
  if (args.n < 1 || args.n > kLsN || args.npad < kLsN || args.n_ls < 1 || args.n_ls > kGradMaxLs) {
    note_launch_error("launch_loo_small: shape outside the one-workgroup kernel's");
    return -1;
  }
  constexpr int kBytes = kLooSmallLdsDoubles * 8;
  static_assert(kBytes <= 160 * 1024, "the one-workgroup LOO kernel's LDS exceeds a CU's");
  const bool xs_lds = kLsN * args.dp <= kLsXs;
  const void* fn = xs_lds ? reinterpret_cast<const void*>(&loo_small_kernel<true>) : reinterpret_cast<const void*>(&loo_small_kernel<false>);
  const int rc = ensure_dyn_lds(fn, kBytes);
  if (rc) return rc;
  if (xs_lds) hipLaunchKernelGGL(loo_small_kernel<true>, dim3(1), dim3(kThreads), kBytes, st, args);
  else hipLaunchKernelGGL(loo_small_kernel<false>, dim3(1), dim3(kThreads), kBytes, st, args);
  return 0;
}

}  // namespace gpso
