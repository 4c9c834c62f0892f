// Sparse GP regression on inducing points (GPflow 2 SGPR, Titsias 2009): the rectangular kernels of
// the bound, its gradient, the install and the greedy choice of the inducing points.  The inducing rows Z are the context's
// resident rows (M, padded to M_pad); the training data X, y (N rows, padded to N_pad) sit in buffers of their own.
// Rectangular matrices are dense [M_pad x N_pad] float64, row-major (leading dimension N_pad), zero on the padding.  The
// products are the fit's LDS-DMA tile GEMM (fit.hip: launch_dgemm_rect), the factorisations its launch_potrf /
// launch_trtri at size M, the Kuu part of the gradient its grad_tile_kernel; api.hip (EngineT::sgpr_*) sequences them.
// Every reduction here runs in a fixed order (no atomics): a call repeated on the same inputs gives the same bits.
#include <climits>
#include <cmath>

#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;

inline unsigned blocks_for(int64_t total) { return total < kThreads ? 1u : (unsigned)((total + kThreads - 1) / kThreads); }

// sum over the workgroup's 256 threads in a fixed order (wave sums, then the four waves left to right); all threads call
__device__ __forceinline__ double block_sum256(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// rows of a 64-row block of scaled inputs into LDS at the odd stride ds (fit.hip: grad_tile_kernel has the reason)
__device__ __forceinline__ void load_rows64(const double* __restrict__ xs, int64_t row0, int64_t rows_pad, int dp, int ds,
                                            double* dst) {
  for (int e = threadIdx.x; e < 64 * dp; e += kThreads) {
    const int r = e / dp, c = e - r * dp;
    dst[r * ds + c] = (row0 + r < rows_pad) ? xs[(row0 + r) * dp + c] : 0.0;
  }
}

// Kuf = k(Z, X): one workgroup per 64 x 64 tile, a thread's 16 entries share their column.  r^2 from direct differences
// (>= 0, free of cancellation); zero on the padding of either side.
__global__ __launch_bounds__(kThreads) void sgpr_cross_gram_kernel(const double* __restrict__ zs, const double* __restrict__ xs,
                                                                   int64_t m, int64_t mpad, int64_t n, int64_t npad, int dp,
                                                                   int kernel, double variance, double* __restrict__ kuf) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int ds = dp | 1;
  double* zi = reinterpret_cast<double*>(lds_raw);  // [64][ds]
  double* xj = zi + 64 * ds;                        // [64][ds]
  const int64_t ti = blockIdx.y, tj = blockIdx.x;
  load_rows64(zs, ti * 64, mpad, dp, ds, zi);
  load_rows64(xs, tj * 64, npad, dp, ds, xj);
  __syncthreads();
  const int jj = threadIdx.x & 63, i0 = threadIdx.x >> 6;
  double r2[16];
#pragma unroll
  for (int p = 0; p < 16; ++p) r2[p] = 0.0;
  for (int k = 0; k < dp; ++k) {
    const double b = xj[jj * ds + k];
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const double df = zi[(i0 + 4 * p) * ds + k] - b;
      r2[p] = fma(df, df, r2[p]);
    }
  }
  const int64_t j = tj * 64 + jj;
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    const int64_t i = ti * 64 + i0 + 4 * p;
    if (i >= mpad || j >= npad) continue;
    kuf[i * npad + j] = (i < m && j < n) ? kern_from_r2_lean(kernel, r2[p], variance) : 0.0;
  }
}

// sum_ij W_ij dKuf_ij / d(lengthscales..., variance), W_ij = g[i][j] + a[i] t[j], over one 64 x 64 tile per workgroup:
// partial[blk * (n_ls + 1) + h].  r^2 is regenerated from the scaled inputs (no dK is stored), as grad_tile_kernel does
// for the square case.
__global__ __launch_bounds__(kThreads) void sgpr_cross_grad_kernel(const double* __restrict__ g, const double* __restrict__ a,
                                                                   const double* __restrict__ t, const double* __restrict__ zs,
                                                                   const double* __restrict__ xs, int64_t m, int64_t mpad,
                                                                   int64_t n, int64_t npad, int dp, int n_ls,
                                                                   const double* __restrict__ ls, int kernel, double variance,
                                                                   double* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int ds = dp | 1;
  double* zi = reinterpret_cast<double*>(lds_raw);
  double* xj = zi + 64 * ds;
  __shared__ double red[4];
  const int64_t ti = blockIdx.y, tj = blockIdx.x;
  const int64_t blk = ti * gridDim.x + tj;
  const int H = n_ls + 1;
  load_rows64(zs, ti * 64, mpad, dp, ds, zi);
  load_rows64(xs, tj * 64, npad, dp, ds, xj);
  __syncthreads();
  const int jj = threadIdx.x & 63, i0 = threadIdx.x >> 6;
  double r2[16], base[16];
#pragma unroll
  for (int p = 0; p < 16; ++p) r2[p] = 0.0;
  for (int k = 0; k < dp; ++k) {
    const double b = xj[jj * ds + k];
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const double df = zi[(i0 + 4 * p) * ds + k] - b;
      r2[p] = fma(df, df, r2[p]);
    }
  }
  const int64_t j = tj * 64 + jj;
  const double tj_v = (j < n) ? t[j] : 0.0;
  double g_var = 0.0, g_iso = 0.0;
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    const int64_t i = ti * 64 + i0 + 4 * p;
    base[p] = 0.0;
    if (i >= m || j >= n) continue;
    const double W = g[i * npad + j] + a[i] * tj_v;
    double kv, dk;
    kern_and_dkern_same(kernel, r2[p], variance, kv, dk);
    g_var += W * kv / variance;
    base[p] = W * dk;
    g_iso += base[p] * (-2.0 * r2[p]);
  }
  const double sv = block_sum256(g_var, red);
  if (n_ls == 1) {
    const double sl = block_sum256(g_iso, red) / ls[0];
    if (threadIdx.x == 0) partial[blk * H + 0] = sl;
  } else {
    for (int d = 0; d < n_ls; ++d) {
      double acc = 0.0;
      const double b = xj[jj * ds + d];
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        const double df = zi[(i0 + 4 * p) * ds + d] - b;
        acc += base[p] * (-2.0 * df * df);
      }
      const double sd = block_sum256(acc, red) / ls[d];
      if (threadIdx.x == 0) partial[blk * H + d] = sd;
    }
  }
  if (threadIdx.x == 0) partial[blk * H + n_ls] = sv;
}

// out[h] = sum over the tiles of partial[blk * H + h] (one workgroup, fixed order)
__global__ __launch_bounds__(kThreads) void sgpr_cross_grad_final_kernel(const double* __restrict__ partial, int64_t nblk,
                                                                         int H, double* __restrict__ out) {
  __shared__ double red[4];
  for (int h = 0; h < H; ++h) {
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += kThreads) acc += partial[b * H + h];
    acc = block_sum256(acc, red);
    if (threadIdx.x == 0) out[h] = acc;
  }
}

// the split-K partial products summed in their fixed order: aat = sum_s part[s] on the real block (zero on the padding),
// bm = I + aat (identity on the padding); *info := INT_MAX
__global__ __launch_bounds__(kThreads) void sgpr_splitk_sum_kernel(const double* __restrict__ part, int nsplit, int64_t m,
                                                                   int64_t mpad, double* __restrict__ aat,
                                                                   double* __restrict__ bm, int* info) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx == 0 && info != nullptr) *info = INT_MAX;
  if (idx >= mpad * mpad) return;
  const int64_t i = idx / mpad, j = idx - i * mpad;
  double v = 0.0;
  if (i < m && j < m)
    for (int s = 0; s < nsplit; ++s) v += part[(int64_t)s * mpad * mpad + idx];
  aat[idx] = v;
  bm[idx] = v + (i == j ? 1.0 : 0.0);
}

// out[i] = alpha * sum_{j<n} A[i][j] x[j] for i < m (one wave per row: coalesced); 0 on the padding
__global__ __launch_bounds__(kThreads) void sgpr_gemv_n_kernel(const double* __restrict__ A, const double* __restrict__ x,
                                                               double alpha, double* __restrict__ out, int64_t m,
                                                               int64_t mpad, int64_t n, int64_t npad) {
  const int64_t i = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= mpad) return;
  double acc = 0.0;
  if (i < m)
    for (int64_t k = lane; k < n; k += kWave) acc += A[i * npad + k] * x[k];
  acc = wave_sum(acc);
  if (lane == 0) out[i] = alpha * acc;
}

// out[j] = alpha * sum_{i<m} A[i][j] x[i] for j < n; 0 on the padding.  64 columns x 4 slices of i per workgroup, the
// slices summed in LDS in a fixed order
__global__ __launch_bounds__(kThreads) void sgpr_gemv_t_kernel(const double* __restrict__ A, const double* __restrict__ x,
                                                               double alpha, double* __restrict__ out, int64_t m, int64_t n,
                                                               int64_t npad) {
  __shared__ double part[4][64];
  const int c = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * 64 + c;
  double acc = 0.0;
  if (j < n)
    for (int64_t i = slice; i < m; i += 4) acc += A[i * npad + j] * x[i];
  part[slice][c] = acc;
  __syncthreads();
  if (slice == 0 && j < npad) out[j] = (j < n) ? alpha * ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) : 0.0;
}

// e = y - c on rows < n, 0 on the padding
__global__ __launch_bounds__(kThreads) void sgpr_resid_kernel(const double* __restrict__ y, double c, double* __restrict__ e,
                                                              int64_t n, int64_t npad) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < npad) e[j] = (j < n) ? y[j] - c : 0.0;
}

// t = p e + q w on rows < n, 0 on the padding
__global__ __launch_bounds__(kThreads) void sgpr_tvec_kernel(const double* __restrict__ e, const double* __restrict__ w,
                                                             double p, double q, double* __restrict__ t, int64_t n,
                                                             int64_t npad) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < npad) t[j] = (j < n) ? p * e[j] + q * w[j] : 0.0;
}

// kin = -g1 / b + b^2 a a^T + p on the real block (= -2 dF/dKuu), zero on the padding
__global__ __launch_bounds__(kThreads) void sgpr_wuu_kernel(const double* __restrict__ g1, const double* __restrict__ p,
                                                            const double* __restrict__ a, double b, double* __restrict__ kin,
                                                            int64_t m, int64_t mpad) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= mpad * mpad) return;
  const int64_t i = idx / mpad, j = idx - i * mpad;
  kin[idx] = (i < m && j < m) ? -g1[idx] / b + b * b * a[i] * a[j] + p[idx] : 0.0;
}

// the scalars of the bound and of its sigma^2 / c derivatives, one workgroup, fixed order:
// out[0] sum log diag LB   [1] e.e   [2] cv.cv   [3] tr(A A^T)   [4] e.w   [5] w.w   [6] sum e   [7] sum w
// [8] |LB^-1|_F^2 (from its squared row norms)      (w, lbinv_rows nullable: the slots stay 0)
__global__ __launch_bounds__(kThreads) void sgpr_sums_kernel(const double* __restrict__ lb, const double* __restrict__ aat,
                                                             const double* __restrict__ cv, const double* __restrict__ e,
                                                             const double* __restrict__ w,
                                                             const double* __restrict__ lbinv_rows, int64_t m, int64_t mpad,
                                                             int64_t n, double* __restrict__ out) {
  __shared__ double red[4];
  double s[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) s[q] = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += kThreads) {
    s[0] += log(lb[i * mpad + i]);
    s[2] += cv[i] * cv[i];
    s[3] += aat[i * mpad + i];
    if (lbinv_rows != nullptr) s[8] += lbinv_rows[i];
  }
  for (int64_t j = threadIdx.x; j < n; j += kThreads) {
    const double ej = e[j];
    s[1] += ej * ej;
    s[6] += ej;
    if (w != nullptr) {
      const double wj = w[j];
      s[4] += ej * wj;
      s[5] += wj * wj;
      s[7] += wj;
    }
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const double v = block_sum256(s[q], red);
    if (threadIdx.x == 0) out[q] = v;
  }
}

// ---- greedy conditional-variance selection (pivoted partial Cholesky of k(X, X)) ------------------------------------------
__global__ __launch_bounds__(kThreads) void sgpr_greedy_init_kernel(double* __restrict__ dvec, double variance, int64_t n,
                                                                    int64_t npad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npad) dvec[i] = (i < n) ? variance : -HUGE_VAL;
}

// p = arg-max of dvec over rows < n (picked rows hold -inf), the lowest index on exact ties: one workgroup of 1024.
// A largest conditional variance that is not above floor (k(X, X) numerically rank-deficient: a square root of it would
// poison every later column) ends the selection: idx[step] = -1, and every later step repeats that verdict.
__global__ __launch_bounds__(1024) void sgpr_greedy_argmax_kernel(const double* __restrict__ dvec, int64_t n, int step,
                                                                  double floor, int64_t* __restrict__ idx,
                                                                  double* __restrict__ pivot) {
  __shared__ double bv[1024];
  __shared__ int64_t bi[1024];
  double v = -HUGE_VAL;
  int64_t at = INT64_MAX;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const double x = dvec[i];
    if (x > v) {  // (ascending i per thread: a later equal value never replaces an earlier one)
      v = x;
      at = i;
    }
  }
  bv[threadIdx.x] = v;
  bi[threadIdx.x] = at;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = bv[threadIdx.x + s];
      const int64_t oi = bi[threadIdx.x + s];
      if (ov > bv[threadIdx.x] || (ov == bv[threadIdx.x] && oi < bi[threadIdx.x])) {
        bv[threadIdx.x] = ov;
        bi[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const bool dead = (step > 0 && idx[step - 1] < 0) || !(bv[0] > floor);
    idx[step] = dead ? -1 : bi[0];
    pivot[0] = bv[0];
  }
}

// column `step` of the partial factor: l_i = (k(x_i, x_p) - sum_{t < step} L[t][i] L[t][p]) / sqrt(d_p), d_i -= l_i^2;
// the picked row leaves the candidates (d_p := -inf).  L is stored [step][N_pad]: a thread's reads are coalesced.
__global__ __launch_bounds__(kThreads) void sgpr_greedy_col_kernel(const double* __restrict__ xs, int dp, int kernel,
                                                                   double variance, const int64_t* __restrict__ idx,
                                                                   const double* __restrict__ pivot, int step,
                                                                   double* __restrict__ lg, double* __restrict__ dvec,
                                                                   int64_t n, int64_t npad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npad) return;
  const int64_t p = idx[step];
  if (i >= n || p < 0 || p >= n) {  // (padding, or a selection that ended: nothing is updated)
    lg[(int64_t)step * npad + i] = 0.0;
    return;
  }
  double r2 = 0.0;
  for (int k = 0; k < dp; ++k) {
    const double df = xs[i * dp + k] - xs[p * dp + k];
    r2 = fma(df, df, r2);
  }
  double v = kern_from_r2_lean(kernel, r2, variance);
  for (int t = 0; t < step; ++t) v -= lg[(int64_t)t * npad + i] * lg[(int64_t)t * npad + p];
  const double l = v / sqrt(pivot[0]);
  lg[(int64_t)step * npad + i] = l;
  const double di = dvec[i];
  dvec[i] = (i == p) ? -HUGE_VAL : (di == -HUGE_VAL ? di : di - l * l);
}

}  // namespace

void launch_sgpr_cross_gram(hipStream_t st, const double* zs, const double* xs, int64_t m, int64_t mpad, int64_t n,
                            int64_t npad, int dp, const KernParams& kp, double* kuf) {
  const size_t lds = (size_t)2 * 64 * (dp | 1) * sizeof(double);
  hipLaunchKernelGGL(sgpr_cross_gram_kernel, dim3((unsigned)(npad / 64), (unsigned)(mpad / 64)), dim3(kThreads), lds, st, zs,
                     xs, m, mpad, n, npad, dp, kp.kernel, kp.variance, kuf);
}

void launch_sgpr_cross_grad(hipStream_t st, const double* g, const double* a, const double* t, const double* zs,
                            const double* xs, int64_t m, int64_t mpad, int64_t n, int64_t npad, int dp, int n_ls,
                            const double* ls, const KernParams& kp, double* partial, double* out) {
  const size_t lds = (size_t)2 * 64 * (dp | 1) * sizeof(double);
  const dim3 grid((unsigned)(npad / 64), (unsigned)(mpad / 64));
  hipLaunchKernelGGL(sgpr_cross_grad_kernel, grid, dim3(kThreads), lds, st, g, a, t, zs, xs, m, mpad, n, npad, dp, n_ls, ls,
                     kp.kernel, kp.variance, partial);
  hipLaunchKernelGGL(sgpr_cross_grad_final_kernel, dim3(1), dim3(kThreads), 0, st, partial, (int64_t)grid.x * grid.y,
                     n_ls + 1, out);
}

void launch_sgpr_splitk_sum(hipStream_t st, const double* part, int nsplit, int64_t m, int64_t mpad, double* aat, double* bm,
                            int* info) {
  hipLaunchKernelGGL(sgpr_splitk_sum_kernel, dim3(blocks_for(mpad * mpad)), dim3(kThreads), 0, st, part, nsplit, m, mpad, aat,
                     bm, info);
}

void launch_sgpr_gemv(hipStream_t st, const double* A, bool trans, const double* x, double alpha, double* out, int64_t m,
                      int64_t mpad, int64_t n, int64_t npad) {
  if (trans)
    hipLaunchKernelGGL(sgpr_gemv_t_kernel, dim3((unsigned)((npad + 63) / 64)), dim3(kThreads), 0, st, A, x, alpha, out, m, n,
                       npad);
  else
    hipLaunchKernelGGL(sgpr_gemv_n_kernel, dim3((unsigned)((mpad + 3) / 4)), dim3(kThreads), 0, st, A, x, alpha, out, m, mpad,
                       n, npad);
}

void launch_sgpr_resid(hipStream_t st, const double* y, double c, double* e, int64_t n, int64_t npad) {
  hipLaunchKernelGGL(sgpr_resid_kernel, dim3(blocks_for(npad)), dim3(kThreads), 0, st, y, c, e, n, npad);
}

void launch_sgpr_tvec(hipStream_t st, const double* e, const double* w, double p, double q, double* t, int64_t n,
                      int64_t npad) {
  hipLaunchKernelGGL(sgpr_tvec_kernel, dim3(blocks_for(npad)), dim3(kThreads), 0, st, e, w, p, q, t, n, npad);
}

void launch_sgpr_wuu(hipStream_t st, const double* g1, const double* p, const double* a, double b, double* kin, int64_t m,
                     int64_t mpad) {
  hipLaunchKernelGGL(sgpr_wuu_kernel, dim3(blocks_for(mpad * mpad)), dim3(kThreads), 0, st, g1, p, a, b, kin, m, mpad);
}

void launch_sgpr_sums(hipStream_t st, const double* lb, const double* aat, const double* cv, const double* e, const double* w,
                      const double* lbinv_rows, int64_t m, int64_t mpad, int64_t n, double* out) {
  hipLaunchKernelGGL(sgpr_sums_kernel, dim3(1), dim3(kThreads), 0, st, lb, aat, cv, e, w, lbinv_rows, m, mpad, n, out);
}

void launch_sgpr_greedy(hipStream_t st, const double* xs, int64_t n, int64_t npad, int dp, const KernParams& kp, int m,
                        double* lg, double* dvec, double* pivot, int64_t* idx) {
  hipLaunchKernelGGL(sgpr_greedy_init_kernel, dim3(blocks_for(npad)), dim3(kThreads), 0, st, dvec, kp.variance, n, npad);
  for (int step = 0; step < m; ++step) {
    hipLaunchKernelGGL(sgpr_greedy_argmax_kernel, dim3(1), dim3(1024), 0, st, dvec, n, step, 1.0e-12 * kp.variance, idx, pivot);
    hipLaunchKernelGGL(sgpr_greedy_col_kernel, dim3(blocks_for(npad)), dim3(kThreads), 0, st, xs, dp, kp.kernel, kp.variance,
                       idx, pivot, step, lg, dvec, n, npad);
  }
}

}  // namespace gpso
