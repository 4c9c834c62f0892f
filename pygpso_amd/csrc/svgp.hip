// Sparse variational GP on inducing points (GPflow 2 SVGP, whitened, full q_sqrt, full batch): the
// column-wise kernels of the SVGP's moments, the column scale ahead of the long-K product, the closed-form Gaussian per-point
// terms and the scalar sums of the -ELBO.  The inducing rows Z are the context's resident rows (M, padded to M_pad); the
// training data sits in the SGPR's buffers (N rows, padded to N_pad).  Rectangular matrices are dense [M_pad x N_pad]
// float64, row-major (leading dimension N_pad), zero on the padding, as in sgpr.hip.  The products, factorisations, the
// cross-Gram, the cross contraction and the quadrature are the existing kernels (fit.hip, sgpr.hip, vgp.hip); api.hip
// (EngineT::svgp_*) sequences them.  Every reduction here runs in a fixed order (no atomics).
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

// the moments of q(f) at the training points, one column j of A = Lu^-1 Kuf (and of B = S^T A) per lane:
//   fm[j] = A_j^T mu + c,   fv[j] = variance - |A_j|^2 + |B_j|^2   (B nullable: the last term is left out)
// 64 columns x 4 slices of the M rows per workgroup (a lane reads consecutive columns: coalesced); the slices are summed
// in LDS in a fixed order.  Zero on the padding.
__global__ __launch_bounds__(kThreads) void svgp_moments_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                                const double* __restrict__ mu, double variance, double c,
                                                                double* __restrict__ fm, double* __restrict__ fv, int64_t m,
                                                                int64_t n, int64_t npad) {
  __shared__ double part[3][4][64];
  const int col = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * 64 + col;
  double sm = 0.0, sa = 0.0, sb = 0.0;
  if (j < n)
    for (int64_t i = slice; i < m; i += 4) {
      const double a = A[i * npad + j];
      sm += a * mu[i];
      sa += a * a;
      if (B != nullptr) {
        const double b = B[i * npad + j];
        sb += b * b;
      }
    }
  part[0][slice][col] = sm;
  part[1][slice][col] = sa;
  part[2][slice][col] = sb;
  __syncthreads();
  if (slice == 0 && j < npad) {
    const double tm = (part[0][0][col] + part[0][1][col]) + (part[0][2][col] + part[0][3][col]);
    const double ta = (part[1][0][col] + part[1][1][col]) + (part[1][2][col] + part[1][3][col]);
    const double tb = (part[2][0][col] + part[2][1][col]) + (part[2][2][col] + part[2][3][col]);
    fm[j] = (j < n) ? tm + c : 0.0;
    fv[j] = (j < n) ? variance - ta + tb : 0.0;
  }
}

// D = A diag(a) on the real block of an [mpad x npad] matrix (column j scaled by a[j]), zero on the padding
__global__ __launch_bounds__(kThreads) void svgp_colscale_kernel(const double* __restrict__ A, const double* __restrict__ a,
                                                                 double* __restrict__ D, int64_t m, int64_t mpad, int64_t n,
                                                                 int64_t npad) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= mpad * npad) return;
  const int64_t i = idx / npad, j = idx - i * npad;
  D[idx] = (i < m && j < n) ? a[j] * A[idx] : 0.0;
}

// the Gaussian likelihood's variational expectation in closed form, one lane per training point (the outputs of
// vgp_quad_kernel): with e = y - fm,  VE = -log(2 pi s2) / 2 - (e^2 + fv) / (2 s2),  gm = dVE/dm = e / s2,
// a = -2 dVE/dv = 1 / s2,  t = gm + a (fm - c),  dve = dVE/ds2 = -1 / (2 s2) + (e^2 + fv) / (2 s2^2).  Zero on the padding.
__global__ __launch_bounds__(kThreads) void svgp_gauss_kernel(const double* __restrict__ y, const double* __restrict__ fm,
                                                              const double* __restrict__ fv, double s2, double c,
                                                              double* __restrict__ gm, double* __restrict__ a,
                                                              double* __restrict__ t, double* __restrict__ ve,
                                                              double* __restrict__ dve, int64_t n, int64_t npad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npad) return;
  if (i >= n) {
    gm[i] = a[i] = t[i] = ve[i] = dve[i] = 0.0;
    return;
  }
  const double e = y[i] - fm[i], q = e * e + fv[i], b = 1.0 / s2;
  gm[i] = e * b;
  a[i] = b;
  t[i] = (y[i] - c) * b;  // (= gm + a (fm - c))
  ve[i] = -0.5 * log(2.0 * M_PI * s2) - 0.5 * q * b;
  dve[i] = -0.5 * b + 0.5 * q * b * b;
}

// the scalar sums of the -ELBO and of its non-theta derivatives (one workgroup, fixed order):
// over the n training points: out[0] sum VE, [1] sum dVE/dp, [2] sum gm, [3] sum a;
// over the m inducing rows:   out[4] sum mu^2, [5] sum of the squared rows of S (tr Sigma), [6] sum log S_ii^2
__global__ __launch_bounds__(kThreads) void svgp_sums_kernel(const double* __restrict__ ve, const double* __restrict__ dve,
                                                             const double* __restrict__ gm, const double* __restrict__ a,
                                                             int64_t n, const double* __restrict__ mu,
                                                             const double* __restrict__ srow, const double* __restrict__ S,
                                                             int64_t m, int64_t mpad, double* __restrict__ out) {
  __shared__ double red[4];
  double s[kSvgpSums];
#pragma unroll
  for (int q = 0; q < kSvgpSums; ++q) s[q] = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += kThreads) {
    s[0] += ve[j];
    s[1] += dve[j];
    s[2] += gm[j];
    s[3] += a[j];
  }
  for (int64_t i = threadIdx.x; i < m; i += kThreads) {
    const double sii = S[i * mpad + i];
    s[4] += mu[i] * mu[i];
    s[5] += srow[i];
    s[6] += log(sii * sii);
  }
#pragma unroll
  for (int q = 0; q < kSvgpSums; ++q) {
    const double v = block_sum256(s[q], red);
    if (threadIdx.x == 0) out[q] = v;
  }
}

}  // namespace

void launch_svgp_moments(hipStream_t st, const double* A, const double* B, const double* mu, double variance, double c,
                         double* fm, double* fv, int64_t m, int64_t n, int64_t npad) {
  hipLaunchKernelGGL(svgp_moments_kernel, dim3((unsigned)((npad + 63) / 64)), dim3(kThreads), 0, st, A, B, mu, variance, c,
                     fm, fv, m, n, npad);
}

void launch_svgp_colscale(hipStream_t st, const double* A, const double* a, double* D, int64_t m, int64_t mpad, int64_t n,
                          int64_t npad) {
  hipLaunchKernelGGL(svgp_colscale_kernel, dim3(blocks_for(mpad * npad)), dim3(kThreads), 0, st, A, a, D, m, mpad, n, npad);
}

void launch_svgp_gauss(hipStream_t st, const double* y, const double* fm, const double* fv, double s2, double c, double* gm,
                       double* a, double* t, double* ve, double* dve, int64_t n, int64_t npad) {
  hipLaunchKernelGGL(svgp_gauss_kernel, dim3(blocks_for(npad)), dim3(kThreads), 0, st, y, fm, fv, s2, c, gm, a, t, ve, dve, n,
                     npad);
}

void launch_svgp_sums(hipStream_t st, const double* ve, const double* dve, const double* gm, const double* a, int64_t n,
                      const double* mu, const double* srow, const double* S, int64_t m, int64_t mpad, double* out) {
  hipLaunchKernelGGL(svgp_sums_kernel, dim3(1), dim3(kThreads), 0, st, ve, dve, gm, a, n, mu, srow, S, m, mpad, out);
}

}  // namespace gpso
