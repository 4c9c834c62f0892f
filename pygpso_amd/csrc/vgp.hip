// Variational GP (GPflow 2 VGP, whitened; the Gaussian likelihood in closed form, other scalar likelihoods through
// Gauss-Hermite quadrature): the element-wise, vector and reduction kernels of the
// natural-gradient step, the -ELBO with its gradient and the install of the predictive.  The
// factorisations, the large products and the gradient contraction are the fit's own kernels (fit.hip: launch_potrf,
// launch_trtri, launch_dgemm, launch_gradient); api.hip (EngineT::vgp_*) sequences them on the context's stream.
// Every matrix here is a dense N_pad x N_pad float64 buffer, row-major; rows / columns >= n are padding.
#include <climits>

#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;

inline unsigned blocks_for(int64_t total) { return total < kThreads ? 1u : (unsigned)((total + kThreads - 1) / kThreads); }

// dst = the lower triangle of src on rows / columns < n, zero above it; padding: pad_diag on the diagonal, zero elsewhere
// (src may be dst)
__global__ __launch_bounds__(kThreads) void vgp_clean_lower_kernel(const double* src, double* dst, int64_t n, int64_t npad,
                                                                   double pad_diag) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npad * npad) return;
  const int64_t i = idx / npad, j = idx - i * npad;
  double v = 0.0;
  if (i < n && j < n) v = (j <= i) ? src[idx] : 0.0;
  else if (i == j) v = pad_diag;
  dst[idx] = v;
}

// padding rows / columns of m := identity (the real block untouched); *info := INT_MAX ("no failing pivot")
__global__ __launch_bounds__(kThreads) void vgp_pad_identity_kernel(double* m, int64_t n, int64_t npad, int* info) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx == 0 && info != nullptr) *info = INT_MAX;
  if (idx >= npad * npad) return;
  const int64_t i = idx / npad, j = idx - i * npad;
  if (i >= n || j >= n) m[idx] = (i == j) ? 1.0 : 0.0;
}

// y = a x + b y (element-wise, len entries)
__global__ __launch_bounds__(kThreads) void vgp_axpby_kernel(const double* x, double* y, int64_t len, double a, double b) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < len) y[idx] = a * x[idx] + b * y[idx];
}

// out[i] = (sub ? sub[i] - v : v),  v = alpha * sum_{k<n} A[i][k] (x[k] - xshift) + add,  for i < n; 0 on the padding.
// One wave per row (k strided over the lanes: coalesced).
__global__ __launch_bounds__(kThreads) void vgp_gemv_n_kernel(const double* __restrict__ A, const double* __restrict__ x,
                                                              double xshift, double alpha, double add,
                                                              const double* __restrict__ sub, double* __restrict__ out,
                                                              int64_t n, int64_t npad) {
  const int64_t i = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= npad) return;
  double acc = 0.0;
  if (i < n)
    for (int64_t k = lane; k < n; k += kWave) acc += A[i * npad + k] * (x[k] - xshift);
  acc = wave_sum(acc);
  if (lane == 0) {
    const double v = alpha * acc + add;
    out[i] = (i < n) ? (sub != nullptr ? sub[i] - v : v) : 0.0;
  }
}

// out[j] = alpha * sum_{k<n} A[k][j] (x[k] - xshift) for j < n; 0 on the padding.  A workgroup = 64 columns x 4 slices
// of k (a lane reads consecutive columns: coalesced); the four slices are summed in LDS in a fixed order.
__global__ __launch_bounds__(kThreads) void vgp_gemv_t_kernel(const double* __restrict__ A, const double* __restrict__ x,
                                                              double xshift, double alpha, double* __restrict__ out,
                                                              int64_t n, int64_t npad) {
  __shared__ double part[4][64];
  const int64_t j = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int slice = threadIdx.x >> 6;
  double acc = 0.0;
  if (j < n)
    for (int64_t k = slice; k < n; k += 4) acc += A[k * npad + j] * (x[k] - xshift);
  part[slice][threadIdx.x & 63] = acc;
  __syncthreads();
  if (slice == 0 && j < npad) {
    const int c = threadIdx.x & 63;
    out[j] = (j < n) ? alpha * ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) : 0.0;
  }
}

// out[i] = sum_{j<n} A[i][j]^2 for i < n (one wave per row); 0 on the padding
__global__ __launch_bounds__(kThreads) void vgp_rownorm_kernel(const double* __restrict__ A, double* __restrict__ out,
                                                               int64_t n, int64_t npad) {
  const int64_t i = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= npad) return;
  double acc = 0.0;
  if (i < n)
    for (int64_t k = lane; k < n; k += kWave) {
      const double a = A[i * npad + k];
      acc += a * a;
    }
  acc = wave_sum(acc);
  if (lane == 0) out[i] = acc;
}

// Lbar = tril(L Sigma - r mu^T) / sigma^2, in place over the buffer holding L Sigma (zero above the diagonal and on the
// padding)
__global__ __launch_bounds__(kThreads) void vgp_lbar_kernel(double* lsig, const double* __restrict__ r,
                                                            const double* __restrict__ mu, int64_t n, int64_t npad,
                                                            double inv_s2) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npad * npad) return;
  const int64_t i = idx / npad, j = idx - i * npad;
  lsig[idx] = (i < n && j <= i) ? (lsig[idx] - r[i] * mu[j]) * inv_s2 : 0.0;
}

// M = Phi(P) + Phi(P)^T, Phi = lower triangle with the diagonal halved: M_ij = P_ij (i > j), P_ji (i < j), P_ii (i == j);
// zero on the padding
__global__ __launch_bounds__(kThreads) void vgp_phi_sym_kernel(const double* __restrict__ p, double* __restrict__ m,
                                                               int64_t n, int64_t npad) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npad * npad) return;
  const int64_t i = idx / npad, j = idx - i * npad;
  double v = 0.0;
  if (i < n && j < n) v = (i >= j) ? p[idx] : p[j * npad + i];
  m[idx] = v;
}

// mode 0: out = J (I - Sigma) J on the real block (J: index reversal), identity on the padding; *info := INT_MAX
// mode 1: out = J G^T J (G = chol of the mode-0 matrix): R, lower triangular, with I - Sigma = R^T R; zero padding
__global__ __launch_bounds__(kThreads) void vgp_reverse_kernel(const double* __restrict__ src, double* __restrict__ out,
                                                               int64_t n, int64_t npad, int mode, int* info) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx == 0 && info != nullptr) *info = INT_MAX;
  if (idx >= npad * npad) return;
  const int64_t i = idx / npad, j = idx - i * npad;
  double v;
  if (i < n && j < n) {
    if (mode == 0) v = (i == j ? 1.0 : 0.0) - src[(n - 1 - i) * npad + (n - 1 - j)];
    else v = (j <= i) ? src[(n - 1 - j) * npad + (n - 1 - i)] : 0.0;
  } else {
    v = (mode == 0 && i == j) ? 1.0 : 0.0;
  }
  out[idx] = v;
}

// the scalar sums of the -ELBO (one workgroup, fixed reduction order):
// out[0] sum r, [1] sum r^2, [2] sum fvar, [3] sum mu^2, [4] sum of the squared rows of S (tr Sigma), [5] sum log S_ii^2
__global__ __launch_bounds__(kThreads) void vgp_elbo_sums_kernel(const double* __restrict__ r, const double* __restrict__ fvar,
                                                                 const double* __restrict__ mu,
                                                                 const double* __restrict__ srow,
                                                                 const double* __restrict__ S, int64_t n, int64_t npad,
                                                                 double* __restrict__ out) {
  __shared__ double red[6][kThreads / kWave];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    const double ri = r[i], si = S[i * npad + i];
    acc[0] += ri;
    acc[1] += ri * ri;
    acc[2] += fvar[i];
    acc[3] += mu[i] * mu[i];
    acc[4] += srow[i];
    acc[5] += log(si * si);
  }
  for (int q = 0; q < 6; ++q) {
    const double v = wave_sum(acc[q]);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int q = threadIdx.x;
    out[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  }
}

// ---- general scalar likelihoods (Gauss-Hermite quadrature, GPflow's ScalarLikelihood.variational_expectations) ----------
// psi(f) = log p(y | f, p) for the likelihood `kind` (GPSO_LIK_*) with parameter p (Student-t: the scale s; Gaussian
// through the quadrature: the variance sigma^2), psi'(f) = d psi / df, dp = d psi / d p.  cst: the f-free part of psi.
__device__ __forceinline__ void vgp_lik_eval(int kind, double y, double f, double p, double nu, double cst, double* psi,
                                             double* dpsi, double* dp) {
  if (kind == 3) {  // Bernoulli, exact probit link: y is a label (success iff y > 0.5), no parameter
    const double s = y > 0.5 ? 1.0 : -1.0;
    const double lp = acq_log_ncdf(s * f, 0.0);
    *psi = lp;
    *dpsi = s * exp(-0.5 * f * f - 0.91893853320467274178 - lp);  // s phi(f) / Phi(s f); 1/2 log 2 pi
    *dp = 0.0;
    return;
  }
  const double e = y - f;
  if (kind == 1) {  // Student-t
    const double den = nu * p * p + e * e;
    *psi = cst - 0.5 * (nu + 1.0) * log1p(e * e / (nu * p * p));
    *dpsi = (nu + 1.0) * e / den;
    *dp = -1.0 / p + (nu + 1.0) * e * e / (p * den);
  } else {  // Gaussian (kind 2)
    *psi = cst - e * e / (2.0 * p);
    *dpsi = e / p;
    *dp = -0.5 / p + e * e / (2.0 * p * p);
  }
}

// One lane per training point i < n: with f_ik = m_i + sqrt(v_i) x_k (x, w: the scaled Gauss-Hermite nodes and weights,
// gh[0, n_gh) and gh[64, 64 + n_gh)), the quadrature sum VE_i = sum_k w_k psi(f_ik) and its derivatives:
//   gm = dVE/dm = sum w psi',  a = -2 dVE/dv = -sum w psi' x / sqrt(v),  t = gm + a (m - c),  ve = VE,  dve = dVE/dp.
// Zero on the padding.
__global__ __launch_bounds__(kThreads) void vgp_quad_kernel(const double* __restrict__ y, const double* __restrict__ m,
                                                            const double* __restrict__ v, const double* __restrict__ gh,
                                                            int n_gh, int kind, double p, double nu, double cst, double c,
                                                            double* __restrict__ gm, double* __restrict__ a,
                                                            double* __restrict__ t, double* __restrict__ ve,
                                                            double* __restrict__ dve, int64_t n, int64_t npad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npad) return;
  double s_gm = 0.0, s_gx = 0.0, s_ve = 0.0, s_dp = 0.0, ai = 0.0, mi = 0.0;
  if (i < n) {
    const double yi = y[i], sv = sqrt(v[i]);
    mi = m[i];
#pragma unroll 4
    for (int k = 0; k < n_gh; ++k) {
      const double xk = gh[k], wk = gh[64 + k];
      double psi, dpsi, dp;
      vgp_lik_eval(kind, yi, mi + sv * xk, p, nu, cst, &psi, &dpsi, &dp);
      s_gm += wk * dpsi;
      s_gx += wk * dpsi * xk;
      s_ve += wk * psi;
      s_dp += wk * dp;
    }
    ai = -s_gx / sv;
  }
  gm[i] = s_gm;
  a[i] = ai;
  t[i] = (i < n) ? s_gm + ai * (mi - c) : 0.0;
  ve[i] = s_ve;
  dve[i] = s_dp;
}

// the scalar sums of the general -ELBO (one workgroup, fixed reduction order):
// out[0] sum VE, [1] sum dVE/dp, [2] sum gm, [3] sum mu^2, [4] sum of the squared rows of S (tr Sigma), [5] sum log S_ii^2
__global__ __launch_bounds__(kThreads) void vgp_lik_sums_kernel(const double* __restrict__ ve, const double* __restrict__ dve,
                                                                const double* __restrict__ gm, const double* __restrict__ mu,
                                                                const double* __restrict__ srow,
                                                                const double* __restrict__ S, int64_t n, int64_t npad,
                                                                double* __restrict__ out) {
  __shared__ double red[6][kThreads / kWave];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    const double si = S[i * npad + i];
    acc[0] += ve[i];
    acc[1] += dve[i];
    acc[2] += gm[i];
    acc[3] += mu[i] * mu[i];
    acc[4] += srow[i];
    acc[5] += log(si * si);
  }
  for (int q = 0; q < 6; ++q) {
    const double v = wave_sum(acc[q]);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int q = threadIdx.x;
    out[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  }
}

// Lbar = tril(diag(a) L Sigma - gm mu^T), in place over the buffer holding L Sigma (zero above the diagonal and on the
// padding): vgp_lbar_kernel with per-point weights
__global__ __launch_bounds__(kThreads) void vgp_lbar_w_kernel(double* lsig, const double* __restrict__ a,
                                                              const double* __restrict__ gm, const double* __restrict__ mu,
                                                              int64_t n, int64_t npad) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npad * npad) return;
  const int64_t i = idx / npad, j = idx - i * npad;
  lsig[idx] = (i < n && j <= i) ? a[i] * lsig[idx] - gm[i] * mu[j] : 0.0;
}

// B = diag(a) A on the real block, zero on the padding
__global__ __launch_bounds__(kThreads) void vgp_rowscale_kernel(const double* __restrict__ A, const double* __restrict__ a,
                                                                double* __restrict__ B, int64_t n, int64_t npad) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npad * npad) return;
  const int64_t i = idx / npad, j = idx - i * npad;
  B[idx] = (i < n && j < n) ? a[i] * A[idx] : 0.0;
}

}  // namespace

void launch_vgp_clean_lower(hipStream_t st, const double* src, double* dst, int64_t n, int64_t npad, double pad_diag) {
  hipLaunchKernelGGL(vgp_clean_lower_kernel, dim3(blocks_for(npad * npad)), dim3(kThreads), 0, st, src, dst, n, npad, pad_diag);
}
void launch_vgp_pad_identity(hipStream_t st, double* m, int64_t n, int64_t npad, int* info) {
  hipLaunchKernelGGL(vgp_pad_identity_kernel, dim3(blocks_for(npad * npad)), dim3(kThreads), 0, st, m, n, npad, info);
}
void launch_vgp_axpby(hipStream_t st, const double* x, double* y, int64_t len, double a, double b) {
  hipLaunchKernelGGL(vgp_axpby_kernel, dim3(blocks_for(len)), dim3(kThreads), 0, st, x, y, len, a, b);
}
void launch_vgp_gemv(hipStream_t st, const double* A, bool trans, const double* x, double xshift, double alpha, double add,
                     const double* sub, double* out, int64_t n, int64_t npad) {
  if (trans)
    hipLaunchKernelGGL(vgp_gemv_t_kernel, dim3((unsigned)(npad / 64)), dim3(kThreads), 0, st, A, x, xshift, alpha, out, n, npad);
  else
    hipLaunchKernelGGL(vgp_gemv_n_kernel, dim3((unsigned)((npad + 3) / 4)), dim3(kThreads), 0, st, A, x, xshift, alpha, add,
                       sub, out, n, npad);
}
void launch_vgp_rownorm(hipStream_t st, const double* A, double* out, int64_t n, int64_t npad) {
  hipLaunchKernelGGL(vgp_rownorm_kernel, dim3((unsigned)((npad + 3) / 4)), dim3(kThreads), 0, st, A, out, n, npad);
}
void launch_vgp_lbar(hipStream_t st, double* lsig, const double* r, const double* mu, int64_t n, int64_t npad, double inv_s2) {
  hipLaunchKernelGGL(vgp_lbar_kernel, dim3(blocks_for(npad * npad)), dim3(kThreads), 0, st, lsig, r, mu, n, npad, inv_s2);
}
void launch_vgp_phi_sym(hipStream_t st, const double* p, double* m, int64_t n, int64_t npad) {
  hipLaunchKernelGGL(vgp_phi_sym_kernel, dim3(blocks_for(npad * npad)), dim3(kThreads), 0, st, p, m, n, npad);
}
void launch_vgp_reverse(hipStream_t st, const double* src, double* out, int64_t n, int64_t npad, int mode, int* info) {
  hipLaunchKernelGGL(vgp_reverse_kernel, dim3(blocks_for(npad * npad)), dim3(kThreads), 0, st, src, out, n, npad, mode, info);
}
void launch_vgp_elbo_sums(hipStream_t st, const double* r, const double* fvar, const double* mu, const double* srow,
                          const double* S, int64_t n, int64_t npad, double* out) {
  hipLaunchKernelGGL(vgp_elbo_sums_kernel, dim3(1), dim3(kThreads), 0, st, r, fvar, mu, srow, S, n, npad, out);
}

void launch_vgp_quad(hipStream_t st, const double* y, const double* m, const double* v, const double* gh, int n_gh, int kind,
                     double p, double nu, double cst, double c, double* gm, double* a, double* t, double* ve, double* dve,
                     int64_t n, int64_t npad) {
  hipLaunchKernelGGL(vgp_quad_kernel, dim3(blocks_for(npad)), dim3(kThreads), 0, st, y, m, v, gh, n_gh, kind, p, nu, cst, c,
                     gm, a, t, ve, dve, n, npad);
}
void launch_vgp_lik_sums(hipStream_t st, const double* ve, const double* dve, const double* gm, const double* mu,
                         const double* srow, const double* S, int64_t n, int64_t npad, double* out) {
  hipLaunchKernelGGL(vgp_lik_sums_kernel, dim3(1), dim3(kThreads), 0, st, ve, dve, gm, mu, srow, S, n, npad, out);
}
void launch_vgp_lbar_w(hipStream_t st, double* lsig, const double* a, const double* gm, const double* mu, int64_t n,
                       int64_t npad) {
  hipLaunchKernelGGL(vgp_lbar_w_kernel, dim3(blocks_for(npad * npad)), dim3(kThreads), 0, st, lsig, a, gm, mu, n, npad);
}
void launch_vgp_rowscale(hipStream_t st, const double* A, const double* a, double* B, int64_t n, int64_t npad) {
  hipLaunchKernelGGL(vgp_rowscale_kernel, dim3(blocks_for(npad * npad)), dim3(kThreads), 0, st, A, a, B, n, npad);
}

}  // namespace gpso
