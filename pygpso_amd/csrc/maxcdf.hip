// The law of the maximum over M leaves taken as independent, at g thresholds (gpso_max_logcdf):
//   logcdf[i] = sum_j log Phi((y_i - mean_j) / s_j),   s_j = sqrt(max(var_j - var_sub, 0)),
// rows with a NaN skipped.  log Phi is acq.hpp's (acq_log_ncdf: the pieces of acq_h, a tail form below -10).
//
// One pass over the leaves.  A workgroup of four waves owns kMaxCdfLeaves consecutive leaves, a thread two of them, held
// in registers (mean, s^2, s) for the whole kernel; the thresholds sit in LDS.  The thresholds are then walked in order: a
// thread adds its two terms, the wave folds the 64 sums with __shfl_xor in a fixed butterfly, lane 0 parks the wave's sum in
// LDS, and thread i adds the four waves' sums of threshold i in wave order -- one partial per workgroup and threshold.  The
// g sums of a thread therefore pass through ONE register after each other instead of lying in 64 pairs side by side: the
// term is some hundred instructions, unrolling it 64 times to keep the sums apart would leave the instruction cache, and a
// runtime-indexed array of sums would live in scratch.  A second launch of one workgroup adds the workgroups' partials in
// index order.  No atomics; the grid depends on m alone; the same call gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "acq.hpp"
#include "kernels.hpp"

namespace gpso {

namespace {

// one row's term at threshold y; the row is valid (no NaN), s2 clamped, s = sqrt(s2)
GPSO_ACQ_HD inline double max_logcdf_term(double y, double mean, double s2, double s) {
  const double d = y - mean;
  if (s == 0.0) return d > 0.0 ? 0.0 : d < 0.0 ? -__builtin_inf() : -0.6931471805599453;
  double z, zl;
  acq_z_diff(y, mean, s2, s, &z, &zl);
  return acq_log_ncdf(z, zl);
}

constexpr int kThreads = 256, kPerThread = kMaxCdfLeaves / kThreads;
static_assert(kPerThread * kThreads == kMaxCdfLeaves, "a thread owns a whole number of leaves");

__global__ __launch_bounds__(kThreads) void max_logcdf_stage1(const double* __restrict__ mean, const double* __restrict__ var,
                                                              int64_t m, double var_sub, const double* __restrict__ y, int g,
                                                              double* __restrict__ partial /* [gridDim.x][kMaxCdfSlots] */) {
  __shared__ double sh_y[kMaxCdfThresholds];
  __shared__ double sh_w[kThreads / 64][kMaxCdfSlots];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < g) sh_y[tid] = y[tid];
  double mu[kPerThread], s2[kPerThread], s[kPerThread];
  bool ok[kPerThread];
  double cnt = 0.0;
#pragma unroll
  for (int l = 0; l < kPerThread; ++l) {
    const int64_t j = (int64_t)blockIdx.x * kMaxCdfLeaves + l * kThreads + tid;
    mu[l] = 0.0;
    s2[l] = 1.0;
    ok[l] = false;
    if (j < m) {
      const double a = mean[j], v = var[j] - var_sub;
      ok[l] = a == a && v == v;
      mu[l] = a;
      s2[l] = v < 0.0 ? 0.0 : v;
    }
    if (!ok[l]) {
      mu[l] = 0.0;
      s2[l] = 1.0;
    }
    s[l] = sqrt(s2[l]);
    cnt += ok[l] ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int i = 0; i <= g; ++i) {  // (slot g: the rows counted)
    double acc = 0.0;
    if (i < g) {
      const double yi = sh_y[i];
#pragma unroll
      for (int l = 0; l < kPerThread; ++l)
        if (ok[l]) acc += max_logcdf_term(yi, mu[l], s2[l], s[l]);
    } else {
      acc = cnt;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) sh_w[wave][i] = acc;
  }
  __syncthreads();
  if (tid <= g) {
    double t = sh_w[0][tid];
    for (int w = 1; w < kThreads / 64; ++w) t += sh_w[w][tid];
    partial[(int64_t)blockIdx.x * kMaxCdfSlots + tid] = t;
  }
}

// one workgroup: thread i adds slot i of every workgroup's partial, in index order -- nblk = m / 512 dependent additions:
// 128 at the 65 536 leaves of a call today, 2 * 10^5 at m = 10^8, where folding in fixed chunks first would be the next step
__global__ __launch_bounds__(128) void max_logcdf_stage2(const double* __restrict__ partial, int nblk, int g,
                                                         double* __restrict__ out /* [g + 1] */) {
  const int i = threadIdx.x;
  if (i > g) return;
  double t = 0.0;
  for (int b = 0; b < nblk; ++b) t += partial[(int64_t)b * kMaxCdfSlots + i];
  out[i] = t;
}

}  // namespace

void launch_max_logcdf(hipStream_t st, const double* mean, const double* var, int64_t m, double var_sub, const double* y_dev, int g,
                       double* partial, double* out) {
  const int nblk = (int)max_logcdf_blocks(m);
  hipLaunchKernelGGL(max_logcdf_stage1, dim3((unsigned)nblk), dim3(kThreads), 0, st, mean, var, m, var_sub, y_dev, g, partial);
  hipLaunchKernelGGL(max_logcdf_stage2, dim3(1), dim3(128), 0, st, partial, nblk, g, out);
}

void max_logcdf_host(const double* mean, const double* var, long long m, double var_sub, const double* y, int g, double* logcdf,
                     long long* n_used) {
  long long used = 0;
  for (int i = 0; i < g; ++i) logcdf[i] = 0.0;
  for (long long j = 0; j < m; ++j) {
    const double a = mean[j], v = var[j] - var_sub;
    if (a != a || v != v) continue;
    ++used;
    const double s2 = v < 0.0 ? 0.0 : v, s = sqrt(s2);
    for (int i = 0; i < g; ++i) logcdf[i] += max_logcdf_term(y[i], a, s2, s);
  }
  if (n_used != nullptr) *n_used = used;
}

}  // namespace gpso
