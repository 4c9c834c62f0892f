// The constrained acquisition's kernels (constraints.hpp holds the fold and the launch records).  The
// columns they read -- the objective's and the J constraint members' (mean, var) of every leaf -- come from
// ens_members_kernel (ensemble.hip), unchanged.
//
// con_fold_kernel: one thread per leaf, constrained_fold_leaf (constraints.hpp) over the J members in index order; the
// members' noise variances are read once per thread from their hyper blocks, thresholds and senses ride in the launch record.
// Column reads and the two stores are coalesced (lane j reads col[i * ld + j]); nothing is shared between threads, so there
// are no atomics and a leaf's bits depend neither on its slot nor on the batch.
// With a success member (section 7s) the fold is success.hip's con_success_fold_kernel: a translation unit of its own, so that
// this one compiles to what it was.
// con_gather_kernel: one thread per segment picks the winner's logpof by the index launch_seg_argmax left.
// Compiled with -ffp-contract=off; every fused multiply-add is written out.
#include "constraints.hpp"
#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void con_fold_kernel(ConFoldLaunch g) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= g.m) return;
  double noise[kConstraintsMax];
  for (int i = 0; i < g.nj; ++i) noise[i] = g.chyper[(int64_t)i * g.hyper_stride + 5];
  double value, logpof;
  constrained_fold_leaf(g.acq, g.con, g.obj_mean[j], g.obj_var[j], g.obj_hyper[5], g.cmean, g.cvar, noise, g.thr, g.sense, g.nj, g.ld, j,
                        &value, &logpof);
  g.value[j] = value;
  g.logpof[j] = logpof;
}

__global__ __launch_bounds__(kThreads) void con_gather_kernel(const double* __restrict__ logpof, const int64_t* __restrict__ seg_off,
                                                              const double* __restrict__ rec, int nseg, double* __restrict__ out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= nseg) return;
  const int64_t idx = __builtin_bit_cast(int64_t, rec[(int64_t)i * 4 + 3]);
  const int64_t len = seg_off[i + 1] - seg_off[i];
  out[i] = (idx >= 0 && idx < len) ? logpof[seg_off[i] + idx] : __builtin_nan("");
}

}  // namespace

void constrained_fold_host(const AcqSpec& a, const ConSpec& c, const double* mean, const double* var, double noise, const double* cmean,
                           const double* cvar, const double* cnoise, const double* thr, const double* sense, int nj, long long m,
                           double* value, double* logpof) {
  for (long long j = 0; j < m; ++j) {
    double v, lp;
    constrained_fold_leaf(a, c, mean ? mean[j] : 0.0, var ? var[j] : 0.0, noise, cmean, cvar, cnoise, thr, sense, nj, (int64_t)m, (int64_t)j, &v,
                          &lp);
    if (value) value[j] = v;
    if (logpof) logpof[j] = lp;
  }
}

void launch_constrained_fold(hipStream_t st, const ConFoldLaunch& g) {
  if (g.smean != nullptr) return launch_constrained_success_fold(st, g);  // (success.hip: the member's term closes logpof)
  hipLaunchKernelGGL(con_fold_kernel, dim3((unsigned)((g.m + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, g);
}

void launch_constrained_gather(hipStream_t st, const double* logpof, const int64_t* seg_off_dev, const double* rec, int nseg, double* out) {
  hipLaunchKernelGGL(con_gather_kernel, dim3((unsigned)((nseg + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, logpof, seg_off_dev, rec,
                     nseg, out);
}

}  // namespace gpso
