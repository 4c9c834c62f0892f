// Bi-objective search (ehvi.hpp holds the maths, the fixed order of the sum and the launch record).
//
// ehvi_fold_kernel: a wave per leaf (four leaves a block).  The leaf's four column entries -- the objective's and objective
// 2's (mean, var) -- are loaded at a wave-uniform address.  Lane k <= P evaluates strip k's two expectations g(a_k) and e_k
// (ehvi_strip_g / ehvi_strip_e: two H evaluations a lane, the P + 1 strips of a leaf side by side where one thread per leaf
// would run them one after the other); it takes g(a_{k+1}) from lane k + 1 by a shuffle, forms its term, and six shuffle-down
// steps (w = 32 .. 1) run ehvi_tree's order: lane 0 holds the EHVI.  The lanes above P carry +0.0, as the host's slots do.
// Lane i < J - 1 computes the logpof term of the i-th member other than objective 2, the next lane the success member's; the
// terms are then added in index order from broadcasts of those lanes.  Lane 0 stores value and logpof.
// The strips ride in the launch record (1 KB of kernel arguments); lane k reads slot k of it with one vector load from the
// kernel-argument segment -- the record is never copied to private memory, and the compiler's resource report shows no
// scratch.  No LDS, no atomics; a leaf's bits depend neither on its slot nor on the batch.
// Compiled with -ffp-contract=off; every fused multiply-add is written out.
#include "ehvi.hpp"
#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kWave = 64;
constexpr int kLeavesPerBlock = 4;
constexpr int kThreads = kWave * kLeavesPerBlock;

__global__ __launch_bounds__(kThreads) void ehvi_fold_kernel(EhviFoldLaunch g) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t j = (int64_t)blockIdx.x * kLeavesPerBlock + (threadIdx.x >> 6);  // (wave-uniform)
  if (j >= g.m) return;
  const double a = g.xa[lane], h = g.xh[lane];  // this lane's strip (lane < kEhviSlots = 64)
  const double* m2 = g.cmean + (int64_t)g.member * g.ld;
  const double* v2 = g.cvar + (int64_t)g.member * g.ld;
  const EhviLeaf l = ehvi_leaf(g.latent, g.obj_mean[j], g.obj_var[j], g.obj_hyper[5], m2[j], v2[j], g.chyper[(int64_t)g.member * g.hyper_stride + 5]);
  double ehvi = l.early;
  if (!l.decided) {  // (wave-uniform: every lane of the wave holds the same leaf)
    const bool live = lane <= g.p;
    const double gk = live ? ehvi_strip_g(l, a) : 0.0;
    const double ek = live ? ehvi_strip_e(l, h) : 0.0;
    double gn = __shfl_down(gk, 1, kWave);
    gn = lane < g.p ? gn : 0.0;  // g(+inf) = 0 behind the last strip
    double term = live ? ehvi_strip_term(gk, gn, ek) : 0.0;
#pragma unroll
    for (int w = kWave / 2; w >= 1; w >>= 1) term += __shfl_down(term, w, kWave);
    ehvi = term;  // (lane 0's is the tree's slot 0)
  }
  // logpof: lane i's term, then the sum in index order
  const int nterm = g.nother + (g.smean != nullptr ? 1 : 0);
  double t = 0.0;
  if (lane < g.nother) {
    const int idx = g.oidx[lane];  // (lane < nother <= kConstraintsMax - 1)
    const double thr = g.othr[lane], sense = g.osense[lane];
    t = con_log_pof_term(g.cmean[(int64_t)idx * g.ld + j], g.cvar[(int64_t)idx * g.ld + j], g.chyper[(int64_t)idx * g.hyper_stride + 5], thr, sense);
  } else if (lane == g.nother && g.smean != nullptr) {
    t = success_log_prob(g.smean[j], g.svar[j]);
  }
  double lp = 0.0;
  if (nterm > 0) {
    lp = __shfl(t, 0, kWave);
    for (int i = 1; i < nterm; ++i) lp += __shfl(t, i, kWave);
  }
  if (lane == 0) {
    g.value[j] = ehvi_value_leaf(g.has_con != 0, g.con, ehvi, lp);
    g.logpof[j] = lp;
  }
}

}  // namespace

void ehvi_fold_host(int latent, int p, const double* xa, const double* xh, bool has_con, const ConSpec& c, const double* mean1,
                    const double* var1, double noise1, const double* mean2, const double* var2, double noise2, const double* omean,
                    const double* ovar, const double* onoise, const double* thr, const double* sense, int k, long long m,
                    const double* smean, const double* svar, double* value, double* logpof) {
  for (long long j = 0; j < m; ++j) {
    const EhviLeaf l = ehvi_leaf(latent, mean1[j], var1[j], noise1, mean2[j], var2[j], noise2);
    const double ehvi = ehvi_leaf_serial(l, p, xa, xh);
    double lp = 0.0;
    if (k > 0) {
      lp = con_log_pof_term(omean[j], ovar[j], onoise[0], thr[0], sense[0]);
      for (int i = 1; i < k; ++i) lp += con_log_pof_term(omean[(long long)i * m + j], ovar[(long long)i * m + j], onoise[i], thr[i], sense[i]);
    }
    if (smean != nullptr) {
      const double ls = success_log_prob(smean[j], svar[j]);
      lp = k > 0 ? lp + ls : ls;
    }
    if (value) value[j] = ehvi_value_leaf(has_con, c, ehvi, lp);
    if (logpof) logpof[j] = lp;
  }
}

void launch_ehvi_fold(hipStream_t st, const EhviFoldLaunch& g) {
  hipLaunchKernelGGL(ehvi_fold_kernel, dim3((unsigned)((g.m + kLeavesPerBlock - 1) / kLeavesPerBlock)), dim3(kThreads), 0, st, g);
}

}  // namespace gpso
