// Monte-Carlo batch acquisition over the resident path draws (qEI / qNoisyEI / qPI as sample averages
// over fixed base samples, picked by sequential greedy selection -- Wilson et al. 2018, Balandat et al. 2020).  No counterpart
// in the reference.  Stage A is paths.hip's paths_eval_kernel, unchanged, writing the call's own S x ld value matrix V
// (draw-major: candidates in columns 0 .. m - 1, pending points from column roundup(m, 64) on).  The rounds are these kernels:
//   mc_init_kernel   one workgroup, a thread a draw: the bars as given, then the pending columns folded in, in column order
//   mc_round_kernel  a lane a row, consecutive lanes consecutive rows, so every draw's row of V is read coalesced; the bars (or
//                    thresholds and flags) staged in LDS once per workgroup; the draw loop in index order (mcbatch.hpp); then
//                    the block's first maximum by a fixed tree (batch.hpp's batch_beats: a total order, so the tree's shape
//                    does not matter) -- one (gain, row) record a block
//   mc_fold_kernel   one workgroup: merges the blocks' records, applies the end rules (mc_verdict), appends the pick's record,
//                    retires the row and applies the pick to the bars or flags, a thread a draw
// All q rounds are enqueued back to back; a round after the end reads the stop word and does nothing.  No atomics, no LDS
// beyond the staged bars and the arg-max tree; compiled with -ffp-contract=off: a device gain has the bits of
// gpso_paths_batch_host on the same V.
#include "mcbatch.hpp"

#include <vector>

#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;
static_assert(kMcMaxDraws <= kThreads, "a thread a draw in mc_init_kernel and mc_fold_kernel");

__global__ __launch_bounds__(kThreads) void mc_init_kernel(McState* st, const double* __restrict__ V, int64_t ld, int s_n, int64_t pcol,
                                                           int b, int kind, double xi) {
  const int s = threadIdx.x;
  if (s >= s_n) return;
  double bar = st->bar[s];
  const double thr = mc_threshold(bar, xi);
  int cleared = 0;
  for (int c = 0; c < b; ++c) {
    const double v = V[(int64_t)s * ld + pcol + c];
    if (kind == kMcQei) mc_apply_qei(v, xi, &bar, &cleared);
    else if (mc_clears(v, thr)) cleared = 1;
  }
  st->bar[s] = bar;
  st->thr[s] = thr;
  st->cleared[s] = cleared;
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void mc_round_kernel(const McState* __restrict__ st, const double* __restrict__ V, int64_t ld, int s_n,
                                                            int64_t m, double xi, const unsigned char* __restrict__ live,
                                                            double* __restrict__ gain0, double* __restrict__ bmax_v,
                                                            int64_t* __restrict__ bmax_i) {
  if (st->stop != 0) return;
  __shared__ double sb[kMcMaxDraws];  // the bars (QEI) or thresholds (QPI)
  __shared__ double sx[kMcMaxDraws];  // QEI: the draws' margins
  __shared__ int si[kMcMaxDraws];     // QPI: the cleared flags
  __shared__ double bv[kThreads];
  __shared__ int64_t bi[kThreads];
  const int tid = threadIdx.x;
  if (tid < s_n) {
    sb[tid] = KIND == kMcQei ? st->bar[tid] : st->thr[tid];
    if (KIND == kMcQei) sx[tid] = mc_margin(st->cleared[tid], xi);
    else si[tid] = st->cleared[tid];
  }
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * kThreads + tid;
  double v = 0.0;
  int64_t vi = -1;
  if (j < m && live[j] != 0) {
    v = KIND == kMcQei ? mc_gain_qei(V + j, ld, sb, sx, s_n) : mc_gain_qpi(V + j, ld, sb, si, s_n);
    vi = j;
    if (gain0 != nullptr) gain0[j] = v;
  }
  bv[tid] = v;
  bi[tid] = vi;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o && batch_beats(bv[tid + o], bi[tid + o], bv[tid], bi[tid])) {
      bv[tid] = bv[tid + o];
      bi[tid] = bi[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    bmax_v[blockIdx.x] = bv[0];
    bmax_i[blockIdx.x] = bi[0];
  }
}

__global__ __launch_bounds__(kThreads) void mc_fold_kernel(McState* st, int t, int kind, const double* __restrict__ bmax_v,
                                                           const int64_t* __restrict__ bmax_i, int64_t nblocks, const double* __restrict__ V,
                                                           int64_t ld, int s_n, double xi, unsigned char* __restrict__ live) {
  if (st->stop != 0) return;  // (every thread reads the word before the first barrier; thread 0 writes it behind the last)
  __shared__ double bv[kThreads];
  __shared__ int64_t bi[kThreads];
  const int tid = threadIdx.x;
  double v = 0.0;
  int64_t vi = -1;
  for (int64_t e = tid; e < nblocks; e += kThreads) {
    if (batch_beats(bmax_v[e], bmax_i[e], v, vi)) {
      v = bmax_v[e];
      vi = bmax_i[e];
    }
  }
  bv[tid] = v;
  bi[tid] = vi;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o && batch_beats(bv[tid + o], bi[tid + o], bv[tid], bi[tid])) {
      bv[tid] = bv[tid + o];
      bi[tid] = bi[tid + o];
    }
    __syncthreads();
  }
  const int64_t p = bi[0];
  const double g = bv[0];
  const int verdict = p < 0 ? 2 : mc_verdict(t, g);  // (no live row left: the batch ends with the picks it has)
  if (tid == 0) {
    if (verdict != 2) {
      st->idx[t] = p;
      st->gain[t] = g;
      st->value[t] = t == 0 ? g : st->value[t - 1] + g;
      st->n_picked = t + 1;
      live[p] = 0;
    }
    if (verdict != 0) st->stop = 1;
  }
  if (verdict != 0 || tid >= s_n) return;
  const double pv = V[(int64_t)tid * ld + p];
  if (kind == kMcQei) mc_apply_qei(pv, xi, &st->bar[tid], &st->cleared[tid]);
  else if (mc_clears(pv, st->thr[tid])) st->cleared[tid] = 1;
}

}  // namespace

int64_t mc_round_blocks(int64_t m) { return (m + kThreads - 1) / kThreads; }

int launch_mc_init(hipStream_t s, const McLaunch& g) {
  if (g.s < 1 || g.s > kMcMaxDraws || g.m < 1 || g.b < 0 || g.b > kMcMaxPending || g.ld < g.pcol + g.b || g.pcol < g.m ||
      (g.kind != kMcQei && g.kind != kMcQpi) || g.st == nullptr || g.V == nullptr) {
    note_launch_error("launch_mc_init: shape outside the kernels'");
    return -1;
  }
  hipLaunchKernelGGL(mc_init_kernel, dim3(1), dim3(kThreads), 0, s, g.st, g.V, g.ld, g.s, g.pcol, g.b, g.kind, g.xi);
  return 0;
}

void launch_mc_round(hipStream_t s, const McLaunch& g, int t, double* gain0) {
  const dim3 grid((unsigned)mc_round_blocks(g.m));
  auto* fn = g.kind == kMcQei ? mc_round_kernel<kMcQei> : mc_round_kernel<kMcQpi>;
  hipLaunchKernelGGL(fn, grid, dim3(kThreads), 0, s, g.st, g.V, g.ld, g.s, g.m, g.xi, g.live, t == 0 ? gain0 : nullptr, g.bmax_v, g.bmax_i);
  hipLaunchKernelGGL(mc_fold_kernel, dim3(1), dim3(kThreads), 0, s, g.st, t, g.kind, g.bmax_v, g.bmax_i, mc_round_blocks(g.m), g.V, g.ld,
                     g.s, g.xi, g.live);
}

// ---- the same rounds on the host, from a given V (gpso_paths_batch_host) -------------------------------------------------------
int mc_batch_host(int kind, double xi, const double* V, int64_t ld, int s_n, int64_t m, int b, const double* bar0, int q, int64_t* idx,
                  double* gain, double* batch_value, int* n_picked, double* gain0) {
  std::vector<double> bar(bar0, bar0 + s_n), thr((size_t)s_n), x((size_t)s_n);
  std::vector<int> cleared((size_t)s_n, 0);
  for (int s = 0; s < s_n; ++s) {
    thr[s] = mc_threshold(bar[s], xi);
    for (int c = 0; c < b; ++c) {
      const double v = V[(int64_t)s * ld + m + c];
      if (kind == kMcQei) mc_apply_qei(v, xi, &bar[s], &cleared[s]);
      else if (mc_clears(v, thr[s])) cleared[s] = 1;
    }
  }
  std::vector<unsigned char> live((size_t)m, 1);
  int np = 0;
  double total = 0.0;
  for (int t = 0; t < q; ++t) {
    double bv = 0.0;
    int64_t p = -1;
    for (int s = 0; s < s_n; ++s) x[s] = mc_margin(cleared[s], xi);
    for (int64_t j = 0; j < m; ++j) {
      if (!live[j]) continue;
      const double v = kind == kMcQei ? mc_gain_qei(V + j, ld, bar.data(), x.data(), s_n) : mc_gain_qpi(V + j, ld, thr.data(), cleared.data(), s_n);
      if (t == 0 && gain0) gain0[j] = v;
      if (batch_beats(v, j, bv, p)) {
        bv = v;
        p = j;
      }
    }
    const int verdict = p < 0 ? 2 : mc_verdict(t, bv);
    if (verdict == 2) break;
    idx[t] = p;
    total = t == 0 ? bv : total + bv;
    if (gain) gain[t] = bv;
    if (batch_value) batch_value[t] = total;
    np = t + 1;
    live[p] = 0;
    if (verdict != 0) break;
    for (int s = 0; s < s_n; ++s) {
      const double pv = V[(int64_t)s * ld + p];
      if (kind == kMcQei) mc_apply_qei(pv, xi, &bar[s], &cleared[s]);
      else if (mc_clears(pv, thr[s])) cleared[s] = 1;
    }
  }
  *n_picked = np;
  return 0;
}

}  // namespace gpso
