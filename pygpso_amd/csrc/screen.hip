// Screened best-UCB calls (screen.hpp): the mean pass, the screen and the ordered compaction.
//
//   leaf_mean_kernel     every leaf's share of k*.alpha per row block of L^-1 -- part_mean[bi][col], the bits the split tile
//                        kernel (leaf_split.hpp: leaf_tiles_bf16_kernel, fp16 split with the fp16 contraction) writes there --
//                        from the generation of the row blocks' diagonal k-steps alone: no L^-1 panel, no apply, no accumulators
//   screen_mean_kernel   my = sum of the shares + mean_c (finalize_leaf's sums), and every block's largest finite my
//   screen_compact_kernel  T', the survive flags, and the survivors' indices (ascending) and raw rows into compact buffers
//
// Built with the split kernels' flags (Makefile: EXTRA_screen): the per-leaf arithmetic is the tile kernel's, instruction for
// instruction.
#include <hip/hip_runtime.h>

#include "leaf_split.hpp"
#include "screen.hpp"

namespace gpso {

// The tile kernel's mean, without the tile kernel.  What it repeats of leaf_tiles_bf16_kernel<2, float, KERNEL, F16, FUSED, C16>,
// operation for operation: the leaf prologue (fp16 pieces of the scaled leaves, their norm; the raw-leaf scaling path), the
// row blocks a workgroup owns (the same zig-zag over gridDim.y), and per row block the generation of its diagonal k-steps
// q_diag0 .. min(q_lim, q_end - 1) -- the steps the fused kernel generates with GMODE 2 / DIAG -- through leaf_bf16_gen<DIAG = true>:
// the same contraction, map, macc order; then the epilogue's shuffles, conversion and un-scaling.
// (The prologue is DUPLICATED from the tile kernel, not shared with it: factored out, the default tile kernel would have to
// keep its 239 VGPRs and its bits through a different inlining -- the copy costs nothing there.  Keep the two in step.)
// The inputs of a k-step (the X fragments' fp16 pieces and 32 alphas) travel global -> registers -> LDS one step ahead of
// their use, two buffers, one workgroup barrier per step.
template <int KERNEL, int C16, int XP>
__global__ __launch_bounds__(512) void leaf_mean_kernel(const unsigned char* __restrict__ xs_h16, const float* __restrict__ alpha,
                                                        const float* __restrict__ leaves_s, double* __restrict__ part_mean,
                                                        int dp4, int64_t mpad, int nbi, float variance, float inv_scale_b,
                                                        const float* __restrict__ c16_scale, int q_max,
                                                        const float* __restrict__ raw, const double* __restrict__ raw_ls,
                                                        int64_t raw_m, int raw_d) {
  using TG = float;
  constexpr int RT = 16, CT = 2, NW = 8, NS = 2;
  constexpr TG SC = (TG)GenScale<KERNEL>::SC;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int S = (int)gridDim.y, split = (int)blockIdx.y;
  const int64_t leaf_tile = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int xstride = Bf16Lds<TG, C16>::xbytes(dp4);
  const int xfrag = Bf16Lds<TG, C16>::xfrag(dp4);
  unsigned char* xsl = lds_raw;  // [2] X buffers: fragments | 64 TG (unused: the norms ride in the contraction) | alphas
  TG* xb = reinterpret_cast<TG*>(xsl + 2 * xstride + (size_t)wave * xfrag);
  const int64_t col0 = (leaf_tile * NW + wave) * (CT * 16);
  const int dp = dp4 * 4;

  // ---- leaf prologue (leaf_tiles_bf16_kernel, C16) ----------------------------------------------------------------------
  TG cm = TG(-2) * SC;
  float nb_c16[CT] = {0, 0};
  {
    const float up = c16_scale[1];
    cm *= (TG)c16_scale[2];
    constexpr int nc = C16;
    u32x4* xb16 = reinterpret_cast<u32x4*>(xb);
    for (int t = 0; t < CT; ++t) {
      float nrm2 = 0.0f;
      for (int cc = 0; cc < nc; ++cc) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = 32 * cc + 8 * (lane >> 4) + j;
          float xv;
          if (raw != nullptr) {  // (workgroup-uniform) the arithmetic of prep_leaves_kernel<float, float>, bit for bit
            const int64_t jrow = col0 + t * 16 + (lane & 15);
            const int kk = k < dp ? k : 0;
            xv = (jrow < raw_m && kk < raw_d) ? (float)((double)raw[jrow * raw_d + kk] / raw_ls[kk]) : 0.0f;
            xv *= up;
          } else {
            xv = (float)leaves_s[(col0 + t * 16 + (lane & 15)) * dp + (k < dp ? k : 0)] * up;
          }
          v[j] = k < dp ? (xv != xv ? xv : fminf(fmaxf(xv, -60000.0f), 60000.0f)) : (k == dp ? 128.0f : 0.0f);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float h0 = (float)(_Float16)v[j];
          const float vp = h0 + (float)(_Float16)(v[j] - h0);
          if (32 * cc + 8 * (lane >> 4) + j < dp) nrm2 += vp * vp;
        }
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
          u32x4 f;
#pragma unroll
          for (int h = 0; h < 4; ++h) f[h] = f16_split_pair(v[2 * h], v[2 * h + 1]);
          xb16[((t * nc + cc) * 2 + pc) * 64 + lane] = f;
        }
      }
      nrm2 += __shfl_xor(nrm2, 16);
      nrm2 += __shfl_xor(nrm2, 32);
      nb_c16[t] = nrm2 * c16_scale[2];
    }
  }
  TG nb[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) nb[t] = (TG)nb_c16[t] * SC;
  float vc[3];
  gen_poly_coeffs<KERNEL>(variance, vc);
  const double unscale_m = (double)inv_scale_b;

  // ---- the k-steps of this workgroup, row block after row block, as one sequence -------------------------------------------
  auto rank_of = [&](int j) { return j * S + ((j & 1) ? S - 1 - split : split); };
  int rbj = 0, bi = 0, q = 0, q_last = -1;
  auto set_row_block = [&](int j_mine) {  // false: no such row block
    const int rank = rank_of(j_mine);
    if (rank >= nbi) return false;
    bi = nbi - 1 - rank;
    const int q_diag0 = bi * (RT / 2), q_end = q_diag0 + RT / 2;
    const int q_lim = min(q_end, q_max);  // (the fused step's: the k-steps from q_max on hold padding points only)
    q = q_diag0;
    q_last = min(q_lim, q_end - 1);
    return true;
  };
  // this thread's share of a step's inputs: one 16-byte word of the fragments (xfrag / 16 <= 512 of them), one alpha
  const bool has_x = tid * 16 < xfrag, has_a = tid < 32;
  u32x4 rx = {0, 0, 0, 0};
  float ra = 0.0f;
  auto fetch = [&](int qq) {
    if (has_x) rx = *reinterpret_cast<const u32x4*>(xs_h16 + (size_t)qq * xfrag + tid * 16);
    if (has_a) ra = alpha[32 * qq + tid];
  };
  auto stash = [&](int buf) {
    unsigned char* xd = xsl + buf * xstride;
    if (has_x) *reinterpret_cast<u32x4*>(xd + tid * 16) = rx;
    if (has_a) *reinterpret_cast<float*>(xd + xfrag + 64 * sizeof(TG) + tid * 4) = ra;
  };
  if (!set_row_block(0)) return;  // (gridDim.y <= nbi: every workgroup owns a row block)
  fetch(q);
  float macc[CT] = {0.0f, 0.0f};
  for (int it = 0;; ++it) {
    const int buf = it & 1;
    stash(buf);  // (buffer `buf` was last read two steps ago: every wave has passed the barrier of the step in between)
    // the step after this one: the next diagonal step of the row block, or the first of the workgroup's next row block
    const int bi_now = bi, q_now = q;
    const bool block_ends = q_now == q_last;
    bool more = true;
    if (block_ends) more = set_row_block(++rbj);
    else ++q;
    if (more) fetch(q);
    __syncthreads();
    bf16x8 bfrag[NS][CT];  // (the pieces of the split are not used: dead code here)
    leaf_bf16_gen<NS, TG, KERNEL, true, true, C16, CT, XP>(lane, dp4, xsl + buf * xstride, xb, nb, cm, vc, bfrag, macc);
    (void)q_now;
    if (block_ends) {  // the tile kernel's epilogue, the mean's half
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        double mm = (double)macc[t];
        mm += __shfl_xor(mm, 16);
        mm += __shfl_xor(mm, 32);
        mm *= unscale_m;
        if (lane < 16) part_mean[(int64_t)bi_now * mpad + col0 + t * 16 + lane] = mm;
        macc[t] = 0.0f;
      }
    }
    if (!more) break;  // (workgroup-uniform)
  }
}

int launch_leaf_mean(hipStream_t st, const KernParams& kp, const LeafMeanLaunch& a) {
  const int dp4 = a.dp4;
  const int c16 = leaf_c16_chunks(dp4);
  if (c16 < 1 || c16 > 2 || a.npad % 256 != 0 || a.mpad % 256 != 0) {
    note_launch_error("launch_leaf_mean: the fp16 contraction has one or two chunks, N_pad and M_pad are multiples of 256");
    return 1;
  }
  const int nbi = (int)(a.npad / 256);
  // the scales of the fp16 split, as launch_leaf_tiles_bf16_ns forms them
  int eb = 0;
  (void)frexp(kp.variance, &eb);
  const float var_arg = (float)ldexp(kp.variance, 14 - eb);
  const float inv_b = (float)ldexp(1.0, eb - 14);
  const int q_max = a.n_rows > 0 ? (int)((a.n_rows + 31) / 32) : (int)(a.npad / 32);
  const int S = leaf_row_splits(a.row_loop, a.mpad / 256, nbi, a.cu_count, true);
  if (a.splits_out != nullptr) *a.splits_out = S;
  const dim3 grid((unsigned)(a.mpad / 256), (unsigned)S);
  const bool xp = dp4 * 4 + 1 - 32 * (c16 - 1) <= 16;
  const size_t xfrag = (size_t)c16 * 4096;
  const size_t lds = 2 * (xfrag + 64 * 4 + 256) + 8 * xfrag;
#define GPSO_M(K, C, X)                                                                                                   \
  do {                                                                                                                    \
    const int rc = ensure_dyn_lds((const void*)leaf_mean_kernel<K, C, X>, (int)lds);                                      \
    if (rc) return rc;                                                                                                    \
    hipLaunchKernelGGL((leaf_mean_kernel<K, C, X>), grid, dim3(512), lds, st, static_cast<const unsigned char*>(a.xs_h16), \
                       a.alpha, a.leaves_s, a.part_mean, dp4, a.mpad, nbi, var_arg, inv_b, a.c16_scale, q_max, a.raw.x,   \
                       a.raw.ls, a.raw.m, a.raw.d);                                                                       \
  } while (0)
#define GPSO_MK(K)                       \
  do {                                   \
    if (c16 == 1) {                      \
      if (xp) GPSO_M(K, 1, 1);           \
      else GPSO_M(K, 1, 0);              \
    } else {                             \
      if (xp) GPSO_M(K, 2, 1);           \
      else GPSO_M(K, 2, 0);              \
    }                                    \
  } while (0)
  switch (kp.kernel) {
    case 0: GPSO_MK(0); break;
    case 1: GPSO_MK(1); break;
    case 2: GPSO_MK(2); break;
    default: GPSO_MK(3); break;
  }
#undef GPSO_MK
#undef GPSO_M
  return 0;
}

// my of every leaf (finalize_leaf's sums: the shares from 0 upwards in row-block order, then + mean_c) and, per block of 256
// leaves, the largest finite one (-inf: none)
__global__ __launch_bounds__(256) void screen_mean_kernel(const double* __restrict__ part_mean, int nbi, int64_t mpad, int64_t m,
                                                          double mean_c, double* __restrict__ my_out,
                                                          double* __restrict__ block_max) {
  __shared__ double sh[4];
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double best = -HUGE_VAL;
  if (j < m) {
    double mu = 0;
    for (int b = 0; b < nbi; ++b) mu += part_mean[(int64_t)b * mpad + j];
    const double my = __dadd_rn(mu, mean_c);
    my_out[j] = my;
    if (screen_finite(my)) best = my;
  }
  for (int off = 32; off > 0; off >>= 1) best = fmax(best, __shfl_xor(best, off));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) block_max[blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// One workgroup of 16 waves.  Wave w owns the leaves [w seg, (w + 1) seg), seg a multiple of 64, and walks them 64 at a
// time (coalesced): a first pass counts its survivors, the waves' counts are scanned, a second pass writes every survivor's
// index at its rank -- ascending -- and its raw row, as long as the rank is below cap.  ctl: [0] live rows of the compact
// buffers (min(count, cap)), [1] the survivors' count, [2] T' (bit-cast double).
// probe (nullable, [2][m]): ub and the flag of every leaf, for gpso_screen_probe.
__global__ __launch_bounds__(1024) void screen_compact_kernel(const double* __restrict__ my, const double* __restrict__ block_max,
                                                              int nblk, int64_t m, double variance, double noise, double varsigma,
                                                              const float* __restrict__ raw, int d, int64_t cap,
                                                              int64_t* __restrict__ key, float* __restrict__ rows_out,
                                                              int64_t* __restrict__ ctl, double* __restrict__ probe) {
  __shared__ double shm[16];
  __shared__ int64_t shc[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double best = -HUGE_VAL;
  for (int b = tid; b < nblk; b += blockDim.x) best = fmax(best, block_max[b]);
  for (int off = 32; off > 0; off >>= 1) best = fmax(best, __shfl_xor(best, off));
  if (lane == 0) shm[wave] = best;
  __syncthreads();
  best = shm[0];
  for (int w = 1; w < 16; ++w) best = fmax(best, shm[w]);
  const double T = screen_threshold(best, noise, varsigma);
  const int64_t seg = ((m + 16 * 64 - 1) / (16 * 64)) * 64;
  const int64_t lo = wave * seg, hi = lo + seg < m ? lo + seg : m;
  // (one leaf per lane and load, kUnroll loads in flight per wave: the walk is a chain of global-memory latencies otherwise,
  // 128 of them per wave at C3)
  constexpr int kUnroll = 8;
  int64_t mine = 0;
  for (int64_t j0 = lo; j0 < hi; j0 += 64 * kUnroll) {
    double y[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t j = j0 + 64 * u + lane;
      y[u] = j < hi ? my[j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t j = j0 + 64 * u + lane;
      const bool f = j < hi && screen_survives(y[u], screen_bound(y[u], variance, noise, varsigma), T);
      mine += __popcll(__ballot(f));
    }
  }
  if (lane == 0) shc[wave] = mine;
  __syncthreads();
  int64_t at = 0, total = 0;
  for (int w = 0; w < 16; ++w) {
    if (w < wave) at += shc[w];
    total += shc[w];
  }
  for (int64_t j0 = lo; j0 < hi; j0 += 64 * kUnroll) {
    double y[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t j = j0 + 64 * u + lane;
      y[u] = j < hi ? my[j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {  // (in order: the ranks ascend with the index)
      const int64_t j = j0 + 64 * u + lane;
      const double ub = screen_bound(y[u], variance, noise, varsigma);
      const bool f = j < hi && screen_survives(y[u], ub, T);
      const unsigned long long mask = __ballot(f);
      if (probe != nullptr && j < hi) {
        probe[j] = ub;
        probe[m + j] = f ? 1.0 : 0.0;
      }
      if (f) {
        const int64_t pos = at + __popcll(mask & ((1ull << lane) - 1ull));
        if (pos < cap) key[pos] = j;
      }
      at += __popcll(mask);
    }
  }
  // the survivors' raw rows, by the whole workgroup at once (copied by the lane that found the survivor, a row's d dependent
  // loads stood in the walk of its wave: 92 us of kernel at C3's 535 survivors)
  __threadfence_block();
  __syncthreads();
  const int64_t live = total < cap ? total : cap;
  for (int64_t e = tid; e < live * d; e += blockDim.x) {
    const int64_t row = e / d;
    rows_out[e] = raw[key[row] * d + (e - row * d)];
  }
  if (tid == 0) {
    ctl[0] = total < cap ? total : cap;
    ctl[1] = total;
    ctl[2] = __builtin_bit_cast(int64_t, T);
  }
}

void launch_screen(hipStream_t st, const ScreenLaunch& a) {
  const int nblk = (int)((a.m + 255) / 256);
  hipLaunchKernelGGL(screen_mean_kernel, dim3(nblk), dim3(256), 0, st, a.part_mean, a.nbi, a.mpad, a.m, a.mean_c, a.my, a.block_max);
  hipLaunchKernelGGL(screen_compact_kernel, dim3(1), dim3(1024), 0, st, a.my, a.block_max, nblk, a.m, a.variance, a.noise,
                     a.varsigma, a.raw, a.d, a.cap, a.key, a.rows_out, a.ctl, a.probe);
}

void screen_eval_host(const double* my, const double* v, double variance, double noise, double varsigma, long long n,
                      double* ucb, double* ub) {
  for (long long i = 0; i < n; ++i) {
    if (ucb) ucb[i] = screen_ucb(my[i], v ? v[i] : 0.0, variance, noise, varsigma);
    if (ub) ub[i] = screen_bound(my[i], variance, noise, varsigma);
  }
}
double screen_threshold_host(double max_my, double noise, double varsigma) { return screen_threshold(max_my, noise, varsigma); }
int screen_survives_host(double my, double ub, double threshold) { return screen_survives(my, ub, threshold) ? 1 : 0; }
int screen_accepts_host(double u_star, double threshold, long long count, long long cap) {
  return screen_accepts(u_star, threshold, count, cap) ? 1 : 0;
}

}  // namespace gpso
