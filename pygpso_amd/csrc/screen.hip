// Screened best-UCB calls (screen.hpp): the mean pass, the screen and the ordered compaction.
//
//   leaf_mean_kernel       every leaf's mean, the bits the split tile kernel (leaf_split.hpp: leaf_tiles_bf16_kernel, fp16 split
//                          with the fp16 contraction) and the finalize stage give it, from the generation of the row blocks'
//                          diagonal k-steps alone: no L^-1 panel, no apply, no accumulators.  A workgroup owns 128 leaves.
//                          FOLD: it walks all their row blocks, ascending, and sums the shares in f64 registers in finalize_leaf's
//                          order -> my, and the workgroup's largest finite my -> block_max.  Otherwise (a batch too small to fill
//                          the chip that way) a leaf tile's row blocks are split over gridDim.y workgroups, the shares go to
//                          part_mean[bi][col], and
//   screen_mean_kernel     sums them: my = sum of the shares + mean_c, and every block's largest finite my
//   screen_count_kernel    T', and how many leaves of every part of the batch (screen.hpp: screen_partition) survive
//   screen_scatter_kernel  every part sums the counts in front of it and writes its survivors' indices (ascending) and raw rows
//                          into the compact buffers.  No workgroup waits for another: the launch boundary is the only ordering.
//
// Built with the split kernels' flags (Makefile: EXTRA_screen): the per-leaf arithmetic is the tile kernel's, instruction for
// instruction.
#include <hip/hip_runtime.h>

#include "leaf_split.hpp"
#include "screen.hpp"

namespace gpso {

// leaves of a workgroup of the mean pass: kMeanWaves waves x kMeanCT column tiles x 16
constexpr int kMeanLeaves = 128;
constexpr int kMeanCT = 2, kMeanWaves = kMeanLeaves / (16 * kMeanCT), kMeanThreads = 64 * kMeanWaves;

// The tile kernel's mean, without the tile kernel.  What it repeats of leaf_tiles_bf16_kernel<2, float, KERNEL, F16, FUSED, C16>,
// operation for operation: the leaf prologue (fp16 pieces of the scaled leaves, their norm; the raw-leaf scaling path) and per
// row block the generation of its diagonal k-steps q_diag0 .. min(q_lim, q_end - 1) -- the steps the fused kernel generates with
// GMODE 2 / DIAG -- through leaf_bf16_gen<DIAG = true>: the same contraction, map, macc order; then the epilogue's shuffles,
// conversion and un-scaling.  A column's arithmetic depends neither on the column tiles per wave nor on the waves per workgroup.
// (The prologue is DUPLICATED from the tile kernel, not shared with it: factored out, the default tile kernel would have to
// keep its 239 VGPRs and its bits through a different inlining -- the copy costs nothing there.  Keep the two in step.)
// The inputs of a k-step (the X fragments' fp16 pieces and 32 alphas) travel global -> registers -> LDS one step ahead of
// their use, two buffers, one workgroup barrier per step.  Two or more workgroups share a CU, each with its own barrier.
template <int KERNEL, int C16, int XP, bool FOLD>
__global__ __launch_bounds__(kMeanThreads) void leaf_mean_kernel(
    const unsigned char* __restrict__ xs_h16, const float* __restrict__ alpha, const float* __restrict__ leaves_s,
    double* __restrict__ part_mean, double* __restrict__ my_out, double* __restrict__ block_max, int dp4, int64_t mpad, int64_t m,
    int nbi, float variance, float inv_scale_b, double mean_c, const float* __restrict__ c16_scale, int q_max,
    const float* __restrict__ raw, const double* __restrict__ raw_ls, int64_t raw_m, int raw_d) {
  using TG = float;
  constexpr int RT = 16, CT = kMeanCT, NW = kMeanWaves, NT = kMeanThreads, NS = 2;
  constexpr TG SC = (TG)GenScale<KERNEL>::SC;
  constexpr int xfrag = Bf16Lds<TG, C16>::xfrag(0);  // (the fp16 contraction's does not depend on D)
  constexpr int xstride = Bf16Lds<TG, C16>::xbytes(0);
  constexpr int XW = (xfrag / 16 + NT - 1) / NT;  // 16-byte words of a step's fragments per thread
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double sh_best[NW];
  const int S = (int)gridDim.y, split = (int)blockIdx.y;
  const int64_t leaf_tile = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char* xsl = lds_raw;  // [2] X buffers: fragments | 64 TG (unused: the norms ride in the contraction) | alphas
  TG* xb = reinterpret_cast<TG*>(xsl + 2 * xstride + (size_t)wave * (xfrag / 2 * CT));
  const int64_t col0 = (leaf_tile * NW + wave) * (CT * 16);
  const int dp = dp4 * 4;

  // ---- leaf prologue (leaf_tiles_bf16_kernel, C16) ----------------------------------------------------------------------
  TG cm = TG(-2) * SC;
  float nb_c16[CT];
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
  // FOLD: every row block, ascending (the order finalize_leaf sums the shares in); otherwise the tile kernel's zig-zag over
  // gridDim.y, heaviest first
  struct Cursor {
    int rbj, bi, q, q_last;
    bool ok;
  };
  auto set_row_block = [&](Cursor& c) {  // the rbj-th row block of this workgroup (ok false: there is none)
    const int rank = FOLD ? c.rbj : c.rbj * S + ((c.rbj & 1) ? S - 1 - split : split);
    c.ok = rank < nbi;
    c.bi = FOLD ? rank : nbi - 1 - rank;
    const int q_diag0 = c.bi * (RT / 2), q_end = q_diag0 + RT / 2;
    const int q_lim = min(q_end, q_max);  // (the fused step's: the k-steps from q_max on hold padding points only)
    c.q = q_diag0;
    c.q_last = min(q_lim, q_end - 1);
  };
  auto advance = [&](Cursor& c) {
    if (c.q == c.q_last) {
      ++c.rbj;
      set_row_block(c);
    } else {
      ++c.q;
    }
  };
  Cursor at{0, 0, 0, 0, false};  // the step to generate next
  set_row_block(at);
  if (!at.ok) return;  // (gridDim.y <= nbi: every workgroup owns a row block)
  Cursor ahead = at;   // the step to fetch next
  // this thread's share of a step's inputs: XW 16-byte words of the fragments, one alpha
  u32x4 rx[XW];
  float ra = 0.0f;
#pragma unroll
  for (int w = 0; w < XW; ++w) rx[w] = u32x4{0, 0, 0, 0};
  auto fetch = [&]() {  // the inputs of step `ahead`, where there is one
    if (!ahead.ok) return;
#pragma unroll
    for (int w = 0; w < XW; ++w)
      if ((tid + NT * w) * 16 < xfrag)
        rx[w] = *reinterpret_cast<const u32x4*>(xs_h16 + (size_t)ahead.q * xfrag + (size_t)(tid + NT * w) * 16);
    if (tid < 32) ra = alpha[32 * ahead.q + tid];
    advance(ahead);
  };
  auto stash = [&](int buf) {
    unsigned char* xd = xsl + buf * xstride;
#pragma unroll
    for (int w = 0; w < XW; ++w)
      if ((tid + NT * w) * 16 < xfrag) *reinterpret_cast<u32x4*>(xd + (tid + NT * w) * 16) = rx[w];
    if (tid < 32) *reinterpret_cast<float*>(xd + xfrag + 64 * sizeof(TG) + tid * 4) = ra;
  };
  fetch();
  float macc[CT];
  double mu[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) macc[t] = 0.0f, mu[t] = 0.0;
  for (int it = 0;; ++it) {
    const int buf = it & 1;
    stash(buf);  // (buffer `buf` was last read two steps ago: every wave has passed the barrier of the step in between)
    fetch();
    __syncthreads();
    bf16x8 bfrag[NS][CT];  // (the pieces of the split are not used: dead code here)
    leaf_bf16_gen<NS, TG, KERNEL, true, true, C16, CT, XP>(lane, dp4, xsl + buf * xstride, xb, nb, cm, vc, bfrag, macc);
    if (at.q == at.q_last) {  // the row block ends: the tile kernel's epilogue, the mean's half
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        double mm = (double)macc[t];
        mm += __shfl_xor(mm, 16);
        mm += __shfl_xor(mm, 32);
        mm *= unscale_m;
        if constexpr (FOLD) mu[t] += mm;  // (finalize_leaf: from 0, the row blocks ascending; built without contraction)
        else if (lane < 16) part_mean[(int64_t)at.bi * mpad + col0 + t * 16 + lane] = mm;
        macc[t] = 0.0f;
      }
    }
    advance(at);
    if (!at.ok) break;  // (workgroup-uniform)
  }
  if constexpr (FOLD) {  // the mean, and the workgroup's largest finite one over its live leaves
    double best = -HUGE_VAL;
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const int64_t col = col0 + t * 16 + (lane & 15);
      const double y = __dadd_rn(mu[t], mean_c);
      if (col < m) {
        if (lane < 16) my_out[col] = y;
        if (screen_finite(y)) best = fmax(best, y);
      }
    }
    for (int off = 32; off > 0; off >>= 1) best = fmax(best, __shfl_xor(best, off));
    if (lane == 0) sh_best[wave] = best;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < NW; ++w) best = fmax(best, sh_best[w]);
      block_max[leaf_tile] = best;
    }
  }
}

// my of every leaf (finalize_leaf's sums: the shares from 0 upwards in row-block order, then + mean_c) and, per block of 256
// leaves, the largest finite one (-inf: none): behind a mean pass whose workgroups split the row blocks
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

int launch_leaf_mean(hipStream_t st, const KernParams& kp, const LeafMeanLaunch& a) {
  const int dp4 = a.dp4;
  const int c16 = leaf_c16_chunks(dp4);
  if (c16 < 1 || c16 > 2 || a.npad % 256 != 0 || a.mpad % 256 != 0 || a.m < 1 || a.m > a.mpad) {
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
  if (a.splits_out != nullptr) *a.splits_out = leaf_row_splits(a.row_loop, a.mpad / 256, nbi, a.cu_count, true);
  // One workgroup per leaf tile and all its row blocks where that leaves two workgroups per CU or more; a smaller batch splits
  // the row blocks of a tile over as many workgroups as brings the grid there (the chain of k-steps of a workgroup shortens as
  // the chip empties), and pays the second launch.  An explicit GPSO_OPT_ROW_LOOP decides here as it does for the tile kernel:
  // -1 one workgroup per tile whatever the batch (tests: a small batch then takes the large batches' path), 0 one row block
  // per workgroup, v >= 2 min(v, row blocks) workgroups.
  const int64_t ltiles = a.mpad / kMeanLeaves;
  const int64_t want = 2 * (int64_t)std::max(a.cu_count, 1);
  int S = ltiles >= want ? 1 : (int)std::min<int64_t>(nbi, (want + ltiles - 1) / ltiles);
  if (a.row_loop < 0) S = 1;
  else if (a.row_loop == 0) S = nbi;
  else if (a.row_loop >= 2) S = std::min(a.row_loop, nbi);
  const bool fold = S == 1;
  const dim3 grid((unsigned)ltiles, (unsigned)S);
  const bool xp = dp4 * 4 + 1 - 32 * (c16 - 1) <= 16;
  const size_t xfrag = (size_t)c16 * 4096;
  const size_t lds = 2 * (xfrag + 64 * 4 + 256) + (size_t)kMeanWaves * (xfrag / 2 * kMeanCT);
#define GPSO_M(K, C, X, F)                                                                                                  \
  do {                                                                                                                      \
    const int rc = ensure_dyn_lds((const void*)leaf_mean_kernel<K, C, X, F>, (int)lds);                                     \
    if (rc) return rc;                                                                                                      \
    hipLaunchKernelGGL((leaf_mean_kernel<K, C, X, F>), grid, dim3(kMeanThreads), lds, st,                                   \
                       static_cast<const unsigned char*>(a.xs_h16), a.alpha, a.leaves_s, a.part_mean, a.my, a.block_max, dp4, \
                       a.mpad, a.m, nbi, var_arg, inv_b, a.mean_c, a.c16_scale, q_max, a.raw.x, a.raw.ls, a.raw.m, a.raw.d); \
  } while (0)
#define GPSO_MF(K, C, X)            \
  do {                              \
    if (fold) GPSO_M(K, C, X, true); \
    else GPSO_M(K, C, X, false);    \
  } while (0)
#define GPSO_MK(K)                       \
  do {                                   \
    if (c16 == 1) {                      \
      if (xp) GPSO_MF(K, 1, 1);          \
      else GPSO_MF(K, 1, 0);             \
    } else {                             \
      if (xp) GPSO_MF(K, 2, 1);          \
      else GPSO_MF(K, 2, 0);             \
    }                                    \
  } while (0)
  switch (kp.kernel) {
    case 0: GPSO_MK(0); break;
    case 1: GPSO_MK(1); break;
    case 2: GPSO_MK(2); break;
    default: GPSO_MK(3); break;
  }
#undef GPSO_MK
#undef GPSO_MF
#undef GPSO_M
  int nblk = (int)ltiles;
  if (!fold) {
    nblk = (int)((a.m + 255) / 256);
    hipLaunchKernelGGL(screen_mean_kernel, dim3(nblk), dim3(256), 0, st, a.part_mean, nbi, a.mpad, a.m, a.mean_c, a.my, a.block_max);
  }
  if (a.nblk_out != nullptr) *a.nblk_out = nblk;
  return 0;
}

// T' by one wave: the largest of the mean pass's block maxima (max is exact: any order gives the same double)
__device__ __forceinline__ double screen_wave_threshold(const double* __restrict__ block_max, int nblk, int lane, double noise,
                                                        double varsigma) {
  double best = -HUGE_VAL;
#pragma unroll 8
  for (int b = lane; b < nblk; b += 64) best = fmax(best, block_max[b]);
  for (int off = 32; off > 0; off >>= 1) best = fmax(best, __shfl_xor(best, off));
  return screen_threshold(best, noise, varsigma);
}

// (one leaf per lane and load, kScreenUnroll loads in flight per wave: a long range is a chain of global-memory latencies otherwise)
constexpr int kScreenUnroll = 8;

// One wave per part of the batch (screen_partition).  counts[w]: the survivors among the part's leaves; ctl[2]: T' (bit-cast
// double), for the scatter kernel and the call's last kernel.
__global__ __launch_bounds__(64) void screen_count_kernel(const double* __restrict__ my, const double* __restrict__ block_max,
                                                          int nblk, int64_t m, double variance, double noise, double varsigma,
                                                          int64_t* __restrict__ counts, int64_t* __restrict__ ctl) {
  const int lane = threadIdx.x, w = blockIdx.x;
  const double T = screen_wave_threshold(block_max, nblk, lane, noise, varsigma);
  const ScreenRange r = screen_partition(m, (int)gridDim.x, w);
  int64_t mine = 0;
  for (int64_t j0 = r.lo; j0 < r.hi; j0 += 64 * kScreenUnroll) {
    double y[kScreenUnroll];
#pragma unroll
    for (int u = 0; u < kScreenUnroll; ++u) {
      const int64_t j = j0 + 64 * u + lane;
      y[u] = j < r.hi ? my[j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kScreenUnroll; ++u) {
      const int64_t j = j0 + 64 * u + lane;
      const bool f = j < r.hi && screen_survives(y[u], screen_bound(y[u], variance, noise, varsigma), T);
      mine += __popcll(__ballot(f));
    }
  }
  if (lane == 0) {
    counts[w] = mine;
    if (w == 0) ctl[2] = __builtin_bit_cast(int64_t, T);
  }
}

// One wave per part again.  It sums the counts of the parts in front of its own -- the rank of its first survivor -- and all of
// them, walks its leaves 64 at a time (coalesced) and writes every survivor's index at its rank -- ascending -- as long as the
// rank is below cap; then the raw rows of its own survivors, and its share of the zero rows between the live count and the next
// multiple of 256 (the survivors' launch scales the compact rows in its prologue: a row of its last live leaf tile must hold
// numbers).  ctl: [0] live rows of the compact buffers (min(count, cap)), [1] the survivors' count; [kScreenCtlNarrow] /
// [kScreenCtlWide]: the live rows again for the launch whose tile this count takes (count <= narrow_max: the narrow one), 0 for
// the other -- which then leaves at once (screen.hpp: survivor_narrow_max).
// probe (nullable, [2][m]): ub and the flag of every leaf, for gpso_screen_probe.
__global__ __launch_bounds__(64) void screen_scatter_kernel(const double* __restrict__ my, const int64_t* __restrict__ counts,
                                                            int64_t m, double variance, double noise, double varsigma,
                                                            const float* __restrict__ raw, int d, int64_t cap,
                                                            int64_t* __restrict__ key, float* __restrict__ rows_out,
                                                            int64_t* __restrict__ ctl, double* __restrict__ probe,
                                                            int64_t narrow_max) {
  const int lane = threadIdx.x, w = blockIdx.x, parts = (int)gridDim.x;
  const double T = __builtin_bit_cast(double, ctl[2]);
  long long at = 0, total = 0;
  for (int g = lane; g < parts; g += 64) {
    const long long c = counts[g];
    total += c;
    if (g < w) at += c;
  }
  for (int off = 32; off > 0; off >>= 1) {
    at += __shfl_xor(at, off);
    total += __shfl_xor(total, off);
  }
  const int64_t first = at;
  const ScreenRange r = screen_partition(m, parts, w);
  for (int64_t j0 = r.lo; j0 < r.hi; j0 += 64 * kScreenUnroll) {
    double y[kScreenUnroll];
#pragma unroll
    for (int u = 0; u < kScreenUnroll; ++u) {
      const int64_t j = j0 + 64 * u + lane;
      y[u] = j < r.hi ? my[j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kScreenUnroll; ++u) {  // (in order: the ranks ascend with the index)
      const int64_t j = j0 + 64 * u + lane;
      const double ub = screen_bound(y[u], variance, noise, varsigma);
      const bool f = j < r.hi && screen_survives(y[u], ub, T);
      const unsigned long long mask = __ballot(f);
      if (probe != nullptr && j < r.hi) {
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
  // the raw rows of this part's survivors, by the whole wave at once (copied by the lane that found the survivor, a row's d
  // dependent loads would stand in the walk)
  __threadfence_block();
  __syncthreads();
  const int64_t p_lo = first < cap ? first : cap, p_hi = at < cap ? (int64_t)at : cap;
  for (int64_t e = lane; e < (p_hi - p_lo) * d; e += 64) {
    const int64_t row = p_lo + e / d;
    const int64_t c = e % d;
    rows_out[row * d + c] = raw[key[row] * d + c];
  }
  const int64_t live = total < cap ? (int64_t)total : cap;
  const int64_t padded = (live + 255) / 256 * 256 < cap ? (live + 255) / 256 * 256 : cap;
  for (int64_t e = live * d + (int64_t)w * 64 + lane; e < padded * d; e += (int64_t)parts * 64) rows_out[e] = 0.0f;
  if (w == 0 && lane == 0) {
    ctl[0] = live;
    ctl[1] = total;
    ctl[kScreenCtlNarrow] = total <= narrow_max ? live : 0;
    ctl[kScreenCtlWide] = total <= narrow_max ? 0 : live;
  }
}

void launch_screen(hipStream_t st, const ScreenLaunch& a) {
  const int parts = screen_parts(a.m);
  hipLaunchKernelGGL(screen_count_kernel, dim3(parts), dim3(64), 0, st, a.my, a.block_max, a.nblk, a.m, a.variance, a.noise,
                     a.varsigma, a.counts, a.ctl);
  hipLaunchKernelGGL(screen_scatter_kernel, dim3(parts), dim3(64), 0, st, a.my, a.counts, a.m, a.variance, a.noise, a.varsigma,
                     a.raw, a.d, a.cap, a.key, a.rows_out, a.ctl, a.probe, a.narrow_max);
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
void screen_partition_host(long long m, int parts, int w, long long* lo, long long* hi) {
  const ScreenRange r = screen_partition(m, parts, w);
  *lo = r.lo;
  *hi = r.hi;
}
int screen_parts_host(long long m) { return screen_parts(m); }

}  // namespace gpso
