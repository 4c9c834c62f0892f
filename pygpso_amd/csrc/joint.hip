// Joint predictive at M <= kPredictGradChunk test points.  The reference's counterpart is GPflow's
// predict_f(Xnew, full_cov=True) / predict_f_samples.  For a resident predictive (C, alpha, c, variance) over the scaled
// rows xs = x / l and the scaled test points t_1 .. t_M:
//     V = C K*  (N x M, K*[i, m] = k(xs_i, t_m)),   mu = K*^T alpha + c,   Sigma = K** - V^T V + diag_add I,
// K**[a, b] = k(t_a, t_b) from direct differences in double.  V comes from predict_grad.hip's pg_apply_kernel as it is
// (launch_predict_grad_apply), in its layout [tile of 64 test points][N_pad][64].  pg_apply writes the rows of V up to
// ceil(N / 128) * 128 and no further: the rows behind that bound hold whatever an earlier, larger problem left there, so
// every contraction here ends at that bound and never at N_pad.
//   pj_cov_kernel     (pair (a >= b) of 64-point tiles x split of the training rows): V_a^T V_b over its rows on
//                     v_mfma_f64_16x16x4_f64, both operands read straight from V (no transpose pass).  One split: the
//                     epilogue follows in the same launch; several: the partial tile goes to the workspace
//   pj_finish_kernel  (several splits only) sums a pair's partial tiles in the order of the splits, then the same epilogue
//   epilogue          K** of the tile regenerated, the product subtracted, diag_add on the diagonal; the tile AND its mirror
//                     are written from the same value (a diagonal tile: from its lower half), so Sigma is exactly symmetric;
//                     entries of padding points (index >= M) are the identity's or are not written at all
//   pj_mean_kernel    one workgroup per test point, a fixed-order sum
//   pj_draw_kernel    F = mu 1^T + Z L^T for S draws (L lower: entries above the diagonal are never read)
//   pj_argmax_kernel  per draw the highest value, the lowest index on ties
// No atomics, every reduction in a fixed order; compiled with -ffp-contract=off, every fused multiply-add written out.
#include <limits.h>

#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;       // test points per tile: pg_apply's
constexpr int kRowBlock = 128;  // pg_apply's row block: V is written up to a multiple of it
constexpr int kWantWorkgroups = 512;  // the contraction is split along N until about this many workgroups run ...
constexpr int kMaxSplits = 16;        // ... into at most this many pieces

struct PjArgs {
  const double* V;   // [mc / 64][npad][64]
  const double* ts;  // [mc * dp] scaled test points, zero rows behind the m live ones
  double* part;      // [pairs][nsplit][16 accumulator tiles][4 registers][64 lanes] (nsplit > 1)
  double* out;       // Sigma, leading dimension ldo
  int64_t npad, nend, chunk, m, ldo;
  int nsplit, dp, kernel, pad_identity;
  double variance, diag_add;
};

// pair index p = a (a + 1) / 2 + b, a >= b
__device__ __forceinline__ void pair_of(int p, int& a, int& b) {
  a = 0;
  while ((a + 1) * (a + 2) / 2 <= p) ++a;
  b = p - a * (a + 1) / 2;
}

// |t - u|^2 from direct differences, dimensions in order (predict_grad.hip's pair_r2)
__device__ __forceinline__ double pair_r2(const double* __restrict__ t, const double* __restrict__ u, int dp) {
  double r2 = 0.0;
  for (int k = 0; k < dp; k += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double df = t[k + q] - u[k + q];
      r2 = fma(df, df, r2);
    }
  }
  return r2;
}

// acc[t][r] of wave w, lane l: the product's entry (point 16 w + (l >> 4) + 4 r of tile ta, point 16 t + (l & 15) of tile tb)
__device__ __forceinline__ void pj_epilogue(const PjArgs& g, int ta, int tb, const f64x4* acc, double* tl) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dp = g.dp, ld = dp + 1;
  double* tla = tl;
  double* tlb = tl + kTile * ld;
  for (int e = tid; e < kTile * dp; e += kThreads) {
    const int c = e / dp, k = e - c * dp;
    tla[c * ld + k] = g.ts[(int64_t)ta * kTile * dp + e];
    tlb[c * ld + k] = g.ts[(int64_t)tb * kTile * dp + e];
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = 16 * wave + (lane >> 4) + 4 * r, q = 16 * t + (lane & 15);
      if (ta == tb && q > p) continue;  // (a diagonal tile: the holder of (q, p) writes this entry as its mirror)
      const int64_t gp = (int64_t)ta * kTile + p, gq = (int64_t)tb * kTile + q;
      double val;
      if (gp < g.m && gq < g.m) {
        double k, dk;
        kern_and_dkern_same(g.kernel, pair_r2(tla + p * ld, tlb + q * ld, dp), g.variance, k, dk);
        val = k - acc[t][r];
        if (gp == gq) val += g.diag_add;
      } else if (g.pad_identity) {
        val = gp == gq ? 1.0 : 0.0;
      } else {
        continue;
      }
      g.out[gp * g.ldo + gq] = val;
      g.out[gq * g.ldo + gp] = val;
    }
  }
}

__global__ __launch_bounds__(kThreads) void pj_cov_kernel(PjArgs g) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ta, tb;
  pair_of((int)blockIdx.x, ta, tb);
  const int64_t r0 = (int64_t)blockIdx.y * g.chunk;
  const int64_t r1 = r0 + g.chunk < g.nend ? r0 + g.chunk : g.nend;  // (never beyond the rows pg_apply wrote)
  const int kq = lane >> 4;
  // A operand: lane l holds V_a[row + (l >> 4)][16 wave + (l & 15)]; B operand: V_b[row + (l >> 4)][16 t + (l & 15)]
  const double* Va = g.V + (int64_t)ta * g.npad * kTile + 16 * wave + (lane & 15);
  const double* Vb = g.V + (int64_t)tb * g.npad * kTile + (lane & 15);
  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  // sixteen rows a trip, their twenty loads issued before the first product (r0, r1 are multiples of 128)
  for (int64_t i = r0; i < r1; i += 16) {
    double af[4], bf[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t ii = i + 4 * q + kq;
      af[q] = Va[ii * kTile];
#pragma unroll
      for (int t = 0; t < 4; ++t) bf[q][t] = Vb[ii * kTile + 16 * t];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[q], bf[q][t], acc[t], 0, 0, 0);
    }
  }
  if (g.nsplit == 1) {
    pj_epilogue(g, ta, tb, acc, reinterpret_cast<double*>(lds_raw));
    return;
  }
  double* dst = g.part + ((int64_t)blockIdx.x * g.nsplit + blockIdx.y) * (kTile * kTile) + (int64_t)wave * 16 * 64 + lane;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(4 * t + r) * 64] = acc[t][r];
  }
}

__global__ __launch_bounds__(kThreads) void pj_finish_kernel(PjArgs g) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ta, tb;
  pair_of((int)blockIdx.x, ta, tb);
  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < g.nsplit; ++s) {
    const double* src = g.part + ((int64_t)blockIdx.x * g.nsplit + s) * (kTile * kTile) + (int64_t)wave * 16 * 64 + lane;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] += src[(4 * t + r) * 64];
    }
  }
  pj_epilogue(g, ta, tb, acc, reinterpret_cast<double*>(lds_raw));
}

// mean[c] = sum_i alpha_i k(xs_i, t_c) + mean_c: thread u sums the rows u, u + 256, ... in their order, then a fixed tree
__global__ __launch_bounds__(kThreads) void pj_mean_kernel(const double* __restrict__ alpha, const double* __restrict__ xs,
                                                           const double* __restrict__ ts, int64_t n, int dp, int kernel,
                                                           double variance, double mean_c, double* __restrict__ mean) {
  __shared__ double tl[48];
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  if (tid < dp) tl[tid] = ts[c * dp + tid];
  __syncthreads();
  double s = 0.0;
  for (int64_t i = tid; i < n; i += kThreads) {
    double k, dk;
    kern_and_dkern_same(kernel, pair_r2(tl, xs + i * dp, dp), variance, k, dk);
    s = fma(alpha[i], k, s);
  }
  red[tid] = s;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) mean[c] = red[0] + mean_c;
}

// f[s][c] = mu[c] + sum_{j <= c} L[c][j] z[s][j]: 16 draws x 16 points a workgroup, j in steps of 16 through LDS, in order
__global__ __launch_bounds__(kThreads) void pj_draw_kernel(const double* __restrict__ L, int64_t ldl, const double* __restrict__ z,
                                                           const double* __restrict__ mu, int64_t m, int64_t s,
                                                           double* __restrict__ f) {
  __shared__ double Lt[16][17], Zt[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t s0 = (int64_t)blockIdx.x * 16, c0 = (int64_t)blockIdx.y * 16;
  double acc = 0.0;
  for (int64_t j0 = 0; j0 <= c0 + 15 && j0 < m; j0 += 16) {
    const int64_t lc = c0 + ty, j = j0 + tx, zs = s0 + ty;
    Lt[ty][tx] = (lc < m && j <= lc) ? L[lc * ldl + j] : 0.0;
    Zt[ty][tx] = (zs < s && j < m) ? z[zs * m + j] : 0.0;
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) acc = fma(Lt[tx][jj], Zt[ty][jj], acc);
    __syncthreads();
  }
  if (c0 + tx < m && s0 + ty < s) f[(s0 + ty) * m + c0 + tx] = mu[c0 + tx] + acc;
}

// per draw: the highest value and, on ties, the lowest index
__global__ __launch_bounds__(kThreads) void pj_argmax_kernel(const double* __restrict__ f, int64_t m, int64_t* __restrict__ idx,
                                                             double* __restrict__ val) {
  __shared__ double bv[kThreads];
  __shared__ int64_t bi[kThreads];
  const int tid = threadIdx.x;
  const double* row = f + (int64_t)blockIdx.x * m;
  double best = 0.0;
  int64_t at = -1;
  for (int64_t i = tid; i < m; i += kThreads) {
    const double v = row[i];
    if (at < 0 || v > best) {
      best = v;
      at = i;
    }
  }
  bv[tid] = best;
  bi[tid] = at;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      const double ov = bv[tid + off];
      const int64_t oi = bi[tid + off];
      if (oi >= 0 && (bi[tid] < 0 || ov > bv[tid] || (ov == bv[tid] && oi < bi[tid]))) {
        bv[tid] = ov;
        bi[tid] = oi;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (idx != nullptr) idx[blockIdx.x] = bi[0];
    if (val != nullptr) val[blockIdx.x] = bv[0];
  }
}

}  // namespace

int joint_splits(int64_t n, int64_t m, int64_t* chunk_rows) {
  const int64_t nrb = (n + kRowBlock - 1) / kRowBlock, tiles = (m + kTile - 1) / kTile, pairs = tiles * (tiles + 1) / 2;
  int64_t want = (kWantWorkgroups + pairs - 1) / pairs;
  if (want > kMaxSplits) want = kMaxSplits;
  const int64_t blocks = (nrb + want - 1) / want;  // row blocks of 128 per split
  if (chunk_rows != nullptr) *chunk_rows = blocks * kRowBlock;
  return (int)((nrb + blocks - 1) / blocks);
}

size_t joint_partial_doubles(int64_t n, int64_t m) {
  const int64_t tiles = (m + kTile - 1) / kTile;
  const int ns = joint_splits(n, m, nullptr);
  return ns > 1 ? (size_t)(tiles * (tiles + 1) / 2) * ns * kTile * kTile : 0;
}

int launch_joint(hipStream_t st, const JointLaunch& g) {
  const int64_t mc = (g.m + kTile - 1) / kTile * kTile;
  if (g.n < 1 || g.n > g.npad || g.npad % kRowBlock != 0 || g.dp < 4 || g.dp % 4 != 0 || g.dp > 48 || g.m < 1 ||
      g.m > kPredictGradChunk || g.ldc < (g.pad_identity ? mc : g.m)) {
    note_launch_error("launch_joint: shape outside the kernels'");
    return -1;
  }
  if (g.mean != nullptr)
    hipLaunchKernelGGL(pj_mean_kernel, dim3((unsigned)g.m), dim3(kThreads), 0, st, g.alpha, g.xs, g.ts, g.n, g.dp, g.kp.kernel,
                       g.kp.variance, g.kp.mean_c, g.mean);
  if (g.cov == nullptr) return 0;
  PjArgs a;
  a.V = g.V; a.ts = g.ts; a.part = g.part; a.out = g.cov;
  a.npad = g.npad; a.nend = (g.n + kRowBlock - 1) / kRowBlock * kRowBlock; a.m = g.m; a.ldo = g.ldc;
  a.nsplit = joint_splits(g.n, g.m, &a.chunk);
  a.dp = g.dp; a.kernel = g.kp.kernel; a.pad_identity = g.pad_identity ? 1 : 0;
  a.variance = g.kp.variance; a.diag_add = g.diag_add;
  const unsigned tiles = (unsigned)(mc / kTile), pairs = tiles * (tiles + 1) / 2;
  const int tile_bytes = 2 * kTile * (g.dp + 1) * 8;
  hipLaunchKernelGGL(pj_cov_kernel, dim3(pairs, (unsigned)a.nsplit), dim3(kThreads), a.nsplit == 1 ? tile_bytes : 0, st, a);
  if (a.nsplit > 1) hipLaunchKernelGGL(pj_finish_kernel, dim3(pairs), dim3(kThreads), tile_bytes, st, a);
  return 0;
}

void launch_joint_draw(hipStream_t st, const double* L, int64_t ldl, const double* z, const double* mu, int64_t m, int64_t s,
                       double* f) {
  hipLaunchKernelGGL(pj_draw_kernel, dim3((unsigned)((s + 15) / 16), (unsigned)((m + 15) / 16)), dim3(kThreads), 0, st, L, ldl, z,
                     mu, m, s, f);
}

void launch_joint_argmax(hipStream_t st, const double* f, int64_t m, int64_t s, int64_t* idx, double* val) {
  hipLaunchKernelGGL(pj_argmax_kernel, dim3((unsigned)s), dim3(kThreads), 0, st, f, m, idx, val);
}

}  // namespace gpso
