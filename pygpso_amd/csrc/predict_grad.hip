// Input gradients of the GP predictive.  No counterpart in the reference: a GPflow user
// differentiates predict_f / predict_y by tf.GradientTape.  For a resident predictive (C, alpha, c, variance, noise) over
// the scaled rows xs = x / l and a test point x* (scaled: t = x* / l):
//     r2_i = |t - xs_i|^2 (direct differences, double: no cancellation),  k_i = k(r2_i),  k'_i = dk/dr2 (r2_i),
//     v = C k*,  w = C^T v,  mean = alpha^T k* + c,  var = variance - |v|^2 + noise,
//     q_i = 2 k'_i (alpha_i | -2 w_i),   d(mean | var)/dx*_d = (t_d sum_i q_i - sum_i q_i xs_i,d) / l_d.
// A pair with r2 <= 1e-36 contributes zero to the gradient (exact for the squared exponential and the Matern-3/2 and
// -5/2; the convention at the Matern-1/2's kink -- gpso_sgpr_bound_uz's).  C is the dense fit-type L^-1 (row-major,
// leading dimension N_pad); entry (i, j) is read only where j <= i < N -- everything else is taken as zero, whatever an
// earlier and larger problem left there.
// Three launches per chunk of at most kPredictGradChunk test points, 64 points (four waves x 16 MFMA columns) a workgroup:
//   pg_apply_kernel  (leaf tile x block of 128 rows): v for its rows on v_mfma_f64_16x16x4_f64, the cross-Gram tile
//                    regenerated on the fly; writes v to the workspace and its partial |v|^2
//   pg_grad_kernel   (leaf tile x block of 64 columns): w = C^T v for its columns on the same instruction, then k, k' and
//                    the differences for those training rows; writes its partial alpha^T k*, sum q and sum q xs
//   pg_final_kernel  sums the partials over the blocks in their order and forms mean, var, dmean, dvar.
// No atomics, every reduction in a fixed order; the file is compiled with -ffp-contract=off and every fused
// multiply-add is written out, so a test point's bits depend neither on its column slot nor on the rest of the batch.
#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;
constexpr int kCols = 64;      // test points per workgroup: 4 waves x 16 columns
constexpr int kRowBlock = 128; // rows of C per pg_apply workgroup (8 accumulator tiles a wave)
constexpr int kColBlock = 64;  // columns of C (training rows) per pg_grad workgroup
constexpr int kStage = 16;     // columns of C staged in LDS per step of pg_apply
constexpr int kStageLd = kStage + 1;

struct PgArgs {
  const double* C;      // [npad * npad] dense fit-type factor
  const double* alpha;  // [npad]
  const double* xs;     // [npad * dp] scaled rows
  const double* ts;     // [mc * dp] scaled test points of this chunk (zero rows behind the live ones)
  double* V;            // [mc / 64][npad][64] v = C k*
  double* pv;           // [nrb][mc] partial |v|^2 per row block
  double* pq;           // [ncb][3 + 2 dp][mc]: alpha^T k*, sum q_mean, sum q_var, then (sum q_mean xs_d, sum q_var xs_d) per d
  int64_t n, npad, mc;
  int dp, kernel;
  double variance;
};

// the 64 scaled test points of leaf tile mt into LDS at an odd row stride
__device__ __forceinline__ void load_leaf_tile(const PgArgs& a, int64_t mt, double* tl) {
  const int dp = a.dp, ld = dp + 1;
  for (int e = threadIdx.x; e < kCols * dp; e += kThreads) {
    const int c = e / dp, k = e - c * dp;
    tl[c * ld + k] = a.ts[mt * kCols * dp + e];
  }
}

// |t - xs_j|^2 from direct differences, dimensions in order (both passes call this: the same bits)
__device__ __forceinline__ double pair_r2(const double* __restrict__ t /* LDS */, const double* __restrict__ xj, int dp) {
  double r2 = 0.0;
  for (int k = 0; k < dp; k += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double df = t[k + q] - xj[k + q];
      r2 = fma(df, df, r2);
    }
  }
  return r2;
}

__global__ __launch_bounds__(kThreads) void pg_apply_kernel(PgArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double* Al = reinterpret_cast<double*>(lds_raw);  // [kRowBlock][kStageLd]: the step's columns of C
  double* Xl = Al + kRowBlock * kStageLd;           // [kStage][dp + 1]: the step's scaled rows
  double* tl = Xl + kStage * (a.dp + 1);            // [kCols][dp + 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t mt = blockIdx.x, i0 = (int64_t)blockIdx.y * kRowBlock;
  const int64_t n = a.n, npad = a.npad;
  const int dp = a.dp, col = 16 * wave + (lane & 15), kq = lane >> 4;
  load_leaf_tile(a, mt, tl);
  const double* tcol = tl + col * (dp + 1);
  f64x4 acc[kRowBlock / 16];
#pragma unroll
  for (int t = 0; t < kRowBlock / 16; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int64_t jend = n < i0 + kRowBlock ? n : i0 + kRowBlock;  // columns at or beyond it meet no row of this block
  const int64_t steps = (jend + kStage - 1) / kStage;
  // thread -> row tid / 2 of the block, 8 consecutive columns of the staged 16
  const int lr = tid >> 1, lc = (tid & 1) * 8;
  const int64_t irow = i0 + lr;
  // ... and up to three of the step's kStage * dp scaled inputs (rows j0 .. j0 + 15 < N_pad: one contiguous piece)
  constexpr int kXPer = (kStage * 48 + kThreads - 1) / kThreads;
  const int xcount = kStage * dp;
  double pre[8], prex[kXPer];
  auto fetch = [&](int64_t j0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t j = j0 + lc + q;
      pre[q] = (irow < n && j <= irow) ? a.C[irow * npad + j] : 0.0;  // (j <= irow < n: j < n too)
    }
#pragma unroll
    for (int u = 0; u < kXPer; ++u) {
      const int e = tid + u * kThreads;
      prex[u] = e < xcount ? a.xs[j0 * dp + e] : 0.0;
    }
  };
  fetch(0);
  for (int64_t s = 0; s < steps; ++s) {
    const int64_t j0 = s * kStage;
    __syncthreads();  // the previous step's reads of Al are done (first step: nothing to wait for but the leaf tile)
#pragma unroll
    for (int q = 0; q < 8; ++q) Al[lr * kStageLd + lc + q] = pre[q];
#pragma unroll
    for (int u = 0; u < kXPer; ++u) {
      const int e = tid + u * kThreads;
      if (e < xcount) Xl[(e / dp) * (dp + 1) + e % dp] = prex[u];
    }
    __syncthreads();
    if (s + 1 < steps) fetch(j0 + kStage);
    // B operand: lane l holds k(xs_j, t_col) for j = j0 + 4 q + (l >> 4), col = l & 15 of the wave's 16
    double kv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t j = j0 + 4 * q + kq;
      kv[q] = 0.0;
      if (j < n) {
        double k, dk;
        kern_and_dkern_same(a.kernel, pair_r2(tcol, Xl + (4 * q + kq) * (dp + 1), dp), a.variance, k, dk);
        kv[q] = k;
      }
    }
#pragma unroll
    for (int t = 0; t < kRowBlock / 16; ++t) {
      if (j0 > i0 + 16 * t + 15) continue;  // (wave-uniform: the tile lies above the diagonal from here on)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double af = Al[(16 * t + (lane & 15)) * kStageLd + 4 * q + kq];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, kv[q], acc[t], 0, 0, 0);
      }
    }
  }
  // register r of tile t: row i0 + 16 t + (l >> 4) + 4 r, column l & 15
  double ss = 0.0;
#pragma unroll
  for (int t = 0; t < kRowBlock / 16; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = i0 + 16 * t + kq + 4 * r;
      a.V[(mt * npad + row) * kCols + col] = acc[t][r];
      ss = fma(acc[t][r], acc[t][r], ss);
    }
  }
  ss += __shfl_xor(ss, 16);
  ss += __shfl_xor(ss, 32);
  if (kq == 0) a.pv[(int64_t)blockIdx.y * a.mc + mt * kCols + col] = ss;
}

__global__ __launch_bounds__(kThreads) void pg_grad_kernel(PgArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double* tl = reinterpret_cast<double*>(lds_raw);  // [kCols][dp + 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t mt = blockIdx.x, j0 = (int64_t)blockIdx.y * kColBlock;
  const int64_t n = a.n, npad = a.npad;
  const int dp = a.dp, col = 16 * wave + (lane & 15), kq = lane >> 4;
  load_leaf_tile(a, mt, tl);
  __syncthreads();
  const double* tcol = tl + col * (dp + 1);
  // w[j] = sum_{i >= j} C[i][j] v[i]: A operand lane l holds C[i + (l >> 4)][j0 + 16 t + (l & 15)], B operand v[i + (l >> 4)][col]
  f64x4 w[kColBlock / 16];
#pragma unroll
  for (int t = 0; t < kColBlock / 16; ++t) w[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  // sixteen rows of v a trip: their twenty loads are issued before the first product (one k-step a trip left every load's
  // latency in the open).  Rows in [n, n16) of v are zeros pg_apply wrote (its row blocks end at multiples of 128)
  const int64_t n16 = (n + 15) / 16 * 16;
  const double* Vt = a.V + mt * npad * kCols + col;
  for (int64_t i = j0; i < n16; i += 16) {
    double b[4], af[4][kColBlock / 16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t ii = i + 4 * q + kq;
      b[q] = Vt[ii * kCols];
#pragma unroll
      for (int t = 0; t < kColBlock / 16; ++t) {
        const int64_t j = j0 + 16 * t + (lane & 15);
        af[q][t] = (ii < n && j <= ii) ? a.C[ii * npad + j] : 0.0;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int t = 0; t < kColBlock / 16; ++t) w[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[q][t], b[q], w[t], 0, 0, 0);
    }
  }
  // register r of tile t: training row j0 + 16 t + (l >> 4) + 4 r, column l & 15
  constexpr int kMine = kColBlock / 4;
  double qm[kMine], qv[kMine];
  double pm = 0.0, sqm = 0.0, sqv = 0.0;
#pragma unroll
  for (int t = 0; t < kColBlock / 16; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t j = j0 + 16 * t + kq + 4 * r;
      double m_ = 0.0, v_ = 0.0;
      if (j < n) {
        const double r2 = pair_r2(tcol, a.xs + j * dp, dp);
        double k, dk;
        kern_and_dkern_same(a.kernel, r2, a.variance, k, dk);
        const double al = a.alpha[j];
        pm = fma(al, k, pm);
        if (r2 > 1e-36) {
          const double dk2 = 2.0 * dk;
          m_ = dk2 * al;
          v_ = dk2 * (-2.0 * w[t][r]);
        }
      }
      qm[4 * t + r] = m_;
      qv[4 * t + r] = v_;
      sqm += m_;
      sqv += v_;
    }
  }
  const int64_t kstride = a.mc;
  double* out = a.pq + (int64_t)blockIdx.y * (3 + 2 * dp) * kstride + mt * kCols + col;
  auto fold = [&](double v) {  // over the four lane groups that share a column
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
  };
  pm = fold(pm);
  sqm = fold(sqm);
  sqv = fold(sqv);
  if (kq == 0) {
    out[0] = pm;
    out[kstride] = sqm;
    out[2 * kstride] = sqv;
  }
  for (int k = 0; k < dp; k += 4) {
    double am[4] = {0.0, 0.0, 0.0, 0.0}, av[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < kColBlock / 16; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double* xj = a.xs + (j0 + 16 * t + kq + 4 * r) * dp + k;  // (rows < N_pad; finite beyond N -- zeros, or an earlier problem's rows --, where q is zero)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          am[u] = fma(qm[4 * t + r], xj[u], am[u]);
          av[u] = fma(qv[4 * t + r], xj[u], av[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double m_ = fold(am[u]), v_ = fold(av[u]);
      if (kq == 0) {
        out[(3 + 2 * (k + u)) * kstride] = m_;
        out[(4 + 2 * (k + u)) * kstride] = v_;
      }
    }
  }
}

// blockIdx.y < d: the gradients in dimension y; blockIdx.y == d: mean and var.  One thread per live test point of the chunk
__global__ __launch_bounds__(kThreads) void pg_final_kernel(PgArgs a, int nrb, int ncb, int d, int64_t m_live,
                                                            const double* __restrict__ ls, double noise, double mean_c,
                                                            double* __restrict__ mean, double* __restrict__ var,
                                                            double* __restrict__ dmean, double* __restrict__ dvar) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= m_live) return;
  const int y = blockIdx.y;
  const int64_t kstride = a.mc, bstride = (int64_t)(3 + 2 * a.dp) * a.mc;
  if (y == d) {
    if (mean != nullptr) {
      double s = 0.0;
      for (int b = 0; b < ncb; ++b) s += a.pq[b * bstride + c];
      mean[c] = s + mean_c;
    }
    if (var != nullptr) {
      double s = 0.0;
      for (int b = 0; b < nrb; ++b) s += a.pv[b * a.mc + c];
      var[c] = (a.variance - s) + noise;
    }
    return;
  }
  const double t = a.ts[c * a.dp + y], l = ls[y];
  if (dmean != nullptr) {
    double sq = 0.0, sx = 0.0;
    for (int b = 0; b < ncb; ++b) {
      sq += a.pq[b * bstride + kstride + c];
      sx += a.pq[b * bstride + (3 + 2 * y) * kstride + c];
    }
    dmean[c * d + y] = (t * sq - sx) / l;
  }
  if (dvar != nullptr) {
    double sq = 0.0, sx = 0.0;
    for (int b = 0; b < ncb; ++b) {
      sq += a.pq[b * bstride + 2 * kstride + c];
      sx += a.pq[b * bstride + (4 + 2 * y) * kstride + c];
    }
    dvar[c * d + y] = (t * sq - sx) / l;
  }
}

}  // namespace

size_t predict_grad_workspace_doubles(int64_t npad, int dp, int64_t mc) {
  const size_t nrb = (size_t)(npad / kRowBlock), ncb = (size_t)(npad / kColBlock);
  return (size_t)mc * npad + nrb * mc + ncb * (size_t)(3 + 2 * dp) * mc;
}

size_t predict_grad_apply_workspace_doubles(int64_t npad, int64_t mc) {
  return (size_t)mc * npad + (size_t)(npad / kRowBlock) * mc;
}

// the apply stage alone, for joint.hip: the launch launch_predict_grad makes first, V and pv at the same places of g.work
int launch_predict_grad_apply(hipStream_t st, const PredictGradLaunch& g) {
  if (g.n < 1 || g.n > g.npad || g.npad % kRowBlock != 0 || g.dp < 4 || g.dp % 4 != 0 || g.dp > 48 || g.m < 1 || g.m > kPredictGradChunk) {
    note_launch_error("launch_predict_grad_apply: shape outside the kernels'");
    return -1;
  }
  const int64_t mc = (g.m + kCols - 1) / kCols * kCols;
  const int nrb = (int)((g.n + kRowBlock - 1) / kRowBlock);
  PgArgs a;
  a.C = g.C; a.alpha = nullptr; a.xs = g.xs; a.ts = g.ts;
  a.V = g.work;
  a.pv = a.V + (size_t)mc * g.npad;
  a.pq = nullptr;
  a.n = g.n; a.npad = g.npad; a.mc = mc; a.dp = g.dp; a.kernel = g.kp.kernel; a.variance = g.kp.variance;
  hipLaunchKernelGGL(pg_apply_kernel, dim3((unsigned)(mc / kCols), (unsigned)nrb), dim3(kThreads),
                     (kRowBlock * kStageLd + kStage * (g.dp + 1)) * 8 + kCols * (g.dp + 1) * 8, st, a);
  return 0;
}

int launch_predict_grad(hipStream_t st, const PredictGradLaunch& g) {
  if (g.n < 1 || g.n > g.npad || g.npad % kRowBlock != 0 || g.dp < 4 || g.dp % 4 != 0 || g.d < 1 || g.d > g.dp || g.dp > 48 || g.m < 1 ||
      g.m > kPredictGradChunk) {
    note_launch_error("launch_predict_grad: shape outside the kernels'");
    return -1;
  }
  const int64_t mc = (g.m + kCols - 1) / kCols * kCols;
  const int nrb = (int)((g.n + kRowBlock - 1) / kRowBlock), ncb = (int)((g.n + kColBlock - 1) / kColBlock);
  PgArgs a;
  a.C = g.C; a.alpha = g.alpha; a.xs = g.xs; a.ts = g.ts;
  a.V = g.work;
  a.pv = a.V + (size_t)mc * g.npad;
  a.pq = a.pv + (size_t)(g.npad / kRowBlock) * mc;
  a.n = g.n; a.npad = g.npad; a.mc = mc; a.dp = g.dp; a.kernel = g.kp.kernel; a.variance = g.kp.variance;
  const int leaf_bytes = kCols * (g.dp + 1) * 8;
  const dim3 tiles((unsigned)(mc / kCols));
  hipLaunchKernelGGL(pg_apply_kernel, dim3(tiles.x, (unsigned)nrb), dim3(kThreads), (kRowBlock * kStageLd + kStage * (g.dp + 1)) * 8 + leaf_bytes, st,
                     a);
  hipLaunchKernelGGL(pg_grad_kernel, dim3(tiles.x, (unsigned)ncb), dim3(kThreads), leaf_bytes, st, a);
  hipLaunchKernelGGL(pg_final_kernel, dim3((unsigned)((g.m + kThreads - 1) / kThreads), (unsigned)(g.d + 1)), dim3(kThreads), 0, st,
                     a, nrb, ncb, g.d, g.m, g.ls, g.kp.noise, g.kp.mean_c, g.mean, g.var, g.dmean, g.dvar);
  return 0;
}

}  // namespace gpso
