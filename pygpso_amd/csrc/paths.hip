// Pathwise posterior draws of the exact GP (Wilson et al. 2020: Matheron's rule over a random-Fourier-
// feature prior).  No counterpart in the reference.  A draw is a function of the (scaled) point t = x / l:
//     value[s](t) = c + sum_{j < F} phi_j(t) w[s][j] + sum_{i < N} k(xs_i, t) v[i][s],
//     phi_j(t) = sqrt(2 variance / F) cos(omega_j . t + b_j),   v = L^-T L^-1 R,
//     R[i][s] = (y_i - c) - sum_j phi_j(xs_i) w[s][j] - sqrt(noise + s_i) eps[s][i].
// k comes from direct differences in double (predict_grad.hip's pair_r2 and kern_and_dkern_same: the same bits as there).
// Kernels:
//   paths_eval_kernel   (tile of 64 points x block of up to 128 draws): the draws are the rows of 16 x 16 accumulator tiles
//                       on v_mfma_f64_16x16x4_f64, the B operand -- first the features, then the cross-Gram column -- is
//                       made in registers from rows staged in LDS and used by every draw tile; the A operand is the
//                       staged block of w, then of v^T.  Both contractions run un-split, in index order, to F and to N.
//                       gpso_paths_draw runs it over the training rows with the kernel part off (Phi(X) w^T)
//   paths_resid_kernel  R from y, that product, the per-point noise and eps
//   paths_tri_kernel    U = L^-1 R, then V^T = (L^-T U)^T on the same instruction; L^-1 is the dense fit-type factor, entry
//                       (i, j) read only where j <= i < N
//   paths_argmax_kernel per (draw, segment) the highest value of a chunk, merged into the running winner: an earlier chunk
//                       keeps a tie, so the lowest index wins
// The draw of a whitened variational posterior (gpso_paths_draw_q; section 7k) keeps the evaluation and replaces the solve:
//     v = beta + Lu^-T (Q eps - Lu^-1 P),   P = Phi(Zr) w^T over the resident rows Zr,
//   paths_q_lay_kernel  P^T and eps^T in the [row][draw] layout of the products, zero padding
//   paths_tri_kernel    with a compile-time epilogue: Lu^-1 P^T; Q eps^T (lower Q, or the transpose of the lower LB^-1) minus
//                       it; Lu^-T of that plus beta, written as v^T
// No atomics, every reduction in a fixed order; compiled with -ffp-contract=off, every fused multiply-add written out: a
// point's bits depend neither on its column slot, nor on the rest of the batch, nor on how many draws there are.
#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;
constexpr int kCols = 64;        // points per workgroup: 4 waves x 16 MFMA columns
constexpr int kDrawBlock = 128;  // draws per workgroup: 8 accumulator tiles a wave
constexpr int kStage = 16;       // features / training rows staged in LDS per step
constexpr int kStageLd = kStage + 1;
constexpr int kTriBlock = 64;    // output rows per paths_tri workgroup

struct PeArgs {
  const double* ts;     // [tiles * 64 * dp] scaled points, finite rows behind the live ones
  const double* xs;     // [npad * dp] scaled training rows
  const double* omega;  // [roundup(f, 16) * dp] frequencies, zero padding
  const double* phase;  // [roundup(f, 16)]
  const double* W;      // [s][ldw] feature weights
  const double* VT;     // [>= s][npad] v^T; nullptr: the kernel part is off
  double* out;          // [s][ldo], ldo >= tiles * 64
  int64_t n, npad, f, ldw, ldo;
  int s, dp, kernel;
  double variance, fscale, mean_c;
};

// |t - xs_j|^2 from direct differences, dimensions in order (predict_grad.hip's pair_r2)
__device__ __forceinline__ double pair_r2(const double* __restrict__ t, const double* __restrict__ xj, int dp) {
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

// acc[t] += A[s0 + 16 t .., 0 .. bound) B, B made from `rows` (PART 0: the features over omega; PART 1: k over xs), sixteen
// indices a step in their order; every index at or beyond `bound` contributes an exact zero
template <int PART>
__device__ __forceinline__ void pe_contract(const PeArgs& a, const double* __restrict__ A, int64_t lda, const double* __restrict__ rows,
                                            int64_t bound, int s0, int ntl, double* Al, double* Xl, double* Pl, const double* tcol,
                                            f64x4 (&acc)[kDrawBlock / 16]) {
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4;
  const int dp = a.dp;
  const int64_t steps = (bound + kStage - 1) / kStage;
  // thread -> draw tid / 2 of the block, 8 consecutive indices of the staged 16
  const int lr = tid >> 1, lc = (tid & 1) * 8;
  const int64_t srow = s0 + lr;
  constexpr int kXPer = (kStage * 48 + kThreads - 1) / kThreads;
  const int xcount = kStage * dp;
  double pre[8], prex[kXPer], prep = 0.0;
  auto fetch = [&](int64_t j0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t j = j0 + lc + q;
      pre[q] = (srow < a.s && j < bound) ? A[srow * lda + j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kXPer; ++u) {
      const int e = tid + u * kThreads;
      prex[u] = e < xcount ? rows[j0 * dp + e] : 0.0;  // (rows j0 .. j0 + 15 exist: both buffers end at a multiple of 16)
    }
    if (PART == 0) prep = tid < kStage ? a.phase[j0 + tid] : 0.0;
  };
  fetch(0);
  for (int64_t s = 0; s < steps; ++s) {
    const int64_t j0 = s * kStage;
    __syncthreads();  // the previous step's reads of Al, Xl and Pl are done (first step: the other part's, or nothing)
#pragma unroll
    for (int q = 0; q < 8; ++q) Al[lr * kStageLd + lc + q] = pre[q];
#pragma unroll
    for (int u = 0; u < kXPer; ++u) {
      const int e = tid + u * kThreads;
      if (e < xcount) Xl[(e / dp) * (dp + 1) + e % dp] = prex[u];
    }
    if (PART == 0 && tid < kStage) Pl[tid] = prep;
    __syncthreads();
    if (s + 1 < steps) fetch(j0 + kStage);
    // B operand: lane l holds the value of index j0 + 4 q + (l >> 4) at the point of column l & 15 of the wave's 16
    double kv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t j = j0 + 4 * q + kq;
      kv[q] = 0.0;
      if (j < bound) {
        const double* rj = Xl + (4 * q + kq) * (dp + 1);
        if (PART == 0) {
          double dot = 0.0;
          for (int k = 0; k < dp; k += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) dot = fma(rj[k + u], tcol[k + u], dot);
          }
          kv[q] = a.fscale * cos(dot + Pl[4 * q + kq]);
        } else {
          double k, dk;
          kern_and_dkern_same(a.kernel, pair_r2(tcol, rj, dp), a.variance, k, dk);
          kv[q] = k;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kDrawBlock / 16; ++t) {
      if (t >= ntl) continue;  // (uniform: no draw lives in this tile)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double af = Al[(16 * t + (lane & 15)) * kStageLd + 4 * q + kq];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, kv[q], acc[t], 0, 0, 0);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void paths_eval_kernel(PeArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double* Al = reinterpret_cast<double*>(lds_raw);  // [kDrawBlock][kStageLd]: the step's block of w or v^T
  double* Xl = Al + kDrawBlock * kStageLd;          // [kStage][dp + 1]: the step's frequencies or scaled rows
  double* Pl = Xl + kStage * (a.dp + 1);            // [kStage]: the step's phases
  double* tl = Pl + kStage;                         // [kCols][dp + 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t mt = blockIdx.x;
  const int s0 = (int)blockIdx.y * kDrawBlock;
  const int dp = a.dp, col = 16 * wave + (lane & 15), kq = lane >> 4;
  const int live = a.s - s0 < kDrawBlock ? a.s - s0 : kDrawBlock, ntl = (live + 15) / 16;
  for (int e = tid; e < kCols * dp; e += kThreads) {
    const int c = e / dp, k = e - c * dp;
    tl[c * (dp + 1) + k] = a.ts[mt * kCols * dp + e];
  }
  const double* tcol = tl + col * (dp + 1);
  f64x4 acc[kDrawBlock / 16];
#pragma unroll
  for (int t = 0; t < kDrawBlock / 16; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  pe_contract<0>(a, a.W, a.ldw, a.omega, a.f, s0, ntl, Al, Xl, Pl, tcol, acc);
  if (a.VT != nullptr) pe_contract<1>(a, a.VT, a.npad, a.xs, a.n, s0, ntl, Al, Xl, Pl, tcol, acc);
  // register r of tile t: draw s0 + 16 t + (l >> 4) + 4 r, column l & 15
#pragma unroll
  for (int t = 0; t < kDrawBlock / 16; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t sd = s0 + 16 * t + kq + 4 * r;
      if (sd < a.s) a.out[sd * a.ldo + mt * kCols + col] = acc[t][r] + a.mean_c;
    }
  }
}

// R[i][sd] = (y_i - c) - P[sd][i] - sqrt(noise + s_i) eps[sd][i] on i < n, sd < s; zero on the draws of the padding
__global__ __launch_bounds__(kThreads) void paths_resid_kernel(const double* __restrict__ y, const double* __restrict__ P, int64_t ldp,
                                                               const double* __restrict__ eps, const double* __restrict__ sdiag,
                                                               double noise, double mean_c, int64_t n, int s, int64_t spad,
                                                               double* __restrict__ R) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n * spad) return;
  const int64_t i = e / spad, sd = e - i * spad;
  double r = 0.0;
  if (sd < s) {
    r = (y[i] - mean_c) - P[sd * ldp + i];
    if (eps != nullptr) {
      const double sig = sqrt(sdiag != nullptr ? noise + sdiag[i] : noise);
      r = r - sig * eps[sd * n + i];
    }
  }
  R[e] = r;
}

// acc[o][col] = sum_{k <= o} C[o][k] B[k][col] (TRANS false; rows o < roundup(n, 64)) or sum_{o <= k < n} C[k][o] B[k][col] (TRANS
// true).  C[i][j] is read only where j <= i < n.  k in index order, sixteen a trip.  Written as out[o][col], or out[col][o] with
// OUT_T, after the compile-time epilogue: kEpiNone acc itself (the exact GP's two products: e and s unused); kEpiMinus acc -
// e[o][col], e laid out as out; kEpiPlusRow acc + e[o] on o < n and col < s
enum { kEpiNone = 0, kEpiMinus = 1, kEpiPlusRow = 2 };
template <bool TRANS, bool OUT_T, int EPI>
__global__ __launch_bounds__(kThreads) void paths_tri_kernel(const double* __restrict__ C, const double* __restrict__ B, double* __restrict__ out,
                                                             int64_t n, int64_t npad, int64_t ldb, int64_t ldo, const double* __restrict__ e,
                                                             int s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const int64_t col = (int64_t)blockIdx.x * kCols + 16 * wave + (lane & 15), o0 = (int64_t)blockIdx.y * kTriBlock;
  const int64_t n16 = (n + 15) / 16 * 16;
  const int64_t k_lo = TRANS ? o0 : 0, k_hi = TRANS ? n16 : (n16 < o0 + kTriBlock ? n16 : o0 + kTriBlock);
  f64x4 acc[kTriBlock / 16];
#pragma unroll
  for (int t = 0; t < kTriBlock / 16; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int64_t k0 = k_lo; k0 < k_hi; k0 += 16) {
    double b[4], af[4][kTriBlock / 16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t kk = k0 + 4 * q + kq;
      b[q] = kk < n ? B[kk * ldb + col] : 0.0;
#pragma unroll
      for (int t = 0; t < kTriBlock / 16; ++t) {
        const int64_t o = o0 + 16 * t + (lane & 15);
        if (TRANS) af[q][t] = (kk < n && o <= kk) ? C[kk * npad + o] : 0.0;
        else af[q][t] = (o < n && kk <= o) ? C[o * npad + kk] : 0.0;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int t = 0; t < kTriBlock / 16; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[q][t], b[q], acc[t], 0, 0, 0);
    }
  }
  // register r of tile t: output row o0 + 16 t + (l >> 4) + 4 r, column l & 15
#pragma unroll
  for (int t = 0; t < kTriBlock / 16; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t o = o0 + 16 * t + kq + 4 * r;
      double v = acc[t][r];
      if (EPI == kEpiMinus) v = v - e[o * ldo + col];
      if (EPI == kEpiPlusRow && o < n && col < s) v = v + e[o];
      if (OUT_T) out[col * ldo + o] = v;
      else out[o * ldo + col] = v;
    }
  }
}

// ---- the draw of a whitened variational posterior ------------------------------------------------------
// Pt[i][sd] = P[sd][i], E[i][sd] = eps[sd][i] (zeros without eps) on i < n, sd < s; zero on the rows up to roundup(n, 64) and on
// the draws of the padding: the [row][draw] layout the triangular products read
__global__ __launch_bounds__(kThreads) void paths_q_lay_kernel(const double* __restrict__ P, int64_t ldp, const double* __restrict__ eps,
                                                               int64_t n, int64_t n64, int s, int64_t spad, double* __restrict__ Pt,
                                                               double* __restrict__ E) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n64 * spad) return;
  const int64_t i = e / spad, sd = e - i * spad;
  const bool live = i < n && sd < s;
  Pt[e] = live ? P[sd * ldp + i] : 0.0;
  E[e] = (live && eps != nullptr) ? eps[sd * n + i] : 0.0;
}

// blockIdx.x: segment, blockIdx.y: draw.  The rows of the segment that lie in [off, off + mc) against the running winner
__global__ __launch_bounds__(kThreads) void paths_argmax_kernel(const double* __restrict__ vals, int64_t ldv, int64_t off, int64_t mc,
                                                                const int64_t* __restrict__ seg_off, int nseg,
                                                                int64_t* __restrict__ best_i, double* __restrict__ best_v) {
  __shared__ double bv[kThreads];
  __shared__ int64_t bi[kThreads];
  const int tid = threadIdx.x;
  const int64_t lo = seg_off[blockIdx.x] > off ? seg_off[blockIdx.x] : off;
  const int64_t hi = seg_off[blockIdx.x + 1] < off + mc ? seg_off[blockIdx.x + 1] : off + mc;
  if (lo >= hi) return;  // (the whole workgroup: nothing of this segment in the chunk)
  const double* row = vals + (int64_t)blockIdx.y * ldv - off;
  double best = 0.0;
  int64_t at = -1;
  for (int64_t i = lo + tid; i < hi; i += kThreads) {
    const double v = row[i];
    if (at < 0 || v > best) {
      best = v;
      at = i;
    }
  }
  bv[tid] = best;
  bi[tid] = at;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const double ov = bv[tid + o];
      const int64_t oi = bi[tid + o];
      if (oi >= 0 && (bi[tid] < 0 || ov > bv[tid] || (ov == bv[tid] && oi < bi[tid]))) {
        bv[tid] = ov;
        bi[tid] = oi;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t slot = (int64_t)blockIdx.y * nseg + blockIdx.x;
    if (best_i[slot] < 0 || bv[0] > best_v[slot]) {  // (an earlier chunk keeps a tie: its index is the lower one)
      best_i[slot] = bi[0];
      best_v[slot] = bv[0];
    }
  }
}

int eval_lds_bytes(int dp) { return (kDrawBlock * kStageLd + kStage * (dp + 1) + kStage + kCols * (dp + 1)) * 8; }

}  // namespace

int launch_paths_eval(hipStream_t st, const PathsEvalLaunch& g) {
  if (g.n < 1 || g.n > g.npad || g.npad % 64 != 0 || g.dp < 4 || g.dp % 4 != 0 || g.dp > 48 || g.m < 1 || g.s < 1 || g.s > kPathsMaxDraws ||
      g.f < 1 || g.ldw < g.f || g.ldo < (g.m + kCols - 1) / kCols * kCols) {
    note_launch_error("launch_paths_eval: shape outside the kernel's");
    return -1;
  }
  PeArgs a;
  a.ts = g.ts; a.xs = g.xs; a.omega = g.omega; a.phase = g.phase; a.W = g.W; a.VT = g.VT; a.out = g.out;
  a.n = g.n; a.npad = g.npad; a.f = g.f; a.ldw = g.ldw; a.ldo = g.ldo;
  a.s = (int)g.s; a.dp = g.dp; a.kernel = g.kp.kernel;
  a.variance = g.kp.variance; a.fscale = sqrt(2.0 * g.kp.variance / (double)g.f); a.mean_c = g.VT != nullptr ? g.kp.mean_c : 0.0;
  hipLaunchKernelGGL(paths_eval_kernel, dim3((unsigned)((g.m + kCols - 1) / kCols), (unsigned)((g.s + kDrawBlock - 1) / kDrawBlock)),
                     dim3(kThreads), eval_lds_bytes(g.dp), st, a);
  return 0;
}

void launch_paths_solve(hipStream_t st, const double* C, const double* y, const double* P, int64_t ldp, const double* eps,
                        const double* sdiag, const KernParams& kp, int64_t n, int64_t npad, int64_t s, double* R, double* U,
                        double* VT) {
  const int64_t spad = (s + kCols - 1) / kCols * kCols;
  hipLaunchKernelGGL(paths_resid_kernel, dim3((unsigned)((n * spad + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, y, P, ldp, eps,
                     sdiag, kp.noise, kp.mean_c, n, (int)s, spad, R);
  const dim3 grid((unsigned)(spad / kCols), (unsigned)((n + kTriBlock - 1) / kTriBlock));
  const double* none = nullptr;
  hipLaunchKernelGGL((paths_tri_kernel<false, false, kEpiNone>), grid, dim3(kThreads), 0, st, C, R, U, n, npad, spad, spad, none, 0);
  hipLaunchKernelGGL((paths_tri_kernel<true, true, kEpiNone>), grid, dim3(kThreads), 0, st, C, U, VT, n, npad, spad, npad, none, 0);
}

void launch_paths_solve_q(hipStream_t st, const double* Lui, const double* Q, bool q_transposed, const double* beta, const double* P,
                          int64_t ldp, const double* eps, int64_t n, int64_t npad, int64_t s, double* Pt, double* E, double* X,
                          double* VT) {
  const int64_t spad = (s + kCols - 1) / kCols * kCols, n64 = (n + kTriBlock - 1) / kTriBlock * kTriBlock;
  hipLaunchKernelGGL(paths_q_lay_kernel, dim3((unsigned)((n64 * spad + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, P, ldp, eps, n,
                     n64, (int)s, spad, Pt, E);
  const dim3 grid((unsigned)(spad / kCols), (unsigned)(n64 / kTriBlock));
  const double* none = nullptr;
  // X = Lu^-1 P^T;  the residual Q eps^T - X over Pt (read by the first product only);  V^T = (Lu^-T residual + beta)^T
  hipLaunchKernelGGL((paths_tri_kernel<false, false, kEpiNone>), grid, dim3(kThreads), 0, st, Lui, Pt, X, n, npad, spad, spad, none, 0);
  if (q_transposed)
    hipLaunchKernelGGL((paths_tri_kernel<true, false, kEpiMinus>), grid, dim3(kThreads), 0, st, Q, E, Pt, n, npad, spad, spad, X, 0);
  else
    hipLaunchKernelGGL((paths_tri_kernel<false, false, kEpiMinus>), grid, dim3(kThreads), 0, st, Q, E, Pt, n, npad, spad, spad, X, 0);
  hipLaunchKernelGGL((paths_tri_kernel<true, true, kEpiPlusRow>), grid, dim3(kThreads), 0, st, Lui, Pt, VT, n, npad, spad, npad, beta,
                     (int)s);
}

void launch_paths_argmax(hipStream_t st, const double* vals, int64_t ldv, int64_t off, int64_t mc, const int64_t* seg_off_dev, int nseg,
                         int64_t s, int64_t* best_i, double* best_v) {
  hipLaunchKernelGGL(paths_argmax_kernel, dim3((unsigned)nseg, (unsigned)s), dim3(kThreads), 0, st, vals, ldv, off, mc, seg_off_dev, nseg,
                     best_i, best_v);
}

}  // namespace gpso
