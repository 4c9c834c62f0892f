// Greedy batch selection under hallucinated updates and the latent cross-covariance it is built on (DESIGN.md section 7n;
// GP-BUCB, Desautels et al. 2014 -- "kriging believer").  No counterpart in the reference.  For the resident predictive
// (C, alpha, c, variance, noise) over the scaled rows xs = x / l the latent posterior covariance between two points is
//     Cov(a, b) = k(t_a, t_b) - sum_{i < N} k(xs_i, t_a) w_b[i],   w_b = C^T (C k_b),   k_b[i] = k(xs_i, t_b),
// one vector of length N per point b.  r2 and k come from direct differences in double (predict_grad.hip's pair_r2 and
// kern_and_dkern_same).  C is the dense fit-type L^-1, entry (i, j) read only where j <= i < N; the rows only below N.
// Kernels:
//   batch_kb_kernel      k_b over the resident rows, one thread a row
//   batch_u_kernel       u = C k_b: a wave a row, the row's columns in steps of 64, then the wave's butterfly
//   batch_w_kernel       w = C^T u: a workgroup 64 columns and one of batch_w_slabs(n) slabs of the rows below them, in four
//                        contiguous pieces (a wave each) whose sums are added in wave order; the slabs are added in their
//                        order where w is read
//   batch_pick_kernel    the point's own latent variance variance - |u|^2; in a round also d_t and the stop test
//   batch_col_kernel     (tile of 64 leaves x up to 8 points b): the cross-Gram column in registers from rows staged in
//                        LDS, 64 a step and 16 a wave, contracted with w by vector fused multiply-adds; the four waves'
//                        sums are added in wave order.  As a round of gpso_best_batch (one point: the pick) it goes on:
//                        history subtraction, G[t][j], the downdate of s2[j], the retire test, the new score and the
//                        tile's first maximum (batch.hpp)
//   batch_init_kernel    round 0: every row live, the blocks' first maxima of the value column
//   batch_finish_kernel  one workgroup: merges the blocks' maxima in block order (lowest index on a tie, a NaN wins),
//                        appends the pick record, fetches the pick's scaled row and its G history, sets the stop word
// A round's launches read the stop word first and do nothing once it is set.  No atomics, every reduction in a fixed order;
// compiled with -ffp-contract=off, every fused multiply-add written out: a row's bits depend neither on its slot in the
// tile, nor on the chunking, nor -- in gpso_cross_cov -- on the rest of either batch.
#include "batch.hpp"

#include <vector>

#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;
constexpr int kCols = 64;   // leaves per batch_col workgroup: one a lane, every wave holds all of them
constexpr int kStage = 64;  // training rows staged in LDS per step: 16 a wave
constexpr int kNb = 8;      // points b per workgroup of the cross-covariance launches

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

__device__ __forceinline__ bool stopped(const BatchState* st) { return st != nullptr && st->stop != 0; }

// Kb[c][i] = k(xs_i, tb_c), i < n; blockIdx.y: the point c
__global__ __launch_bounds__(kThreads) void batch_kb_kernel(const BatchState* st, const double* __restrict__ xs,
                                                            const double* __restrict__ tb, int64_t n, int64_t npad, int dp, int kernel,
                                                            double variance, double* __restrict__ Kb) {
  if (stopped(st)) return;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= n) return;
  double k, dk;
  kern_and_dkern_same(kernel, pair_r2(tb + (int64_t)c * dp, xs + i * dp, dp), variance, k, dk);
  Kb[c * npad + i] = k;
}

// U[c][i] = sum_{j <= i} C[i][j] Kb[c][j], i < n: row 4 blockIdx.x + wave, points NB blockIdx.y ..
template <int NB>
__global__ __launch_bounds__(kThreads) void batch_u_kernel(const BatchState* st, const double* __restrict__ C, const double* __restrict__ Kb,
                                                           int64_t n, int64_t npad, int b, double* __restrict__ U) {
  if (stopped(st)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  const int c0 = (int)blockIdx.y * NB;
  if (i >= n) return;  // (the whole wave; no barrier below)
  double acc[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u) acc[u] = 0.0;
  int64_t j = lane;
  for (; j + 192 <= i; j += 256) {  // four steps a trip: their loads are issued before the first product; the order of the sums stays
    double cij[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) cij[r] = C[i * npad + j + 64 * r];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (c0 + u < b) acc[u] = fma(cij[r], Kb[(int64_t)(c0 + u) * npad + j + 64 * r], acc[u]);
    }
  }
  for (; j <= i; j += 64) {
    const double cij = C[i * npad + j];
#pragma unroll
    for (int u = 0; u < NB; ++u)
      if (c0 + u < b) acc[u] = fma(cij, Kb[(int64_t)(c0 + u) * npad + j], acc[u]);
  }
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    double v = acc[u];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0 && c0 + u < b) U[(int64_t)(c0 + u) * npad + i] = v;
  }
}

// the four waves' partial sums of a workgroup, added in wave order into pl[lane][NB]; every wave reads the sums afterwards
template <int NB>
__device__ __forceinline__ void fold_waves(double (&acc)[NB], double* pl, int lane, int wave) {
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int u = 0; u < NB; ++u) pl[lane * NB + u] = w == 0 ? acc[u] : pl[lane * NB + u] + acc[u];
    }
    __syncthreads();
  }
}

// Wp[z][c][j] = sum over the rows i of slab z of C[i][j] U[c][i], j < n: columns 64 blockIdx.x .., points NB blockIdx.y .., slab
// blockIdx.z.  The rows j0 .. n - 1 below the block's columns are cut into 4 nz contiguous pieces, piece 4 z + wave to a wave; the
// column launch adds the nz slabs in their order (w_entry).  nz = batch_w_slabs(n) depends on n alone, so the bits of w do too
template <int NB>
__global__ __launch_bounds__(kThreads) void batch_w_kernel(const BatchState* st, const double* __restrict__ C, const double* __restrict__ U,
                                                           int64_t n, int64_t npad, int b, double* __restrict__ Wp) {
  if (stopped(st)) return;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double* pl = reinterpret_cast<double*>(lds_raw);  // [64][NB]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * 64, j = j0 + lane;
  const int c0 = (int)blockIdx.y * NB;
  const int64_t pieces = 4 * (int64_t)gridDim.z, per = (n - j0 + pieces - 1) / pieces;
  const int64_t lo = j0 + (4 * (int64_t)blockIdx.z + wave) * per, hi = lo + per < n ? lo + per : n;
  double acc[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u) acc[u] = 0.0;
  int64_t i = lo;
  for (; i + 3 < hi; i += 4) {  // four rows a trip: their loads are issued before the first product
    double cij[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) cij[r] = (j <= i + r && j < n) ? C[(i + r) * npad + j] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (c0 + u < b) acc[u] = fma(cij[r], U[(int64_t)(c0 + u) * npad + i + r], acc[u]);
    }
  }
  for (; i < hi; ++i) {
    const double cij = (j <= i && j < n) ? C[i * npad + j] : 0.0;
#pragma unroll
    for (int u = 0; u < NB; ++u)
      if (c0 + u < b) acc[u] = fma(cij, U[(int64_t)(c0 + u) * npad + i], acc[u]);
  }
  fold_waves<NB>(acc, pl, lane, wave);
  if (wave == 0 && j < n) {
#pragma unroll
    for (int u = 0; u < NB; ++u)
      if (c0 + u < b) Wp[((int64_t)blockIdx.z * b + c0 + u) * npad + j] = pl[lane * NB + u];
  }
}

// lv[c] = variance - |U[c]|^2 (blockIdx.x: the point c).  In a round (st given; one point): d_t, its root and the stop test
__global__ __launch_bounds__(kThreads) void batch_pick_kernel(BatchState* st, int t, const double* __restrict__ U, int64_t n, int64_t npad,
                                                              double variance, double obs_noise, double* __restrict__ lv) {
  if (stopped(st)) return;
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const double* u = U + (int64_t)blockIdx.x * npad;
  double ss = 0.0;
  for (int64_t i = tid; i < n; i += kThreads) ss = fma(u[i], u[i], ss);
  red[tid] = ss;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid != 0) return;
  const double v = variance - red[0];
  lv[blockIdx.x] = v;
  if (st != nullptr) {
    const double d = batch_pick_d(v, st->gp, t, obs_noise);
    st->d = d;
    st->root_d = sqrt(d);
    if (!batch_d_usable(d)) st->stop = 1;
  }
}

struct ColArgs {
  const double* ts;     // [tiles * 64 * dp] scaled leaves, zero rows behind the live ones
  const double* tnorm;  // [tiles * 64] their squared norms (a NaN marks a row with a NaN coordinate)
  const double* xs;     // [npad * dp] scaled resident rows
  const double* W;      // [nz][b][npad]: the slabs of w (batch_w_kernel)
  int nz;
  const double* tb;     // [b][dp] the scaled points b
  const double* bnorm;  // [b], nullable
  int64_t n, npad, m;   // m: live leaves
  int b, dp, kernel;
  double variance;
  double* cov;          // cross: cov[c * ldc + j]
  int64_t ldc;
  // a round of gpso_best_batch
  BatchState* st;
  int t, rank;          // rank 0: downdate only (the last pick of a call that wants var_after)
  double* G;            // [q][m]
  double* s2;           // [m]
  const double* mean;   // [m]
  unsigned char* live;  // [m]
  AcqSpec acq;
  double noise;
  double* bmax_v;       // [tiles]
  int64_t* bmax_i;
};

// w_c[i]: the slabs in their order
__device__ __forceinline__ double w_entry(const ColArgs& a, int c, int64_t i) {
  double w = a.W[(int64_t)c * a.npad + i];
  for (int z = 1; z < a.nz; ++z) w += a.W[((int64_t)z * a.b + c) * a.npad + i];
  return w;
}

// MES: the instance that scores by GPSO_ACQ_MES carries its loop over the maxima; the other kinds' instance does not (acq.hpp)
template <int NB, bool ROUND, bool MES = false>
__global__ __launch_bounds__(kThreads) void batch_col_kernel(ColArgs a) {
  if (ROUND && stopped(a.st)) return;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int dp = a.dp, ld = dp + 1;
  double* tl = reinterpret_cast<double*>(lds_raw);  // [kCols][ld]
  double* Xl = tl + kCols * ld;                      // [kStage][dp]: the step's scaled rows (every lane reads the same entry: no padding)
  double* wl = Xl + kStage * ld;                     // [NB][kStage]: the step's entries of w
  double* pl = wl + NB * kStage;                     // [kCols][NB]: the waves' sums
  double* bl = pl + kCols * NB;                      // [NB][ld]: the points b
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t mt = blockIdx.x, n = a.n;
  const int c0 = (int)blockIdx.y * NB;
  for (int e = tid; e < kCols * dp; e += kThreads) {
    const int c = e / dp, k = e - c * dp;
    tl[c * ld + k] = a.ts[mt * kCols * dp + e];
  }
  for (int e = tid; e < NB * dp; e += kThreads) {
    const int c = e / dp, k = e - c * dp;
    bl[c * ld + k] = c0 + c < a.b ? a.tb[(int64_t)(c0 + c) * dp + k] : 0.0;
  }
  const double* tcol = tl + lane * ld;
  double acc[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u) acc[u] = 0.0;
  const int64_t steps = (n + kStage - 1) / kStage;
  for (int64_t s = 0; s < steps; ++s) {
    const int64_t i0 = s * kStage;
    __syncthreads();  // the previous step's reads of Xl and wl are done
    for (int e = tid; e < kStage * dp; e += kThreads) {
      const int r = e / dp;
      Xl[e] = i0 + r < n ? a.xs[i0 * dp + e] : 0.0;
    }
    for (int e = tid; e < NB * kStage; e += kThreads) {
      const int c = e / kStage, r = e - c * kStage;
      wl[e] = (i0 + r < n && c0 + c < a.b) ? w_entry(a, c0 + c, i0 + r) : 0.0;
    }
    __syncthreads();
    // the wave's 16 rows four at a time: one read of the leaf's coordinate serves four differences (the staged rows are read
    // by every lane at once).  Each r2 is pair_r2's sum, dimensions in order; the products enter acc in row order
    for (int g = 0; g < kStage / 16; ++g) {
      const int rr = (kStage / 4) * wave + 4 * g;
      if (i0 + rr >= n) break;  // (the whole wave)
      const double* x0 = Xl + rr * dp;
      double r2[4] = {0.0, 0.0, 0.0, 0.0};
      for (int k = 0; k < dp; k += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double t = tcol[k + q];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double df = t - x0[r * dp + k + q];
            r2[r] = fma(df, df, r2[r]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (i0 + rr + r >= n) break;  // (rows at or beyond n were staged as zeros and contribute nothing)
        double k, dk;
        kern_and_dkern_same(a.kernel, r2[r], a.variance, k, dk);
#pragma unroll
        for (int u = 0; u < NB; ++u) acc[u] = fma(k, wl[u * kStage + rr + r], acc[u]);
      }
    }
  }
  fold_waves<NB>(acc, pl, lane, wave);
  if (wave != 0) return;
  const int64_t j = mt * kCols + lane;
  const bool row = j < a.m;
  const bool row_nan = row && a.tnorm[j] != a.tnorm[j];
  double v = 0.0;
  int64_t vi = -1;
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    if (!row || c0 + u >= a.b) continue;
    const double r2 = pair_r2(tcol, bl + u * ld, dp);
    double k, dk;
    kern_and_dkern_same(a.kernel, r2, a.variance, k, dk);
    double cv = k - pl[lane * NB + u];
    if (row_nan || (a.bnorm != nullptr && a.bnorm[c0 + u] != a.bnorm[c0 + u])) cv = __builtin_nan("");
    if (!ROUND) {
      a.cov[(int64_t)(c0 + u) * a.ldc + j] = cv;
    } else {
      const double g = batch_row_g(cv, a.G + j, a.m, a.st->gp, a.t, a.st->root_d);
      a.G[(int64_t)a.t * a.m + j] = g;
      const double s2 = batch_downdate(a.s2[j], g);
      a.s2[j] = s2;
      bool alive = a.live[j] != 0;
      if (alive && batch_same_point(r2)) {
        alive = false;
        a.live[j] = 0;
      }
      if (alive && a.rank) {
        v = batch_score<MES>(a.acq, a.mean[j], s2, a.noise);
        vi = j;
      }
    }
  }
  if (!ROUND || !a.rank) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int64_t oi = __shfl_xor((long long)vi, off);
    if (batch_beats(ov, oi, v, vi)) {
      v = ov;
      vi = oi;
    }
  }
  if (lane == 0) {
    a.bmax_v[mt] = v;
    a.bmax_i[mt] = vi;
  }
}

// round 0: every row live; the first maximum of `value` over the 256 rows of the block
__global__ __launch_bounds__(kThreads) void batch_init_kernel(const double* __restrict__ value, int64_t m, unsigned char* __restrict__ live,
                                                              double* __restrict__ bmax_v, int64_t* __restrict__ bmax_i) {
  __shared__ double bv[kThreads];
  __shared__ int64_t bi[kThreads];
  const int tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * kThreads + tid;
  const bool row = j < m;
  if (row) live[j] = 1;
  bv[tid] = row ? value[j] : 0.0;
  bi[tid] = row ? j : -1;
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

// one workgroup: the pick of round t from the blocks' maxima
__global__ __launch_bounds__(kThreads) void batch_finish_kernel(BatchState* st, int t, const double* __restrict__ bmax_v,
                                                                const int64_t* __restrict__ bmax_i, int64_t nblocks, const double* __restrict__ ts,
                                                                int dp, const double* __restrict__ mean, const double* __restrict__ s2,
                                                                const double* __restrict__ G, int64_t m, unsigned char* __restrict__ live,
                                                                double* __restrict__ tp) {
  if (stopped(st)) return;
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
  if (p < 0) {  // no live row is left: the batch ends with the picks it has
    if (tid == 0) st->stop = 1;
    return;
  }
  if (tid == 0) {
    st->idx[t] = p;
    st->mean[t] = mean[p];
    st->var[t] = s2[p];
    st->value[t] = bv[0];
    st->n_picked = t + 1;
    live[p] = 0;
    if (bv[0] != bv[0]) st->stop = 1;  // a NaN value: reported, and the batch ends after it
  }
  for (int k = tid; k < dp; k += kThreads) tp[k] = ts[p * dp + k];
  for (int s = tid; s < t; s += kThreads) st->gp[s] = G[(int64_t)s * m + p];
}

int col_lds_bytes(int dp, int nb) { return ((kCols + kStage + nb) * (dp + 1) + nb * kStage + kCols * nb) * 8; }

bool shape_ok(int64_t n, int64_t npad, int dp, int b) {
  return n >= 1 && n <= npad && npad % 64 == 0 && dp >= 4 && dp % 4 == 0 && dp <= 48 && b >= 1 && b <= kBatchMaxPicks;
}

template <int NB>
void pick_vectors(hipStream_t s, const BatchPickLaunch& g) {
  const unsigned groups = (unsigned)((g.b + NB - 1) / NB);
  hipLaunchKernelGGL(batch_kb_kernel, dim3((unsigned)((g.n + kThreads - 1) / kThreads), (unsigned)g.b), dim3(kThreads), 0, s, g.st, g.xs, g.tb,
                     g.n, g.npad, g.dp, g.kp.kernel, g.kp.variance, g.Kb);
  hipLaunchKernelGGL(batch_u_kernel<NB>, dim3((unsigned)((g.n + 3) / 4), groups), dim3(kThreads), 0, s, g.st, g.C, g.Kb, g.n, g.npad, g.b, g.U);
  hipLaunchKernelGGL(batch_w_kernel<NB>, dim3((unsigned)((g.n + 63) / 64), groups, (unsigned)batch_w_slabs(g.n)), dim3(kThreads), 64 * NB * 8, s,
                     g.st, g.C, g.U, g.n, g.npad, g.b, g.W);
  hipLaunchKernelGGL(batch_pick_kernel, dim3((unsigned)g.b), dim3(kThreads), 0, s, g.st, g.t, g.U, g.n, g.npad, g.kp.variance, g.obs_noise,
                     g.lv);
}

}  // namespace

int batch_w_slabs(int64_t n) {
  const int64_t z = (n + 255) / 256;
  return (int)(z < 1 ? 1 : z > 16 ? 16 : z);
}
size_t batch_pick_workspace_doubles(int64_t n, int64_t npad, int b) { return (size_t)(2 + batch_w_slabs(n)) * b * npad; }

int launch_batch_pick_vectors(hipStream_t s, const BatchPickLaunch& g) {
  if (!shape_ok(g.n, g.npad, g.dp, g.b) || (g.st != nullptr && g.b != 1)) {
    note_launch_error("launch_batch_pick_vectors: shape outside the kernels'");
    return -1;
  }
  if (g.b == 1) pick_vectors<1>(s, g);
  else pick_vectors<kNb>(s, g);
  return 0;
}

int launch_batch_cross(hipStream_t s, const BatchColLaunch& g) {
  if (!shape_ok(g.n, g.npad, g.dp, g.b) || g.m < 1 || g.ldc < g.m) {
    note_launch_error("launch_batch_cross: shape outside the kernel's");
    return -1;
  }
  ColArgs a{};
  a.ts = g.ts; a.tnorm = g.tnorm; a.xs = g.xs; a.W = g.W; a.tb = g.tb; a.bnorm = g.bnorm; a.n = g.n; a.npad = g.npad; a.m = g.m;
  a.b = g.b; a.dp = g.dp; a.kernel = g.kp.kernel; a.variance = g.kp.variance; a.cov = g.cov; a.ldc = g.ldc; a.nz = batch_w_slabs(g.n);
  const unsigned tiles = (unsigned)((g.m + kCols - 1) / kCols);
  if (g.b == 1)
    hipLaunchKernelGGL((batch_col_kernel<1, false>), dim3(tiles, 1), dim3(kThreads), col_lds_bytes(g.dp, 1), s, a);
  else
    hipLaunchKernelGGL((batch_col_kernel<kNb, false>), dim3(tiles, (unsigned)((g.b + kNb - 1) / kNb)), dim3(kThreads), col_lds_bytes(g.dp, kNb),
                       s, a);
  return 0;
}

int launch_batch_round(hipStream_t s, const BatchColLaunch& g) {
  if (!shape_ok(g.n, g.npad, g.dp, 1) || g.m < 1 || g.t < 0 || g.t >= kBatchMaxPicks || g.st == nullptr) {
    note_launch_error("launch_batch_round: shape outside the kernel's");
    return -1;
  }
  ColArgs a{};
  a.ts = g.ts; a.tnorm = g.tnorm; a.xs = g.xs; a.W = g.W; a.tb = g.tb; a.bnorm = nullptr; a.n = g.n; a.npad = g.npad; a.m = g.m;
  a.b = 1; a.dp = g.dp; a.kernel = g.kp.kernel; a.variance = g.kp.variance; a.nz = batch_w_slabs(g.n);
  a.st = g.st; a.t = g.t; a.rank = g.rank ? 1 : 0; a.G = g.G; a.s2 = g.s2; a.mean = g.mean; a.live = g.live; a.acq = g.acq;
  a.noise = g.kp.noise; a.bmax_v = g.bmax_v; a.bmax_i = g.bmax_i;
  auto* fn = g.acq.kind == GPSO_ACQ_MES ? batch_col_kernel<1, true, true> : batch_col_kernel<1, true, false>;
  hipLaunchKernelGGL(fn, dim3((unsigned)((g.m + kCols - 1) / kCols), 1), dim3(kThreads), col_lds_bytes(g.dp, 1), s, a);
  return 0;
}

int64_t batch_init_blocks(int64_t m) { return (m + kThreads - 1) / kThreads; }
int64_t batch_round_blocks(int64_t m) { return (m + kCols - 1) / kCols; }

void launch_batch_init(hipStream_t s, const double* value, int64_t m, unsigned char* live, double* bmax_v, int64_t* bmax_i) {
  hipLaunchKernelGGL(batch_init_kernel, dim3((unsigned)batch_init_blocks(m)), dim3(kThreads), 0, s, value, m, live, bmax_v, bmax_i);
}

void launch_batch_finish(hipStream_t s, BatchState* st, int t, const double* bmax_v, const int64_t* bmax_i, int64_t nblocks, const double* ts,
                         int dp, const double* mean, const double* s2, const double* G, int64_t m, unsigned char* live, double* tp) {
  hipLaunchKernelGGL(batch_finish_kernel, dim3(1), dim3(kThreads), 0, s, st, t, bmax_v, bmax_i, nblocks, ts, dp, mean, s2, G, m, live, tp);
}

// ---- the same rounds on the host, from a given mean, s2 and latent covariance (gpso_batch_greedy_host) -------------------------
int batch_greedy_host(const AcqSpec& a, const double* mean, const double* s2, const double* cov, double noise, double obs_noise,
                      int64_t m, int q, int64_t* idx, double* var, double* value, int* n_picked, double* var_after) {
  std::vector<double> s2w(s2, s2 + m), G((size_t)q * m, 0.0), gp((size_t)q, 0.0);
  std::vector<unsigned char> live((size_t)m, 1);
  int np = 0;
  for (int t = 0; t < q; ++t) {
    double bv = 0.0;
    int64_t p = -1;
    for (int64_t j = 0; j < m; ++j) {
      if (!live[j]) continue;
      const double v = batch_score(a, mean[j], s2w[j], noise);
      if (batch_beats(v, j, bv, p)) {
        bv = v;
        p = j;
      }
    }
    if (p < 0) break;
    idx[t] = p;
    if (var) var[t] = s2w[p];
    if (value) value[t] = bv;
    np = t + 1;
    live[p] = 0;
    if (bv != bv) break;
    for (int s = 0; s < t; ++s) gp[s] = G[(size_t)s * m + p];
    const double cpp = cov[p * m + p];
    const double d = batch_pick_d(cpp, gp.data(), t, obs_noise);
    if (!batch_d_usable(d)) break;
    const double root = sqrt(d);
    for (int64_t j = 0; j < m; ++j) {
      const double cjp = cov[j * m + p];
      const double g = batch_row_g(cjp, G.data() + j, m, gp.data(), t, root);
      G[(size_t)t * m + j] = g;
      s2w[j] = batch_downdate(s2w[j], g);
      if (live[j] && batch_same_point_cov(cov[j * m + j], cjp, cpp)) live[j] = 0;
    }
  }
  *n_picked = np;
  if (var_after)
    for (int64_t j = 0; j < m; ++j) var_after[j] = s2w[j];
  return 0;
}

}  // namespace gpso
