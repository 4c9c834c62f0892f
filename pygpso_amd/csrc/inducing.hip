// The gradient of the sparse models' objectives in the inducing points Z.  Every kernel here is
// stationary in r^2 = sum_d (z_d - x_d)^2 / l_d^2; with zs = Z / l, xs = X / l (the scaled rows the device holds), k' = dk/dr^2
// and an objective F whose weights are Wc = dF/dKuf [M x N] and the symmetric Wu = dF/dKuu [M x M]:
//   Vc = Wc (.) k'(Z, X),   Vu = 2 Wu (.) k'(Z, Z) with its diagonal := 0   (z_m sits in row m AND column m of Kuu)
//   dF/dZ[m, d] = (2 / l_d) (zs[m, d] (rowsum(Vc)[m] + rowsum(Vu)[m]) - (Vc xs)[m, d] - (Vu zs)[m, d])
// One pass over the 64 x 64 tiles of the weights forms V on the fly (r^2 regenerated from the scaled rows by direct
// differences, as sgpr_cross_grad_kernel does; no [M x N] intermediate is stored) and contracts it with the tile's scaled rows
// on the float64 matrix cores (v_mfma_f64_16x16x4_f64), V staged through LDS; a column of ones behind the D_pad inputs makes
// the same product deliver rowsum(V).  A workgroup owns a 64-row block of Z and walks a contiguous slice of the column
// tiles with its accumulators in registers; the slices' partial results (at most 16 slices from M_pad = 1024 on, up to 64
// below) are added in a fixed order by
// inducing_final_kernel (no atomics: a call repeated on the same inputs gives the same bits).
// COINCIDENT PAIRS: a pair with r^2 <= 1e-36 contributes zero, as in GPflow (sqrt(max(r^2, 1e-36)) and a zero difference).
// For the Matern-3/2, -5/2 and the squared exponential that is the exact derivative (k' is finite, z - x is 0); the
// Matern-1/2 has a kink there and 0 is the convention.
#include <algorithm>
#include <cmath>

#include "kernels.hpp"

namespace gpso {

namespace {

constexpr int kThreads = 256;
constexpr int kVStride = 65;  // V tile [64][65]: an odd stride (the MFMA's A operand reads 16 rows x 4 columns per wave)

// part[slice][row][0 .. dp - 1] = (V xs)[row][.], part[slice][row][dp] = rowsum(V)[row] over the slice's column tiles.
// kuu == 0:  W[i][j] = g[i * npad + j] + a[i] t[j]   (the form sgpr_cross_grad_kernel contracts with dKuf/dtheta)
// kuu != 0:  xs is zs, npad is mpad, W[i][j] = g[max(i, j) * mpad + min(i, j)] (the lower triangle, as grad_tile_kernel
//            reads it), the diagonal skipped; a and t are not read
// NB: 16-column blocks of the product, ceil((dp + 1) / 16)
template <int NB>
__global__ __launch_bounds__(kThreads) void inducing_contract_kernel(const double* __restrict__ g, const double* __restrict__ a,
                                                                     const double* __restrict__ t,
                                                                     const double* __restrict__ zs,
                                                                     const double* __restrict__ xs, int64_t m, int64_t mpad,
                                                                     int64_t n, int64_t npad, int dp, int kernel,
                                                                     double variance, int kuu, int tiles_per_slice,
                                                                     double* __restrict__ part) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int ds = dp | 1;
  double* zi = reinterpret_cast<double*>(lds_raw);  // [64][ds]
  double* xj = zi + 64 * ds;                        // [64][ds]
  double* vt = xj + 64 * ds;                        // [64][kVStride]
  const int64_t ti = blockIdx.y;
  const int slice = blockIdx.x;
  const int ntile = (int)(npad / 64);
  const int t0 = slice * tiles_per_slice;
  const int t1 = min(t0 + tiles_per_slice, ntile);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jj = lane, i0 = wave;
  f64x4 acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int e = threadIdx.x; e < 64 * dp; e += kThreads) {
    const int r = e / dp, c = e - r * dp;
    zi[r * ds + c] = (ti * 64 + r < mpad) ? zs[(ti * 64 + r) * dp + c] : 0.0;
  }
  for (int tj = t0; tj < t1; ++tj) {
    __syncthreads();  // (the previous tile's products have read xj and vt)
    for (int e = threadIdx.x; e < 64 * dp; e += kThreads) {
      const int r = e / dp, c = e - r * dp;
      xj[r * ds + c] = ((int64_t)tj * 64 + r < npad) ? xs[((int64_t)tj * 64 + r) * dp + c] : 0.0;
    }
    __syncthreads();
    double r2[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) r2[p] = 0.0;
    for (int k = 0; k < dp; ++k) {
      const double b = xj[jj * ds + k];
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        const double df = zi[(i0 + 4 * p) * ds + k] - b;
        r2[p] = fma(df, df, r2[p]);
      }
    }
    const int64_t j = (int64_t)tj * 64 + jj;
    const double tj_v = (!kuu && j < n) ? t[j] : 0.0;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int64_t i = ti * 64 + i0 + 4 * p;
      double v = 0.0;
      if (i < m && j < n && r2[p] > 1e-36 && !(kuu && i == j)) {
        const double W = kuu ? (i > j ? g[i * npad + j] : g[j * npad + i]) : g[i * npad + j] + a[i] * tj_v;
        double kv, dk;
        kern_and_dkern_same(kernel, r2[p], variance, kv, dk);
        v = W * dk;
      }
      vt[(i0 + 4 * p) * kVStride + jj] = v;
    }
    __syncthreads();
    // rows 16 wave .. 16 wave + 15 of the block: (V xs | rowsum V) += V[16 x 64] [xs | 1][64 x 16 NB], four columns of V a step
    const int ar = 16 * wave + (lane & 15), kq = lane >> 4;
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
      const double av = vt[ar * kVStride + 4 * kk + kq];
      const double* xr = xj + (4 * kk + kq) * ds;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int c = 16 * b + (lane & 15);
        const double xv = xr[c < dp ? c : dp - 1];
        const double bv = c < dp ? xv : (c == dp ? 1.0 : 0.0);
        acc[b] = Mfma<double>::mma(av, bv, acc[b]);
      }
    }
  }
  const int ps = dp + 1;
  double* out = part + ((int64_t)slice * mpad + ti * 64 + 16 * wave) * ps;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int c = 16 * b + (lane & 15);
    if (c > dp) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(int64_t)Mfma<double>::crow(lane, r) * ps + c] = acc[b][r];
  }
}

// grad_z[row * d + c] = (2 / ls[c]) (zs[row][c] (cc Sc + cu Su) - (cc Pc + cu Pu)), S the rowsum column and P the product
// columns of the cross (c: nslice slices, added left to right) and the Kuu (u: one slice) contraction
__global__ __launch_bounds__(kThreads) void inducing_final_kernel(const double* __restrict__ part_c, int nslice,
                                                                  const double* __restrict__ part_u,
                                                                  const double* __restrict__ zs,
                                                                  const double* __restrict__ ls, int64_t m, int64_t mpad,
                                                                  int d, int dp, double cc, double cu,
                                                                  double* __restrict__ grad_z) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * d) return;
  const int64_t row = idx / d;
  const int c = (int)(idx - row * d);
  const int ps = dp + 1;
  double sc = 0.0, pc = 0.0;
  for (int s = 0; s < nslice; ++s) {
    const double* p = part_c + ((int64_t)s * mpad + row) * ps;
    sc += p[dp];
    pc += p[c];
  }
  const double* pu = part_u + row * ps;
  grad_z[idx] = (2.0 / ls[c]) * (zs[row * dp + c] * (cc * sc + cu * pu[dp]) - (cc * pc + cu * pu[c]));
}

template <int NB>
int contract(hipStream_t st, const double* g, const double* a, const double* t, const double* zs, const double* xs, int64_t m,
             int64_t mpad, int64_t n, int64_t npad, int dp, const KernParams& kp, int kuu, int nslice, double* part) {
  const size_t lds = ((size_t)2 * 64 * (dp | 1) + (size_t)64 * kVStride) * sizeof(double);
  if (lds > 64 * 1024) {
    const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(&inducing_contract_kernel<NB>), (int)lds);
    if (rc) return rc;
  }
  const int ntile = (int)(npad / 64);
  const int tps = (ntile + nslice - 1) / nslice;
  hipLaunchKernelGGL((inducing_contract_kernel<NB>), dim3((unsigned)nslice, (unsigned)(mpad / 64)), dim3(kThreads), lds, st, g,
                     a, t, zs, xs, m, mpad, n, npad, dp, kp.kernel, kp.variance, kuu, tps, part);
  return 0;
}

int contract_nb(hipStream_t st, const double* g, const double* a, const double* t, const double* zs, const double* xs,
                int64_t m, int64_t mpad, int64_t n, int64_t npad, int dp, const KernParams& kp, int kuu, int nslice,
                double* part) {
  switch ((dp + 1 + 15) / 16) {
    case 1: return contract<1>(st, g, a, t, zs, xs, m, mpad, n, npad, dp, kp, kuu, nslice, part);
    case 2: return contract<2>(st, g, a, t, zs, xs, m, mpad, n, npad, dp, kp, kuu, nslice, part);
    case 3: return contract<3>(st, g, a, t, zs, xs, m, mpad, n, npad, dp, kp, kuu, nslice, part);
    default: return contract<4>(st, g, a, t, zs, xs, m, mpad, n, npad, dp, kp, kuu, nslice, part);
  }
}

}  // namespace

int inducing_slices(int64_t mpad, int64_t npad) {
  const int ntile = (int)(npad / 64), rows = (int)(mpad / 64);
  int ns = 1;
  // enough workgroups for the 256 compute units, no more (a slice without a tile still writes its zero partials).  From
  // M_pad = 1024 on at most kInducingSlicesLargeM slices; a smaller M_pad may take more, up to kInducingSlicesMax, as long
  // as its partials stay within the kInducingSlicesLargeM x 1024 rows of that case
  int cap = kInducingSlicesLargeM;
  if (mpad < 1024) cap = (int)std::min<int64_t>(kInducingSlicesMax, (int64_t)kInducingSlicesLargeM * 1024 / mpad);
  while (ns * 2 <= cap && ns * 2 <= ntile && rows * ns < 256) ns *= 2;
  return ns;
}

int launch_inducing_grad(hipStream_t st, const double* wc, const double* a, const double* t, const double* kin,
                         const double* zs, const double* xs, int64_t m, int64_t mpad, int64_t n, int64_t npad, int d, int dp,
                         const double* ls, const KernParams& kp, double cc, double cu, double* part, double* grad_z) {
  const int ns = inducing_slices(mpad, npad);
  double* part_u = part + (size_t)ns * mpad * (dp + 1);
  int rc = contract_nb(st, wc, a, t, zs, xs, m, mpad, n, npad, dp, kp, 0, ns, part);
  if (rc) return rc;
  if ((rc = contract_nb(st, kin, nullptr, nullptr, zs, zs, m, mpad, m, mpad, dp, kp, 1, 1, part_u))) return rc;
  const int64_t total = m * d;
  hipLaunchKernelGGL(inducing_final_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part,
                     ns, part_u, zs, ls, m, mpad, d, dp, cc, cu, grad_z);
  return 0;
}

}  // namespace gpso
