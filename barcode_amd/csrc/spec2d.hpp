// spec2d.hpp -- measure_spec2D (tools/2D_powspec.cc:25-110): the anisotropic power spectrum P(k_perp, k_par).
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
#pragma once
#include "common.hpp"

namespace bchmc {

// ------------------------------------------------------------------------------------------------------
// The tool bins every mode (i, j, k) of the full complex grid by nbin_perp = (ULONG)(sqrt(kx*kx + ky*ky) / dk) and
// nbin_par = (ULONG)(sqrt(kz*kz) / dk), line of sight = z, and sums ktot = sqrt(kx*kx + ky*ky + kz*kz), |x^|^2 and 1
// into element nbin_par + n_bin * nbin_perp.  A mode and its conjugate partner (-i, -j, -k) share all three numbers,
// so on the half-complex array the sum with the Hermitian weight hw(k) -- 1 for k = 0 and for the Nyquist column of an
// even n, 2 otherwise -- is the full-grid sum bin by bin.
//
// Without atomics, like the 2-D correlation function (corr.hpp): nbin_perp belongs to a row (i, j), nbin_par to k, and
// k is the fastest axis.  The host sorts the n^2 rows by perp bin (once per (n, n_bin)) and cuts every perp bin into
// slices of rows.  The grid is (slice, chunk of kSpecChunk columns): lane l of every wave owns column
// k = chunk * kSpecChunk + l, the kSpecWaves waves of the workgroup share the slice's rows (wave w takes rows w,
// w + kSpecWaves, ...), every load of a wave is one contiguous row segment, and every thread keeps ONE running double
// sum.  The waves' sums are added through LDS in wave order: part[slice][k], k < nh.  The row padding k >= nh is never
// loaded (the idle lanes of the last chunk read column nh - 1 again and their sums are dropped).  Every order is fixed by the indices alone, so the result does not depend on scheduling.
// The sums are formed in double from the loaded pair, on fp32 handles too.
//   GEOM: the summand is ktot of the mode instead of |x^|^2, in the tool's operand order, IEEE sqrt, no FMA contraction
//         (the whole kernel is compiled without it, which also makes |x^|^2 = re*re + im*im one fixed expression).
// The array is read once per call and is larger than the caches at the sizes that matter, so the loads carry the `nt`
// hint (BCHMC_NT_SPEC2D = 0 builds without it; both measured in DESIGN 9.6).
// ------------------------------------------------------------------------------------------------------
constexpr int kSpecChunk = kWave;  // columns per workgroup: one per lane
constexpr int kSpecWaves = 4;      // waves per workgroup, sharing the slice's rows
constexpr int kSpecUnroll = 4;     // row segments a wave has in flight

#ifndef BCHMC_NT_SPEC2D
#define BCHMC_NT_SPEC2D 1
#endif
typedef double spec_dv2 __attribute__((ext_vector_type(2)));
typedef float spec_fv2 __attribute__((ext_vector_type(2)));
// one complex element as a pair of doubles
__device__ __forceinline__ double2 spec_load(const double2 *p) {
  const spec_dv2 t = stream_load<BCHMC_NT_SPEC2D != 0>(reinterpret_cast<const spec_dv2 *>(p));
  return make_double2(t.x, t.y);
}
__device__ __forceinline__ double2 spec_load(const float2 *p) {
  const spec_fv2 t = stream_load<BCHMC_NT_SPEC2D != 0>(reinterpret_cast<const spec_fv2 *>(p));
  return make_double2((double)t.x, (double)t.y);
}

template <typename T, bool GEOM>
__global__ void __launch_bounds__(kSpecChunk * kSpecWaves)
k_spec2d_slices(Geo g, const C2<T> *__restrict__ xk, const int *__restrict__ rows, const int2 *__restrict__ slices,
                double *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double s_w[kSpecWaves][kSpecChunk];
  const int lane = threadIdx.x % kSpecChunk;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kSpecChunk);  // wave-uniform: the row indices are scalar loads
  const int k = blockIdx.y * kSpecChunk + lane;
  const bool live = k < g.nh;  // false in the last chunk's tail: such a lane reads column nh - 1 again and stores nothing
  const int kc = min(k, g.nh - 1);
  const int2 sl = slices[blockIdx.x];  // { first row of the slice in `rows`, number of rows }
  const int *my = rows + sl.x;
  const double kz = kval(kc, g.n, g.kfac);
  // the summand of row `row` at this thread's column
  auto term = [&](int row) -> double {
    if (GEOM) {
      const double kx = kval(row / g.n, g.n, g.kfac), ky = kval(row % g.n, g.n, g.kfac);
      return sqrt(kx * kx + ky * ky + kz * kz);
    }
    const double2 v = spec_load(xk + ((long long)row * g.nhp + kc));
    return v.x * v.x + v.y * v.y;
  };
  // rows w, w + kSpecWaves, ... in this order; kSpecUnroll of them are loaded before the first is added
  double acc = 0.;
  int r = w;
  for (; r + (kSpecUnroll - 1) * kSpecWaves < sl.y; r += kSpecUnroll * kSpecWaves) {
    double t[kSpecUnroll];
#pragma unroll
    for (int u = 0; u < kSpecUnroll; u++) t[u] = term(my[r + u * kSpecWaves]);
#pragma unroll
    for (int u = 0; u < kSpecUnroll; u++) acc += t[u];
  }
  for (; r < sl.y; r += kSpecWaves) acc += term(my[r]);
  s_w[w][lane] = acc;
  __syncthreads();
  if (w == 0 && live) {
    double v = s_w[0][lane];
#pragma unroll
    for (int u = 1; u < kSpecWaves; u++) v += s_w[u][lane];
    part[(long long)blockIdx.x * g.nh + k] = v;
  }
}

// out[p][c] = sum over the run of k of populated par bin c, in ascending k, of hw(k) * (sum of part[s][k] over the slices
// s of perp bin p, in slice order); 0 for a perp bin without rows.  One workgroup per perp bin, the column sums in LDS
// (nh doubles).  par_start[c] .. par_start[c + 1] is the run of k of par bin c: sqrt(kz*kz) grows with k <= n / 2, so
// every par bin is one run.  There is no k <-> n - k fold as in k_corr2d_slices: the half-complex array holds k <= n / 2
// only, and hw takes its place.
__global__ void __launch_bounds__(256)
k_spec2d_reduce(int n, int nh, const double *__restrict__ part, const int *__restrict__ perp_slice,
                const int *__restrict__ par_start, int npb, double *__restrict__ out) {
  extern __shared__ double s_col[];
  const int p = blockIdx.x, s0 = perp_slice[p], s1 = perp_slice[p + 1];
  for (int k = threadIdx.x; k < nh; k += blockDim.x) {
    double v = 0.;
#pragma unroll 8
    for (int s = s0; s < s1; s++) v += part[(long long)s * nh + k];
    const double hw = (k == 0 || ((n & 1) == 0 && k == n / 2)) ? 1. : 2.;
    s_col[k] = hw * v;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < npb; c += blockDim.x) {
    double v = 0.;
    for (int k = par_start[c]; k < par_start[c + 1]; k++) v += s_col[k];
    out[(long long)p * npb + c] = v;
  }
}

}  // namespace bchmc
