// corr.hpp -- measure_corr_grid (tools/corr_fct.cc:20-80) and measure_corr2D (tools/2D_corr_fct.cc:23-124).
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
#pragma once
#include "common.hpp"

namespace bchmc {

// pacman_center_on_origin (pacman.cpp:66-71)
__host__ __device__ __forceinline__ double corr_pos(int ix, int n, double d) {
  return (ix <= n / 2) ? d * (double)ix : -d * (double)(n - ix);
}

// ------------------------------------------------------------------------------------------------------
// |x^|^2 * scale of a half-complex array into `out` (may be `xk` itself), imaginary part 0.  The row padding is
// processed like data.  With scale = 1 / N the C2R that follows gives A(r) = sum_x delta(x) delta(x + r).
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
k_corr_abs2(long long Nhp, const C2<T> *xk, C2<T> *out, double scale) {
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < Nhp;
       idx += (long long)gridDim.x * blockDim.x) {
    const double2 x = ld2<T>(xk, idx);
    st2<T>(out, idx, (x.x * x.x + x.y * x.y) * scale, 0.);
  }
}

// ------------------------------------------------------------------------------------------------------
// The 1-D function's bin sums.  The bin of a cell depends on all three indices, so every workgroup keeps an LDS
// histogram and flushes it once.  The accumulators are 64-bit INTEGERS: integer adds are associative, so the sums
// are the same bits whatever order the LDS and the flush atomics land in, on every handle.
//   GEOM  : out = [3][n_bin] { rtot high limb, rtot low limb, count }.  rtot * rscale (a power of two, exact) is an
//           integer below 2^63 -- every rtot is a multiple of ulp(d) and below 2 rmax -- so the two 31-bit-split limb
//           sums hold the EXACT sum of the bin's distances.
//   !GEOM : out = [2][n_bin] { A high limb, A low limb }, out[2 n_bin] = the scale.  A * 2^(59 - exponent of A(0))
//           truncated to an integer: |A(r)| <= A(0), so a term stays below 2^61 and loses at most 2^-59 of A(0).
// A high limb is below 2^32, a low one below 2^31: their sums over N <= 2^30 cells (n <= 1024) fit 63 bits.
// Compiled without FMA contraction so that rtot and the bin index are the reference's (x86-64, no FMA) numbers.
// ------------------------------------------------------------------------------------------------------
constexpr int kCorrLimb = 31;

template <typename T, bool GEOM>
__global__ void __launch_bounds__(256)
k_corr1d(Geo g, const T *__restrict__ A, int n_bin, double dr, double rscale, unsigned long long *__restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ unsigned long long s_hist[];
  const int nacc = (GEOM ? 3 : 2) * n_bin;
  for (int b = threadIdx.x; b < nacc; b += blockDim.x) s_hist[b] = 0ull;
  __syncthreads();
  // One lane works out the scale: 2^(59 - exponent of A(0)), the exponent clamped so that the power of two stays finite
  // for a subnormal A(0).  A(0) <= 0 (a zero field): 0, every sum is 0.  A(0) not finite: NaN, which the host turns
  // into NaN in every populated bin, as the host tool's sums would be.
  __shared__ double s_sc;
  if (!GEOM && threadIdx.x == 0) {
    const double a0 = (double)A[0];
    double v = 0.;
    if (!(a0 == a0) || a0 > 1.7e308 || a0 < -1.7e308) v = a0 - a0;  // NaN
    else if (a0 > 0.) v = ldexp(1., max(-960, min(960, 59 - ilogb(a0))));
    s_sc = v;
    if (blockIdx.x == 0) out[2 * n_bin] = (unsigned long long)__double_as_longlong(v);  // for the host
  }
  __syncthreads();
  const double sc = GEOM ? 0. : s_sc;
  const bool live = GEOM || sc > 0.;  // nothing to add for a zero or non-finite field
  const unsigned n = (unsigned)g.n, N = (unsigned)g.N;
  for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < N; idx += gridDim.x * blockDim.x) {
    const unsigned ij = idx / n;
    const int k = (int)(idx - ij * n), i = (int)(ij / n), j = (int)(ij - (ij / n) * n);
    const double x = corr_pos(i, g.n, g.d), y = corr_pos(j, g.n, g.d), z = corr_pos(k, g.n, g.d);
    const double rtot = sqrt(x * x + y * y + z * z);
    const unsigned long long nbin = (unsigned long long)(rtot / dr);
    if (live && nbin < (unsigned long long)n_bin) {
      if (GEOM) {
        const unsigned long long v = (unsigned long long)(rtot * rscale);
        atomicAdd(&s_hist[nbin], v >> kCorrLimb);
        atomicAdd(&s_hist[n_bin + nbin], v & ((1ull << kCorrLimb) - 1));
        atomicAdd(&s_hist[2 * n_bin + nbin], 1ull);
      } else {
        const long long v = (long long)((double)A[idx] * sc);
        atomicAdd(&s_hist[nbin], (unsigned long long)(v >> kCorrLimb));  // arithmetic shift: v = hi 2^31 + lo, lo >= 0
        atomicAdd(&s_hist[n_bin + nbin], (unsigned long long)(v & ((1ll << kCorrLimb) - 1)));
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nacc; b += blockDim.x)
    if (s_hist[b] != 0ull) atomicAdd(&out[b], s_hist[b]);
}

// ------------------------------------------------------------------------------------------------------
// The 2-D function's bin sums, without atomics.  nbin_perp belongs to a row (i, j), nbin_par to k, and z is the
// fastest axis: the host sorts the n^2 rows by perp bin (once per (n, n_bin)) and cuts every perp bin into slices of
// rows.  One workgroup per slice; thread t owns k = t + c * blockDim (c < KPT) and sums its k over the slice's rows in
// a register, every load a contiguous row.  Then k and n - k are folded through LDS, and one thread per populated par
// bin adds that bin's run of |z| in ascending order.  part[slice][c] = that sum, c = index of the populated par bin
// (par_start[c] .. par_start[c + 1] is its run of kk = min(k, n - k); nbin_par is monotone in kk).
//   GEOM: the summand is rtot = sqrt(x*x + y*y + z*z) of the cell instead of A (no FMA contraction, as above).
// ------------------------------------------------------------------------------------------------------
template <typename T, int KPT, bool GEOM>
__global__ void __launch_bounds__(256)
k_corr2d_slices(Geo g, const T *__restrict__ A, const int *__restrict__ rows, const int2 *__restrict__ slices,
                const int *__restrict__ par_start, int npb, double *__restrict__ part) {
#pragma clang fp contract(off)
  extern __shared__ double s_k[];  // n sums per k, then n / 2 + 1 folded ones
  const int n = g.n, t = threadIdx.x, bd = blockDim.x;
  const int2 sl = slices[blockIdx.x];  // { first row of the slice in `rows`, number of rows }
  double acc[KPT];
  double z2[KPT];
#pragma unroll
  for (int c = 0; c < KPT; c++) {
    acc[c] = 0.;
    const double z = corr_pos(min(t + c * bd, n - 1), n, g.d);
    z2[c] = z * z;
  }
#pragma unroll 4
  for (int r = 0; r < sl.y; r++) {
    const int row = rows[sl.x + r];
    if (GEOM) {
      const double x = corr_pos(row / n, n, g.d), y = corr_pos(row % n, n, g.d);
      const double r2 = x * x + y * y;
#pragma unroll
      for (int c = 0; c < KPT; c++) acc[c] += sqrt(r2 + z2[c]);
    } else {
      const T *a = A + (long long)row * n;
#pragma unroll
      for (int c = 0; c < KPT; c++) {
        const int k = t + c * bd;
        if (k < n) acc[c] += (double)a[k];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < KPT; c++) {
    const int k = t + c * bd;
    if (k < n) s_k[k] = acc[c];
  }
  __syncthreads();
  double *s_f = s_k + n;
  const int nf = n / 2 + 1;
  for (int kk = t; kk < nf; kk += bd) s_f[kk] = (kk > 0 && kk < n - kk) ? s_k[kk] + s_k[n - kk] : s_k[kk];
  __syncthreads();
  for (int c = t; c < npb; c += bd) {
    double v = 0.;
    for (int kk = par_start[c]; kk < par_start[c + 1]; kk++) v += s_f[kk];
    part[(long long)blockIdx.x * npb + c] = v;
  }
}

// out[p][c] = sum of part[s][c] over the slices s of perp bin p, in slice order (0 for a perp bin without rows)
__global__ void __launch_bounds__(256)
k_corr2d_reduce(const double *__restrict__ part, const int *__restrict__ perp_slice, int n_perp, int npb,
                double *__restrict__ out) {
  const long long total = (long long)n_perp * npb;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int p = (int)(idx / npb), c = (int)(idx - (long long)p * npb);
    double v = 0.;
    for (int s = perp_slice[p]; s < perp_slice[p + 1]; s++) v += part[(long long)s * npb + c];
    out[idx] = v;
  }
}

}  // namespace bchmc
