// cross_spectrum.hpp -- the cross-spectrum of two fields in measure_spectrum's bins (bchmc_measure_cross_spectrum).
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
#pragma once
#include "common.hpp"

namespace bchmc {

// ------------------------------------------------------------------------------------------------------
// k_spectrum (spectrum.hpp) over two half-complex transforms at once: the same bins -- (ULONG)(ktot / dk), IEEE sqrt and
// divide, no FMA contraction -- and the same Hermitian mode weights, both arrays read once.  Per bin the sums of |k|, of
// |A|^2, of |B|^2 and of Re(A conj B) = re_a re_b + im_a im_b, and the mode count.  (Im(A conj B) of a mode and of its
// conjugate partner cancel, so the weighted real part alone is the full-grid sum.)
// bins = [5][n_bin] doubles (ksum, paa, pbb, pab, count); LDS histogram per workgroup, one flush, with the float atomics
// of k_spectrum: the last bits depend on the order in which they land.
// ------------------------------------------------------------------------------------------------------
constexpr int kCrossSums = 5;

template <typename T>
__global__ void __launch_bounds__(256)
k_cross_spectrum(Geo g, const C2<T> *__restrict__ ak, const C2<T> *__restrict__ bk, int n_bin, double dk,
                 double *__restrict__ bins) {
#pragma clang fp contract(off)
  extern __shared__ double s_bins[];
  for (int b = threadIdx.x; b < kCrossSums * n_bin; b += blockDim.x) s_bins[b] = 0.;
  __syncthreads();
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < g.Nhp;
       idx += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(idx % g.nhp);
    if (k >= g.nh) continue;
    const long long ij = idx / g.nhp;
    const int j = (int)(ij % g.n), i = (int)(ij / g.n);
    const double kx = kval(i, g.n, g.kfac), ky = kval(j, g.n, g.kfac), kz = kval(k, g.n, g.kfac);
    const double ktot = sqrt(kx * kx + ky * ky + kz * kz);
    const unsigned long long nbin = (unsigned long long)(ktot / dk);
    if (nbin < (unsigned long long)n_bin) {
      const double hw = (k == 0 || ((g.n & 1) == 0 && k == g.n / 2)) ? 1. : 2.;
      const double2 a = ld2<T>(ak, idx), b = ld2<T>(bk, idx);
      atomic_add_r(&s_bins[nbin], hw * ktot);
      atomic_add_r(&s_bins[n_bin + nbin], hw * (a.x * a.x + a.y * a.y));
      atomic_add_r(&s_bins[2 * n_bin + nbin], hw * (b.x * b.x + b.y * b.y));
      atomic_add_r(&s_bins[3 * n_bin + nbin], hw * (a.x * b.x + a.y * b.y));
      atomic_add_r(&s_bins[4 * n_bin + nbin], hw);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kCrossSums * n_bin; b += blockDim.x)
    if (s_bins[b] != 0.) atomic_add_r(&bins[b], s_bins[b]);
}

}  // namespace bchmc
