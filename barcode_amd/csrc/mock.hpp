// mock.hpp -- setup_random_test / make_initial_guess (barcoderunner.cc:42-247) on the device.
//
// The reference makes the random test's mock data from the SAME serial gsl_rng the chain later draws its momenta from:
// 2 N Gaussians for the truth field (create_GARFIELD), then one gsl_ran_gaussian(sigma_i) per cell with window > 0, in
// cell order.  mt_draw.hpp delivers the g-th Gaussian of the stream; what this header adds is the map cell -> g:
//   * k_mock_window: the window from delta_eul, and how many windowed cells each tile of kMockTile cells holds;
//   * k_mock_scan: exclusive scan of those counts, one workgroup per 1024 tiles (k_mt_scan then scans the workgroup
//     totals), so that rank(cell) = goff[tile / 1024] + off[tile] + (windowed cells before it in its tile);
//   * k_mock_noise: Lambda, sigma, nobs, noise and the clamp of every cell, reading Gaussian rank(cell) in the split form
//     (y, sqrt(-2 log r2 / r2)) of k_mt_pairs<true, true>: gsl_ran_gaussian returns sigma * y * root, products in that
//     order, which sigma * (y * root) misses by an ulp when sigma != 1.
// Plus the initial guesses that need the stream (k_mock_guess_noise) and the smoothed one (k_mock_smooth).
#pragma once
#include "common.hpp"
#include "mt_draw.hpp"

namespace bchmc {

constexpr int kMockThreads = 256;
constexpr int kMockTile = 4 * kMockThreads;  // cells per workgroup: 4 consecutive ones per thread

struct MockPar {
  int window_type, data_model, likelihood, negative_obs;
  double sigma_min, sigma_fac, rho_c, delta_min;
};

// a[p .. p+4) of an N-element array; `vec`: a + p is 16-byte aligned and p + 4 <= N (two 16-byte loads)
__device__ __forceinline__ void mock_ld4(const double *__restrict__ a, long long p, long long N, bool vec, double v[4]) {
  if (vec) {
    const double2 lo = *reinterpret_cast<const double2 *>(a + p), hi = *reinterpret_cast<const double2 *>(a + p + 2);
    v[0] = lo.x, v[1] = lo.y, v[2] = hi.x, v[3] = hi.y;
  } else {
    for (int q = 0; q < 4; q++) v[q] = p + q < N ? a[p + q] : 0.;
  }
}
__device__ __forceinline__ void mock_ld4(const float *__restrict__ a, long long p, long long N, bool vec, double v[4]) {
  if (vec) {
    const float4 x = *reinterpret_cast<const float4 *>(a + p);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
  } else {
    for (int q = 0; q < 4; q++) v[q] = p + q < N ? (double)a[p + q] : 0.;
  }
}
__device__ __forceinline__ void mock_st4(double *__restrict__ a, long long p, long long N, bool vec, const double v[4]) {
  if (vec) {
    *reinterpret_cast<double2 *>(a + p) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2 *>(a + p + 2) = make_double2(v[2], v[3]);
  } else {
    for (int q = 0; q < 4; q++)
      if (p + q < N) a[p + q] = v[q];
  }
}
__device__ __forceinline__ void mock_st4(float *__restrict__ a, long long p, long long N, bool vec, const double v[4]) {
  if (vec) {
    *reinterpret_cast<float4 *>(a + p) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  } else {
    for (int q = 0; q < 4; q++)
      if (p + q < N) a[p + q] = (float)v[q];
  }
}
template <typename U>
__device__ __forceinline__ bool mock_vec_ok(const U *a, long long p, long long N) {
  return p + 4 <= N && (reinterpret_cast<uintptr_t>(a + p) & 15) == 0;
}

// Exclusive scan of v over the kMockThreads threads of a workgroup; returns the total (all threads).
__device__ __forceinline__ unsigned mock_block_scan(unsigned v, unsigned *excl) {
  __shared__ unsigned wsum[kMockThreads / kWave];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  unsigned inc = v;
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned o = __shfl_up(inc, off, kWave);
    if (lane >= off) inc += o;
  }
  if (lane == kWave - 1) wsum[wv] = inc;
  __syncthreads();
  unsigned before = 0, total = 0;
  for (int i = 0; i < kMockThreads / kWave; i++) {
    const unsigned s = wsum[i];
    if (i < wv) before += s;
    total += s;
  }
  __syncthreads();
  *excl = before + inc - v;
  return total;
}

// The window of barcoderunner.cc:91-113 from delta_eul, and cnt[tile] = its cells with window > 0.
// Type 1: ones.  Type 10: zeros in the first N / 2 cells, ones after.  Type 23: one where delta_eul > 3, else zero
// (upstream's code; its comment says the opposite).
template <typename T>
__global__ void __launch_bounds__(kMockThreads)
k_mock_window(long long N, int window_type, const double *__restrict__ deul, T *__restrict__ window,
              unsigned long long *__restrict__ cnt) {
  const long long p = (long long)blockIdx.x * kMockTile + 4 * (long long)threadIdx.x;
  double w[4] = {0., 0., 0., 0.};
  unsigned c = 0;
  if (p < N) {
    if (window_type == 23) {
      double d[4];
      mock_ld4(deul, p, N, mock_vec_ok(deul, p, N), d);
      for (int q = 0; q < 4; q++) w[q] = d[q] > 3 ? 1. : 0.;
    } else {
      for (int q = 0; q < 4; q++) w[q] = (window_type == 10 && p + q < N / 2) ? 0. : 1.;
    }
    for (int q = 0; q < 4; q++) c += (p + q < N && w[q] > 0.);
    mock_st4(window, p, N, mock_vec_ok(window, p, N), w);
  }
  unsigned ex;
  const unsigned tot = mock_block_scan(c, &ex);
  if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

// off[i] = sum of cnt[b 1024 .. i) for i in workgroup b's 1024 entries, gsum[b] = that group's total.
__global__ void __launch_bounds__(kMtThreads)
k_mock_scan(const unsigned long long *__restrict__ cnt, long long n, unsigned long long *__restrict__ off,
            unsigned long long *__restrict__ gsum) {
  const long long i = (long long)blockIdx.x * kMtThreads + threadIdx.x;
  unsigned long long ex;
  const unsigned long long tot = mt_block_scan(i < n ? cnt[i] : 0ull, &ex);
  if (i < n) off[i] = ex;
  if (threadIdx.x == 0) gsum[blockIdx.x] = tot;
}

// gsl_ran_gaussian(r, sigma) = sigma * y * sqrt(-2 log r2 / r2) from the split pair, no contraction
__device__ __forceinline__ double mock_gaussian(double sigma, double2 yr) {
#pragma clang fp contract(off)
  return sigma * yr.x * yr.y;
}

// nobs and noise of barcoderunner.cc:117-188 for every cell; the Gaussian of a windowed cell is number rank(cell) of
// the split stream gs.  res[1] = smallest index of a windowed cell with noise == 0 (likelihoods 1 and 3, :190-198).
// Upstream leaves noise_sf of an unwindowed cell unwritten; here it is 0.
template <typename T>
__global__ void __launch_bounds__(kMockThreads)
k_mock_noise(long long N, MockPar mp, const double *__restrict__ dlag, const double *__restrict__ deul,
             const T *__restrict__ window, const unsigned long long *__restrict__ off,
             const unsigned long long *__restrict__ goff, const double2 *__restrict__ gs, T *__restrict__ nobs,
             T *__restrict__ noise, unsigned long long *__restrict__ res) {
#pragma clang fp contract(off)
  const long long p = (long long)blockIdx.x * kMockTile + 4 * (long long)threadIdx.x;
  double w[4] = {0., 0., 0., 0.}, de[4] = {0., 0., 0., 0.}, dl[4] = {0., 0., 0., 0.};
  unsigned c = 0;
  if (p < N) {
    mock_ld4(window, p, N, mock_vec_ok(window, p, N), w);
    mock_ld4(deul, p, N, mock_vec_ok(deul, p, N), de);
    if (mp.likelihood == 3) mock_ld4(dlag, p, N, mock_vec_ok(dlag, p, N), dl);
    for (int q = 0; q < 4; q++) c += (p + q < N && w[q] > 0.);
  }
  unsigned ex;
  mock_block_scan(c, &ex);
  if (p >= N) return;
  unsigned long long r = goff[blockIdx.x / kMtThreads] + off[blockIdx.x] + ex;
  double no[4], sg[4];
  for (int q = 0; q < 4; q++) {
    const bool in = p + q < N && w[q] > 0.;
    double sigma = 0., v;
    if (mp.data_model == 0) {
      const double Lambda = mp.rho_c * (1. + de[q]);
      v = 0.;
      if (in) {
        if (mp.likelihood == 1) {
          sigma = mp.sigma_min + mp.sigma_fac * Lambda;
          v = Lambda + mock_gaussian(sigma, gs[r]);
          if (!mp.negative_obs && v < 0) v = 0;
        } else {  // GRF
          sigma = mp.sigma_min + mp.sigma_fac * (dl[q] * dl[q]);
          v = dl[q] + mock_gaussian(sigma, gs[r]);
        }
      }
    } else {
      double dx = de[q];  // lognormal_likelihood_f_delta_x_i_calc, lognormal_independent.cpp:57-64
      if (dx < mp.delta_min) dx = mp.delta_min;
      const double Lambda = log(mp.rho_c * (1. + dx));
      if (in) {
        sigma = mp.sigma_fac;
        v = Lambda + mock_gaussian(sigma, gs[r]);
      } else {
        const double b = mp.rho_c * (1 + mp.delta_min);
        v = log(b * b);
      }
    }
    if (in) {
      r++;
      if ((mp.likelihood == 1 || mp.likelihood == 3) && sigma == 0.) atomicMin(res + 1, (unsigned long long)(p + q));
    }
    no[q] = v, sg[q] = sigma;
  }
  mock_st4(nobs, p, N, mock_vec_ok(nobs, p, N), no);
  mock_st4(noise, p, N, mock_vec_ok(noise, p, N), sg);
}

// initial_guess 4 (barcoderunner.cc:232-240): out[i] = 0 + gsl_ran_gaussian(r, sigma), cells in order
__global__ void __launch_bounds__(kMockThreads)
k_mock_guess_noise(long long N, double sigma, const double2 *__restrict__ gs, double *__restrict__ out) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x)
    out[i] = 0. + mock_gaussian(sigma, gs[i]);
}

// initial_guess 3: kernelcomp(smol, filtertype 1) o convcomp as one k-space multiply, K = exp(-k^2 smol^2 / 2) / wtot
// (convolution.cpp:224-377; the same table k_alpt_kernel_table tabulates)
template <typename T>
__global__ void __launch_bounds__(256) k_mock_smooth(Geo g, C2<T> *__restrict__ xk, double smol, double inv_wtot) {
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < g.Nhp;
       idx += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(idx % g.nhp);
    const long long ij = idx / g.nhp;
    const int j = (int)(ij % g.n), i = (int)(ij / g.n);
    const double kx = kval(i, g.n, g.kfac), ky = kval(j, g.n, g.kfac), kz = kval(k, g.n, g.kfac);
    const double K = exp(-(kx * kx + ky * ky + kz * kz) * smol * smol / 2.) * inv_wtot;
    const double2 v = ld2<T>(xk, idx);
    st2<T>(xk, idx, K * v.x, K * v.y);
  }
}

}  // namespace bchmc
