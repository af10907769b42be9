// poisson.hpp -- Poisson samples of a density field (bchmc_poisson_*, bchmc_setup_random_test_poisson): counts per cell, their scan, particle positions.
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
//
// discrete_poisson_sample (tools/poisson_upres.cc:23-65) and the Poissonian mock of setup_random_test
// (barcoderunner.cc:117-131) draw gsl_ran_poisson per cell from a serial stream, a data-dependent number of words each.
// Here the count of cell c is a pure function of (seed, stream, c, lambda_c): counter-based Philox4x32-10 uniforms in
// k_white_noise's convention, inversion by sequential search below lambda = 10 and Hoermann's PTRS (1993) from there on
// -- exact in distribution, not upstream's stream.  The sample itself is never stored: the handle keeps the exclusive
// scan off[0 .. N] of the counts, and particle p is recomputed wherever it is needed from the cell c with
// off[c] <= p < off[c + 1] and its index kk = p - off[c] in that cell (k_pois_positions).
//   * k_pois_counts: lambda, the count, the scan inside a workgroup of kPoisThreads cells and the workgroup's total;
//   * k_mock_scan / k_mt_scan (mock.hpp, mt_draw.hpp) scan the totals, as they scan the window's;
//   * k_pois_offsets adds the two levels back onto off.
#pragma once
#include "common.hpp"
#include "mt_draw.hpp"
#include "rng.hpp"

namespace bchmc {

constexpr int kPoisThreads = kMtThreads;  // cells per workgroup of k_pois_counts: one per thread
constexpr int kPoisInvCap = 256;          // steps of the sequential search (u can round to 1.0)
constexpr int kPoisPtrsCap = 64;          // iterations of the rejection loop
constexpr double kPoisLambdaMax = 1073741824.;  // 2^30: a count and an index inside a cell fit 32 bits

// words of the status block (unsigned long long each)
enum { kPoisBad = 0, kPoisDrawn = 1, kPoisMaxCount = 2, kPoisCapped = 3, kPoisLambdaBits = 4, kPoisWords = 5 };

// the 53-bit uniform of k_white_noise from two words
__device__ __forceinline__ double pois_u53(unsigned hi, unsigned lo) {
#pragma clang fp contract(off)
  return ((double)((((unsigned long long)hi << 32) | lo) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// The count of cell c at rate lam > 0.  All arithmetic in double, uncontracted, in the operand order of the header's
// description, so that the same lines in numpy float64 take the same decisions up to the last bits of exp / log / lgamma.
// A cell that runs into a cap returns the last candidate and sets `capped`.
__device__ __forceinline__ unsigned pois_count(double lam, unsigned long long c, unsigned stream, uint2 key, bool &capped) {
#pragma clang fp contract(off)
  const unsigned clo = (unsigned)c, chi = (unsigned)(c >> 32);
  capped = false;
  if (lam < 10.) {
    const uint4 r = philox4x32_10(make_uint4(clo, chi, 0u, 2u * stream), key);
    const double u = pois_u53(r.x, r.y);
    double p = exp(-lam), s = p;
    int k = 0;
    while (u > s && k < kPoisInvCap) {
      k++;
      p = p * lam / (double)k;
      s = s + p;
    }
    capped = k >= kPoisInvCap;
    return (unsigned)k;
  }
  const double b = 0.931 + 2.53 * sqrt(lam), a = -0.059 + 0.02483 * b;
  const double inv_alpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.);
  const double loglam = log(lam);
  double kf = 0.;
  for (int j = 0; j < kPoisPtrsCap; j++) {
    const uint4 r = philox4x32_10(make_uint4(clo, chi, (unsigned)j, 2u * stream), key);
    const double u = pois_u53(r.x, r.y), v = pois_u53(r.z, r.w);
    const double U = u - 0.5, us = 0.5 - fabs(U);
    kf = floor((2. * a / us + b) * U + lam + 0.43);
    if (us >= 0.07 && v <= vr) return (unsigned)kf;
    if (kf < 0. || (us < 0.013 && v > us)) continue;
    const double lhs = log(v) + log(inv_alpha) - log(a / (us * us) + b);
    const double rhs = -lam + kf * loglam - lgamma(kf + 1.);
    if (lhs <= rhs) return (unsigned)kf;
  }
  capped = true;
  return kf > 0. ? (unsigned)kf : 0u;
}

__device__ __forceinline__ unsigned long long pois_wave_max(unsigned long long v) {
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(v, off, kWave);
    v = o > v ? o : v;
  }
  return v;  // lane 0 holds the wave's
}

// One cell per thread.  lambda = scale (1 + x) (rate_mode 0) or scale x (1) from x in its storage type U, widened; a
// cell whose window (W, may be null) is not > 0 draws nothing.  cd (may be null): the counts as doubles.  off (may be
// null, with cnt): off[c] = counts before c inside its workgroup, cnt[workgroup] = the workgroup's total.
// stat: kPoisBad = smallest index of a cell whose lambda is NaN, +infinity or above 2^30 (atomicMin, as k_mock_noise's
// noise == 0), the others sums and maxima over the cells that drew (lambda_max as the bits of a positive double, which
// order like the doubles).
template <typename U, typename W>
__global__ void __launch_bounds__(kPoisThreads)
k_pois_counts(long long N, uint2 key, unsigned stream, int rate_mode, double scale, const U *__restrict__ x,
              const W *__restrict__ window, double *__restrict__ cd, unsigned long long *__restrict__ off,
              unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ stat) {
#pragma clang fp contract(off)
  const long long c = (long long)blockIdx.x * kPoisThreads + threadIdx.x;
  unsigned long long k = 0, lam_bits = 0;
  bool drew = false, capped = false;
  if (c < N && (!window || (double)window[c] > 0.)) {
    const double xv = (double)x[c];
    const double lam = rate_mode == 0 ? scale * (1. + xv) : scale * xv;
    if (!(lam <= kPoisLambdaMax)) {
      atomicMin(stat + kPoisBad, (unsigned long long)c);
    } else if (lam > 0.) {
      drew = true;
      k = pois_count(lam, (unsigned long long)c, stream, key, capped);
      lam_bits = (unsigned long long)__double_as_longlong(lam);
    }
  }
  if (c < N && cd) cd[c] = (double)k;
  // the statistics: reduced per wave, then per workgroup in LDS, then one global atomic per workgroup and word (a
  // million waves adding to the same four addresses cost a hundred times the kernel's memory traffic)
  __shared__ unsigned long long s_stat[4];
  if (threadIdx.x < 4) s_stat[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long nd = __popcll(__ballot(drew)), nc = __popcll(__ballot(capped));
  const unsigned long long mk = pois_wave_max(k), ml = pois_wave_max(lam_bits);
  if ((threadIdx.x & (kWave - 1)) == 0 && nd) {
    atomicAdd(&s_stat[0], nd);
    atomicMax(&s_stat[1], mk);
    atomicMax(&s_stat[2], ml);
    if (nc) atomicAdd(&s_stat[3], nc);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_stat[0]) {
    atomicAdd(stat + kPoisDrawn, s_stat[0]);
    atomicMax(stat + kPoisMaxCount, s_stat[1]);
    atomicMax(stat + kPoisLambdaBits, s_stat[2]);
    if (s_stat[3]) atomicAdd(stat + kPoisCapped, s_stat[3]);
  }
  unsigned long long ex;
  const unsigned long long tot = mt_block_scan(k, &ex);
  if (off) {
    if (c < N) off[c] = ex;
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
  }
}

// off[c] += counts of the workgroups before c's: boff within its group of kMtThreads workgroups (k_mock_scan), goff of
// the groups before (k_mt_scan, which left the total in res[0]); off[N] = the total.
__global__ void __launch_bounds__(kPoisThreads)
k_pois_offsets(long long N, const unsigned long long *__restrict__ boff, const unsigned long long *__restrict__ goff,
               const unsigned long long *__restrict__ res, unsigned long long *__restrict__ off) {
  const long long c = (long long)blockIdx.x * kPoisThreads + threadIdx.x;
  if (c < N) off[c] += goff[blockIdx.x / kMtThreads] + boff[blockIdx.x];
  if (c == N - 1) off[N] = res[0];
}

// The cell of particle p among cells lo .. hi: the largest c with off[c] <= p (off[lo] <= p is the caller's).  off is
// non-decreasing and an empty cell repeats its successor's offset, so the search steps over runs of empty cells and
// ends on the cell with off[c] <= p < off[c + 1].  Reads off[lo + 1 .. hi] only.
__device__ __forceinline__ long long pois_cell(const unsigned long long *__restrict__ off, long long lo, long long hi,
                                               unsigned long long p) {
  while (lo < hi) {
    const long long mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Particles first .. first + m - 1 of the sample (first + m <= off[N], m >= 1), one thread each, upstream's order: cells
// in order, kk within a cell.  discrete_poisson_sample's position (:52-58) with gsl_rng_uniform's 32-bit resolution,
// w = philox4x32_10((c_lo, c_hi, kk, 2 stream + 1), seed): x = d_in i + (w.x 2^-32) d_in, uncontracted, in box
// coordinates.  A workgroup first narrows the search to the cells of its own first and last particle.
__global__ void __launch_bounds__(256)
k_pois_positions(long long N, int n, double d_in, uint2 key, unsigned stream, const unsigned long long *__restrict__ off,
                 unsigned long long first, int m, double *__restrict__ x, double *__restrict__ y, double *__restrict__ z) {
#pragma clang fp contract(off)
  __shared__ long long s_cell[2];
  const int b0 = blockIdx.x * 256;  // < m: the grid is ceil(m / 256)
  if ((threadIdx.x & (kWave - 1)) == 0 && threadIdx.x < 2 * kWave) {  // lane 0 of the first two waves: one search each
    const int which = (int)threadIdx.x / kWave;
    const int bl = which == 0 ? b0 : (b0 + 255 < m ? b0 + 255 : m - 1);
    s_cell[which] = pois_cell(off, 0, N - 1, first + (unsigned long long)bl);
  }
  __syncthreads();
  const int b = b0 + (int)threadIdx.x;
  if (b >= m) return;
  const unsigned long long p = first + (unsigned long long)b;
  const long long c = pois_cell(off, s_cell[0], s_cell[1], p);
  const unsigned kk = (unsigned)(p - off[c]);
  const int k = (int)(c % n);
  const long long ij = c / n;
  const int j = (int)(ij % n), i = (int)(ij / n);
  const uint4 w = philox4x32_10(make_uint4((unsigned)c, (unsigned)((unsigned long long)c >> 32), kk, 2u * stream + 1u), key);
  const double r32 = 1.0 / 4294967296.0;
  x[b] = d_in * (double)i + ((double)w.x * r32) * d_in;
  y[b] = d_in * (double)j + ((double)w.y * r32) * d_in;
  z[b] = d_in * (double)k + ((double)w.z * r32) * d_in;
}

}  // namespace bchmc
