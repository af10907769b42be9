// ensemble.hpp -- running mean and variance of an ensemble of fields (bchmc_ensemble_*): Welford's update for one more
// sample, Chan, Golub & LeVeque's pairwise update for another accumulator, and the variance / standard deviation.
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
#pragma once
#include "common.hpp"

namespace bchmc {

// ------------------------------------------------------------------------------------------------------
// A slot is two dense arrays of N doubles, mean and m2 (the sum of squared deviations from the mean), in the cell order
// of the real-space fields, on fp32 handles too.  Every kernel is one pass over them and nothing else: 40 bytes per cell
// for an update from a double source (8 read + 16 read + 16 written), 48 for a merge.  A thread takes two neighbouring
// cells per trip, so mean and m2 move in 16-byte accesses; the grid is sized to the device (ens_blocks) and strides over
// the pairs; an odd N leaves one cell, which thread 0 takes as scalars.
// The arithmetic is the caller's contract (include/bchmc.h): double, no FMA contraction, IEEE divide and sqrt, the
// operand order written out below, so that a numpy restatement of the same lines gives the same bits.
// mean and m2 are read once and written once per call and are larger than the caches at the sizes that matter:
// BCHMC_NT_ENSEMBLE = 1 gives their accesses and the source's loads the `nt` hint, 0 builds plain ones (both measured
// in DESIGN 9.9).
// ------------------------------------------------------------------------------------------------------
#ifndef BCHMC_NT_ENSEMBLE
#define BCHMC_NT_ENSEMBLE 1
#endif
constexpr int kEnsBlock = 256;
constexpr int kEnsBlocksPerCu = 8;

typedef double ens_dv2 __attribute__((ext_vector_type(2)));
typedef float ens_fv2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ ens_dv2 ens_ld2(const double *p) {
  return stream_load<BCHMC_NT_ENSEMBLE != 0>(reinterpret_cast<const ens_dv2 *>(p));
}
__device__ __forceinline__ ens_dv2 ens_ld2(const float *p) {  // an fp32 source is widened on load
  const ens_fv2 t = stream_load<BCHMC_NT_ENSEMBLE != 0>(reinterpret_cast<const ens_fv2 *>(p));
  ens_dv2 r;
  r.x = (double)t.x, r.y = (double)t.y;
  return r;
}
__device__ __forceinline__ void ens_st2(double *p, ens_dv2 v) {
  stream_store<BCHMC_NT_ENSEMBLE != 0>(reinterpret_cast<ens_dv2 *>(p), v);
}

// One Welford step of one cell, c = (double)(count + 1).  A sample that is not finite makes the cell NaN for good
// (x - x is NaN exactly then); no other cell sees it.
__device__ __forceinline__ void ens_welford(double x, double c, double &mean, double &m2) {
#pragma clang fp contract(off)
  const double d = x - mean;
  mean = mean + d / c;
  m2 = m2 + d * (x - mean);
  const double bad = x - x;
  if (bad != 0.) mean = bad, m2 = bad;
}

template <typename S>
__global__ void __launch_bounds__(kEnsBlock)
k_ens_add(long long N, const S *__restrict__ x, double *__restrict__ mean, double *__restrict__ m2, double c) {
  const long long pairs = N >> 1, stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (long long p = t0; p < pairs; p += stride) {
    const ens_dv2 xv = ens_ld2(x + 2 * p);
    ens_dv2 mv = ens_ld2(mean + 2 * p), sv = ens_ld2(m2 + 2 * p);
    double m0 = mv.x, m1 = mv.y, s0 = sv.x, s1 = sv.y;
    ens_welford(xv.x, c, m0, s0);
    ens_welford(xv.y, c, m1, s1);
    mv.x = m0, mv.y = m1, sv.x = s0, sv.y = s1;
    ens_st2(mean + 2 * p, mv);
    ens_st2(m2 + 2 * p, sv);
  }
  if (t0 == 0 && (N & 1)) {  // the last cell of an odd grid
    const long long i = N - 1;
    double m = mean[i], s = m2[i];
    ens_welford((double)x[i], c, m, s);
    mean[i] = m, m2[i] = s;
  }
}

// The pairwise update with another accumulator (mean_b, m2_b) of nb samples into one of na:
// w = nb / (na + nb), c = na nb / (na + nb), both formed on the host.
__device__ __forceinline__ void ens_chan(double mean_b, double m2_b, double w, double c, double &mean, double &m2) {
#pragma clang fp contract(off)
  const double d = mean_b - mean;
  mean = mean + d * w;
  m2 = (m2 + m2_b) + (d * d) * c;
}

// mean_b and m2_b are staged one behind the other, so the second starts at an odd element on an odd grid: they are
// read as scalars, two per thread and trip (a wave still reads whole lines).
__global__ void __launch_bounds__(kEnsBlock)
k_ens_merge(long long N, const double *__restrict__ mean_b, const double *__restrict__ m2_b, double *__restrict__ mean,
            double *__restrict__ m2, double w, double c) {
  const long long pairs = N >> 1, stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (long long p = t0; p < pairs; p += stride) {
    const double b0 = stream_load<BCHMC_NT_ENSEMBLE != 0>(mean_b + 2 * p), b1 = stream_load<BCHMC_NT_ENSEMBLE != 0>(mean_b + 2 * p + 1);
    const double q0 = stream_load<BCHMC_NT_ENSEMBLE != 0>(m2_b + 2 * p), q1 = stream_load<BCHMC_NT_ENSEMBLE != 0>(m2_b + 2 * p + 1);
    ens_dv2 mv = ens_ld2(mean + 2 * p), sv = ens_ld2(m2 + 2 * p);
    double m0 = mv.x, m1 = mv.y, s0 = sv.x, s1 = sv.y;
    ens_chan(b0, q0, w, c, m0, s0);
    ens_chan(b1, q1, w, c, m1, s1);
    mv.x = m0, mv.y = m1, sv.x = s0, sv.y = s1;
    ens_st2(mean + 2 * p, mv);
    ens_st2(m2 + 2 * p, sv);
  }
  if (t0 == 0 && (N & 1)) {
    const long long i = N - 1;
    double m = mean[i], s = m2[i];
    ens_chan(mean_b[i], m2_b[i], w, c, m, s);
    mean[i] = m, m2[i] = s;
  }
}

// out = m2 / cm1 (the variance, cm1 = (double)(count - 1)) or its square root; m2 is left as it is and will be read
// again, so its loads are plain.
template <bool STD>
__global__ void __launch_bounds__(kEnsBlock)
k_ens_moment(long long N, const double *__restrict__ m2, double *__restrict__ out, double cm1) {
#pragma clang fp contract(off)
  const long long pairs = N >> 1, stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (long long p = t0; p < pairs; p += stride) {
    ens_dv2 v = *reinterpret_cast<const ens_dv2 *>(m2 + 2 * p);
    v.x = v.x / cm1, v.y = v.y / cm1;
    if (STD) v.x = sqrt(v.x), v.y = sqrt(v.y);
    *reinterpret_cast<ens_dv2 *>(out + 2 * p) = v;
  }
  if (t0 == 0 && (N & 1)) {
    const double v = m2[N - 1] / cm1;
    out[N - 1] = STD ? sqrt(v) : v;
  }
}

}  // namespace bchmc
