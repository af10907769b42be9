// multipoles.hpp -- the Legendre multipoles about the line of sight z of a sample: P_l(k) in measure_spectrum's bins and
// xi_l(s) in measure_corr_grid's, l = 0, 2, 4 (upstream: none; computed there from dumped fields).
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
#pragma once
#include "common.hpp"
#include "corr.hpp"
#include "spec2d.hpp"

namespace bchmc {

// ------------------------------------------------------------------------------------------------------
// Both forms bin an element (i, j, k) of a grid by t = sqrt(x*x + y*y + z*z) and weigh it by L_l(mu), mu^2 = z*z / t^2:
// (x, y, z) = kval of the indices on the half-complex transform, pacman_center_on_origin of them on the real grid A(r).
// Either coordinate is +-u m with m = min(index, n - index) and u = kfac or d, so its square depends on m only, and
// floating-point addition commutes: the (up to eight) rows (i, j) with the same unordered pair {m_i, m_j} -- a CLASS --
// share x*x + y*y bit for bit and with it the whole column of t, bin and mu^2 against z.  Rows that merely share
// m_i^2 + m_j^2 do not ((0, 5) and (3, 4) may round differently) and are not merged.  The column index is folded the
// same way: kk = k <= n / 2 on the half-complex array, where the Hermitian weight hw stands for the partner that is not
// stored, kk = min(k, n - k) on the real grid, where both cells are there and are added.  hw(kk) = 1 for kk = 0 and for
// kk = n / 2 of an even n, 2 otherwise, is the number of cells behind kk in both forms.
//
// 1. k_mp_classes: part[class][kk] = the sum of the summand over the class's rows (and the two cells of kk on the real
//    grid).  The only pass over the array.  A wave owns one class and kSpecChunk columns, a lane one column: the row
//    indices are wave-uniform scalar loads, all (at most eight) row segments of the class are loaded before the first is
//    added, in the order of the host's row list, which is ascending.  No LDS, no barrier, no atomics.  NS = 3 keeps the
//    sums aa, bb, ab of two transforms from one read of each; its aa is the same expression in the same order as NS = 1's.
// 2. k_mp_shells: workgroup (b, s) sums bin b over the classes of segment s of mp_segments(n_bin) equal segments of the class
//    list.  Thread t takes classes t, t + 256, ... of the segment in ascending order; the bin does not decrease with kk,
//    so the class's entries of bin b are one run of kk: its ends are estimated from the bin's edges and then moved until
//    the very expression that defines the bin confirms them, and the run is added in ascending kk.  The threads' sums are added by a tree over the thread index through LDS.  The host adds
//    the segments of a bin in ascending order.  Every order is fixed by the indices alone: bitwise repeatable.
//    Bin n_bin (the extra row of workgroups) collects what lies past the last bin -- the corner that both upstream
//    functions drop -- so that a non-finite element anywhere shows in the total.
//    GEOM: the summands are hw * rows {1, t, L_2, L_4}: nmode and the sums behind kmode / rmode and leg.  Once per
//    (n, n_bin, form).
// The element t = 0 (k = 0, r = 0) has no mu: it counts in l = 0, in the count and in the sum of t, and as 0 elsewhere.
// Compiled without FMA contraction so that t, the bin index and L_l are one fixed expression each, the same as the
// host tools' (x86-64, no FMA) and numpy's.
// ------------------------------------------------------------------------------------------------------
constexpr int kMpRows = 8;      // rows of a class at most: (+-a, +-b) and (+-b, +-a)
constexpr int kMpWaves = 4;     // classes per workgroup of k_mp_classes, one per wave
constexpr int kMpBlock = 256;   // threads of k_mp_shells
constexpr int kMpGeom = 4;      // sums of the GEOM pass: count, t, L_2, L_4

// segments the class list is cut into per bin: about 1024 workgroups in all, a function of n_bin alone
__host__ __device__ inline int mp_segments(int n_bin) {
  const int s = (1024 + n_bin - 1) / n_bin;
  return s > 256 ? 256 : s;
}
__host__ __device__ inline int mp_classes(int n) { return (n / 2 + 1) * (n / 2 + 2) / 2; }

__device__ __forceinline__ double mp_real(const double *p) { return stream_load<BCHMC_NT_SPEC2D != 0>(p); }
__device__ __forceinline__ double mp_real(const float *p) { return (double)stream_load<BCHMC_NT_SPEC2D != 0>(p); }

// rows: kMpRows entries per class, ascending, -1 where the class has fewer.  a / b: the half-complex transforms (C2<T>)
// or, REAL, the real grid A (T) in `a`.  part: NS tables of ncls * nh doubles, `stride` apart.
template <typename T, int NS, bool REAL>
__global__ void __launch_bounds__(kSpecChunk * kMpWaves)
k_mp_classes(Geo g, const void *a_, const void *b_, const int *__restrict__ rows, int ncls, double *__restrict__ part,
             long long stride) {
#pragma clang fp contract(off)
  static_assert(NS == 1 || (NS == 3 && !REAL), "one sum, or aa / bb / ab of two transforms");
  const int lane = threadIdx.x % kSpecChunk;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kSpecChunk);
  const int c = blockIdx.x * kMpWaves + w;  // wave-uniform
  if (c >= ncls) return;
  const int k = blockIdx.y * kSpecChunk + lane;
  const bool live = k < g.nh;  // false in the last chunk's tail: such a lane reads column nh - 1 again and stores nothing
  const int kc = min(k, g.nh - 1);
  const bool two = REAL && kc > 0 && kc < g.n - kc;  // the cell n - kc is another one
  const int *my = rows + (long long)c * kMpRows;
  double t[NS][kMpRows];
#pragma unroll
  for (int r = 0; r < kMpRows; r++) {
    const int row = my[r];
#pragma unroll
    for (int s = 0; s < NS; s++) t[s][r] = 0.;
    if (row < 0) continue;
    if (REAL) {
      const T *p = reinterpret_cast<const T *>(a_) + (long long)row * g.n;
      const double v = mp_real(p + kc);
      t[0][r] = two ? v + mp_real(p + (g.n - kc)) : v;
    } else {
      const long long e = (long long)row * g.nhp + kc;
      const double2 x = spec_load(reinterpret_cast<const C2<T> *>(a_) + e);
      t[0][r] = x.x * x.x + x.y * x.y;
      if (NS == 3) {
        const double2 y = spec_load(reinterpret_cast<const C2<T> *>(b_) + e);
        t[1][r] = y.x * y.x + y.y * y.y;
        t[2][r] = x.x * y.x + x.y * y.y;
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int s = 0; s < NS; s++) {
    double acc = t[s][0];
#pragma unroll
    for (int r = 1; r < kMpRows; r++) acc += t[s][r];  // + 0. for a row the class does not have
    part[s * stride + (long long)c * g.nh + k] = acc;
  }
}

// cls: { m_a, m_b, rows of the class, 0 } per class.  u: kfac or d.  dt: the bin width.  out: [n_bin + 1][nseg][NACC]
// with NACC = kMpGeom (GEOM) or 3 NS { l = 0, 2, 4 of table 0, of table 1, ... }.  data_hw: the class sums are weighed by
// hw (the half-complex transform, whose partner modes are not stored); 0 on the real grid, where k_mp_classes has added
// both cells of kk already.  The GEOM sums count hw elements per kk in both forms.
template <int NS, bool GEOM>
__global__ void __launch_bounds__(kMpBlock)
k_mp_shells(int n, int nh, double u, double dt, int n_bin, int ncls, const int4 *__restrict__ cls,
            const double *__restrict__ part, long long stride, int data_hw, double *__restrict__ out) {
#pragma clang fp contract(off)
  constexpr int NACC = GEOM ? kMpGeom : 3 * NS;
  __shared__ double s_red[NACC][kMpBlock];
  const int b = blockIdx.x, nseg = gridDim.y, seg = blockIdx.y, tid = threadIdx.x;
  const int c0 = (int)((long long)ncls * seg / nseg), c1 = (int)((long long)ncls * (seg + 1) / nseg);
  double acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; a++) acc[a] = 0.;
  // the squared edges of bin b as estimates (the bin itself is always taken from bin_of) and the end of the column
  const double edge_lo = (double)b * dt, edge_hi = (double)(b + 1) * dt;
  const double edge_lo2 = edge_lo * edge_lo, edge_hi2 = edge_hi * edge_hi, zmax = u * (double)(nh - 1);
  const float inv_u = (float)(1. / u);
  for (int c = c0 + tid; c < c1; c += kMpBlock) {
    const int4 cl = cls[c];
    const double x = u * (double)cl.x, y = u * (double)cl.y;
    const double r2 = x * x + y * y;
    // the bin of kk, clamped to n_bin (the row of what lies past the last bin)
    auto bin_of = [&](int kk) -> int {
      const double z = u * (double)kk;
      const double t = sqrt(r2 + z * z);
      const unsigned long long q = (unsigned long long)(t / dt);
      return q < (unsigned long long)n_bin ? (int)q : n_bin;
    };
    // Classes whose column lies wholly before or after the bin, decided on the squares with a margin far above the
    // rounding of either side: a class that passes is decided below by bin_of itself.
    if (b < n_bin && r2 > edge_hi2 * (1. + 1e-9)) continue;
    if (r2 + zmax * zmax < edge_lo2 * (1. - 1e-9)) continue;
    // k0 = the first kk with bin >= b, k1 = the first with bin > b (the bin does not decrease with kk): an estimate in
    // float from the bin's edges, then moved until bin_of itself says so on both sides -- the run is exact whatever
    // the estimate was, the estimate only saves evaluations (it is off by one at most)
    int k0 = edge_lo2 > r2 ? min(nh, (int)(sqrtf((float)(edge_lo2 - r2)) * inv_u)) : 0;
    while (k0 > 0 && bin_of(k0 - 1) >= b) k0--;
    while (k0 < nh && bin_of(k0) < b) k0++;
    int k1 = nh;
    if (b < n_bin) {
      k1 = edge_hi2 > r2 ? min(nh, (int)(sqrtf((float)(edge_hi2 - r2)) * inv_u) + 1) : 0;
      k1 = max(k1, k0);
      while (k1 > k0 && bin_of(k1 - 1) > b) k1--;
      while (k1 < nh && bin_of(k1) <= b) k1++;
    }
    for (int kk = k0; kk < k1; kk++) {
      const double z = u * (double)kk;
      const double z2 = z * z;
      const double t2 = r2 + z2;
      const double hw = (kk == 0 || ((n & 1) == 0 && kk == n / 2)) ? 1. : 2.;
      double l2 = 0., l4 = 0.;
      if (t2 > 0.) {
        const double mu2 = z2 / t2;
        l2 = 1.5 * mu2 - 0.5;
        l4 = (35. * mu2 * mu2 - 30. * mu2 + 3.) / 8.;
      }
      if (GEOM) {
        const double m = hw * (double)cl.z;
        acc[0] += m;
        acc[1] += m * sqrt(t2);
        acc[2] += m * l2;
        acc[3] += m * l4;
      } else {
#pragma unroll
        for (int s = 0; s < NS; s++) {
          const double v = (data_hw ? hw : 1.) * part[s * stride + (long long)c * nh + kk];
          acc[3 * s] += v;
          acc[3 * s + 1] += v * l2;
          acc[3 * s + 2] += v * l4;
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NACC; a++) s_red[a][tid] = acc[a];
  __syncthreads();
  for (int half = kMpBlock / 2; half > 0; half /= 2) {
    if (tid < half) {
#pragma unroll
      for (int a = 0; a < NACC; a++) s_red[a][tid] += s_red[a][tid + half];
    }
    __syncthreads();
  }
  if (tid < NACC) out[((long long)b * nseg + seg) * NACC + tid] = s_red[tid][0];
}

}  // namespace bchmc
