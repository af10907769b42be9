// interp_particles.hpp -- A grid field read at the positions of a free particle catalogue (bchmc_interp_particles): the
// gather that is the reverse of catalogue.hpp's scatter.  Count per tile, fill of indexed records, LDS gather, direct form.
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
//
// interpolate_CIC / interpolate_TSC / interpolate_TSC_multi (interpolate_grid.cpp:82-120, 134-202, 207-286) for N_part
// particles that are no lattice and up to four fields at once.  k_interp_tsc_tile / k_interp_tsc (tiles_low.hpp,
// variants.hpp) hold the same TSC arithmetic for the lattice particles of calc_h = 3 and interp_field (upres.hpp) the CIC
// one for the centres of a regular grid; neither takes a free list.  The batch pipeline is the catalogue's: k_cat_positions
// and k_cat_scan are used as they are, count and fill have forms of their own here because the domain test and the home
// cell are the interpolators' (no min1..3 upstream: box coordinates) and a record carries the particle's index in the
// batch where the catalogue's carries a weight.
//
// The arithmetic of one particle is two functions, the same in the tile kernel and in the direct one: itp_stencil (cells
// and weights) and itp_sum (the sum over a functor load(i, j, k, f) that returns the value of field f at stencil slot
// (i, j, k), widened to double).  Double throughout, the reference's expressions in its operand order, no FMA
// contraction: a particle's result is a function of its position and the fields alone, whatever the path, the batch or
// the order inside a tile, and nothing is accumulated across particles (no atomics on the result).
#pragma once
#include "common.hpp"
#include "catalogue.hpp"
#include "tile_walk.hpp"
#include "tiles_low.hpp"

#include <cfloat>

namespace bchmc {

constexpr int kItpMaxFields = 4;  // BCHMC_INTERP_MAX_FIELDS
constexpr int kItpHalo = 1;       // CIC reaches cell_index1 + 1, TSC the particle's cell +- 1

struct ItpRec {  // one record in tile order: the position as the storage type holds it, and the index in the batch
  double x, y, z;
  long long idx;
};
static_assert(sizeof(ItpRec) == 32, "a record is three doubles and an index");

// Cells and weights of one particle.  CIC (MK = 1): slot 0 is cell_index1 with weight tx, slot 1 cell_index2 with dx.
// TSC (MK = 2): slots 0, 1, 2 are the particle's cell - 1, the cell, the cell + 1 with wx / wy / wz[0 .. 2].
template <int MK>
struct ItpStencil {
  static constexpr int W = MK == 1 ? 2 : 3;
  int c[3][W];
  double w[3][W];
};

// false: the particle is lost.  CIC folds every finite coordinate into the box (getCICcells / getCICweights with both
// folds of pacman_coordinate, interpolate_grid.cpp:27-79).  TSC (:142-180) casts xp / d to unsigned without a test,
// which is undefined below 0 and reads past the array from cell n on: a particle is kept if 0 <= x and xp / d < n on
// every axis -- for a quotient an unsigned can hold, exactly (unsigned)(xp / d) < n.  x < L would not do: with n = 9,
// L = 1 the double below 1.0 divided by d gives 9.  A non-finite coordinate fails under either kernel.
template <int MK>
__device__ __forceinline__ bool itp_stencil(const Geo &g, double x, double y, double z, ItpStencil<MK> &s) {
#pragma clang fp contract(off)
  const int n = g.n;
  const double d = g.d, L = g.L;
  const double p[3] = {x, y, z};
  if (MK == 1) {
    if (!(fabs(x) <= DBL_MAX && fabs(y) <= DBL_MAX && fabs(z) <= DBL_MAX)) return false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      double q = p[a] - 0.5 * d;
      q = pacman(q, L);
      long long c = (long long)(q / d);
      c = (c + n) % n;
      s.c[a][0] = (int)c;
      s.c[a][1] = (int)((c + 1) % n);
      const double dx = q / d - (double)c;
      s.w[a][1] = dx;
      s.w[a][0] = 1. - dx;
    }
  } else {
    double qk[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      qk[a] = p[a] / d;
      if (!(p[a] >= 0. && qk[a] < (double)n)) return false;
    }
    double dd[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const unsigned c = (unsigned)qk[a], un = (unsigned)n;
      s.c[a][1] = (int)c;
      s.c[a][0] = (int)((c - 1 + un) % un);
      s.c[a][2] = (int)((c + 1) % un);
      dd[a] = qk[a] - ((double)c + 0.5);
      s.w[a][1] = 0.75 - dd[a] * dd[a];
      const double lo = 1.5 - fabs(dd[a] + 1);
      s.w[a][0] = 0.5 * (lo * lo);
    }
    // interpolate_grid.cpp:166-168: the upper weights of x and y are computed from dz, kept bug for bug
    const double hi = 1.5 - fabs(dd[2] - 1);
    s.w[0][2] = s.w[1][2] = s.w[2][2] = 0.5 * (hi * hi);
  }
  return true;
}

// The interpolated values of K fields: interpolate_grid.cpp:92-99 (eight terms, each F * a * b * c left to right, summed
// in source order) or :183-188 (27 terms in i, j, k order, each wx[i] * wy[j] * wz[k] * F, added to an output that starts
// at 0).
template <int MK, int K, typename Load>
__device__ __forceinline__ void itp_sum(const ItpStencil<MK> &s, Load &&load, double (&out)[K]) {
#pragma clang fp contract(off)
  if (MK == 1) {
    constexpr int order[8][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
#pragma unroll
    for (int t = 0; t < 8; t++) {
      const int i = order[t][0], j = order[t][1], k = order[t][2];
#pragma unroll
      for (int f = 0; f < K; f++) {
        const double term = load(i, j, k, f) * s.w[0][i] * s.w[1][j] * s.w[2][k];
        out[f] = t == 0 ? term : out[f] + term;
      }
    }
  } else {
#pragma unroll
    for (int f = 0; f < K; f++) out[f] = 0.;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const double w = s.w[0][i] * s.w[1][j] * s.w[2][k];
#pragma unroll
          for (int f = 0; f < K; f++) out[f] += w * load(i, j, k, f);
        }
  }
}

// The cell whose tile a particle is binned under: cell_index1 for CIC, the particle's cell for TSC
template <int MK>
__device__ __forceinline__ int itp_home_tile(const TilePar &tp, const ItpStencil<MK> &s) {
  const int a = MK == 1 ? 0 : 1;
  return cat_tile(tp, s.c[0][a], s.c[1][a], s.c[2][a]);
}

__device__ __forceinline__ double itp_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// One pass over a batch: domain test, tile of the home cell, particles per tile; the kept ones of a wave are counted
// with one atomic.  tile_of[p] = -1 for a lost particle, whose K results become quiet NaNs here.
template <typename T, int MK>
__global__ void __launch_bounds__(256)
k_itp_count(Geo g, TilePar tp, int m, int K, const double *__restrict__ x, const double *__restrict__ y,
            const double *__restrict__ z, int *__restrict__ tile_of, unsigned *__restrict__ cnt,
            double *__restrict__ out, unsigned long long *__restrict__ stat) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  bool in = false;
  if (p < m) {
    ItpStencil<MK> s;
    in = itp_stencil<MK>(g, (double)(T)x[p], (double)(T)y[p], (double)(T)z[p], s);
    if (in) {
      const int t = itp_home_tile<MK>(tp, s);
      tile_of[p] = t;
      atomicAdd(cnt + t, 1u);
    } else {
      tile_of[p] = -1;
      for (int f = 0; f < K; f++) out[(size_t)f * kCatBatch + p] = itp_nan();
    }
  }
  const unsigned long long kept = __ballot(in);
  if ((threadIdx.x & (kWave - 1)) == 0 && kept) atomicAdd(stat + kCatIn, (unsigned long long)__popcll(kept));
}

// Records into tile order; the order inside a tile is that of the atomics, which no result depends on
template <typename T>
__global__ void __launch_bounds__(256)
k_itp_fill(int m, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
           const int *__restrict__ tile_of, const unsigned *__restrict__ off, unsigned *__restrict__ cursor,
           ItpRec *__restrict__ rec) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const int t = tile_of[p];
  if (t < 0) return;
  const unsigned slot = off[t] + atomicAdd(cursor + t, 1u);
  rec[slot] = ItpRec{(double)(T)x[p], (double)(T)y[p], (double)(T)z[p], (long long)p};
}

// One workgroup per work item: the tile and a halo of one cell of each of the K fields staged in LDS in the storage type
// (component-major, 1800 cells per field for 8 x 8 x 16 tiles: 57.6 KB for four fp64 fields), then 8 or 27 LDS reads per
// particle per field.  An image coordinate is (cell - image origin) mod n; every cell a particle of the tile reads lies
// inside the image by the halo's definition, except on a grid narrower than the image, where the halo folds: such a
// particle reads the grid, as in k_interp_tsc_tile.  Results go to out[f * kCatBatch + index in the batch].
template <typename T, int MK, int K>
__global__ void __launch_bounds__(256)
k_itp_gather_tile(Geo g, TilePar tp, const CatItem *__restrict__ items, const unsigned long long *__restrict__ stat,
                  const ItpRec *__restrict__ rec, const T *__restrict__ src, double *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char itp_smem[];
  T *img = reinterpret_cast<T *>(itp_smem);
  if ((unsigned long long)blockIdx.x >= stat[kCatItems]) return;
  const CatItem it = items[blockIdx.x];
  const int n = g.n;
  const int lx = tp.tx + 2 * kItpHalo, ly = tp.ty + 2 * kItpHalo, lz = tp.tz + 2 * kItpHalo;
  const int ncell = lx * ly * lz;
  const int tk = it.tile % tp.ntz, tij = it.tile / tp.ntz;
  const int ox = (tij / tp.nty) * tp.tx - kItpHalo, oy = (tij % tp.nty) * tp.ty - kItpHalo, oz = tk * tp.tz - kItpHalo;
  tile_walk(lx, ly, lz, ox, oy, oz, n, (int)threadIdx.x, (int)blockDim.x, [&](int c, int cell) {
#pragma unroll
    for (int f = 0; f < K; f++) img[c + f * ncell] = src[cell + f * g.N];
  });
  __syncthreads();
  constexpr int W = ItpStencil<MK>::W;
  for (int r = threadIdx.x; r < it.count; r += blockDim.x) {
    const ItpRec q = rec[it.first + r];
    ItpStencil<MK> s;
    itp_stencil<MK>(g, q.x, q.y, q.z, s);  // kept by k_itp_count, from the same three values
    int ax[W], ay[W], az[W];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < W; a++) {
      ax[a] = low_local(s.c[0][a], ox, lx, n);
      ay[a] = low_local(s.c[1][a], oy, ly, n);
      az[a] = low_local(s.c[2][a], oz, lz, n);
      inside = inside && ax[a] >= 0 && ay[a] >= 0 && az[a] >= 0;
    }
    double o[K];
    if (inside)
      itp_sum<MK, K>(s, [&](int i, int j, int k, int f) { return (double)img[az[k] + lz * (ay[j] + ly * ax[i]) + f * ncell]; }, o);
    else
      itp_sum<MK, K>(s, [&](int i, int j, int k, int f) {
        return (double)src[s.c[2][k] + (long long)n * (s.c[1][j] + (long long)n * s.c[0][i]) + f * g.N];
      }, o);
#pragma unroll
    for (int f = 0; f < K; f++) out[(size_t)f * kCatBatch + q.idx] = o[f];
  }
}

// Direct version (no tile partition, or a catalogue too sparse to pay for tile images): one thread per particle, global
// reads, the same two functions.
template <typename T, int MK, int K>
__global__ void __launch_bounds__(256)
k_itp_gather_direct(Geo g, int m, const double *__restrict__ x, const double *__restrict__ y,
                    const double *__restrict__ z, const T *__restrict__ src, double *__restrict__ out,
                    unsigned long long *__restrict__ stat) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  bool in = false;
  if (p < m) {
    ItpStencil<MK> s;
    in = itp_stencil<MK>(g, (double)(T)x[p], (double)(T)y[p], (double)(T)z[p], s);
    double o[K];
    if (in) {
      const int n = g.n;
      itp_sum<MK, K>(s, [&](int i, int j, int k, int f) {
        return (double)src[s.c[2][k] + (long long)n * (s.c[1][j] + (long long)n * s.c[0][i]) + f * g.N];
      }, o);
    } else {
#pragma unroll
      for (int f = 0; f < K; f++) o[f] = itp_nan();
    }
#pragma unroll
    for (int f = 0; f < K; f++) out[(size_t)f * kCatBatch + p] = o[f];
  }
  const unsigned long long kept = __ballot(in);
  if ((threadIdx.x & (kWave - 1)) == 0 && kept) atomicAdd(stat + kCatIn, (unsigned long long)__popcll(kept));
}

}  // namespace bchmc
