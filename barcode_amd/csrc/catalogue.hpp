// catalogue.hpp -- Mass assignment of a free particle catalogue (bchmc_density_particles): count per tile, scan into work items, fill of weighted records, LDS scatter, direct fallback.
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
//
// getDensity_NGP / _CIC / _TSC / _SPH (massFunctions.cc:49-495) for N_part particles that are no lattice: any number of
// them, any weight, any clustering.  The trajectory's binning (tiles.hpp) keys a record on its Lagrangian lattice index,
// gives it weight one and sizes a tile's slots from a mean occupancy of one particle per cell; none of that holds here,
// so the catalogue has kernels of its own.  They share the handle's tile shape (TilePar::tx, ty, tz, chunk) and nothing
// else.  The arithmetic of one particle is cat_deposit, the same function in the tile kernel and in the direct one: the
// expressions of k_scatter_low_order / k_scatter_sph (variants.hpp, forward_model.hpp) with the particle's weight as the
// reference's `mass`.
#pragma once
#include "common.hpp"
#include "forward_model.hpp"
#include "tile_plan.hpp"

namespace bchmc {

constexpr int kCatBatch = 1 << 20;  // particles staged per pass: device memory of a call does not grow with N_part

// words of the catalogue's status block (unsigned long long each)
enum { kCatIn = 0, kCatMaxTile = 1, kCatItems = 2, kCatSat = 3, kCatWords = 4 };

constexpr int kCatSph81 = 4;  // template value of the kernels: SPH through the standard 81-cell hull (h = d), halo 2

struct CatRec {  // one record in tile order: the position as the storage type holds it, and the weight
  double x, y, z, w;
};
static_assert(sizeof(CatRec) == 32, "a record is four doubles");

struct CatItem {  // one work item: a run of at most TilePar::chunk records of one tile
  int tile, first, count, pad;
};

// The kernel's own domain test on the position the storage type holds (massFunctions.cc:75, 116, 426; :195 for TSC is
// closed above).  A non-finite coordinate fails every comparison.
__device__ __forceinline__ bool cat_in_domain(const Geo &g, const SphPar &sp, int mk, double x, double y, double z) {
  const double L = g.L;
  if (mk == 2)
    return (x >= sp.min1 && x <= sp.min1 + L) && (y >= sp.min2 && y <= sp.min2 + L) && (z >= sp.min3 && z <= sp.min3 + L);
  return (x >= sp.min1 && x < sp.min1 + L) && (y >= sp.min2 && y < sp.min2 + L) && (z >= sp.min3 && z < sp.min3 + L);
}

// Home cell of a particle that passed the domain test: NGP / CIC / TSC floor((x - min) / d) mod n (CIC's pair of cells
// is this one and a neighbour), SPH (ULONG)(x / d) mod n without min (massFunctions.cc:434-436).
__device__ __forceinline__ void cat_home(const Geo &g, const SphPar &sp, int mk, double x, double y, double z, int &ci,
                                         int &cj, int &ck) {
  const unsigned n = (unsigned)g.n;
  if (mk == 3) {
    ci = (int)((unsigned long long)(x / g.d) % n);
    cj = (int)((unsigned long long)(y / g.d) % n);
    ck = (int)((unsigned long long)(z / g.d) % n);
  } else {
    ci = (int)((unsigned)floor((x - sp.min1) / g.d) % n);
    cj = (int)((unsigned)floor((y - sp.min2) / g.d) % n);
    ck = (int)((unsigned)floor((z - sp.min3) / g.d) % n);
  }
}

// Everything one particle adds to the grid: sink(i, j, k, value) with wrapped cell indices in [0, n).  The CIC and TSC
// products are rounded to the storage type once, like the handle's own kernels round them; SPH and NGP stay double.
template <typename T, int MK, typename Sink>
__device__ __forceinline__ void cat_deposit(const Geo &g, const SphPar &sp, double x, double y, double z, double mass,
                                            Sink &&sink) {
  const int n = g.n;
  const double d = g.d, L = g.L;
  if (MK == 0) {
    int ci, cj, ck;
    cat_home(g, sp, 0, x, y, z, ci, cj, ck);
    sink(ci, cj, ck, mass);
  } else if (MK == 1) {
    double q[3] = {x - 0.5 * d, y - 0.5 * d, z - 0.5 * d};
    int c1[3], c2[3];
    double dx[3], tx[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      q[a] = pacman(q[a], L);
      long long c = (long long)(q[a] / d);
      c = (c + n) % n;
      c1[a] = (int)c;
      c2[a] = (int)((c + 1) % n);
      dx[a] = q[a] / d - (double)c;
      tx[a] = 1. - dx[a];
    }
    sink(c1[0], c1[1], c1[2], (double)(T)(mass * tx[0] * tx[1] * tx[2]));
    sink(c2[0], c1[1], c1[2], (double)(T)(mass * dx[0] * tx[1] * tx[2]));
    sink(c1[0], c2[1], c1[2], (double)(T)(mass * tx[0] * dx[1] * tx[2]));
    sink(c1[0], c1[1], c2[2], (double)(T)(mass * tx[0] * tx[1] * dx[2]));
    sink(c2[0], c2[1], c1[2], (double)(T)(mass * dx[0] * dx[1] * tx[2]));
    sink(c2[0], c1[1], c2[2], (double)(T)(mass * dx[0] * tx[1] * dx[2]));
    sink(c1[0], c2[1], c2[2], (double)(T)(mass * tx[0] * dx[1] * dx[2]));
    sink(c2[0], c2[1], c2[2], (double)(T)(mass * dx[0] * dx[1] * dx[2]));
  } else if (MK == 2) {
    const double pos[3] = {(x - sp.min1) / d, (y - sp.min2) / d, (z - sp.min3) / d};
    int c[3][3];
    double w[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const unsigned ci = (unsigned)floor(pos[a]) % (unsigned)n;
      c[a][1] = (int)ci;
      c[a][2] = (int)((ci + 1) % (unsigned)n);
      c[a][0] = (int)((ci - 1 + (unsigned)n) % (unsigned)n);
      const double dd = pos[a] - ((double)ci + 0.5);
      w[a][1] = 0.75 - dd * dd;
      w[a][2] = 0.5 * (0.5 + dd) * (0.5 + dd);
      w[a][0] = 0.5 * (0.5 - dd) * (0.5 - dd);
    }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++)
#pragma unroll
        for (int e = 0; e < 3; e++) sink(c[0][a], c[1][b], c[2][e], (double)(T)(mass * w[0][a] * w[1][b] * w[2][e]));
  } else if (MK == kCatSph81) {
    // h = d (any h whose stencil hull is the standard one and exact, cat_hull_is_81): the 81 cells of the hull instead
    // of the cube's 343, fully unrolled, q from the rsq seed and the folded spline -- the arithmetic of
    // k_scatter_tile's hull branch, in double.  No cell outside the hull can pass r / h <= 2 (build_hull's `exact`).
    const long long ix = (long long)(x / d), iy = (long long)(y / d), iz = (long long)(z / d);
    const double ccx = ((double)ix + 0.5) * d, ccy = ((double)iy + 0.5) * d, ccz = ((double)iz + 0.5) * d;
    int kz[5];
#pragma unroll
    for (int e = 0; e < 5; e++) kz[e] = (int)((iz + (e - 2) + (long long)n * 4) % n);
#pragma unroll
    for (int a = 0; a < 5; a++) {
      const double ddx = x - (ccx + (double)(a - 2) * d);
      const double dx2 = ddx * ddx;
      const int kx = (int)((ix + (a - 2) + (long long)n * 4) % n);
#pragma unroll
      for (int b = 0; b < 5; b++) {
        const int zw = hull81_zw(a, b);
        if (zw < 0) continue;
        const double ddy = y - (ccy + (double)(b - 2) * d);
        const double r2ab = dx2 + ddy * ddy;
        if (r2ab > sp.r2_lim) continue;
        const int ky = (int)((iy + (b - 2) + (long long)n * 4) % n);
#pragma unroll
        for (int e = 0; e < 5; e++) {
          if (e - 2 < -zw || e - 2 > zw) continue;
          const double ddz = z - (ccz + (double)(e - 2) * d);
          const double r2 = r2ab + ddz * ddz;
          if (r2 > sp.r2_lim) continue;
          const double q = (r2 * fast_rsqrt(r2 + tiny_pos<double>())) * sp.h_inv;
          if (q <= 2.) sink(kx, ky, kz[e], sph_w_folded<double>(q, sp.w_norm) * mass);
        }
      }
    }
  } else {
    // the (2 reach + 1)^3 cube of getDensity_SPH with its r / h <= 2 decision, columns and cells rejected on the squared
    // distance before the square root (k_scatter_sph)
    const long long ix = (long long)(x / d), iy = (long long)(y / d), iz = (long long)(z / d);
    const double ccx = ((double)ix + 0.5) * d, ccy = ((double)iy + 0.5) * d, ccz = ((double)iz + 0.5) * d;
    const int R = sp.reach;
    for (int i1 = -R; i1 <= R; ++i1) {
      const double ddx = x - (ccx + (double)i1 * d);
      const double dx2 = ddx * ddx;
      if (dx2 > sp.r2_lim) continue;
      const int kx = (int)((ix + i1 + (long long)n * 4) % n);
      for (int i2 = -R; i2 <= R; ++i2) {
        const double ddy = y - (ccy + (double)i2 * d);
        const double r2ab = dx2 + ddy * ddy;
        if (r2ab > sp.r2_lim) continue;
        const int ky = (int)((iy + i2 + (long long)n * 4) % n);
        for (int i3 = -R; i3 <= R; ++i3) {
          const double ddz = z - (ccz + (double)i3 * d);
          const double r2 = r2ab + ddz * ddz;
          if (r2 > sp.r2_lim) continue;
          const double q = sqrt(r2) / sp.h;
          if (q <= 2.) sink(kx, ky, (int)((iz + i3 + (long long)n * 4) % n), sph_w(q, sp.w_norm) * mass);
        }
      }
    }
  }
}

// The accumulator of a call: doubles (hardware atomics), or 64-bit fixed point on deterministic handles
template <bool FIX> struct CatCell { using type = double; };
template <> struct CatCell<true> { using type = long long; };

// Fixed point.  The scale makes the largest contribution the kernel can produce 2^46, and a work item holds at most 2^11
// records, so an LDS sum of contributions below 2^51 each stays below 2^62.  A contribution out of that proportion (only
// upstream's TSC weights of a particle at x == min + L get there) goes to the grid directly.  On the grid every add looks
// at the sum it produced: the first one that takes a cell beyond 2^62 in magnitude -- 2^16 maximal contributions --
// sets the saturation word before anything can wrap, whatever the number of particles.
constexpr long long kCatFixOne = 1ll << 51, kCatFixLimit = 1ll << 62;

// llrint(v scale); false (and the word set) for a single contribution that is itself beyond the limit
__device__ __forceinline__ bool cat_fix(double v, double scale, long long &t, unsigned long long *stat) {
  const double s = v * scale;
  if (!(fabs(s) < (double)kCatFixLimit)) {
    stat[kCatSat] = 1;  // benign race: every writer stores 1
    return false;
  }
  t = __double2ll_rn(s);
  return true;
}
__device__ __forceinline__ void cat_add_grid(double *p, double v, unsigned long long *) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void cat_add_grid(long long *p, long long t, unsigned long long *stat) {
  const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)t);
  const long long now = (long long)(old + (unsigned long long)t);
  if (now > kCatFixLimit || now < -kCatFixLimit) stat[kCatSat] = 1;
}
// One contribution v for grid cell `cell`, through the LDS image cell `img` where there is one (nullptr: none)
__device__ __forceinline__ void cat_add(double *cell, double *img, double v, double, unsigned long long *stat) {
  // the image cell through an LDS-typed pointer: ds_add_f64, which a pointer merged with `cell` would not give
  if (img) __hip_atomic_fetch_add((__attribute__((address_space(3))) double *)img, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else unsafeAtomicAdd(cell, v);
}
__device__ __forceinline__ void cat_add(long long *cell, long long *img, double v, double scale, unsigned long long *stat) {
  long long t;
  if (!cat_fix(v, scale, t, stat)) return;
  if (img && t < kCatFixOne && t > -kCatFixOne) atomicAdd(reinterpret_cast<unsigned long long *>(img), (unsigned long long)t);
  else cat_add_grid(cell, t, stat);
}

// Tile of a home cell
__device__ __forceinline__ int cat_tile(const TilePar &tp, int ci, int cj, int ck) {
  return ((ci / tp.tx) * tp.nty + cj / tp.ty) * tp.ntz + ck / tp.tz;
}

// The own particles of the handle as a catalogue batch: particle_pos of lattice particles p0 .. p0 + m - 1
template <typename T>
__global__ void __launch_bounds__(256)
k_cat_positions(Geo g, PosPar pp, const T *__restrict__ psi, long long p0, int m, double *__restrict__ x,
                double *__restrict__ y, double *__restrict__ z) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m) return;
  const long long p = p0 + b;
  const int k = (int)(p % g.n);
  const long long ij = p / g.n;
  const int j = (int)(ij % g.n), i = (int)(ij / g.n);
  T xt, yt, zt;
  particle_pos<T>(pp, i, j, k, psi[p], psi[p + g.N], psi[p + 2 * g.N], xt, yt, zt);
  x[b] = (double)xt;
  y[b] = (double)yt;
  z[b] = (double)zt;
}

// One pass over a batch: domain test, tile of the home cell, particles per tile.  tile_of[p] = -1 for a lost particle.
template <typename T>
__global__ void __launch_bounds__(256)
k_cat_count(Geo g, SphPar sp, TilePar tp, int mk, int m, const double *__restrict__ x, const double *__restrict__ y,
            const double *__restrict__ z, int *__restrict__ tile_of, unsigned *__restrict__ cnt,
            unsigned long long *__restrict__ stat) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const double xp = (double)(T)x[p], yp = (double)(T)y[p], zp = (double)(T)z[p];
  if (!cat_in_domain(g, sp, mk, xp, yp, zp)) {
    tile_of[p] = -1;
    return;
  }
  int ci, cj, ck;
  cat_home(g, sp, mk, xp, yp, zp, ci, cj, ck);
  const int t = cat_tile(tp, ci, cj, ck);
  tile_of[p] = t;
  atomicAdd(cnt + t, 1u);
  atomicAdd(stat + kCatIn, 1ull);
}

// Exclusive scan of the tile populations, and the list of work items: a tile of c records becomes ceil(c / chunk) runs,
// an empty tile none.  One workgroup; the tiles go through it 1024 at a time.
__global__ void __launch_bounds__(1024)
k_cat_scan(int ntiles, int chunk, const unsigned *__restrict__ cnt, unsigned *__restrict__ off,
           unsigned *__restrict__ cursor, CatItem *__restrict__ items, unsigned long long *__restrict__ stat) {
  __shared__ unsigned s_rec[1024], s_item[1024];
  __shared__ unsigned carry[2];
  const int tid = threadIdx.x;
  if (tid == 0) carry[0] = carry[1] = 0;
  __syncthreads();
  unsigned mx = 0;
  for (int base = 0; base < ntiles; base += 1024) {
    const int t = base + tid;
    const unsigned c = t < ntiles ? cnt[t] : 0u;
    const unsigned ni = (c + (unsigned)chunk - 1) / (unsigned)chunk;
    s_rec[tid] = c;
    s_item[tid] = ni;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const unsigned a = tid >= o ? s_rec[tid - o] : 0u, b = tid >= o ? s_item[tid - o] : 0u;
      __syncthreads();
      s_rec[tid] += a;
      s_item[tid] += b;
      __syncthreads();
    }
    const unsigned first = carry[0] + s_rec[tid] - c, item0 = carry[1] + s_item[tid] - ni;
    if (t < ntiles) {
      off[t] = first;
      cursor[t] = 0;
      for (unsigned j = 0; j < ni; j++) {
        const unsigned left = c - j * (unsigned)chunk;
        items[item0 + j] = CatItem{t, (int)(first + j * (unsigned)chunk), (int)(left < (unsigned)chunk ? left : (unsigned)chunk), 0};
      }
      mx = c > mx ? c : mx;
    }
    __syncthreads();
    if (tid == 1023) {
      carry[0] += s_rec[1023];
      carry[1] += s_item[1023];
    }
    __syncthreads();
  }
  if (tid == 0) stat[kCatItems] = carry[1];
  if (mx) atomicMax(stat + kCatMaxTile, (unsigned long long)mx);
}

// Records into tile order; the order inside a tile is that of the atomics
template <typename T>
__global__ void __launch_bounds__(256)
k_cat_fill(int m, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
           const double *__restrict__ w, const int *__restrict__ tile_of, const unsigned *__restrict__ off,
           unsigned *__restrict__ cursor, CatRec *__restrict__ rec) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const int t = tile_of[p];
  if (t < 0) return;
  const unsigned slot = off[t] + atomicAdd(cursor + t, 1u);
  rec[slot] = CatRec{(double)(T)x[p], (double)(T)y[p], (double)(T)z[p], w ? w[p] : 1.};
}

// One workgroup per work item: an LDS image of the tile and a halo of H cells (0 NGP, 1 CIC / TSC, the cube's reach for
// SPH), 8 bytes per cell, accumulated with LDS atomics and flushed to the grid with periodic wrap.  Several items may
// share a tile, and neighbouring tiles share halo cells: the flush adds with global atomics.  An image coordinate is
// (cell - tile origin + H) mod n, which lies inside the image for every cell a particle of the tile can reach; on a
// grid narrower than the image the halo folds onto the cells it wraps to.  A cell that fell outside all the same (it
// cannot, by the halo's definition) would be added to the grid directly rather than dropped or written out of bounds.
template <typename T, int MK, bool FIX>
__global__ void __launch_bounds__(256)
k_cat_scatter(Geo g, SphPar sp, TilePar tp, int H, const CatItem *__restrict__ items,
              unsigned long long *__restrict__ stat, const CatRec *__restrict__ rec,
              typename CatCell<FIX>::type *__restrict__ acc, double fix_scale) {
  using Cell = typename CatCell<FIX>::type;
  extern __shared__ __attribute__((aligned(16))) char cat_smem[];
  Cell *img = reinterpret_cast<Cell *>(cat_smem);
  if ((unsigned long long)blockIdx.x >= stat[kCatItems]) return;
  const CatItem it = items[blockIdx.x];
  const int n = g.n;
  const int lx = tp.tx + 2 * H, ly = tp.ty + 2 * H, lz = tp.tz + 2 * H;
  const int ncell = lx * ly * lz;
  const int tk = it.tile % tp.ntz, tij = it.tile / tp.ntz;
  const int ox = (tij / tp.nty) * tp.tx - H, oy = (tij % tp.nty) * tp.ty - H, oz = tk * tp.tz - H;  // image origin
  for (int c = threadIdx.x; c < ncell; c += blockDim.x) img[c] = Cell(0);
  __syncthreads();
  auto sink = [&](int ci, int cj, int ck, double v) {
    int a = ci - ox, b = cj - oy, e = ck - oz;  // in (-n, 2 n): H <= n
    a = a < 0 ? a + n : (a >= n ? a - n : a);
    b = b < 0 ? b + n : (b >= n ? b - n : b);
    e = e < 0 ? e + n : (e >= n ? e - n : e);
    Cell *cell = acc + (ck + (long long)n * (cj + (long long)n * ci));
    if (a < lx && b < ly && e < lz) cat_add(cell, img + (e + lz * (b + ly * a)), v, fix_scale, stat);
    else cat_add(cell, (Cell *)nullptr, v, fix_scale, stat);
  };
  for (int r = threadIdx.x; r < it.count; r += blockDim.x) {
    const CatRec q = rec[it.first + r];
    cat_deposit<T, MK>(g, sp, q.x, q.y, q.z, q.w, sink);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < ncell; c += blockDim.x) {
    const Cell v = img[c];
    if (v == Cell(0)) continue;
    const int e = c % lz, ab = c / lz;
    const int b = ab % ly, a = ab / ly;
    const int ci = ((ox + a) % n + n) % n, cj = ((oy + b) % n + n) % n, ck = ((oz + e) % n + n) % n;
    cat_add_grid(acc + (ck + (long long)n * (cj + (long long)n * ci)), v, stat);
  }
}

// Direct version (no tile partition, or an image that would not leave two workgroups per CU): one thread per particle,
// global atomics, the same cat_deposit.
template <typename T, int MK, bool FIX>
__global__ void __launch_bounds__(256)
k_cat_direct(Geo g, SphPar sp, int m, const double *__restrict__ x, const double *__restrict__ y,
             const double *__restrict__ z, const double *__restrict__ w, typename CatCell<FIX>::type *__restrict__ acc,
             double fix_scale, unsigned long long *__restrict__ stat) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const double xp = (double)(T)x[p], yp = (double)(T)y[p], zp = (double)(T)z[p];
  if (!cat_in_domain(g, sp, MK, xp, yp, zp)) return;
  atomicAdd(stat + kCatIn, 1ull);
  const int n = g.n;
  auto sink = [&](int ci, int cj, int ck, double v) {
    cat_add(acc + (ck + (long long)n * (cj + (long long)n * ci)), (typename CatCell<FIX>::type *)nullptr, v, fix_scale, stat);
  };
  cat_deposit<T, MK>(g, sp, xp, yp, zp, w ? w[p] : 1., sink);
}

// The accumulator as the ABI's doubles.  Fixed point: one conversion per cell (no order to depend on); a cell beyond
// sat_limit (2^62: 2^16 maximal contributions, within a factor two of wrapping) sets the flag like the adds do.
template <bool FIX>
__global__ void __launch_bounds__(256)
k_cat_finish(long long N, const typename CatCell<FIX>::type *__restrict__ acc, double inv_scale, long long sat_limit,
             double *__restrict__ out, unsigned long long *__restrict__ stat) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    if (FIX) {
      const long long f = (long long)acc[i];
      if (f > sat_limit || f < -sat_limit) stat[kCatSat] = 1;  // benign race: every writer stores 1
      out[i] = (double)f * inv_scale;
    } else {
      out[i] = (double)acc[i];
    }
  }
}

}  // namespace bchmc
