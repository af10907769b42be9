// mass.hpp -- Hamiltonian_mass (HMC_mass.cc:315-368): the element-wise masses and the Jasche+13 first-order diagonal.
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
#pragma once
#include "common.hpp"
#include "forward_model.hpp"

namespace bchmc {

// ------------------------------------------------------------------------------------------------------
// Element-wise masses on the full N^3 grid, in double whatever T is.  invP = 1/P for P > 0, else 0 (inv_ps, 117-124).
//   MASS_ONE   1                                 fill_one (mass_type 0, and 60 before its switch)
//   MASS_INVP  invP                              inverse_power_spectrum_mass (163-172)
//   MASS_FORCE 2 invP + sqrt(invP Pf[bin(k)])    likeli_force_mass (127-142) with Hamiltonian_mass_likeli_force (53-83)
//   MASS_MEAN  2 invP + sqrt(invP fbar)          mean_likeli_force_mass (145-160)
//   MASS_PS    P                                 copyArray of signal_PS (338)
// times `factor` (mass_factor for the types that have a mass_f, 362-363).  bin(k) = (ULONG)(|k| / dk) with |k| as
// k_spectrum computes it (no FMA contraction: a mode on a bin edge lands where the reference puts it); the k = 0 cell
// gets 0, and the corner mode (N/2, N/2, N/2), bin n_bin, which upstream reads one past the end of likeli_power,
// gets an empty bin (0) -- the one deliberate deviation.
// ------------------------------------------------------------------------------------------------------
enum { MASS_ONE = 0, MASS_INVP = 1, MASS_FORCE = 2, MASS_MEAN = 3, MASS_PS = 4 };

template <typename T>
__global__ void __launch_bounds__(256)
k_mass_elementwise(Geo g, int mode, const T *__restrict__ sigPS, const double *__restrict__ Pf, int n_bin, double dk,
                   double fbar, double factor, double *__restrict__ out) {
#pragma clang fp contract(off)
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < g.N; p += (long long)gridDim.x * blockDim.x) {
    double v = 1.;
    if (mode != MASS_ONE) {
      const double P = (double)sigPS[p];
      const double invP = P > 0. ? 1. / P : 0.;
      if (mode == MASS_INVP) {
        v = invP;
      } else if (mode == MASS_PS) {
        v = P;
      } else if (mode == MASS_MEAN) {
        v = 2 * invP + sqrt(invP * fbar);
      } else {
        const int k = (int)(p % g.n);
        const long long ij = p / g.n;
        const int j = (int)(ij % g.n), i = (int)(ij / g.n);
        const double kx = kval(i, g.n, g.kfac), ky = kval(j, g.n, g.kfac), kz = kval(k, g.n, g.kfac);
        const double kr = sqrt(kx * kx + ky * ky + kz * kz);
        double pf = 0.;
        if (kr > 0.) {
          const unsigned long long nbin = (unsigned long long)(kr / dk);
          if (nbin < (unsigned long long)n_bin) pf = Pf[nbin];
        }
        v = 2 * invP + sqrt(invP * pf);
      }
    }
    out[p] = factor * v;
  }
}

// ------------------------------------------------------------------------------------------------------
// Jasche diagonal (likeli_force_1st_order_diagonal_mass, 230-306), by linearity:
//   D_l[i'] = C2R[ sum_j grad_inv_lap_FS_j( R2C[W'_{.l,j}] ) ][i'] / N = sum_{i in S_l} sum_j G_j[(i' - i) mod n] W'_ij
//   G_j = C2R[ grad_inv_lap_FS_j(1) ] / N,   mass_r[i'] = m^2 window[i'] / noise[i']^2 sum_{l: window[l] > 0} D_l[i']^2
// S_l: the particles within 2h of the centre of cell l (W' = 0 beyond, so the sparse sum is the dense one).
// ------------------------------------------------------------------------------------------------------

// grad_inv_lap_FS_j of the all-ones spectrum (gradient.cpp:157-211: -i k_j / k^2, 0 at k = 0 and wherever any index is
// at Nyquist), divided by N, for the three j into Ck[0 .. 3 Nhp).  Padding (k >= nh) gets zeros.  G goes through the
// handle's own C2R plan, so an fp32 handle builds G in float (~1e-7 relative) before it is widened to double -- the one
// place where its mass arithmetic is not double; everything after G is double.
template <typename T>
__global__ void __launch_bounds__(256) k_glap_impulse(Geo g, C2<T> *__restrict__ Ck) {
  const double invN = 1. / (double)g.N;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < g.Nhp;
       idx += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(idx % g.nhp);
    const long long ij = idx / g.nhp;
    const int j = (int)(ij % g.n), i = (int)(ij / g.n);
    const double kx = kval(i, g.n, g.kfac), ky = kval(j, g.n, g.kfac), kz = kval(k, g.n, g.kfac);
    const double kmod = kx * kx + ky * ky + kz * kz;
    const bool zero = k >= g.nh || i == g.n / 2 || j == g.n / 2 || k == g.n / 2 || !(kmod > 0);
    const double f = zero ? 0. : 1 / kmod;
    st2<T>(Ck, idx, 0., -(kx * f) * invN);
    st2<T>(Ck, idx + g.Nhp, 0., -(ky * f) * invN);
    st2<T>(Ck, idx + 2 * g.Nhp, 0., -(kz * f) * invN);
  }
}

// One (particle, cell) pair of S_l: the particle's Lagrangian cell packed as (x << 20 | y << 10 | z) -- the order of
// the flat index i -- and W'_il (Wprime_il, 179-227).
struct JRec {
  int key, pad;
  double wx, wy, wz;
};

struct JaschePar {
  double h, norm;  // SPH scale, 1 / (pi h^5)
  int reach;       // (int)(2h / d) + 1: every cell with q < 2 lies within this many cells of the particle's home cell
};

// Wprime_il for the particle at (x, y, z) and the centre of cell (lx, ly, lz) (no `min` offset), upstream's operation
// order without FMA contraction, pacman_difference's sign quirk kept (pacman.cpp:42-47: d > L/2 becomes L - d).
// false: q >= 2 (W' = 0).
__device__ __forceinline__ bool wprime(const Geo &g, const JaschePar &jp, double x, double y, double z, int lx, int ly,
                                       int lz, double &wx, double &wy, double &wz) {
#pragma clang fp contract(off)
  double d[3] = {x - ((double)lx + 0.5) * g.d, y - ((double)ly + 0.5) * g.d, z - ((double)lz + 0.5) * g.d};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (d[c] > g.L / 2) d[c] = g.L - d[c];
    if (d[c] < -(g.L / 2)) d[c] = g.L + d[c];
  }
  const double r = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const double q = r / jp.h;
  if (q >= 2) return false;
  const double common = q >= 1 ? jp.norm * (3 - 0.75 * q - 3. / q) : jp.norm * (2.25 * q - 3);
  wx = d[0] * common;
  wy = d[1] * common;
  wz = d[2] * common;
  return true;
}

// Count (FILL = false) or place (FILL = true) the pairs (particle, cell l) with q < 2 and window[l] > 0.  One thread
// per particle walks the cells around its home cell; offsets [-R, min(R, n - 1 - R)] visit every residue mod n at
// most once, also where 2R + 1 > n.  The placement order inside a cell is fixed afterwards by k_jasche_sort.
template <typename T, bool FILL>
__global__ void __launch_bounds__(256)
k_jasche_pairs(Geo g, PosPar pp, JaschePar jp, const T *__restrict__ psi, const T *__restrict__ window,
               int *__restrict__ cnt, const int *__restrict__ off, JRec *__restrict__ rec) {
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < g.N; p += (long long)gridDim.x * blockDim.x) {
    const int pk = (int)(p % g.n);
    const long long ij = p / g.n;
    const int pj = (int)(ij % g.n), pi = (int)(ij / g.n);
    T xs, ys, zs;
    particle_pos<T>(pp, pi, pj, pk, psi[p], psi[p + g.N], psi[p + 2 * g.N], xs, ys, zs);
    if (!pos_ok<T>(g, xs, ys, zs)) continue;  // non-finite positions are never used as indices
    const double x = (double)xs, y = (double)ys, z = (double)zs;
    const int hx = min((int)(x / g.d), g.n - 1), hy = min((int)(y / g.d), g.n - 1), hz = min((int)(z / g.d), g.n - 1);
    const int R = jp.reach, hi = min(R, g.n - 1 - R);
    for (int a = -R; a <= hi; a++) {
      const int lx = (hx + a + 2 * g.n) % g.n;
      for (int b = -R; b <= hi; b++) {
        const int ly = (hy + b + 2 * g.n) % g.n;
        for (int c = -R; c <= hi; c++) {
          const int lz = (hz + c + 2 * g.n) % g.n;
          const long long l = lz + (long long)g.n * (ly + (long long)g.n * lx);
          if (!((double)window[l] > 0.)) continue;
          double wx, wy, wz;
          if (!wprime(g, jp, x, y, z, lx, ly, lz, wx, wy, wz)) continue;
          const int slot = atomicAdd(&cnt[l], 1);
          if (FILL && off[l] + slot < off[l + 1]) {  // the counting pass saw the same pairs: always true
            JRec r;
            r.key = (pi << 20) | (pj << 10) | pk;
            r.pad = 0;
            r.wx = wx;
            r.wy = wy;
            r.wz = wz;
            rec[off[l] + slot] = r;
          }
        }
      }
    }
  }
}

// Exclusive prefix sum of n counts into off[0 .. n] with one workgroup (each thread owns a contiguous run); *total gets
// the full 64-bit sum, which the host checks against the int range before any pair is placed.
__global__ void __launch_bounds__(1024) k_jasche_scan(long long n, const int *__restrict__ cnt,
                                                      long long *__restrict__ total, int *__restrict__ off) {
  __shared__ long long part[1024];
  const long long per = (n + blockDim.x - 1) / blockDim.x;
  const long long b = threadIdx.x * per, e = (b + per < n) ? b + per : n;
  long long s = 0;
  for (long long i = b; i < e; i++) s += cnt[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long acc = 0;
    for (unsigned t = 0; t < blockDim.x; t++) {
      const long long v = part[t];
      part[t] = acc;
      acc += v;
    }
    *total = acc;
    off[n] = (int)(acc < 0x7fffffffLL ? acc : 0x7fffffffLL);
  }
  __syncthreads();
  long long acc = part[threadIdx.x];
  for (long long i = b; i < e; i++) {
    off[i] = (int)(acc < 0x7fffffffLL ? acc : 0x7fffffffLL);
    acc += cnt[i];
  }
}

// Orders each cell's pairs by particle index, so that the sums below do not depend on the order the atomics landed in.
// Insertion sort by one thread per cell: O(m^2) in the cell's pair count m (about 33 at h = d); measured 7 ms at 64^3
// against 3.4 s for the sums (profiles/mass_kernel_stats_64.csv).
__global__ void __launch_bounds__(256) k_jasche_sort(long long n, const int *__restrict__ off, JRec *__restrict__ rec) {
  for (long long l = blockIdx.x * (long long)blockDim.x + threadIdx.x; l < n; l += (long long)gridDim.x * blockDim.x) {
    const int b = off[l], e = off[l + 1];
    for (int a = b + 1; a < e; a++) {
      const JRec v = rec[a];
      int c = a - 1;
      while (c >= b && rec[c].key > v.key) {
        rec[c + 1] = rec[c];
        c--;
      }
      rec[c + 1] = v;
    }
  }
}

// acc[i'] += sum_{l in [l0, l1)} D_l[i']^2.  One thread per output i'; every thread walks the same pairs, so the pair
// loads are uniform across the wavefront (broadcasts) and only G is gathered per lane -- consecutive i' read
// consecutive elements of G, which (3 N doubles) stays in L2 / the Infinity Cache.  No atomics: each output is owned by
// one thread and its sums run in a fixed order.
__global__ void __launch_bounds__(256)
k_jasche_accum(Geo g, const JRec *__restrict__ rec, const int *__restrict__ off, long long l0, long long l1,
               const double *__restrict__ G, double *__restrict__ acc) {
  const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (p >= g.N) return;
  const int n = g.n;
  const int zp = (int)(p % n);
  const long long ij = p / n;
  const int yp = (int)(ij % n), xp = (int)(ij / n);
  const double *Gx = G, *Gy = G + g.N, *Gz = G + 2 * g.N;
  double s = acc[p];
  for (long long l = l0; l < l1; l++) {
    const int b = off[l], e = off[l + 1];
    if (b == e) continue;
    double D = 0.;
    for (int r = b; r < e; r++) {
      const JRec v = rec[r];
      int tx = xp - (v.key >> 20), ty = yp - ((v.key >> 10) & 1023), tz = zp - (v.key & 1023);
      tx += tx < 0 ? n : 0;
      ty += ty < 0 ? n : 0;
      tz += tz < 0 ? n : 0;
      const long long gi = tz + (long long)n * (ty + (long long)n * tx);
      D += v.wx * Gx[gi] + v.wy * Gy[gi] + v.wz * Gz[gi];
    }
    s += D * D;
  }
  acc[p] = s;
}

// mass_r = m^2 window / noise^2 sum_l D_l^2   (297, 305)
template <typename T>
__global__ void __launch_bounds__(256)
k_jasche_final(long long N, const double *__restrict__ acc, const T *__restrict__ window, const T *__restrict__ noise,
               double m2, double *__restrict__ out) {
#pragma clang fp contract(off)
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < N; p += (long long)gridDim.x * blockDim.x) {
    const double s = (double)noise[p];
    out[p] = m2 * ((double)window[p] * (acc[p] / (s * s)));
  }
}

}  // namespace bchmc
