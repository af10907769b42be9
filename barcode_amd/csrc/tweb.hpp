// tweb.hpp -- the cosmic-web type of every cell of a sample (bchmc_tweb_*): the tidal tensor T_ab = d_a d_b phi of the
// potential laplace(phi) = x, its three eigenvalues per cell, the number of them above a threshold (0 void, 1 sheet,
// 2 filament, 3 knot; Hahn et al. 2007, Forero-Romero et al. 2009), per-type counts and masses, and the per-cell counters
// of a posterior over an ensemble of samples (Leclercq, Jasche & Wandelt 2015).
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
#pragma once
#include "common.hpp"

namespace bchmc {

constexpr int kTwebBlock = 256;
constexpr int kTwebSweeps = 4;       // cyclic Jacobi sweeps of k_tweb_eigen (tests/tweb_bound.py derives its bound from it)
constexpr int kTwebWords = 9;        // per workgroup and in the result: n_type[4], n_nonfinite, mass_type[4]
constexpr int kTwebNonFinite = 255;  // the type of a cell whose tensor is not finite

// ------------------------------------------------------------------------------------------------------
// One component of the tensor in k-space: out = (k_a k_b / k^2) exp(-k^2 R^2 / 2) / N x^, 0 at k = 0, from the
// unnormalised transform x^ (1 / N is folded in here: the C2R that follows is unnormalised).  a, b: 0, 1, 2 = x, y, z.
// Even n: an off-diagonal component is 0 wherever the index of axis a or of axis b is n / 2 -- there k_a k_b changes
// sign between a mode and its conjugate partner, which is the same stored element, so the product is not the transform
// of a real field; k_a^2 is even and the diagonal components keep those modes.  At odd n no mode is its own partner.
// With this rule every array written here is the transform of a real field and the three diagonal components sum to
// W x^ for every k != 0.  The padding columns k >= nh are processed like data (see Geo).
// half_r2 = R^2 / 2.
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kTwebBlock)
k_tweb_component(Geo g, const C2<T> *__restrict__ xk, C2<T> *__restrict__ out, int a, int b, double half_r2, double inv_n) {
  const int h = g.n / 2;
  const bool even = (g.n & 1) == 0;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < g.Nhp;
       idx += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(idx % g.nhp);
    const long long ij = idx / g.nhp;
    const int j = (int)(ij % g.n), i = (int)(ij / g.n);
    const double kx = kval(i, g.n, g.kfac), ky = kval(j, g.n, g.kfac), kz = kval(k, g.n, g.kfac);
    const double k2 = kx * kx + ky * ky + kz * kz;
    const double ka = a == 0 ? kx : (a == 1 ? ky : kz), kb = b == 0 ? kx : (b == 1 ? ky : kz);
    const int ia = a == 0 ? i : (a == 1 ? j : k), ib = b == 0 ? i : (b == 1 ? j : k);
    double f = 0.;
    if (k2 > 0. && !(even && a != b && (ia == h || ib == h))) f = (ka * kb / k2) * exp(-k2 * half_r2) * inv_n;
    const double2 x = ld2<T>(xk, idx);
    st2<T>(out, idx, f * x.x, f * x.y);
  }
}

// ------------------------------------------------------------------------------------------------------
// Eigenvalues of a real symmetric 3 x 3 matrix by cyclic Jacobi: kTwebSweeps sweeps over the pairs (0, 1), (0, 2),
// (1, 2), written out so that no register array is indexed dynamically.  A rotation is an orthogonal similarity, so
// the method is backward stable whatever the spectrum: a degenerate tensor such as (lambda, 0, 0) in general position --
// the commonest one in the sheets of a smooth field -- comes back to a few ulp of |T|, where the closed form through acos
// loses half the digits (d phi ~ sqrt(eps) at r = +-1).  The matrix is scaled by a power of two first (exact), so
// tensors of any magnitude take the same path.  A sweep starts only while off(T) > eps |T|_F: a diagonal tensor comes
// back as its diagonal, bit for bit.
// ------------------------------------------------------------------------------------------------------
// one rotation annihilating apq; r is the third index
__device__ __forceinline__ void tweb_rotate(double &app, double &aqq, double &apq, double &arp, double &arq) {
  if (apq == 0.) return;
  const double theta = (aqq - app) / (2. * apq);  // +-inf when apq is tiny: t = 0, the rotation is the identity
  const double t = copysign(1., theta) / (fabs(theta) + sqrt(theta * theta + 1.));
  const double c = 1. / sqrt(t * t + 1.), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.;
  const double tp = c * arp - s * arq;
  arq = s * arp + c * arq;
  arp = tp;
}

// l1 >= l2 >= l3.  The six entries must be finite.
__device__ __forceinline__ void tweb_eigenvalues(double a00, double a01, double a02, double a11, double a12, double a22,
                                                 double &l1, double &l2, double &l3) {
  const double m = fmax(fmax(fmax(fabs(a00), fabs(a11)), fmax(fabs(a22), fabs(a01))), fmax(fabs(a02), fabs(a12)));
  int e = 0;
  if (m > 0.) (void)frexp(m, &e);
  const double sc = ldexp(1., -e);
  a00 *= sc, a01 *= sc, a02 *= sc, a11 *= sc, a12 *= sc, a22 *= sc;
  const double eps2 = 4.930380657631324e-32;  // (2^-52)^2
#pragma unroll 1
  for (int sweep = 0; sweep < kTwebSweeps; sweep++) {
    const double off2 = a01 * a01 + a02 * a02 + a12 * a12;
    const double all2 = a00 * a00 + a11 * a11 + a22 * a22 + 2. * off2;
    if (off2 <= eps2 * all2) break;
    tweb_rotate(a00, a11, a01, a02, a12);  // (p, q, r) = (0, 1, 2): a_rp = a02, a_rq = a12
    tweb_rotate(a00, a22, a02, a01, a12);  // (0, 2, 1): a_rp = a01, a_rq = a12
    tweb_rotate(a11, a22, a12, a01, a02);  // (1, 2, 0): a_rp = a01, a_rq = a02
  }
  const double hi = fmax(a00, fmax(a11, a22)), lo = fmin(a00, fmin(a11, a22));
  const double mid = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));
  l1 = ldexp(hi, e), l2 = ldexp(mid, e), l3 = ldexp(lo, e);
}

struct TwebTensor {
  const void *c[6];  // xx, xy, xz, yy, yz, zz: N elements of the storage type each
};

// One thread per cell and trip: six coalesced loads (widened to double), the eigenvalues, the type = the number of them
// strictly above lambda_th, one byte stored, three doubles stored when lam is given (lambda_1 block, lambda_2 block,
// lambda_3 block).  A cell whose tensor is not finite gets type 255 and NaN eigenvalues and counts as non-finite only.
// x: the unsmoothed source in real space (S = double: the staged host array; else the storage type), or null (the
// probe): 1 + x is summed per type.  Workgroup b writes its kTwebWords partials to part[b * kTwebWords ..]: the four
// counts and the non-finite count as 64-bit integers, the four masses as doubles, each summed in a fixed order -- a
// thread's cells in order, then block_sum's tree; the counts travel through it as doubles, exactly (< 2^53).
template <typename T, typename S>
__global__ void __launch_bounds__(kTwebBlock)
k_tweb_eigen(long long N, TwebTensor t, const S *__restrict__ x, double lambda_th, double *__restrict__ lam,
             unsigned char *__restrict__ type, unsigned long long *__restrict__ part) {
  __shared__ double red[kTwebBlock / kWave];
  const T *__restrict__ txx = static_cast<const T *>(t.c[0]), *__restrict__ txy = static_cast<const T *>(t.c[1]);
  const T *__restrict__ txz = static_cast<const T *>(t.c[2]), *__restrict__ tyy = static_cast<const T *>(t.c[3]);
  const T *__restrict__ tyz = static_cast<const T *>(t.c[4]), *__restrict__ tzz = static_cast<const T *>(t.c[5]);
  double n0 = 0., n1 = 0., n2 = 0., n3 = 0., nbad = 0., m0 = 0., m1 = 0., m2 = 0., m3 = 0.;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    const double a00 = (double)txx[i], a01 = (double)txy[i], a02 = (double)txz[i];
    const double a11 = (double)tyy[i], a12 = (double)tyz[i], a22 = (double)tzz[i];
    const bool finite = fabs(a00) <= 1.7976931348623157e308 && fabs(a01) <= 1.7976931348623157e308 &&
                        fabs(a02) <= 1.7976931348623157e308 && fabs(a11) <= 1.7976931348623157e308 &&
                        fabs(a12) <= 1.7976931348623157e308 && fabs(a22) <= 1.7976931348623157e308;
    double l1, l2, l3;
    int ty;
    if (finite) {
      tweb_eigenvalues(a00, a01, a02, a11, a12, a22, l1, l2, l3);
      ty = (l1 > lambda_th ? 1 : 0) + (l2 > lambda_th ? 1 : 0) + (l3 > lambda_th ? 1 : 0);
      const double w = x ? 1. + (double)x[i] : 1.;
      n0 += ty == 0 ? 1. : 0., n1 += ty == 1 ? 1. : 0., n2 += ty == 2 ? 1. : 0., n3 += ty == 3 ? 1. : 0.;
      m0 += ty == 0 ? w : 0., m1 += ty == 1 ? w : 0., m2 += ty == 2 ? w : 0., m3 += ty == 3 ? w : 0.;
    } else {
      l1 = l2 = l3 = __builtin_nan("");
      ty = kTwebNonFinite;
      nbad += 1.;
    }
    type[i] = (unsigned char)ty;
    if (lam) lam[i] = l1, lam[N + i] = l2, lam[2 * N + i] = l3;
  }
  const double sums[kTwebWords] = {block_sum(n0, red), block_sum(n1, red),   block_sum(n2, red),
                                   block_sum(n3, red), block_sum(nbad, red), block_sum(m0, red),
                                   block_sum(m1, red), block_sum(m2, red),   block_sum(m3, red)};
  if (threadIdx.x == 0) {
    unsigned long long *p = part + (size_t)blockIdx.x * kTwebWords;
#pragma unroll
    for (int w = 0; w < 5; w++) p[w] = (unsigned long long)sums[w];
#pragma unroll
    for (int w = 5; w < kTwebWords; w++) p[w] = (unsigned long long)__double_as_longlong(sums[w]);
  }
}

// The reduction of the partials in one fixed order: workgroup w of kTwebWords, one wave, takes word w; lane l adds the
// rows l, l + 64, l + 128, ... in order, then wave_sum's tree.  The counts are added as doubles, exactly (< 2^53).
// (One thread per word walking all rows took 0.57 ms for the 2048 rows of 256^3: 2048 dependent trips to memory.)
__global__ void __launch_bounds__(kWave)
k_tweb_reduce(int nblk, const unsigned long long *__restrict__ part, unsigned long long *__restrict__ res) {
  const int w = blockIdx.x;
  double s = 0.;
  for (int b = threadIdx.x; b < nblk; b += kWave) {
    const unsigned long long v = part[(size_t)b * kTwebWords + w];
    s += w < 5 ? (double)v : __longlong_as_double((long long)v);
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) res[w] = w < 5 ? (unsigned long long)s : (unsigned long long)__double_as_longlong(s);
}

// ------------------------------------------------------------------------------------------------------
// The posterior accumulator: four uint32 counters per cell, type-major (cnt[ty * N + i]).  One more sample: the counter
// of each cell's type + 1.  A thread takes four neighbouring cells per trip, whose types arrive in one 4-byte load (the
// map comes from hipMalloc and 4 p is a multiple of 4); the last N mod 4 cells go one by one.  No cell is touched by two
// threads, nothing is atomic.  A type above 3 (a non-finite cell) adds nothing; the host does not launch this pass
// for a sample that has one.
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTwebBlock)
k_tweb_accumulate(long long N, const unsigned char *__restrict__ type, unsigned int *__restrict__ cnt) {
  const long long quads = N >> 2, stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (long long p = t0; p < quads; p += stride) {
    const unsigned int four = reinterpret_cast<const unsigned int *>(type)[p];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const unsigned int ty = (four >> (8 * e)) & 0xffu;
      if (ty < 4u) cnt[(long long)ty * N + 4 * p + e] += 1u;
    }
  }
  const long long i = 4 * quads + t0;
  if (i < N) {
    const unsigned int ty = type[i];
    if (ty < 4u) cnt[(long long)ty * N + i] += 1u;
  }
}

// another chain's counters (count elements = 4 N) added in; integer adds, so any merge order gives the same bits
__global__ void __launch_bounds__(kTwebBlock)
k_tweb_merge(long long count, const unsigned int *__restrict__ b, unsigned int *__restrict__ cnt) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x)
    cnt[i] += b[i];
}

// probability of one type: (double)count / (double)samples, IEEE divide
__global__ void __launch_bounds__(kTwebBlock)
k_tweb_probability(long long N, const unsigned int *__restrict__ cnt, double samples, double *__restrict__ out) {
#pragma clang fp contract(off)
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x)
    out[i] = (double)cnt[i] / samples;
}

}  // namespace bchmc
