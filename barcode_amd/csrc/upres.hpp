// upres.hpp -- the up-resolving steps of tools/2D_corr_fct_interp.cc: interp_field (tools/interp_upres.cc:59-86, CIC
// interpolation of a field onto another grid) and the zero-padded embedding of a power spectrum in a finer
// half-complex array (measure_corr2D_FFTzeropad, 2D_corr_fct_interp.cc:205-222).
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
#pragma once
#include "common.hpp"

namespace bchmc {

// ------------------------------------------------------------------------------------------------------
// interp_field: out(io, jo, ko) = interpolate_CIC (interpolate_grid.cpp:82-103) of the n^3 field `in` at the centre of
// fine cell (io, jo, ko).  The grid is a cube, so one host table serves the three axes: cell pair (i0[m], i1[m]) and
// weight dx[m] of fine index m, tx = 1 - dx (getCICcells / getCICweights, made on the host in the reference's own
// double expressions: the pair depends on the rounding of xpos / d).
// One workgroup per fine row (io, jo): the four coarse rows (i0 | i1, j0 | j1) go to LDS, threads run along ko, so every
// global load and store is a contiguous row.  The eight terms and their products are in the reference's order
// (interpolate_grid.cpp:92-99, `F * wx * wy * wz` left to right), in double, without FMA contraction: on an fp64
// handle the result is the reference's bit for bit.  n_out < n (down-sampling) is legal, as in the tool.
// LDS: 4 n elements of T (32 KiB at n = 1024 in fp64).
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
k_interp_cic(int n, int n_out, const T *__restrict__ in, T *__restrict__ out, const int *__restrict__ i0,
             const int *__restrict__ i1, const double *__restrict__ dx) {
#pragma clang fp contract(off)
  extern __shared__ double s_rows_raw[];
  T *s_rows = reinterpret_cast<T *>(s_rows_raw);  // [4][n]: (i0, j0), (i1, j0), (i0, j1), (i1, j1)
  const int io = blockIdx.x / n_out, jo = blockIdx.x - io * n_out, t = threadIdx.x, bd = blockDim.x;
  const int ia = i0[io], ib = i1[io], ja = i0[jo], jb = i1[jo];
  const T *r00 = in + ((long long)ia * n + ja) * n, *r10 = in + ((long long)ib * n + ja) * n;
  const T *r01 = in + ((long long)ia * n + jb) * n, *r11 = in + ((long long)ib * n + jb) * n;
  for (int k = t; k < n; k += bd) {
    s_rows[k] = r00[k];
    s_rows[n + k] = r10[k];
    s_rows[2 * n + k] = r01[k];
    s_rows[3 * n + k] = r11[k];
  }
  __syncthreads();
  const double dx0 = dx[io], tx0 = 1. - dx0, dx1 = dx[jo], tx1 = 1. - dx1;
  T *o = out + ((long long)io * n_out + jo) * n_out;
  for (int ko = t; ko < n_out; ko += bd) {
    const int ka = i0[ko], kb = i1[ko];
    const double dx2 = dx[ko], tx2 = 1. - dx2;
    const double f000 = (double)s_rows[ka], f100 = (double)s_rows[n + ka], f010 = (double)s_rows[2 * n + ka],
                 f110 = (double)s_rows[3 * n + ka];
    const double f001 = (double)s_rows[kb], f101 = (double)s_rows[n + kb], f011 = (double)s_rows[2 * n + kb],
                 f111 = (double)s_rows[3 * n + kb];
    const double v = f000 * tx0 * tx1 * tx2 + f100 * dx0 * tx1 * tx2 + f010 * tx0 * dx1 * tx2 + f001 * tx0 * tx1 * dx2 +
                     f110 * dx0 * dx1 * tx2 + f101 * dx0 * tx1 * dx2 + f011 * tx0 * dx1 * dx2 + f111 * dx0 * dx1 * dx2;
    o[ko] = (T)v;
  }
}

// ------------------------------------------------------------------------------------------------------
// The zero-padded power spectrum: a gather over the fine half-complex array `out` (geometry f), which writes every
// element once -- the row padding of `out` too, with 0 -- so no memset comes before it.  The tool's map of a coarse
// index (2D_corr_fct_interp.cc:205-222) is I = i for i < n / 2, else n_out - (n - i), the same for J, and K = k for
// k <= n / 2 (integer n / 2, literally, for odd n too); upres_src inverts it (-1: no coarse mode lands on I).  It is
// one-to-one for n_out >= n only, which the host checks.
// Value: |x^(i, j, k)|^2 * scale in double, rounded once to T; imaginary part 0 (U2: the tool carries i Im x^, which
// cancels in every bin); 0 where no coarse mode lands.
// K = 0 plane (U1): the tool sends row i = n / 2 to frequency -n / 2 only, so for n_out > n its K = 0 plane is not
// Hermitian, and its complex-to-real transform returns the transform of the Hermitian part.  That part is written here
// explicitly, (P(I, J, 0) + P(-I mod n_out, -J mod n_out, 0)) / 2, so the transform is never handed anything else.
// ------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int upres_src(int I, int n, int n_out) {
  if (I < n / 2) return I;
  const int i = I - (n_out - n);
  return (i >= n / 2 && i < n) ? i : -1;
}

template <typename T>
__device__ __forceinline__ double upres_power(const Geo &c, const C2<T> *__restrict__ xk, int I, int J, int K, int n_out) {
  const int i = upres_src(I, c.n, n_out), j = upres_src(J, c.n, n_out);
  if (i < 0 || j < 0 || K > c.n / 2) return 0.;
  const double2 x = ld2<T>(xk, K + (long long)c.nhp * (j + (long long)c.n * i));
  return x.x * x.x + x.y * x.y;
}

template <typename T>
__global__ void __launch_bounds__(256)
k_zeropad_embed(Geo c, Geo f, const C2<T> *__restrict__ xk, C2<T> *__restrict__ out, double scale) {
  const int no = f.n;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < f.Nhp;
       idx += (long long)gridDim.x * blockDim.x) {
    const long long ij = idx / f.nhp;
    const int K = (int)(idx - ij * f.nhp), I = (int)(ij / no), J = (int)(ij - (long long)I * no);
    double v = 0.;
    if (K < f.nh) {
      v = upres_power<T>(c, xk, I, J, K, no);
      if (K == 0) v = 0.5 * (v + upres_power<T>(c, xk, I ? no - I : 0, J ? no - J : 0, 0, no));
    }
    st2<T>(out, idx, v * scale, 0.);
  }
}

}  // namespace bchmc
