// xtile_kernels.hpp -- the permutation passes around the x-column tile layout (xtile.hpp): the weight pair once per upload,
// the closing pass of a tiled trajectory, and the un-tiling k_scale_c of the early q.  None of them runs inside a step.
// Include after kernels.hpp (bchmc.hip, fft_probe.hip).
#pragma once
#include "common.hpp"
#include "xtile.hpp"

namespace bchmc {

// pair[e] = {wS, wM} of the element whose tiled index is e: contiguous 16-byte stores, the reads are the 64-byte
// segments.  kb: elements per row of a tile (pass_kb of the storage type).
__global__ void __launch_bounds__(256)
k_xtile_weights(Geo g, int kb, const double *__restrict__ wS, const double *__restrict__ wM, double2 *__restrict__ pair) {
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < g.Nhp; e += (long long)gridDim.x * blockDim.x) {
    const long long idx = xtile_inverse(g.n, g.nhp, kb, e);
    pair[e] = make_double2(wS[idx], wM[idx]);
  }
}

// The closing pass of a tiled trajectory, in k_rollback's place.  q[b], p[b] are the ping-pong pairs, tiled; boundary s
// read pair (s + 1) % 2 (the opening wrote pair 1).  `fin` is the pair the last boundary read.
//   Not stopped: the final q, tiled in q[fin], goes natural into q_dst (the other pair's q, which nobody reads any more; the
//     last boundary has written p natural beside it).
//   Stopped by boundary s >= 1 (k_rollback's comment): q of the pair boundary s - 1 read and the mean of the momenta it read
//     and wrote go natural into sq, sp -- scratch, because either pair may be a source here; k_xtile_restore copies them on.
template <typename T>
__global__ void __launch_bounds__(256)
k_xtile_finish(Geo g, const int *__restrict__ stop, const unsigned long long *__restrict__ steps_done, const C2<T> *q0,
               const C2<T> *p0, const C2<T> *q1, const C2<T> *p1, int fin, C2<T> *q_dst, C2<T> *sq, C2<T> *sp) {
  constexpr int KB = 128 / (int)sizeof(C2<T>);
  const bool stopped = *stop != 0;
  const unsigned long long s = *steps_done;
  const bool read_is_0 = stopped ? (s & 1) == 0 : fin == 0;  // boundary s - 1 read pair s % 2
  const C2<T> *qr = read_is_0 ? q0 : q1, *pr = read_is_0 ? p0 : p1, *pw = read_is_0 ? p1 : p0;
  C2<T> *qd = stopped ? sq : q_dst;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < g.Nhp; i += (long long)gridDim.x * blockDim.x) {
    const long long e = xtile_of(g.n, g.nhp, KB, i);
    const double2 q = ld2<T>(qr, e);
    st2<T>(qd, i, q.x, q.y);
    if (stopped) {
      const double2 a = ld2<T>(pr, e), b = ld2<T>(pw, e);
      st2<T>(sp, i, 0.5 * a.x + 0.5 * b.x, 0.5 * a.y + 0.5 * b.y);
    }
  }
}
template <typename T>
__global__ void __launch_bounds__(256)
k_xtile_restore(long long n, const int *__restrict__ stop, const C2<T> *__restrict__ sq, const C2<T> *__restrict__ sp,
                C2<T> *__restrict__ q_dst, C2<T> *__restrict__ p_dst) {
  if (!*stop) return;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    q_dst[i] = sq[i];
    p_dst[i] = sp[i];
  }
}

// k_scale_c from a tiled source: out (natural) = in (tiled) * s
template <typename T>
__global__ void __launch_bounds__(256)
k_xtile_scale_c(Geo g, const C2<T> *__restrict__ in, C2<T> *__restrict__ out, double s) {
  constexpr int KB = 128 / (int)sizeof(C2<T>);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < g.Nhp; i += (long long)gridDim.x * blockDim.x) {
    const double2 v = ld2<T>(in, xtile_of(g.n, g.nhp, KB, i));
    st2<T>(out, i, v.x * s, v.y * s);
  }
}

}  // namespace bchmc
