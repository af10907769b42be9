// mt_draw.hpp -- draw_momenta (HMC_momenta.cc:42-94) on the device from the caller's GSL mt19937 stream.
//
// The reference takes every random number of an HMC attempt from ONE serial gsl_rng (mt19937): 2 n^3 polar
// Box-Muller Gaussians for the Fourier-space momenta, in the shell-by-shell order of
// resolution_independent_random_grid_FS (random.hpp:35-120), then n^3 more for a real-space mass.  Three facts make
// that draw parallel without changing a single number:
//   * MT19937 is linear over GF(2): the word sequence x_k (k >= 1 after any state) satisfies the recurrence of its
//     characteristic polynomial phi (degree 19937), so x_{P+J+t} = sum_i c_i x_{P+1+i+t} with x^(J-1) mod phi =
//     sum_i c_i x^i.  A segment of the stream starts from the XOR of 624-word windows of the first 20560 words
//     (jump-ahead, Haramoto et al. 2008): one workgroup per segment.
//   * gsl_ran_gaussian skips zero words (uniform_pos) and rejects a pair when r2 > 1 or r2 == 0; both depend on the
//     words alone, so the g-th Gaussian is located by two prefix sums: over non-zero words (pairing parity) and over
//     accepted pairs.
//   * the walk of random_grid_FS has a closed form (mt_walk_index): layer L = max of the corner-folded coordinates
//     starts at cell (2L)^3.
// Host side (once per handle): phi by Berlekamp-Massey over one output bit, the segment jump polynomials by
// carry-less multiplication with a byte-table reduction.  DESIGN.md "Exact momentum draw" has the arithmetic and
// the measured costs.
#pragma once
#include "common.hpp"

#include <cmath>
#include <cstring>
#include <vector>
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <wmmintrin.h>
#define BCHMC_MT_PCLMUL 1
#endif

namespace bchmc {

constexpr int kMtN = 624, kMtM = 397;
constexpr int kMtDeg = 19937;                   // degree of phi = dimension of the MT19937 state
constexpr int kMtWin = kMtDeg + kMtN - 1;       // 20560 words: every window x_{P+1+i .. P+i+624}, i < 19937
constexpr int kMtPolyWords = kMtN;              // a residue mod phi as 624 uint32 words (19937 bits used)
constexpr int kMtThreads = 1024;
constexpr int kMtTile = 4 * kMtThreads;         // words per tile of the pairing kernel
constexpr size_t kMtSegLds = (size_t)(kMtWin + 4 * kMtN) * sizeof(uint32_t);  // 92224 B: window + 4 partial states

__host__ __device__ __forceinline__ uint32_t mt_next(uint32_t x0, uint32_t x1, uint32_t xm) {
  const uint32_t y = (x0 & 0x80000000U) | (x1 & 0x7fffffffU);
  return xm ^ (y >> 1) ^ ((y & 1U) ? 0x9908b0dfU : 0U);
}
__host__ __device__ __forceinline__ uint32_t mt_temper(uint32_t k) {
  k ^= (k >> 11);
  k ^= (k << 7) & 0x9d2c5680U;
  k ^= (k << 15) & 0xefc60000U;
  k ^= (k >> 18);
  return k;
}

// Position of cell (a, b, c) of the n^3 cube in the walk of resolution_independent_random_grid_FS (random.hpp:64-112,
// half_size = false).  Coordinates fold onto the corner they are nearest to (f = min(a, n-1-a), mirror bit s); the
// walk visits layer L = max(fa, fb, fc) after the (2L)^3 cells of the inner layers.  Per layer: for each k = fc <= L
// the "slim" side (fa = L, fb < L: 8 L cells) then the "broad" side (fb = L, fa <= L: 8 (L+1) cells), then the
// "roof" (fc = L, fa, fb < L); within each position the 8 mirrors in the order sa + 2 sb + 4 sc.
__host__ __device__ __forceinline__ unsigned long long mt_walk_index(int n, int a, int b, int c) {
  const int m = n - 1;
  const int sa = a > m - a, sb = b > m - b, sc = c > m - c;
  const long long fa = sa ? m - a : a, fb = sb ? m - b : b, fc = sc ? m - c : c;
  const long long L = fa > fb ? (fa > fc ? fa : fc) : (fb > fc ? fb : fc);
  const long long corner = sa + 2 * sb + 4 * sc;
  long long idx = 8 * L * L * L;
  if (fa < L && fb < L) {  // roof (fc == L)
    idx += 8 * (L + 1) * (2 * L + 1) + 8 * (fa * L + fb);
  } else if (fb < L) {     // slim side: fa == L
    idx += fc * (16 * L + 8) + 8 * fb;
  } else {                 // broad side: fb == L
    idx += fc * (16 * L + 8) + 8 * L + 8 * fa;
  }
  return (unsigned long long)(idx + corner);
}

// r2 of gsl_ran_gaussian (randist/gauss.c) with separately rounded products and sum, as a non-FMA GSL build forms it:
// a fused x*x + y*y moves accept / reject decisions at the r2 == 1 boundary.
__device__ __forceinline__ double mt_polar_r2(double x, double y) {
#pragma clang fp contract(off)
  return x * x + y * y;
}

// ---- device kernels ----------------------------------------------------------------------------------------

// b = the 624 words after block a (x_{q+624+k} = f(x_{q+k}, x_{q+k+1}, x_{q+k+397})), in three dependency phases.
__device__ __forceinline__ void mt_block_next(const uint32_t *a, uint32_t *b, int t) {
  if (t < 227) b[t] = mt_next(a[t], a[t + 1], a[t + kMtM]);
  __syncthreads();
  if (t >= 227 && t < 454) b[t] = mt_next(a[t], a[t + 1], b[t - 227]);
  __syncthreads();
  if (t >= 454 && t < kMtN) b[t] = mt_next(a[t], t < kMtN - 1 ? a[t + 1] : b[0], b[t - 227]);
  __syncthreads();
}

// win[0 .. 624 nblk) = x_{P ...} from the window st = x_{P .. P+623} (one workgroup).
__global__ void __launch_bounds__(kMtThreads) k_mt_window(const uint32_t *__restrict__ st, uint32_t *__restrict__ win,
                                                           int nblk) {
  __shared__ uint32_t buf[2][kMtN];
  const int t = threadIdx.x;
  if (t < kMtN) buf[0][t] = st[t];
  __syncthreads();
  for (int r = 0; r < nblk; r++) {
    const uint32_t *a = buf[r & 1];
    if (t < kMtN) win[(size_t)r * kMtN + t] = a[t];
    if (r + 1 < nblk) mt_block_next(a, buf[(r + 1) & 1], t);
  }
}

// One workgroup per segment b: start state = the window itself (b = 0) or the XOR of the windows x_{P+1+i ..} over
// the set bits i of poly[b-1] = x^(b S - 1) mod phi; then S untempered words into words[b S ..] and their count of
// non-zero words into nz[b] (tempering maps 0 to 0 and nothing else to 0).
__global__ void __launch_bounds__(kMtThreads) k_mt_segments(const uint32_t *__restrict__ win,
                                                             const uint32_t *__restrict__ poly, long long S,
                                                             uint32_t *__restrict__ words,
                                                             unsigned long long *__restrict__ nz) {
  extern __shared__ uint32_t lds[];
  uint32_t *w = lds, *part = lds + kMtWin;
  const int t = threadIdx.x, b = blockIdx.x;
  if (b == 0) {
    if (t < kMtN) w[t] = win[t];
  } else {
    for (int i = t; i < kMtWin; i += kMtThreads) w[i] = win[1 + i];
    __syncthreads();
    // 4 groups of 256 threads split the polynomial's 624 words; each thread accumulates state words l, l+256, l+512
    const int g = t >> 8, l = t & 255;
    const uint32_t *pb = poly + (size_t)(b - 1) * kMtPolyWords;
    uint32_t a0 = 0, a1 = 0, a2 = 0;
    const bool has2 = l + 512 < kMtN;
    for (int wd = g * (kMtPolyWords / 4); wd < (g + 1) * (kMtPolyWords / 4); wd++) {
      uint32_t bits = pb[wd];
      while (bits) {
        const int i = wd * 32 + __builtin_ctz(bits);
        bits &= bits - 1;
        const uint32_t *src = w + i + l;
        a0 ^= src[0];
        a1 ^= src[256];
        if (has2) a2 ^= src[512];
      }
    }
    part[g * kMtN + l] = a0;
    part[g * kMtN + l + 256] = a1;
    if (has2) part[g * kMtN + l + 512] = a2;
    __syncthreads();
    if (t < kMtN) w[t] = part[t] ^ part[kMtN + t] ^ part[2 * kMtN + t] ^ part[3 * kMtN + t];
  }
  __syncthreads();
  // generate: two 624-word blocks at the start of w (the window is no longer needed)
  uint32_t *buf[2] = {w, w + kMtN};
  const long long nblk = S / kMtN;
  unsigned cnt = 0;
  uint32_t *out = words + (size_t)b * (size_t)S;
  for (long long r = 0; r < nblk; r++) {
    const uint32_t *a = buf[r & 1];
    if (t < kMtN) {
      const uint32_t x = a[t];
      out[r * kMtN + t] = x;
      cnt += x != 0;
    }
    if (r + 1 < nblk) mt_block_next(a, buf[(r + 1) & 1], t);
  }
  // workgroup sum
  __shared__ unsigned red[kMtThreads / kWave];
  for (int off = kWave / 2; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, kWave);
  if ((t & (kWave - 1)) == 0) red[t / kWave] = cnt;
  __syncthreads();
  if (t == 0) {
    unsigned long long s = 0;
    for (int i = 0; i < kMtThreads / kWave; i++) s += red[i];
    nz[b] = s;
  }
}

// Exclusive scan of v[0 .. n) within one workgroup of kMtThreads; returns the total (all threads).
__device__ __forceinline__ unsigned long long mt_block_scan(unsigned long long v, unsigned long long *excl) {
  __shared__ unsigned long long wsum[kMtThreads / kWave];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  unsigned long long inc = v;
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned long long o = __shfl_up(inc, off, kWave);
    if (lane >= off) inc += o;
  }
  if (lane == kWave - 1) wsum[wv] = inc;
  __syncthreads();
  unsigned long long before = 0, total = 0;
  for (int i = 0; i < kMtThreads / kWave; i++) {
    const unsigned long long s = wsum[i];
    if (i < wv) before += s;
    total += s;
  }
  __syncthreads();  // wsum is reused by the next call
  *excl = before + inc - v;
  return total;
}

// out[b] = sum of in[0 .. b) (one workgroup); res[slot] = total.  With lastend: res[1] = the largest lastend.
__global__ void __launch_bounds__(kMtThreads) k_mt_scan(const unsigned long long *__restrict__ in, int n,
                                                         unsigned long long *__restrict__ out,
                                                         unsigned long long *__restrict__ res, int slot,
                                                         const unsigned long long *__restrict__ lastend) {
  unsigned long long carry = 0, mx = 0;
  for (int base = 0; base < n; base += kMtThreads) {
    const int i = base + (int)threadIdx.x;
    const unsigned long long v = i < n ? in[i] : 0;
    if (lastend && i < n && lastend[i] > mx) mx = lastend[i];
    unsigned long long ex;
    const unsigned long long tot = mt_block_scan(v, &ex);
    if (i < n) out[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) res[slot] = carry;
  if (lastend) {
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_down(mx, off, kWave);
      mx = o > mx ? o : mx;
    }
    __shared__ unsigned long long wmx[kMtThreads / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) wmx[threadIdx.x / kWave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < kMtThreads / kWave; i++) mx = wmx[i] > mx ? wmx[i] : mx;
      res[1] = mx;
    }
  }
}

// Polar Box-Muller over segment b's pairs: the pairs whose first word lies in the segment (the second may lie in a
// later one).  nzoff[b] = non-zero words before the segment: when odd, its first non-zero word completes the last
// pair of an earlier segment.  Count pass (EMIT = false): acc[b] = accepted pairs, lastend[b] = 1 + position of the
// second word of the segment's last complete pair.  Emit pass: Gaussian accoff[b] + r goes to gauss[..] while below
// G; the one numbered G - 1 records 1 + the position of its second word in res[2] (= words used by this pass).
// SPLIT: gauss[2 g], gauss[2 g + 1] = y and sqrt(-2 log r2 / r2) apart, for callers that form gsl_ran_gaussian's
// sigma * y * root in GSL's product order (mock.hpp); the unit Gaussian y * root otherwise.
template <bool EMIT, bool SPLIT = false>
__global__ void __launch_bounds__(kMtThreads) k_mt_pairs(const uint32_t *__restrict__ words, long long C, long long S,
                                                          const unsigned long long *__restrict__ nzoff,
                                                          const unsigned long long *__restrict__ accoff,
                                                          unsigned long long *__restrict__ acc,
                                                          unsigned long long *__restrict__ lastend, long long G,
                                                          double *__restrict__ gauss,
                                                          unsigned long long *__restrict__ res) {
  __shared__ uint32_t cv[kMtTile + 1], cp[kMtTile + 1];
  const int t = threadIdx.x, b = blockIdx.x;
  const long long s0 = (long long)b * S, s1 = s0 + S;
  int skip = (int)(nzoff[b] & 1ull), carry = 0;
  unsigned long long nacc = 0, last = 0;
  const unsigned long long g0 = EMIT ? accoff[b] : 0;
  auto emit = [&](double y, double r2, unsigned long long gi, uint32_t p2) {
    if (gi < (unsigned long long)G) {
      if (SPLIT) {
        gauss[2 * gi] = y;
        gauss[2 * gi + 1] = sqrt(-2.0 * log(r2) / r2);
      } else {
        gauss[gi] = y * sqrt(-2.0 * log(r2) / r2);
      }
      if (gi == (unsigned long long)G - 1) res[2] = (unsigned long long)p2 + 1;
    }
  };
  for (long long base = s0; base < s1; base += kMtTile) {
    const long long p = base + 4 * (long long)t;
    uint32_t v[4] = {0, 0, 0, 0};
    if (p < s1) {  // S and the tile are multiples of 4 words
      const uint4 q = *reinterpret_cast<const uint4 *>(words + p);
      v[0] = mt_temper(q.x), v[1] = mt_temper(q.y), v[2] = mt_temper(q.z), v[3] = mt_temper(q.w);
    }
    const unsigned c = (v[0] != 0) + (v[1] != 0) + (v[2] != 0) + (v[3] != 0);
    unsigned long long ex;
    const int tot = (int)mt_block_scan(c, &ex);
    int o = carry + (int)ex;
    for (int q = 0; q < 4; q++)
      if (v[q]) {
        cv[o] = v[q];
        cp[o] = (uint32_t)(p + q);
        o++;
      }
    __syncthreads();
    const int M = carry + tot;
    int avail = M - skip, j0 = skip;
    if (avail < 0) avail = 0;
    else skip = 0;
    const int np = avail / 2;
    // thread t: pairs 2t and 2t+1 of the tile (pair order = thread order for the scan)
    double ys[2] = {0., 0.}, r2s[2] = {1., 1.};
    unsigned ok[2] = {0, 0};
    for (int e = 0; e < 2; e++) {
      const int pi = 2 * t + e;
      if (pi < np) {
        const int j = j0 + 2 * pi;
        const double x = -1.0 + 2.0 * ((double)cv[j] * (1.0 / 4294967296.0));
        const double y = -1.0 + 2.0 * ((double)cv[j + 1] * (1.0 / 4294967296.0));
        const double r2 = mt_polar_r2(x, y);
        ok[e] = !(r2 > 1.0 || r2 == 0);
        ys[e] = y, r2s[e] = r2;
      }
    }
    unsigned long long aex;
    const unsigned long long atot = mt_block_scan(ok[0] + ok[1], &aex);
    if (EMIT) {
      unsigned long long gi = g0 + nacc + aex;
      for (int e = 0; e < 2; e++)
        if (ok[e]) emit(ys[e], r2s[e], gi++, cp[j0 + 2 * (2 * t + e) + 1]);
    }
    nacc += atot;
    if (np > 0) last = (unsigned long long)cp[j0 + 2 * np - 1] + 1;
    const int ncarry = (avail & 1);
    __syncthreads();
    if (ncarry && t == 0) {
      cv[0] = cv[M - 1];
      cp[0] = cp[M - 1];
    }
    carry = ncarry;
    __syncthreads();
  }
  // a first word left over: its partner is the next non-zero word after the segment (usually the very first one)
  if (carry && t == 0) {
    for (long long p = s1; p < C; p++) {
      const uint32_t y2 = mt_temper(words[p]);
      if (!y2) continue;
      const double x = -1.0 + 2.0 * ((double)cv[0] * (1.0 / 4294967296.0));
      const double y = -1.0 + 2.0 * ((double)y2 * (1.0 / 4294967296.0));
      const double r2 = mt_polar_r2(x, y);
      const bool okk = !(r2 > 1.0 || r2 == 0);
      if (EMIT && okk) emit(y, r2, g0 + nacc, (uint32_t)p);
      nacc += okk;
      last = (unsigned long long)p + 1;
      break;
    }
  }
  if (!EMIT && t == 0) {
    acc[b] = nacc;
    lastend[b] = last;
  }
}

// State GSL holds after the pass: position Q = P + res[2] (P = the pass's start, counted from the first word of the
// caller's mt[] block), mti = (Q - 1) mod 624 + 1, mt[] = x_{Q-mti ..}.  res[3] = 1 when those 624 words lie in this
// pass's buffer (else the host jumps there).
__global__ void k_mt_final(const uint32_t *__restrict__ words, long long C, unsigned long long P,
                           unsigned long long *__restrict__ res, uint32_t *__restrict__ st_out) {
  const unsigned long long end = res[2];
  const unsigned long long Q = P + end;
  const long long base = (long long)(Q - ((Q - 1) % kMtN + 1));
  const long long off = base - (long long)P;
  const bool in = end > 0 && Q > 0 && off >= 0 && off + kMtN <= C;
  for (int t = threadIdx.x; t < kMtN; t += blockDim.x)
    if (in) st_out[t] = words[off + t];
  if (threadIdx.x == 0) res[3] = in ? 1 : 0;
}

// create_GARFIELD's Hermitian assembly (random.cpp:48-511: its 27 index classes are one rule) straight into the
// half-complex momenta: one thread per (i, j, k) in [0, n/2]^3, Gaussians 2c and 2c+1 for walk cell c.  Only elements
// with k <= n/2 exist in cp (element (a, b, c) at c + nhp (b + n a)); cp = R2C[C2R[G] / N] = G for the Hermitian G.
template <typename T>
__global__ void k_mt_place(int n, int nhp, const double *__restrict__ g, const T *__restrict__ power, double amp,
                           C2<T> *__restrict__ cp) {
  const int h = n / 2;
  const long long tot = (long long)(h + 1) * (h + 1) * (h + 1);
  for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x; id < tot;
       id += (long long)gridDim.x * blockDim.x) {
    const int i = (int)(id / ((h + 1) * (h + 1))), j = (int)((id / (h + 1)) % (h + 1)), k = (int)(id % (h + 1));
    const double sigma = sqrt(amp * (double)power[k + (long long)n * (j + (long long)n * i)] / 2.);
    const int idx[3] = {i, j, k};
    int freeax[3], nfree = 0;
    for (int a = 0; a < 3; a++)
      if (idx[a] > 0 && idx[a] < h) freeax[nfree++] = a;
    if (nfree == 0) {
      double re = 0.;
      if (i || j || k) re = g[2 * mt_walk_index(n, i, j, k)] * (sqrt(2.) * sigma);
      st2<T>(cp, k + (long long)nhp * (j + (long long)n * i), re, 0.);
      continue;
    }
    const int nrep = nfree == 3 ? 4 : (nfree == 2 ? 2 : 1);
    for (int r = 0; r < nrep; r++) {
      int a[3] = {i, j, k};
      if (r > 0) {
        const int ax = nfree == 3 ? freeax[r - 1] : freeax[0];
        a[ax] = n - a[ax];
      }
      int bb[3];
      for (int q = 0; q < 3; q++) bb[q] = (n - a[q]) % n;
      const unsigned long long c = mt_walk_index(n, a[0], a[1], a[2]);
      const double re = g[2 * c] * sigma, im = g[2 * c + 1] * sigma;
      if (a[2] <= h) st2<T>(cp, a[2] + (long long)nhp * (a[1] + (long long)n * a[0]), re, im);
      if (bb[2] <= h) st2<T>(cp, bb[2] + (long long)nhp * (bb[1] + (long long)n * bb[0]), re, -im);
    }
  }
}

// draw_real_space_momenta (HMC_momenta.cc:76-94): out[t] = sqrt(mass_r[t]) * gaussian t, cells in (i, j, k) order
template <typename T>
__global__ void k_mt_real_space(long long N, const double *__restrict__ g, const T *__restrict__ mass_r,
                                T *__restrict__ out) {
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < N; t += (long long)gridDim.x * blockDim.x)
    out[t] = (T)(sqrt((double)mass_r[t]) * g[t]);
}

// ---- host side: GF(2) polynomials modulo phi ---------------------------------------------------------------
namespace mt_host {

constexpr int kW = (kMtDeg + 63) / 64;  // 312 64-bit words per residue
using Poly = std::vector<uint64_t>;

#ifdef BCHMC_MT_PCLMUL
__attribute__((target("pclmul,sse2"))) inline void clmul(uint64_t a, uint64_t b, uint64_t &lo, uint64_t &hi) {
  const __m128i r = _mm_clmulepi64_si128(_mm_cvtsi64_si128((long long)a), _mm_cvtsi64_si128((long long)b), 0);
  lo = (uint64_t)_mm_cvtsi128_si64(r);
  hi = (uint64_t)_mm_cvtsi128_si64(_mm_unpackhi_epi64(r, r));
}
#else
inline void clmul(uint64_t a, uint64_t b, uint64_t &lo, uint64_t &hi) {
  uint64_t l = 0, h = 0;
  for (int i = 0; i < 64; i++)
    if ((b >> i) & 1) {
      l ^= a << i;
      if (i) h ^= a >> (64 - i);
    }
  lo = l, hi = h;
}
#endif

inline int getbit(const uint64_t *p, long long i) { return (int)((p[i >> 6] >> (i & 63)) & 1); }
inline uint64_t get64(const uint64_t *p, size_t nw, long long bit) {  // bits [bit, bit+64), zero beyond the array
  const long long w = bit >> 6;
  const int s = (int)(bit & 63);
  const uint64_t lo = (size_t)w < nw ? p[w] : 0, hi = (size_t)(w + 1) < nw ? p[w + 1] : 0;
  return s ? (lo >> s) | (hi << (64 - s)) : lo;
}
// r ^= a << sh (a: na words)
inline void xor_shifted(uint64_t *r, size_t nr, const uint64_t *a, size_t na, long long sh) {
  const size_t w = (size_t)(sh >> 6);
  const int s = (int)(sh & 63);
  for (size_t i = 0; i < na; i++) {
    if (w + i < nr) r[w + i] ^= a[i] << s;
    if (s && w + i + 1 < nr) r[w + i + 1] ^= a[i] >> (64 - s);
  }
}

struct Phi {
  Poly low;                   // phi - x^19937
  std::vector<Poly> tab;      // tab[v] = v(x) x^19937 mod phi, v < 256
  bool ok = false;
};

// phi by Berlekamp-Massey over bit 0 of x_1, x_2, ... (any non-zero bit sequence of the stream has phi as its minimal
// polynomial: phi is primitive, the period 2^19937 - 1 a Mersenne prime).
inline Phi make_phi() {
  Phi P;
  const int nbits = 2 * kMtDeg + 200;
  std::vector<uint32_t> x(kMtN);
  x[0] = 5489U;
  for (int i = 1; i < kMtN; i++) x[i] = 1812433253U * (x[i - 1] ^ (x[i - 1] >> 30)) + (uint32_t)i;
  x.reserve(nbits + kMtN + 1);
  while ((int)x.size() < nbits + 1) {
    const size_t k = x.size() - kMtN;
    x.push_back(mt_next(x[k], x[k + 1], x[k + kMtM]));
  }
  // reversed sequence s_n = bit 0 of x_{1+n}: rv bit (nbits-1-n) = s_n
  const size_t nw = (nbits + 63) / 64;
  Poly rv(nw, 0);
  for (int n = 0; n < nbits; n++)
    if (x[1 + n] & 1) rv[(nbits - 1 - n) >> 6] |= 1ull << ((nbits - 1 - n) & 63);
  const size_t cw = nw + 2;
  Poly Cp(cw, 0), Bp(cw, 0), Tp;
  Cp[0] = Bp[0] = 1;
  int L = 0, m = 1;
  for (int n = 0; n < nbits; n++) {
    const long long o = nbits - 1 - n;  // d = sum_{i=0..L} c_i s_{n-i} = parity(C & rv[o ..])
    uint64_t acc = 0;
    for (int w = 0; w <= L / 64; w++) acc ^= Cp[w] & get64(rv.data(), nw, o + 64LL * w);
    if (!__builtin_parityll(acc)) {
      m++;
    } else if (2 * L <= n) {
      Tp = Cp;
      xor_shifted(Cp.data(), cw, Bp.data(), cw, m);
      L = n + 1 - L;
      Bp = Tp;
      m = 1;
    } else {
      xor_shifted(Cp.data(), cw, Bp.data(), cw, m);
      m++;
    }
  }
  if (L != kMtDeg) return P;
  // phi(x) = x^L C(1/x): phi_i = c_{L-i}
  P.low.assign(kW, 0);
  for (int i = 0; i < kMtDeg; i++)
    if (getbit(Cp.data(), kMtDeg - i)) P.low[i >> 6] |= 1ull << (i & 63);
  // tab[1 << e] = x^(19937 + e) mod phi, by multiplying by x
  std::vector<Poly> pw(8);
  pw[0] = P.low;
  for (int e = 1; e < 8; e++) {
    Poly q(kW + 1, 0);
    for (int i = 0; i < kW; i++) {
      q[i] |= pw[e - 1][i] << 1;
      q[i + 1] |= pw[e - 1][i] >> 63;
    }
    if (getbit(q.data(), kMtDeg)) {
      q[kMtDeg >> 6] &= ~(1ull << (kMtDeg & 63));
      for (int i = 0; i < kW; i++) q[i] ^= P.low[i];
    }
    q.resize(kW);
    pw[e] = q;
  }
  P.tab.assign(256, Poly(kW, 0));
  for (int v = 1; v < 256; v++)
    for (int e = 0; e < 8; e++)
      if ((v >> e) & 1)
        for (int i = 0; i < kW; i++) P.tab[v][i] ^= pw[e][i];
  P.ok = true;
  return P;
}

// r (2 kW words, degree < 2 * 19937) mod phi, top-down one byte at a time
inline Poly reduce(const Phi &P, Poly r) {
  r.resize(2 * kW + 1, 0);
  const long long top = 64LL * (long long)r.size() - kMtDeg;
  for (long long j = (top / 8) * 8; j >= 0; j -= 8) {
    const long long bit = kMtDeg + j;
    const unsigned v = (unsigned)(get64(r.data(), r.size(), bit) & 0xff);
    if (!v) continue;
    for (int e = 0; e < 8; e++)
      if ((v >> e) & 1) r[(bit + e) >> 6] &= ~(1ull << ((bit + e) & 63));
    xor_shifted(r.data(), r.size(), P.tab[v].data(), kW, j);
  }
  r.resize(kW);
  return r;
}

inline Poly mulmod(const Phi &P, const Poly &a, const Poly &b) {
  Poly r(2 * kW, 0);
  for (int i = 0; i < kW; i++) {
    if (!a[i]) continue;
    for (int j = 0; j < kW; j++) {
      uint64_t lo, hi;
      clmul(a[i], b[j], lo, hi);
      r[i + j] ^= lo;
      r[i + j + 1] ^= hi;
    }
  }
  return reduce(P, std::move(r));
}

// x^e mod phi
inline Poly xpow(const Phi &P, unsigned long long e) {
  Poly r(kW, 0);
  r[0] = 1;
  for (int bit = 63; bit >= 0; bit--) {
    r = mulmod(P, r, r);
    if ((e >> bit) & 1) {  // times x
      Poly q(kW + 1, 0);
      for (int i = 0; i < kW; i++) {
        q[i] |= r[i] << 1;
        q[i + 1] |= r[i] >> 63;
      }
      if (getbit(q.data(), kMtDeg)) {
        q[kMtDeg >> 6] &= ~(1ull << (kMtDeg & 63));
        for (int i = 0; i < kW; i++) q[i] ^= P.low[i];
      }
      q.resize(kW);
      r = q;
    }
  }
  return r;
}

// residue -> the 624 uint32 words the segment kernel reads
inline void to_words(const Poly &p, uint32_t *out) {
  for (int i = 0; i < kMtPolyWords; i++) out[i] = (uint32_t)(p[i / 2] >> (32 * (i & 1)));
}

// words y_{P+1 ..} from the window y_{P .. P+623}: out[m] = y_{P+1+m}, m < nout
inline void gen_after(const uint32_t *st, uint32_t *out, int nout) {
  std::vector<uint32_t> y(st, st + kMtN);
  y.reserve(nout + 1 + kMtN);
  while ((int)y.size() < nout + 1) {
    const size_t k = y.size() - kMtN;
    y.push_back(mt_next(y[k], y[k + 1], y[k + kMtM]));
  }
  std::memcpy(out, y.data() + 1, sizeof(uint32_t) * nout);
}

// the window y_{P+J .. P+J+623} from the window y_{P ..} (J >= 1)
inline void window_ahead(const Phi &P, const uint32_t *st, unsigned long long J, uint32_t *out) {
  if (J <= 2ull * kMtWin) {  // near: run the recurrence
    std::vector<uint32_t> y((size_t)J + kMtN);
    gen_after(st, y.data(), (int)(J - 1 + kMtN));
    std::memcpy(out, y.data() + (J - 1), sizeof(uint32_t) * kMtN);
    return;
  }
  const Poly c = xpow(P, J - 1);
  std::vector<uint32_t> w(kMtWin);
  gen_after(st, w.data(), kMtWin);
  uint32_t acc[kMtN] = {0};
  for (int i = 0; i < kMtDeg; i++)
    if (getbit(c.data(), i))
      for (int t = 0; t < kMtN; t++) acc[t] ^= w[i + t];
  std::memcpy(out, acc, sizeof acc);
}

// GSL state (mt[], mti) -> the window at its next output, y_{mti ..}
inline void gsl_to_window(const uint32_t *mt, int mti, uint32_t *win) {
  std::vector<uint32_t> y(mt, mt + kMtN);
  for (int k = 0; k < mti; k++) y.push_back(mt_next(y[k], y[k + 1], y[k + kMtM]));
  std::memcpy(win, y.data() + mti, sizeof(uint32_t) * kMtN);
}

}  // namespace mt_host
}  // namespace bchmc
