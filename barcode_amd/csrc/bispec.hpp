// bispec.hpp -- the bispectrum of a sample (bchmc_bispectrum): the FFT estimator of Scoccimarro (2015) and Sefusatti et
// al. (2016).  The transform x^ is cut into n_shell spherical shells of |k|; each shell goes back to real space
// (D_s = C2R[x^ 1_s], and once per set of shells I_s = C2R[1_s]); the sums over cells of D_s1 D_s2 D_s3 and of
// I_s1 I_s2 I_s3 are the sum of x^1 x^2 x^3 over closed triangles and their number.  Three kernels: the per-shell
// statistics of x^, the shell filter in front of each C2R, and the contraction of n_shell arrays of N cells into
// T = n_shell (n_shell + 1) (n_shell + 2) / 6 sums, plus the ordered reduction of per-workgroup partials they share.
// Part of the bchmc engine's kernel set; include through kernels.hpp (definition order matters).
#pragma once
#include "common.hpp"

#include <algorithm>

namespace bchmc {

constexpr int kBispecMaxShell = 32;
constexpr int kBispecStatBlock = kWave;  // k_bispec_stats: one wave, every lane its own LDS column per (sum, shell)
constexpr int kBispecStatGrid = 2048;
// its dynamic LDS at 32 shells is exactly the 48 KiB a kernel may take without hipFuncSetAttribute
static_assert(3 * kBispecMaxShell * kWave * sizeof(double) <= 48 * 1024, "k_bispec_stats is launched without the attribute");
constexpr int kBispecCells = 128;        // cells of one LDS tile of the contraction
constexpr int kBispecGrid = 512;         // workgroups of the contraction at most: two per compute unit
constexpr int kBispecMaxItems = 272;     // row pairs of 32 shells: sum over s2 of ceil((s2 + 1) / 2)
constexpr int kBispecMaxWaves = (kBispecMaxItems + kWave - 1) / kWave;
constexpr int kBispecMaxThreads = kBispecMaxWaves * kWave;

// ---- triplets (host and device) ------------------------------------------------------------------------------------------
// All (s1, s2, s3) with s1 <= s2 <= s3 in lexicographic order
__host__ __device__ inline int bispec_triplets(int n) { return n * (n + 1) * (n + 2) / 6; }
__host__ __device__ inline int bispec_index(int n, int s1, int s2, int s3) {
  int t = 0;
  for (int a = 0; a < s1; a++) t += (n - a) * (n - a + 1) / 2;
  for (int b = s1; b < s2; b++) t += n - b;
  return t + (s3 - s2);
}

// The shell of the mode (i, j, k), or -1: s = (ULONG)((|k| - k_min) / dk) for |k| >= k_min and s < n_shell; the mode
// k = 0 has none.  |k| as k_spectrum forms it: IEEE sqrt and divide, no FMA contraction.
__device__ __forceinline__ int bispec_shell(const Geo &g, int i, int j, int k, double k_min, double dk, int n_shell,
                                            double &ktot) {
#pragma clang fp contract(off)
  const double kx = kval(i, g.n, g.kfac), ky = kval(j, g.n, g.kfac), kz = kval(k, g.n, g.kfac);
  ktot = sqrt(kx * kx + ky * ky + kz * kz);
  if ((i | j | k) == 0 || !(ktot >= k_min)) return -1;
  const unsigned long long s = (unsigned long long)((ktot - k_min) / dk);
  return s < (unsigned long long)n_shell ? (int)s : -1;
}

// ------------------------------------------------------------------------------------------------------
// Shell statistics: x^ -> per shell (sum hw, sum hw |k|, sum hw |x^|^2), hw = the number of full-grid modes a stored
// one stands for.  A workgroup is one wave; lane l keeps its own column acc[(q n_shell + s) 64 + l] in LDS and adds its
// modes in the order it meets them, so nothing is atomic; at the end each of the 3 n_shell rows is summed over the
// lanes by wave_sum's tree and written to part[workgroup][q n_shell + s].  k_bispec_reduce adds the workgroups.  The
// counts are sums of 1 and 2 in double: exact below 2^53.
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kBispecStatBlock)
k_bispec_stats(Geo g, const C2<T> *__restrict__ xk, double k_min, double dk, int n_shell, double *__restrict__ part) {
#pragma clang fp contract(off)
  extern __shared__ double s_acc[];  // 3 n_shell rows of 64
  const int lane = threadIdx.x, rows = 3 * n_shell;
  for (int r = 0; r < rows; r++) s_acc[r * kWave + lane] = 0.;
  for (long long idx = blockIdx.x * (long long)kBispecStatBlock + lane; idx < g.Nhp;
       idx += (long long)gridDim.x * kBispecStatBlock) {
    const int k = (int)(idx % g.nhp);
    if (k >= g.nh) continue;
    const long long ij = idx / g.nhp;
    const int j = (int)(ij % g.n), i = (int)(ij / g.n);
    double ktot;
    const int s = bispec_shell(g, i, j, k, k_min, dk, n_shell, ktot);
    if (s < 0) continue;
    const double hw = (k == 0 || ((g.n & 1) == 0 && k == g.n / 2)) ? 1. : 2.;
    const double2 x = ld2<T>(xk, idx);
    s_acc[s * kWave + lane] += hw;
    s_acc[(n_shell + s) * kWave + lane] += hw * ktot;
    s_acc[(2 * n_shell + s) * kWave + lane] += hw * (x.x * x.x + x.y * x.y);
  }
  for (int r = 0; r < rows; r++) {
    const double v = wave_sum(s_acc[r * kWave + lane]);
    if (lane == 0) part[(size_t)blockIdx.x * rows + r] = v;
  }
}

// ------------------------------------------------------------------------------------------------------
// Shell filter: out = x^ inside shell s, 0 outside (ONES: 1 inside, for I_s); the unnormalised C2R follows.  The shell
// of a mode depends on |k| only, so `out` is the transform of a real field, Nyquist planes of an even n included.  x^
// is read only inside the shell -- a small fraction of the array; the padding columns k >= nh get zeros.
// ------------------------------------------------------------------------------------------------------
template <typename T, bool ONES>
__global__ void __launch_bounds__(256)
k_bispec_filter(Geo g, const C2<T> *__restrict__ xk, C2<T> *__restrict__ out, double k_min, double dk, int n_shell, int s) {
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < g.Nhp;
       idx += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(idx % g.nhp);
    const long long ij = idx / g.nhp;
    const int j = (int)(ij % g.n), i = (int)(ij / g.n);
    double ktot;
    const bool in = k < g.nh && bispec_shell(g, i, j, k, k_min, dk, n_shell, ktot) == s;
    double2 v = make_double2(0., 0.);
    if (in) v = ONES ? make_double2(1., 0.) : ld2<T>(xk, idx);
    st2<T>(out, idx, v.x, v.y);
  }
}

// ------------------------------------------------------------------------------------------------------
// The triple contraction: n_shell arrays of M cells -> T sums over cells of A_s1 A_s2 A_s3.
//
// Work is cut into ITEMS: a pair of rows (s1, s2) and (s1 + 1, s2) of the triplet table (the second is missing when
// s1 + 1 > s2) with the s3 they sweep, s3 = s2 .. s2 + len - 1.  A lane owns one item for the whole kernel: its
// 2 len accumulators stay in registers (indexed at compile time: the sweep is unrolled over NS >= n_shell), and no
// cross-lane add happens anywhere -- every triplet belongs to exactly one lane of a workgroup.  Per cell a lane forms
// the two products A_s1 A_s2 once and sweeps s3 with one 8-byte LDS read per two FMAs: ds_read_b64 moves 256 B per
// clock and CU against 128 fp64 FMA lanes per clock and CU, so one read per FMA would be LDS-bound by two and one per
// two FMAs balances them.  Items are ordered by s2, so the lanes of a wave sweep rows of similar length; a wave runs
// to the longest sweep of its lanes (wlen, uniform) in groups of four s3, a lane past its own len adds into
// accumulators that are never stored.
//
// A workgroup takes tiles of kBispecCells cells, grid-stride: the n_shell values of a cell, widened to double, lie in
// one LDS row (s contiguous) of an odd number of doubles, so the fill (lanes along cells) is conflict-free, and the
// sweep's reads -- every lane of a wave is at the same cell -- hit one row: distinct banks or a broadcast.  The row has
// NS doubles of zero padding, which a lane past its len reads.  128 cells x 65 doubles = 65 KiB: two workgroups per CU.
//
// Workgroup b writes its T partial sums to part[b T ..]; k_bispec_reduce adds the workgroups in a fixed order.  A
// lane's sum runs over its cells in order, so all bits are a function of (M, n_shell, plan, gridDim) alone.
// ------------------------------------------------------------------------------------------------------
struct BispecArrays {
  const void *a[kBispecMaxShell];  // M elements of the storage type each
};
struct BispecPlan {
  int items;
  unsigned char s1[kBispecMaxItems], s2[kBispecMaxItems], len[kBispecMaxItems];
  unsigned char wlen[kBispecMaxWaves];  // the longest len of each wave's items
};

template <typename T, int NS>
__global__ void __launch_bounds__(kBispecMaxThreads)
k_bispec_triple(long long M, int n_shell, BispecArrays arr, BispecPlan plan, double *__restrict__ part) {
  extern __shared__ double s_tile[];  // kBispecCells rows of `stride`
  const int stride = (n_shell + NS) | 1;
  const int tid = threadIdx.x;
  const bool active = tid < plan.items;
  const int s1a = active ? plan.s1[tid] : 0, s2 = active ? plan.s2[tid] : 0;
  const bool has_b = active && s1a + 1 <= s2;
  const int s1b = has_b ? s1a + 1 : s1a;
  const int wlen = __builtin_amdgcn_readfirstlane((int)plan.wlen[tid / kWave]);
  double acc_a[NS], acc_b[NS];
#pragma unroll
  for (int j = 0; j < NS; j++) acc_a[j] = acc_b[j] = 0.;
  for (int e = tid; e < kBispecCells * stride; e += blockDim.x) s_tile[e] = 0.;  // the padding stays zero
  const long long ntile = (M + kBispecCells - 1) / kBispecCells;
  for (long long t = blockIdx.x; t < ntile; t += gridDim.x) {
    const long long cell0 = t * kBispecCells;
    __syncthreads();
    for (int e = tid; e < n_shell * kBispecCells; e += blockDim.x) {
      const int s = e / kBispecCells, c = e % kBispecCells;
      const long long cell = cell0 + c;
      s_tile[c * stride + s] = cell < M ? (double)static_cast<const T *>(arr.a[s])[cell] : 0.;
    }
    __syncthreads();
    if (wlen == 0) continue;
    for (int c = 0; c < kBispecCells; c++) {
      const double *r = s_tile + c * stride;
      const double d2 = r[s2];
      const double pa = r[s1a] * d2, pb = r[s1b] * d2;
      const double *sweep = r + s2;
#pragma unroll
      for (int j0 = 0; j0 < NS; j0 += 4) {  // four s3 per uniform branch: the reads of a group issue together
        if (j0 < wlen) {
#pragma unroll
          for (int j = j0; j < j0 + 4; j++) {
            const double d3 = sweep[j];
            acc_a[j] = fma(pa, d3, acc_a[j]);
            acc_b[j] = fma(pb, d3, acc_b[j]);
          }
        }
      }
    }
  }
  if (!active) return;
  double *p = part + (size_t)blockIdx.x * bispec_triplets(n_shell);
  const int ta = bispec_index(n_shell, s1a, s2, s2), tb = bispec_index(n_shell, s1b, s2, s2), row = n_shell - s2;
#pragma unroll
  for (int j = 0; j < NS; j++) {
    if (j < row) {
      p[ta + j] = acc_a[j];
      if (has_b) p[tb + j] = acc_b[j];
    }
  }
}

// The reduction of `nrow` partial rows of W words in one fixed order: a workgroup takes 64 columns, its four waves the
// rows r = w, w + 4, ... of them in order (loads coalesced along the columns), then (w0 + w1) + (w2 + w3).
__global__ void __launch_bounds__(256)
k_bispec_reduce(int nrow, int W, const double *__restrict__ part, double *__restrict__ res) {
  __shared__ double s_sum[4][kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const int col = blockIdx.x * kWave + lane;
  double a = 0.;
  if (col < W)
    for (int r = w; r < nrow; r += 4) a += part[(size_t)r * W + col];
  s_sum[w][lane] = a;
  __syncthreads();
  if (w == 0 && col < W) res[col] = (s_sum[0][lane] + s_sum[1][lane]) + (s_sum[2][lane] + s_sum[3][lane]);
}

// ---- host side: the plan and the launches, shared by the engine and the probe -----------------------------------------------
// s3_end[s1][s2]: one past the last s3 the row (s1, s2) computes (n_shell: the whole row; B4 of include/bchmc.h cuts it).
// An item sweeps as far as the longer of its two rows; what it computes beyond a row's end the host discards.
inline BispecPlan bispec_plan(int n_shell, const unsigned char (*s3_end)[kBispecMaxShell]) {
  BispecPlan p{};
  for (int s2 = 0; s2 < n_shell; s2++)
    for (int s1 = 0; s1 <= s2; s1 += 2) {
      const int it = p.items++;
      int end = s3_end ? s3_end[s1][s2] : n_shell;
      if (s1 + 1 <= s2) end = std::max(end, s3_end ? (int)s3_end[s1 + 1][s2] : n_shell);
      p.s1[it] = (unsigned char)s1, p.s2[it] = (unsigned char)s2, p.len[it] = (unsigned char)std::max(end - s2, 0);
      p.wlen[it / kWave] = std::max(p.wlen[it / kWave], p.len[it]);
    }
  return p;
}

// workgroups of the contraction over M cells: a function of M alone, and with it the order of every sum
inline int bispec_grid(long long M) { return (int)std::min<long long>((M + kBispecCells - 1) / kBispecCells, kBispecGrid); }
inline int bispec_threads(const BispecPlan &p) { return (p.items + kWave - 1) / kWave * kWave; }

// k_bispec_triple and k_bispec_reduce: arr -> res[T]; part holds bispec_grid(M) * T doubles
template <typename T, int NS>
hipError_t launch_bispec_triple_ns(hipStream_t stream, long long M, int n_shell, const BispecArrays &arr, const BispecPlan &plan,
                                   double *part, double *res) {
  const size_t lds = (size_t)kBispecCells * ((n_shell + NS) | 1) * sizeof(double);
  // once per instantiation and device: the largest tile of this NS (65 KiB at 32 shells, above the 48 KiB a kernel may
  // take without asking)
  constexpr size_t lds_max = (size_t)kBispecCells * ((2 * NS) | 1) * sizeof(double);
  static_assert(lds_max <= 160 * 1024, "the tile must fit the LDS of a compute unit");
  if (lds_max > 48 * 1024) {
    static thread_local int asked_on = -1;
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev != asked_on) {
      e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bispec_triple<T, NS>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
      if (e == hipSuccess) asked_on = dev;
    }
    if (e != hipSuccess) return e;
  }
  const int grid = bispec_grid(M), W = bispec_triplets(n_shell);
  k_bispec_triple<T, NS><<<grid, bispec_threads(plan), lds, stream>>>(M, n_shell, arr, plan, part);
  k_bispec_reduce<<<(W + kWave - 1) / kWave, 256, 0, stream>>>(grid, W, part, res);
  return hipGetLastError();
}
template <typename T>
hipError_t launch_bispec_triple(hipStream_t stream, long long M, int n_shell, const BispecArrays &arr, const BispecPlan &plan,
                                double *part, double *res) {
  if (n_shell <= 8) return launch_bispec_triple_ns<T, 8>(stream, M, n_shell, arr, plan, part, res);
  if (n_shell <= 16) return launch_bispec_triple_ns<T, 16>(stream, M, n_shell, arr, plan, part, res);
  return launch_bispec_triple_ns<T, 32>(stream, M, n_shell, arr, plan, part, res);
}

}  // namespace bchmc
