// fft_probe.hip -- libbchmc_fft_probe.so: the engine's own FFT passes run alone on host arrays, for the tests that
// compare them with a high-precision DFT (tests/test_gpu_fft_passes.py).  Not part of the product: nothing in the
// engine or bench.py loads it.
//
// Every pass below is the engine's kernel code itself (kernels.hpp), and its launch is the engine's launch: the typed
// launchers of pass_launch.hpp that bchmc.hip calls (forward_rest, particle_stage, the planes-mode R2C, probe_z) choose
// template arguments, grid, block and dynamic LDS here too, on the null stream.  Row stride and twiddles come from
// fft_host.hpp, which the engine uses too.  The only kernel of its own is k_probe_xfft, a bare wrapper around
// xfft_inplace, on the block size of the engine's tables.
//
// Every device array is followed by kCanary bytes of a known pattern; an entry point copies its host arrays in,
// launches, synchronises, copies back and checks the canaries.  Return value: 0 = ok, -1 = arguments outside the
// engine's instantiations, -2 = HIP error, k > 0 = the canary after device array k changed (1 = the twiddle table,
// then the arrays in argument order).
#include "kernels.hpp"
#include "fft_host.hpp"
#include "pass_launch.hpp"

#include <cmath>
#include <cstring>
#include <vector>

using namespace bchmc;

namespace {

constexpr size_t kCanary = 64 * 1024;
constexpr unsigned char kCanaryByte = 0x5b;

// xfft_inplace alone: workgroup b owns the n x kb interleaved columns data[(b n + i) kb + c]; bit-reversed fill of
// the LDS tile (as k_ypass / k_step_boundary_x do it), the transform, natural-order store.
template <typename T, int NT>
__global__ void __launch_bounds__(NT)
k_probe_xfft(int n, int log2n, int kb, int inverse, const C2<T> *__restrict__ twiddle, C2<T> *data) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw_p[];
  C2<T> *s = reinterpret_cast<C2<T> *>(s_raw_p);  // n * kb
  C2<T> *tw = s + (size_t)n * kb;                 // n / 2
  for (int t = threadIdx.x; t < n / 2; t += NT) tw[t] = twiddle[t];
  C2<T> *col = data + (long long)blockIdx.x * n * kb;
  const int shift = 32 - log2n;
  for (int e = threadIdx.x; e < n * kb; e += NT) {
    const int i = e / kb, c = e % kb;
    s[(int)(__brev((unsigned)i) >> shift) * kb + c] = col[e];
  }
  __syncthreads();
  xfft_inplace<T>(s, tw, n, log2n, kb, inverse != 0);
  for (int e = threadIdx.x; e < n * kb; e += NT) col[e] = s[e];
}

int ilog2(int n) {
  int l = 0;
  while ((1 << l) < n) l++;
  return (1 << l) == n ? l : -1;
}

struct Probe {
  std::vector<void *> bufs;
  std::vector<size_t> sizes;
  int err = 0;  // first failure

  ~Probe() {
    for (void *p : bufs) (void)hipFree(p);
  }
  bool ok(hipError_t e) {
    if (e != hipSuccess && !err) err = -2;
    return e == hipSuccess;
  }
  // device array of `bytes` followed by the canary; `host` (may be null) copied in
  void *alloc(size_t bytes, const void *host) {
    void *d = nullptr;
    if (!ok(hipMalloc(&d, bytes + kCanary))) return nullptr;
    bufs.push_back(d);
    sizes.push_back(bytes);
    ok(hipMemset(static_cast<char *>(d) + bytes, kCanaryByte, kCanary));
    if (host) ok(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    return d;
  }
  // after the launch: synchronise, copy each (device array index, host array) of `outs` back, check every canary
  int finish(const std::vector<std::pair<int, void *>> &outs) {
    if (err) return err;
    if (!ok(hipGetLastError()) || !ok(hipDeviceSynchronize())) return err;
    for (const auto &o : outs)
      if (!ok(hipMemcpy(o.second, bufs[o.first], sizes[o.first], hipMemcpyDeviceToHost))) return err;
    std::vector<unsigned char> c(kCanary);
    for (size_t i = 0; i < bufs.size(); i++) {
      if (!ok(hipMemcpy(c.data(), static_cast<char *>(bufs[i]) + sizes[i], kCanary, hipMemcpyDeviceToHost))) return err;
      for (unsigned char b : c)
        if (b != kCanaryByte) return (int)i + 1;
    }
    return 0;
  }
  template <typename T> const C2<T> *twiddles(int n) {
    const std::vector<T> tw = fft_twiddles<T>(n);
    return static_cast<const C2<T> *>(alloc(tw.size() * sizeof(T), tw.data()));
  }
  // what the engine's launchers take: the null stream, the geometry, the twiddle table (device array 0)
  template <typename T> PassCtx<T> ctx(const Geo &g) { return {nullptr, g, ilog2(g.n), twiddles<T>(g.n)}; }
};

Geo probe_geo(int n, int esz) {
  Geo g;
  g.n = n;
  g.nh = n / 2 + 1;
  g.nhp = fft_row_stride(n, esz);
  g.N = (long long)n * n * n;
  g.Nh = (long long)n * n * g.nh;
  g.Nhp = (long long)n * n * g.nhp;
  g.L = (double)n;
  g.d = 1.;
  g.kfac = 2. * M_PI / g.L;
  return g;
}

template <typename T, int NT>
void launch_xfft(Probe &pr, int groups, int n, int kb, int inverse, const C2<T> *tw, C2<T> *d) {
  const size_t lds = ((size_t)n * kb + n / 2) * sizeof(C2<T>);
  pr.ok(launch_dyn_lds(nullptr, k_probe_xfft<T, NT>, groups, NT, lds, n, ilog2(n), kb, inverse, tw, d));
}

template <typename T> int xfft(int n, int kb, int inverse, int groups, void *data) {
  if (ilog2(n) < 5 || n > 512 || groups < 1 || (kb != pass_kb(sizeof(T)) && kb != 6)) return -1;
  // the engine's block size for this n: k_step_boundary_x / k_alpt_mix_x / k_ypass (kb = KB), one thread per element
  // of a z row in k_zbin_direct / k_zr2c (kb = 6)
  const int nt = kb == 6 ? n : x_shape(sizeof(T), n).nt;
  Probe pr;
  const size_t bytes = (size_t)groups * n * kb * sizeof(C2<T>);
  const C2<T> *tw = pr.twiddles<T>(n);
  C2<T> *d = static_cast<C2<T> *>(pr.alloc(bytes, data));
  if (pr.err) return pr.err;
  switch (nt) {
    case 32: launch_xfft<T, 32>(pr, groups, n, kb, inverse, tw, d); break;
    case 64: launch_xfft<T, 64>(pr, groups, n, kb, inverse, tw, d); break;
    case 128: launch_xfft<T, 128>(pr, groups, n, kb, inverse, tw, d); break;
    case 256: launch_xfft<T, 256>(pr, groups, n, kb, inverse, tw, d); break;
    case 512: launch_xfft<T, 512>(pr, groups, n, kb, inverse, tw, d); break;
    case 1024: launch_xfft<T, 1024>(pr, groups, n, kb, inverse, tw, d); break;
    default: return -1;
  }
  return pr.finish({{1, data}});
}

// k_ypass as forward_rest (inverse) and the planes-mode R2C at 512^3 (forward) launch it
template <typename T> int ypass(int n, int inverse, void *ck) {
  if (!y_shape(sizeof(T), n).nt || (!inverse && n != 512)) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T));
  if (g.nhp % pass_kb(sizeof(T))) return -1;
  Probe pr;
  const PassCtx<T> x = pr.ctx<T>(g);
  C2<T> *d = static_cast<C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), ck));
  if (pr.err) return pr.err;
  pr.ok(inverse ? launch_ypass<T>(x, d) : launch_ypass<T, false>(x, d));
  return pr.finish({{1, ck}});
}

// k_zr2c as the planes-mode R2C at 512^3 launches it, and as bchmc_probe_displacement_z does at 128^3 and 256^3;
// ck goes in as well, so that the row padding the kernel leaves alone comes back as it went in
template <typename T> int zr2c(int n, const void *V, void *ck) {
  if (!z_shape(sizeof(T), n).nt) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T));
  Probe pr;
  const PassCtx<T> x = pr.ctx<T>(g);
  const T *dv = static_cast<const T *>(pr.alloc((size_t)3 * g.N * sizeof(T), V));
  C2<T> *dc = static_cast<C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), ck));
  if (pr.err) return pr.err;
  pr.ok(launch_zr2c<T>(x, dv, dc));
  return pr.finish({{2, ck}});
}

// k_zbin_direct<T, NZ, true> as particle_stage launches it after an overflowed binning (*ovf set): the z C2R of the three
// displacement components into psi (3 n^3 reals).  Its positions / binning arguments are not read on this path.
template <typename T> int zc2r(int n, const void *ck, void *psi) {
  if (!z_shape(sizeof(T), n).nt) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T));
  Probe pr;
  const PassCtx<T> x = pr.ctx<T>(g);
  const C2<T> *dc = static_cast<const C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), ck));
  const int ovf_h[3] = {1, 0, 0};
  int *ovf = static_cast<int *>(pr.alloc(sizeof(ovf_h), ovf_h));
  T *dp = static_cast<T *>(pr.alloc((size_t)3 * g.N * sizeof(T), nullptr));
  if (pr.err) return pr.err;
  pr.ok((launch_zbin<T, true>(x, PosPar{}, SphPar{}, TilePar{}, dc, nullptr, ovf, nullptr, nullptr, nullptr, nullptr, nullptr,
                              dp)));
  return pr.finish({{3, psi}});
}

}  // namespace

// prec: 0 = double, 1 = float (the engine's storage type T); arrays are of that type, complex ones interleaved
extern "C" {

// half-complex row stride (complex elements) the engine uses for this n and precision
int fftp_row_stride(int n, int prec) { return fft_row_stride(n, prec ? 4 : 8); }

// xfft_inplace on `groups` workgroups of n x kb interleaved columns, in place
int fftp_xfft(int prec, int n, int kb, int inverse, int groups, void *data) {
  return prec ? xfft<float>(n, kb, inverse, groups, data) : xfft<double>(n, kb, inverse, groups, data);
}

// k_ypass over three planes-space components (3 n^2 nhp complex), in place
int fftp_ypass(int prec, int n, int inverse, void *ck) {
  return prec ? ypass<float>(n, inverse, ck) : ypass<double>(n, inverse, ck);
}

// k_zr2c: V (3 n^3 real) -> ck (3 n^2 nhp complex; the row padding comes back as it went in)
int fftp_zr2c(int prec, int n, const void *V, void *ck) {
  return prec ? zr2c<float>(n, V, ck) : zr2c<double>(n, V, ck);
}

// k_zbin_direct<PSI_ONLY>: ck (3 n^2 nhp complex) -> psi (3 n^3 real)
int fftp_zc2r(int prec, int n, const void *ck, void *psi) {
  return prec ? zc2r<float>(n, ck, psi) : zc2r<double>(n, ck, psi);
}

}  // extern "C"
