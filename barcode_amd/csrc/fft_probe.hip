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
// The k-space step kernels (tests/test_gpu_kstep.py) run the same way: the planes-mode step boundary and ALPT mix through
// launch_step_boundary_x / launch_step_boundary_x2 / launch_alpt_mix_x, their 3-D twins (grid-stride kernels, any n) on
// nblk_stride(Nhp) x 256 and k_parseval on kRedBlocks x 256 as bchmc.hip launches them.  Their geometry takes a box
// length, so that kfac is not 2 pi / n.
//
// The real-space ALPT and calc_h 0 / 3 kernels (tests/test_gpu_rs.py) run the same way: k_alpt_grad and k_alpt_sources on
// stencil_grid(n) x 256 (k_alpt_sources with either pointer layout of alpt_middle: a_out == d1 on the planes path,
// b_out == d1 on the 3-D path), k_alpt_kernel_table on nblk_stride(Nhp), k_gradfft_mult and k_conv_kernel on
// nblk_stride(Nh), k_mul3 and k_findif_mul on nblk_stride(N), k_interp_tsc on nblk_full(N).  k_conv_kernel takes its table
// F from the caller (build_conv_table is host code and not under test); k_interp_tsc takes the PosPar scalars (PosPar has
// no lower corner: the domain of this kernel is [0, L] and periodic, as make_pos sets it).
//
// The Philox momentum draw's kernels (tests/test_gpu_draw.py) run the same way, as chain_draw launches them: k_white_noise
// on nblk_stride((n + 1) / 2) x 256 over n values of any parity (seed words, attempt and stream as the kernel takes them,
// var may be null), k_color_momenta on nblk_stride(nh) x 256 over nh complex elements (wM may be null; pk goes in too).
//
// The generic trajectory's real-space mass and GRF kernels (tests/test_gpu_massrs.py) run the same way over `count`
// elements: k_div_mass_r (in place too, as the engine calls it), k_grf_grad, k_scale_c and k_add_r on nblk_stride(count) x
// 256, k_kin_rs and k_grf_loglike on kRedBlocks x 256 with every partial handed back.
//
// Every device array is followed by kCanary bytes of a known pattern; an entry point copies its host arrays in,
// launches, synchronises, copies back and checks the canaries.  Return value: 0 = ok, -1 = arguments outside the
// engine's instantiations, -2 = HIP error, k > 0 = the canary after device array k changed (1 = the twiddle table,
// then the arrays in argument order).
#include "kernels.hpp"
#include "fft_host.hpp"
#include "pass_launch.hpp"
#include "launch_grid.hpp"
#include "xtile_kernels.hpp"

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

Geo probe_geo(int n, int esz, double L = 0.) {
  Geo g;
  g.n = n;
  g.nh = n / 2 + 1;
  g.nhp = fft_row_stride(n, esz);
  g.N = (long long)n * n * n;
  g.Nh = (long long)n * n * g.nh;
  g.Nhp = (long long)n * n * g.nhp;
  g.L = L > 0. ? L : (double)n;
  g.d = g.L / n;
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

// k_ypass as forward_rest (inverse) and the planes-mode R2C at 512^3 (forward) launch it; forward at 128 and 256: the
// three-array reference of k_ypass_fwd_pair
template <typename T> int ypass(int n, int inverse, void *ck) {
  if (!y_shape(sizeof(T), n).nt) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T));
  if (g.nhp % pass_kb(sizeof(T))) return -1;
  Probe pr;
  const PassCtx<T> x = pr.ctx<T>(g);
  C2<T> *d = static_cast<C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), ck));
  if (pr.err) return pr.err;
  pr.ok(inverse ? launch_ypass<T>(x, d) : launch_ypass<T, false>(x, d));
  return pr.finish({{1, ck}});
}

// k_ypass_pair as forward_rest launches it after a boundary kernel that stored Psi^_x | B: components 0 and 1 are read,
// all three written
template <typename T> int ypass_pair(int n, double box_len, void *ck) {
  if (!ypair_shape(sizeof(T), n).nt) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), box_len);
  if (g.nhp % pass_kb(sizeof(T))) return -1;
  Probe pr;
  const PassCtx<T> x = pr.ctx<T>(g);
  C2<T> *d = static_cast<C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), ck));
  if (pr.err) return pr.err;
  pr.ok(launch_ypass_pair<T>(x, d));
  return pr.finish({{1, ck}});
}

// k_ypass_fwd_pair as the planes-mode R2C launches it after k_zr2c: the three components are read, 0 (V^_x) and 1 (W) written
template <typename T> int ypass_fwd_pair(int n, double box_len, void *ck) {
  if (!yfwd_pair_shape(sizeof(T), n).nt) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), box_len);
  if (g.nhp % pass_kb(sizeof(T))) return -1;
  Probe pr;
  const PassCtx<T> x = pr.ctx<T>(g);
  C2<T> *d = static_cast<C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), ck));
  if (pr.err) return pr.err;
  pr.ok(launch_ypass_fwd_pair<T>(x, d));
  return pr.finish({{1, ck}});
}

// k_zr2c as the planes-mode R2C launches it, and as bchmc_probe_displacement_z does; REC: V is n^3 records of 4 (the
// gather's V records), else 3 n^3.  ck goes in as well, so that the row padding the kernel leaves alone comes back as it
// went in
template <typename T, bool REC = false> int zr2c(int n, const void *V, void *ck) {
  if (!z_shape(sizeof(T), n).nt) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T));
  Probe pr;
  const PassCtx<T> x = pr.ctx<T>(g);
  const T *dv = static_cast<const T *>(pr.alloc((size_t)(REC ? 4 : 3) * g.N * sizeof(T), V));
  C2<T> *dc = static_cast<C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), ck));
  if (pr.err) return pr.err;
  pr.ok((launch_zr2c<T, REC>(x, dv, dc)));
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
                              dp, nullptr)));
  return pr.finish({{3, psi}});
}

// ---- the k-space step kernels ------------------------------------------------------------------------------------------

// the trajectory-control words of a probe call: stop, steps_done and guard_prev live on the device and come back
struct CtlArgs {
  int *stop;
  unsigned long long *steps_done;
  const double *guard_prev;  // may be null: no guard test, as at step 0
  double guard_limit;
  unsigned long long step_index;
};
struct CtlDev {
  StepCtl ctl{};
  int i_stop = -1, i_done = -1;
};
CtlDev ctl_alloc(Probe &pr, const CtlArgs &c) {
  CtlDev d;
  d.ctl.stop = static_cast<int *>(pr.alloc(sizeof(int), c.stop));
  d.i_stop = (int)pr.bufs.size() - 1;
  d.ctl.steps_done = static_cast<unsigned long long *>(pr.alloc(sizeof(unsigned long long), c.steps_done));
  d.i_done = (int)pr.bufs.size() - 1;
  d.ctl.guard_prev = c.guard_prev ? static_cast<const double *>(pr.alloc(sizeof(double), c.guard_prev)) : nullptr;
  d.ctl.guard_limit = c.guard_limit;
  d.ctl.step_index = c.step_index;
  return d;
}

// a device copy of a host array that may be null (then null on the device too); idx receives its device array index
template <typename U> U *opt(Probe &pr, size_t bytes, const void *host, int *idx = nullptr) {
  if (!host) return nullptr;
  U *d = static_cast<U *>(pr.alloc(bytes, host));
  if (idx) *idx = (int)pr.bufs.size() - 1;
  return d;
}

using Outs = std::vector<std::pair<int, void *>>;
void out(Outs &o, int idx, void *host) {
  if (host && idx >= 0) o.push_back({idx, host});
}

// k_step_boundary_x<T, NT, PER, MODE, ALPT> / k_step_boundary_x2<T, NT, PER> as the engine launches them.
// scal = {a, b, half_eps, eps, c_za}
template <typename T>
int step_boundary_x(int n, double L, int mode, int alpt, int two_tile, void *Ck, const void *q_in, const void *p_in,
                    const void *g_in, void *q_out, void *p_out, void *g_out, const double *wS, const double *wM,
                    const double *scal, double *guard_slot, const CtlArgs &ca, int vpair = 0, const void *wpair = nullptr) {
  if (mode < BX_INTERIOR || mode > BX_LAST || (alpt && mode == BX_LAST)) return -1;
  const bool xt = wpair != nullptr;  // the XT instantiations: state and weights in x-column tiles (xtile.hpp)
  if (xt && (alpt || !wM || !p_in || (mode != BX_LAST && !q_out) || !p_out || (mode == BX_FIRST && !g_in))) return -1;
  if (vpair && (alpt || mode == BX_FIRST)) return -1;
  if (two_tile ? (!x2_shape(sizeof(T), n).nt || mode != BX_INTERIOR || alpt) : !x_shape(sizeof(T), n).nt) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  if (g.nhp % pass_kb(sizeof(T)) || !Ck || !q_in || !scal) return -1;
  // what each mode dereferences must be there (the kernels do not test for it)
  const bool first_kick = mode == BX_FIRST && g_in, last_kick = mode == BX_LAST && p_out;
  if (mode == BX_INTERIOR && !(p_in && q_out && p_out && guard_slot)) return -1;
  if (first_kick && !(p_in && q_out && p_out)) return -1;
  if (mode == BX_LAST && (!g_out || (last_kick && !(p_in && guard_slot)))) return -1;
  if (mode != BX_FIRST && scal[0] != 0. && !wS) return -1;
  Probe pr;
  const PassCtx<T> x = pr.ctx<T>(g);
  const size_t cb = (size_t)g.Nhp * sizeof(C2<T>), db = (size_t)g.Nhp * sizeof(double);
  int i_ck, i_qo = -1, i_po = -1, i_go = -1, i_gs = -1;
  C2<T> *d_ck = opt<C2<T>>(pr, 3 * cb, Ck, &i_ck);
  BoundaryX<T> a;
  a.qi = opt<const C2<T>>(pr, cb, q_in);
  a.pi = opt<const C2<T>>(pr, cb, p_in);
  a.g_in = opt<const C2<T>>(pr, cb, g_in);
  a.qo = opt<C2<T>>(pr, cb, q_out, &i_qo);
  a.po = opt<C2<T>>(pr, cb, p_out, &i_po);
  a.g_out = opt<C2<T>>(pr, cb, g_out, &i_go);
  const double *d_ws = opt<const double>(pr, db, wS);
  a.wM = opt<const double>(pr, db, wM);
  a.a = scal[0], a.b = scal[1], a.half_eps = scal[2], a.eps = scal[3], a.c_za = scal[4];
  a.guard_slot = opt<double>(pr, sizeof(double), guard_slot, &i_gs);
  const CtlDev cd = ctl_alloc(pr, ca);
  a.ctl = cd.ctl;
  a.vpair = vpair != 0;
  a.wpair = opt<const double2>(pr, (size_t)g.Nhp * sizeof(double2), wpair);
  if (pr.err) return pr.err;
  hipError_t e = hipErrorInvalidConfiguration;
  if (xt && two_tile) e = launch_step_boundary_x2<T, true>(x, d_ck, d_ws, a);
  else if (xt && mode == BX_INTERIOR) e = launch_step_boundary_x<T, BX_INTERIOR, false, true>(x, d_ck, d_ws, a);
  else if (xt && mode == BX_FIRST) e = launch_step_boundary_x<T, BX_FIRST, false, true>(x, d_ck, d_ws, a);
  else if (xt) e = launch_step_boundary_x<T, BX_LAST, false, true>(x, d_ck, d_ws, a);
  else if (two_tile) e = launch_step_boundary_x2<T>(x, d_ck, d_ws, a);
  else if (mode == BX_INTERIOR) e = alpt ? launch_step_boundary_x<T, BX_INTERIOR, true>(x, d_ck, d_ws, a)
                                         : launch_step_boundary_x<T, BX_INTERIOR, false>(x, d_ck, d_ws, a);
  else if (mode == BX_FIRST) e = alpt ? launch_step_boundary_x<T, BX_FIRST, true>(x, d_ck, d_ws, a)
                                      : launch_step_boundary_x<T, BX_FIRST, false>(x, d_ck, d_ws, a);
  else e = launch_step_boundary_x<T, BX_LAST, false>(x, d_ck, d_ws, a);
  pr.ok(e);
  Outs o;
  out(o, i_ck, Ck), out(o, i_qo, q_out), out(o, i_po, p_out), out(o, i_go, g_out), out(o, i_gs, guard_slot);
  out(o, cd.i_stop, ca.stop), out(o, cd.i_done, ca.steps_done);
  return pr.finish(o);
}

template <typename T> int alpt_mix_x(int n, double L, void *Ck, double smol, double inv_wtot, double inv_n) {
  if (!x_shape(sizeof(T), n).nt) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  if (g.nhp % pass_kb(sizeof(T))) return -1;
  Probe pr;
  const PassCtx<T> x = pr.ctx<T>(g);
  C2<T> *d = static_cast<C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), Ck));
  if (pr.err) return pr.err;
  pr.ok(launch_alpt_mix_x<T>(x, d, smol, inv_wtot, inv_n));
  return pr.finish({{1, Ck}});
}

// The 3-D twins: element-wise over the padded half-complex array, any n >= 2.
bool ok3d(int n) { return n >= 2 && n <= 512; }

// scal = {half_eps, eps, c_za}
template <typename T>
int kick_drift_za(int n, double L, int drift, void *qk, void *pk, const void *gk, const double *wM, const void *extra,
                  void *Ck, const double *scal, const CtlArgs &ca) {
  if (!ok3d(n) || !qk || !Ck || !scal || (drift && !(pk && gk))) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  Probe pr;
  const size_t cb = (size_t)g.Nhp * sizeof(C2<T>);
  int i_q, i_p = -1, i_ck;
  C2<T> *dq = opt<C2<T>>(pr, cb, qk, &i_q), *dp = opt<C2<T>>(pr, cb, pk, &i_p);
  const C2<T> *dg = opt<const C2<T>>(pr, cb, gk);
  const double *dw = opt<const double>(pr, (size_t)g.Nhp * sizeof(double), wM);
  const C2<T> *dx = opt<const C2<T>>(pr, cb, extra);
  C2<T> *dc = opt<C2<T>>(pr, 3 * cb, Ck, &i_ck);
  const CtlDev cd = ctl_alloc(pr, ca);
  if (pr.err) return pr.err;
  if (drift)
    k_kick_drift_za<T, true><<<nblk_stride(g.Nhp), 256>>>(g, dq, dp, dg, dw, dx, dc, scal[0], scal[1], scal[2], cd.ctl);
  else
    k_kick_drift_za<T, false><<<nblk_stride(g.Nhp), 256>>>(g, dq, dp, dg, dw, dx, dc, scal[0], scal[1], scal[2], cd.ctl);
  Outs o;
  out(o, i_q, qk), out(o, i_p, pk), out(o, i_ck, Ck), out(o, cd.i_stop, ca.stop), out(o, cd.i_done, ca.steps_done);
  return pr.finish(o);
}

// scal = {a, b, c_kick}
template <typename T>
int assemble(int n, double L, int kick, const void *Ck, const void *qk, const double *wS, void *gk, void *pk,
             const double *scal, int like_mode, double *guard_slot, int *stop) {
  if (!ok3d(n) || !Ck || !gk || !scal || like_mode < 0 || like_mode > 2 || (scal[0] != 0. && !(qk && wS))) return -1;
  if (kick && !(pk && guard_slot && stop)) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  Probe pr;
  const size_t cb = (size_t)g.Nhp * sizeof(C2<T>);
  int i_g, i_p = -1, i_gs = -1;
  const C2<T> *dc = opt<const C2<T>>(pr, 3 * cb, Ck), *dq = opt<const C2<T>>(pr, cb, qk);
  const double *dw = opt<const double>(pr, (size_t)g.Nhp * sizeof(double), wS);
  C2<T> *dg = opt<C2<T>>(pr, cb, gk, &i_g), *dp = opt<C2<T>>(pr, cb, pk, &i_p);
  double *dgs = opt<double>(pr, sizeof(double), guard_slot, &i_gs);
  const int *ds = opt<const int>(pr, sizeof(int), stop);
  if (pr.err) return pr.err;
  if (kick)
    k_assemble<T, true><<<nblk_stride(g.Nhp), 256>>>(g, dc, dq, dw, dg, dp, scal[0], scal[1], like_mode, scal[2], dgs, ds);
  else
    k_assemble<T, false><<<nblk_stride(g.Nhp), 256>>>(g, dc, dq, dw, dg, dp, scal[0], scal[1], like_mode, scal[2], dgs, ds);
  Outs o;
  out(o, i_g, gk), out(o, i_p, pk), out(o, i_gs, guard_slot);
  return pr.finish(o);
}

// scal = {a, b, half_eps, eps, c_za}
template <typename T>
int step_boundary(int n, double L, int last, void *Ck, const void *q_in, const void *p_in, void *q_out, void *p_out,
                  void *gk, const double *wS, const double *wM, const double *scal, int like_mode, double *guard_slot,
                  const CtlArgs &ca) {
  if (!ok3d(n) || !Ck || !q_in || !p_in || !p_out || !scal || !guard_slot || like_mode < 0 || like_mode > 2) return -1;
  if ((last && !gk) || (!last && !q_out) || (scal[0] != 0. && !wS)) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  Probe pr;
  const size_t cb = (size_t)g.Nhp * sizeof(C2<T>), db = (size_t)g.Nhp * sizeof(double);
  int i_ck, i_qo = -1, i_po, i_g = -1, i_gs;
  C2<T> *dc = opt<C2<T>>(pr, 3 * cb, Ck, &i_ck);
  const C2<T> *dqi = opt<const C2<T>>(pr, cb, q_in), *dpi = opt<const C2<T>>(pr, cb, p_in);
  C2<T> *dqo = opt<C2<T>>(pr, cb, q_out, &i_qo), *dpo = opt<C2<T>>(pr, cb, p_out, &i_po), *dg = opt<C2<T>>(pr, cb, gk, &i_g);
  const double *dws = opt<const double>(pr, db, wS), *dwm = opt<const double>(pr, db, wM);
  double *dgs = opt<double>(pr, sizeof(double), guard_slot, &i_gs);
  const CtlDev cd = ctl_alloc(pr, ca);
  if (pr.err) return pr.err;
  if (last)
    k_step_boundary<T, true><<<nblk_stride(g.Nhp), 256>>>(g, dc, dqi, dpi, dqo, dpo, dg, dws, dwm, scal[0], scal[1], like_mode,
                                                         scal[2], scal[3], scal[4], dgs, cd.ctl);
  else
    k_step_boundary<T, false><<<nblk_stride(g.Nhp), 256>>>(g, dc, dqi, dpi, dqo, dpo, dg, dws, dwm, scal[0], scal[1],
                                                          like_mode, scal[2], scal[3], scal[4], dgs, cd.ctl);
  Outs o;
  out(o, i_ck, Ck), out(o, i_qo, q_out), out(o, i_po, p_out), out(o, i_g, gk), out(o, i_gs, guard_slot);
  out(o, cd.i_stop, ca.stop), out(o, cd.i_done, ca.steps_done);
  return pr.finish(o);
}

template <typename T> int alpt_poisson(int n, double L, const void *qk, void *d1k, void *phik, double scale) {
  if (!ok3d(n) || !qk || !d1k || !phik) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  Probe pr;
  const size_t cb = (size_t)g.Nhp * sizeof(C2<T>);
  const C2<T> *dq = static_cast<const C2<T> *>(pr.alloc(cb, qk));
  C2<T> *d1 = static_cast<C2<T> *>(pr.alloc(cb, d1k)), *dph = static_cast<C2<T> *>(pr.alloc(cb, phik));
  if (pr.err) return pr.err;
  k_alpt_poisson<T><<<nblk_stride(g.Nhp), 256>>>(g, dq, d1, dph, scale);
  return pr.finish({{1, d1k}, {2, phik}});
}

template <typename T> int alpt_mix(int n, double L, void *Ck, double smol, double inv_wtot, double inv_n) {
  if (!ok3d(n) || !Ck) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  Probe pr;
  C2<T> *d = static_cast<C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), Ck));
  if (pr.err) return pr.err;
  k_alpt_mix<T><<<nblk_stride(g.Nhp), 256>>>(g, d, smol, inv_wtot, inv_n);
  return pr.finish({{0, Ck}});
}

// k_prepare_mult: corr (n^3, full grid) -> mult (n^2 nhp; goes in too, the row padding must come back as it went in)
int prepare_mult(int n, int esz, const double *corr, double *mult, double normFS) {
  if (!ok3d(n) || !corr || !mult) return -1;
  const Geo g = probe_geo(n, esz);
  Probe pr;
  const double *dc = static_cast<const double *>(pr.alloc((size_t)g.N * sizeof(double), corr));
  double *dm = static_cast<double *>(pr.alloc((size_t)g.Nhp * sizeof(double), mult));
  if (pr.err) return pr.err;
  k_prepare_mult<<<nblk_stride(g.Nhp), 256>>>(g, dc, dm, normFS);
  return pr.finish({{1, mult}});
}

// k_parseval: kRedBlocks partials
template <typename T> int parseval(int n, const void *xk, const double *w, double *partials) {
  if (!ok3d(n) || !xk || !w || !partials) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T));
  Probe pr;
  const C2<T> *dx = static_cast<const C2<T> *>(pr.alloc((size_t)g.Nhp * sizeof(C2<T>), xk));
  const double *dw = static_cast<const double *>(pr.alloc((size_t)g.Nhp * sizeof(double), w));
  double *dp = static_cast<double *>(pr.alloc((size_t)kRedBlocks * sizeof(double), partials));
  if (pr.err) return pr.err;
  k_parseval<T><<<kRedBlocks, 256>>>(g, dx, dw, dp);
  return pr.finish({{2, partials}});
}

// k_rollback over `count` complex elements of the two ping-pong pairs
template <typename T>
int rollback(long long count, const int *stop, const unsigned long long *steps_done, const void *q0, const void *p0,
             const void *q1, const void *p1, void *q_dst, void *p_dst) {
  if (count < 1 || count > (1ll << 28) || !stop || !steps_done || !q0 || !p0 || !q1 || !p1 || !q_dst || !p_dst) return -1;
  if (*stop && *steps_done < 1) return -1;
  Probe pr;
  const size_t cb = (size_t)count * sizeof(C2<T>);
  const int *ds = static_cast<const int *>(pr.alloc(sizeof(int), stop));
  const unsigned long long *dd = static_cast<const unsigned long long *>(pr.alloc(sizeof(unsigned long long), steps_done));
  const C2<T> *a0 = static_cast<const C2<T> *>(pr.alloc(cb, q0)), *b0 = static_cast<const C2<T> *>(pr.alloc(cb, p0));
  const C2<T> *a1 = static_cast<const C2<T> *>(pr.alloc(cb, q1)), *b1 = static_cast<const C2<T> *>(pr.alloc(cb, p1));
  C2<T> *dq = static_cast<C2<T> *>(pr.alloc(cb, q_dst)), *dp = static_cast<C2<T> *>(pr.alloc(cb, p_dst));
  if (pr.err) return pr.err;
  k_rollback<T><<<nblk_stride(count), 256>>>(count, ds, dd, a0, b0, a1, b1, dq, dp);
  return pr.finish({{6, q_dst}, {7, p_dst}});
}

// ---- the real-space ALPT and calc_h 0 / 3 kernels ----------------------------------------------------------------------

// the stencil kernels index rows as int slots and wrap with c +- 2: the engine's smallest grid is 4
bool ok_rs(int n) { return n >= 4 && n <= 512; }

// k_alpt_grad: phi (n^3) -> g3 (3 n^3; goes in too)
template <typename T> int alpt_grad(int n, double L, const void *phi, void *g3) {
  if (!ok_rs(n) || !phi || !g3) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  Probe pr;
  const T *dp = static_cast<const T *>(pr.alloc((size_t)g.N * sizeof(T), phi));
  T *dg = static_cast<T *>(pr.alloc((size_t)3 * g.N * sizeof(T), g3));
  if (pr.err) return pr.err;
  k_alpt_grad<T><<<stencil_grid(g.n), 256>>>(g, dp, dg);
  return pr.finish({{1, g3}});
}

// k_alpt_sources with alpt_middle's pointer layouts.  layout 0 (planes path): a_out == d1, b_out = other;
// layout 1 (3-D path): b_out == d1, a_out = other.  d1 and other (n^3 each) go in and come back.
template <typename T> int alpt_sources(int n, double L, int layout, const void *g3, void *d1, void *other, double D1, double D2) {
  if (!ok_rs(n) || !g3 || !d1 || !other || (layout != 0 && layout != 1)) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  Probe pr;
  const T *dg = static_cast<const T *>(pr.alloc((size_t)3 * g.N * sizeof(T), g3));
  T *dd = static_cast<T *>(pr.alloc((size_t)g.N * sizeof(T), d1));
  T *dx = static_cast<T *>(pr.alloc((size_t)g.N * sizeof(T), other));
  if (pr.err) return pr.err;
  k_alpt_sources<T><<<stencil_grid(g.n), 256>>>(g, dg, dd, layout ? dx : dd, layout ? dd : dx, D1, D2);
  return pr.finish({{1, d1}, {2, other}});
}

// k_alpt_kernel_table: out (n^2 nhp complex; goes in too)
template <typename T> int alpt_kernel_table(int n, double L, void *tab, double smol) {
  if (!ok3d(n) || !tab) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  Probe pr;
  C2<T> *d = static_cast<C2<T> *>(pr.alloc((size_t)g.Nhp * sizeof(C2<T>), tab));
  if (pr.err) return pr.err;
  k_alpt_kernel_table<T><<<nblk_stride(g.Nhp), 256>>>(g, d, smol);
  return pr.finish({{0, tab}});
}

// k_findif_mul: dX, plike (n^3) -> V (3 n^3; goes in too)
template <typename T>
int findif_mul(int n, double L, int likelihood, double rho_c, double delta_min, const void *dX, const void *plike, void *V) {
  if (!ok_rs(n) || !dX || !plike || !V || likelihood < 0 || likelihood > 2) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  LikePar lp{};
  lp.rho_c = rho_c, lp.biasP = 1., lp.biasE = 1., lp.delta_min = delta_min, lp.likelihood = likelihood, lp.bias_is_identity = 1;
  Probe pr;
  const T *dx = static_cast<const T *>(pr.alloc((size_t)g.N * sizeof(T), dX));
  const T *dl = static_cast<const T *>(pr.alloc((size_t)g.N * sizeof(T), plike));
  T *dv = static_cast<T *>(pr.alloc((size_t)3 * g.N * sizeof(T), V));
  if (pr.err) return pr.err;
  k_findif_mul<T><<<nblk_stride(g.N), 256>>>(g, lp, dx, dl, dv);
  return pr.finish({{2, V}});
}

// k_gradfft_mult / k_conv_kernel: one half-complex array in (n^2 nhp), three out (3 n^2 nhp; go in too)
template <typename T> int gradfft_mult(int n, double L, const void *fk, void *Ck, double inv_n) {
  if (!ok3d(n) || !fk || !Ck) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  Probe pr;
  const C2<T> *df = static_cast<const C2<T> *>(pr.alloc((size_t)g.Nhp * sizeof(C2<T>), fk));
  C2<T> *dc = static_cast<C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), Ck));
  if (pr.err) return pr.err;
  k_gradfft_mult<T><<<nblk_stride(g.Nh), 256>>>(g, df, dc, inv_n);
  return pr.finish({{1, Ck}});
}

template <typename T> int conv_kernel(int n, double L, const void *pl, const double *F, void *Ck, double hh, double inv_n) {
  if (!ok3d(n) || !pl || !F || !Ck) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  Probe pr;
  const C2<T> *dl = static_cast<const C2<T> *>(pr.alloc((size_t)g.Nhp * sizeof(C2<T>), pl));
  const double *df = static_cast<const double *>(pr.alloc((size_t)g.Nhp * sizeof(double), F));
  C2<T> *dc = static_cast<C2<T> *>(pr.alloc((size_t)3 * g.Nhp * sizeof(C2<T>), Ck));
  if (pr.err) return pr.err;
  k_conv_kernel<T><<<nblk_stride(g.Nh), 256>>>(g, dl, df, dc, hh, inv_n);
  return pr.finish({{2, Ck}});
}

// k_mul3 over `count` elements: a (count), b3 (3 count) -> out3 (3 count; goes in too)
template <typename T> int mul3(long long count, const void *a, const void *b3, void *out3) {
  if (count < 1 || count > (1ll << 27) || !a || !b3 || !out3) return -1;
  Probe pr;
  const T *da = static_cast<const T *>(pr.alloc((size_t)count * sizeof(T), a));
  const T *db = static_cast<const T *>(pr.alloc((size_t)3 * count * sizeof(T), b3));
  T *dout = static_cast<T *>(pr.alloc((size_t)3 * count * sizeof(T), out3));
  if (pr.err) return pr.err;
  k_mul3<T><<<nblk_stride(count), 256>>>(count, da, db, dout);
  return pr.finish({{2, out3}});
}

// k_interp_tsc: psi, conv (3 n^3 each) -> V (3 n^3; goes in too).  pos = {cpecvel, v_norm}; periodic as make_pos sets it.
template <typename T>
int interp_tsc(int n, double L, int rsd, const double *pos, double f1, const void *psi, const void *conv, void *V) {
  if (!ok3d(n) || !pos || !psi || !conv || !V || (rsd != 0 && rsd != 1)) return -1;
  const Geo g = probe_geo(n, (int)sizeof(T), L);
  PosPar pp{};
  pp.d = g.d, pp.L = g.L, pp.cpecvel = pos[0], pp.v_norm = pos[1], pp.rsd = rsd, pp.periodic = 1;
  Probe pr;
  const T *dp = static_cast<const T *>(pr.alloc((size_t)3 * g.N * sizeof(T), psi));
  const T *dc = static_cast<const T *>(pr.alloc((size_t)3 * g.N * sizeof(T), conv));
  T *dv = static_cast<T *>(pr.alloc((size_t)3 * g.N * sizeof(T), V));
  if (pr.err) return pr.err;
  k_interp_tsc<T><<<nblk_full(g.N), 256>>>(g, pp, f1, dp, dc, dv);
  return pr.finish({{2, V}});
}

// k_tweb_eigen<T, double> and k_tweb_reduce on `count` cells as bchmc_tweb_classify launches them: t6 = six arrays of T one
// after the other (xx, xy, xz, yy, yz, zz), x (count doubles, may be null: every mass weight is 1), lam (3 count
// doubles, may be null), type (count bytes), res (kTwebWords 64-bit words: n_type[4], n_nonfinite, the bits of
// mass_type[4]).  Device arrays: t6, x if given, lam if given, type, the partials.
template <typename T>
int tweb_eigen(long long count, const void *t6, const double *x, double lambda_th, double *lam, unsigned char *type,
               unsigned long long *res) {
  if (count < 1 || count > (1ll << 27) || !t6 || !type || !res) return -1;
  Probe pr;
  const T *dt = static_cast<const T *>(pr.alloc((size_t)6 * count * sizeof(T), t6));
  const double *dx = opt<double>(pr, (size_t)count * sizeof(double), x);
  int i_lam = -1;
  double *dl = opt<double>(pr, (size_t)3 * count * sizeof(double), lam, &i_lam);
  unsigned char *dty = static_cast<unsigned char *>(pr.alloc((size_t)count, type));
  const int i_ty = (int)pr.bufs.size() - 1;
  const int nblk = nblk_stride(count);
  unsigned long long *dp = static_cast<unsigned long long *>(pr.alloc(((size_t)nblk + 1) * kTwebWords * sizeof(unsigned long long), nullptr));
  if (pr.err) return pr.err;
  TwebTensor t;
  for (int c = 0; c < 6; c++) t.c[c] = dt + (size_t)c * count;
  k_tweb_eigen<T, double><<<nblk, kTwebBlock>>>(count, t, dx, lambda_th, dl, dty, dp);
  k_tweb_reduce<<<kTwebWords, kWave>>>(nblk, dp, dp + (size_t)nblk * kTwebWords);
  Outs o{{i_ty, type}};
  out(o, i_lam, lam);
  const int rc = pr.finish(o);
  if (rc) return rc;
  if (!pr.ok(hipMemcpy(res, dp + (size_t)nblk * kTwebWords, kTwebWords * sizeof(unsigned long long), hipMemcpyDeviceToHost)))
    return pr.err;
  return 0;
}

// k_bispec_triple and k_bispec_reduce on n_shell arrays of `count` cells as bchmc_bispectrum launches them: arrays = n_shell
// arrays of T one after the other, s3_end (kBispecMaxShell x kBispecMaxShell bytes: one past the last s3 the row
// (s1, s2) computes; null: every triplet is computed), sums (T doubles; a triplet beyond its row's end may hold anything),
// ms (may be null): the event time of the two kernels.  Device arrays: the arrays, the partials with the sums behind them.
template <typename T>
int bispec_triple(int n_shell, long long count, const void *arrays, const unsigned char *s3_end, double *sums, float *ms) {
  if (n_shell < 1 || n_shell > kBispecMaxShell || count < 1 || count > (1ll << 27) || !arrays || !sums) return -1;
  Probe pr;
  const T *da = static_cast<const T *>(pr.alloc((size_t)n_shell * count * sizeof(T), arrays));
  const int grid = bispec_grid(count), W = bispec_triplets(n_shell);
  double *dp = static_cast<double *>(pr.alloc(((size_t)grid + 1) * W * sizeof(double), nullptr));
  if (pr.err) return pr.err;
  const BispecPlan plan = bispec_plan(n_shell, reinterpret_cast<const unsigned char(*)[kBispecMaxShell]>(s3_end));
  BispecArrays arr{};
  for (int s = 0; s < n_shell; s++) arr.a[s] = da + (size_t)s * count;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (ms && (!pr.ok(hipEventCreate(&e0)) || !pr.ok(hipEventCreate(&e1)))) return pr.err;
  if (ms) pr.ok(hipEventRecord(e0, nullptr));
  pr.ok(launch_bispec_triple<T>(nullptr, count, n_shell, arr, plan, dp, dp + (size_t)grid * W));
  if (ms) pr.ok(hipEventRecord(e1, nullptr));
  int rc = pr.finish({});
  if (!rc && ms && !pr.ok(hipEventElapsedTime(ms, e0, e1))) rc = pr.err;
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (rc) return rc;
  if (!pr.ok(hipMemcpy(sums, dp + (size_t)grid * W, (size_t)W * sizeof(double), hipMemcpyDeviceToHost))) return pr.err;
  return 0;
}

// k_white_noise over n values as chain_draw launches it: var (n values of T, may be null), out (n values; goes in too)
template <typename T>
int white_noise(long long n, unsigned seed_lo, unsigned seed_hi, unsigned attempt, unsigned stream, const void *var, void *out_) {
  if (n < 1 || n > (1ll << 27) || !out_) return -1;
  Probe pr;
  const T *dv = opt<const T>(pr, (size_t)n * sizeof(T), var);
  T *dout = static_cast<T *>(pr.alloc((size_t)n * sizeof(T), out_));
  const int i_out = (int)pr.bufs.size() - 1;
  if (pr.err) return pr.err;
  k_white_noise<T><<<nblk_stride((n + 1) / 2), 256>>>(n, make_uint2(seed_lo, seed_hi), attempt, stream, dv, dout);
  return pr.finish({{i_out, out_}});
}

// k_color_momenta over nh complex elements: wk (nh complex), wM (nh doubles, may be null), pk (nh complex; goes in too)
template <typename T> int color_momenta(long long nh, const void *wk, const double *wM, void *pk, int accumulate) {
  if (nh < 1 || nh > (1ll << 27) || !wk || !pk) return -1;
  Probe pr;
  const C2<T> *dw = static_cast<const C2<T> *>(pr.alloc((size_t)nh * sizeof(C2<T>), wk));
  const double *dm = opt<const double>(pr, (size_t)nh * sizeof(double), wM);
  C2<T> *dp = static_cast<C2<T> *>(pr.alloc((size_t)nh * sizeof(C2<T>), pk));
  const int i_pk = (int)pr.bufs.size() - 1;
  if (pr.err) return pr.err;
  k_color_momenta<T><<<nblk_stride(nh), 256>>>(nh, dw, dm, dp, accumulate);
  return pr.finish({{i_pk, pk}});
}

// ---- the generic trajectory's real-space mass and GRF kernels ----------------------------------------------------------

// what a probe over `count` elements accepts (the engine's largest grid is 512^3 = 2^27 cells)
bool ok_count(long long count) { return count >= 1 && count <= (1ll << 27); }

// k_div_mass_r over `count` cells: p, mass_r -> out (goes in too).  out == p is the engine's call (in place on iop): then
// one device array holds both.
template <typename T> int div_mass_r(long long count, const void *p, const void *mass_r, void *out_) {
  if (!ok_count(count) || !p || !mass_r || !out_) return -1;
  Probe pr;
  const size_t rb = (size_t)count * sizeof(T);
  const bool in_place = out_ == p;
  T *dp = static_cast<T *>(pr.alloc(rb, p));
  const T *dm = static_cast<const T *>(pr.alloc(rb, mass_r));
  T *dout = in_place ? dp : static_cast<T *>(pr.alloc(rb, out_));
  if (pr.err) return pr.err;
  k_div_mass_r<T><<<nblk_stride(count), 256>>>(count, dp, dm, dout);
  return pr.finish({{in_place ? 0 : 2, out_}});
}

// k_kin_rs over `count` cells: kRedBlocks partials (go in too)
template <typename T> int kin_rs(long long count, const void *p, const void *mass_r, double *partials) {
  if (!ok_count(count) || !p || !mass_r || !partials) return -1;
  Probe pr;
  const size_t rb = (size_t)count * sizeof(T);
  const T *dp = static_cast<const T *>(pr.alloc(rb, p)), *dm = static_cast<const T *>(pr.alloc(rb, mass_r));
  double *dpart = static_cast<double *>(pr.alloc((size_t)kRedBlocks * sizeof(double), partials));
  if (pr.err) return pr.err;
  k_kin_rs<T><<<kRedBlocks, 256>>>(count, dp, dm, dpart);
  return pr.finish({{2, partials}});
}

// k_grf_grad / k_grf_loglike over `count` cells: q, nobs, noise, window -> out (goes in too) / kRedBlocks partials (go in too)
template <typename T, bool ENERGY>
int grf(long long count, const void *q, const void *nobs, const void *noise, const void *window, void *out_) {
  if (!ok_count(count) || !q || !nobs || !noise || !window || !out_) return -1;
  Probe pr;
  const size_t rb = (size_t)count * sizeof(T);
  const T *dq = static_cast<const T *>(pr.alloc(rb, q)), *dn = static_cast<const T *>(pr.alloc(rb, nobs));
  const T *ds = static_cast<const T *>(pr.alloc(rb, noise)), *dw = static_cast<const T *>(pr.alloc(rb, window));
  void *dout = pr.alloc(ENERGY ? (size_t)kRedBlocks * sizeof(double) : rb, out_);
  if (pr.err) return pr.err;
  if (ENERGY)
    k_grf_loglike<T><<<kRedBlocks, 256>>>(count, dq, dn, ds, dw, static_cast<double *>(dout));
  else
    k_grf_grad<T><<<nblk_stride(count), 256>>>(count, dq, dn, ds, dw, static_cast<T *>(dout));
  return pr.finish({{4, out_}});
}

// k_scale_c over `count` complex elements: in -> out (goes in too)
template <typename T> int scale_c(long long count, const void *in, void *out_, double s) {
  if (!ok_count(count) || !in || !out_) return -1;
  Probe pr;
  const size_t cb = (size_t)count * sizeof(C2<T>);
  const C2<T> *din = static_cast<const C2<T> *>(pr.alloc(cb, in));
  C2<T> *dout = static_cast<C2<T> *>(pr.alloc(cb, out_));
  if (pr.err) return pr.err;
  k_scale_c<T><<<nblk_stride(count), 256>>>(count, din, dout, s);
  return pr.finish({{1, out_}});
}

// k_add_r over `count` cells: a, b -> out (goes in too)
template <typename T> int add_r(long long count, const void *a, const void *b, void *out_) {
  if (!ok_count(count) || !a || !b || !out_) return -1;
  Probe pr;
  const size_t rb = (size_t)count * sizeof(T);
  const T *da = static_cast<const T *>(pr.alloc(rb, a)), *db = static_cast<const T *>(pr.alloc(rb, b));
  T *dout = static_cast<T *>(pr.alloc(rb, out_));
  if (pr.err) return pr.err;
  k_add_r<T><<<nblk_stride(count), 256>>>(count, da, db, dout);
  return pr.finish({{2, out_}});
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

// k_ypass_pair: components 0 (Psi^_x) and 1 (B) of ck -> the inverse y transforms of Psi^_x, ky B, kz B in components 0, 1, 2
int fftp_ypass_pair(int prec, int n, double box_len, void *ck) {
  return prec ? ypass_pair<float>(n, box_len, ck) : ypass_pair<double>(n, box_len, ck);
}

// k_zr2c: V (3 n^3 real) -> ck (3 n^2 nhp complex; the row padding comes back as it went in)
int fftp_zr2c(int prec, int n, const void *V, void *ck) {
  return prec ? zr2c<float>(n, V, ck) : zr2c<double>(n, V, ck);
}

// k_zr2c from the gather's V records: V (n^3 records {vx, vy, vz, unused}) -> ck as fftp_zr2c
int fftp_zr2c_rec(int prec, int n, const void *V, void *ck) {
  return prec ? zr2c<float, true>(n, V, ck) : zr2c<double, true>(n, V, ck);
}

// k_ypass_fwd_pair: the three z-transformed components of V in ck -> the forward y transforms of component 0 in component 0
// and W = ky V^_y + kz V^_z in component 1; component 2 comes back as it went in
int fftp_ypass_fwd_pair(int prec, int n, double box_len, void *ck) {
  return prec ? ypass_fwd_pair<float>(n, box_len, ck) : ypass_fwd_pair<double>(n, box_len, ck);
}

// k_zbin_direct<PSI_ONLY>: ck (3 n^2 nhp complex) -> psi (3 n^3 real)
int fftp_zc2r(int prec, int n, const void *ck, void *psi) {
  return prec ? zc2r<float>(n, ck, psi) : zc2r<double>(n, ck, psi);
}

// ---- the k-space step kernels.  box_len: the box side L (kfac = 2 pi / L); <= 0 means L = n.  Host arrays that the engine
// may pass as null may be null here; output arrays go in as well and come back, so what a kernel leaves alone is seen.

// k_step_boundary_x (mode 0 interior, 1 first, 2 last; alpt; two_tile: k_step_boundary_x2).  scal = {a, b, half_eps, eps,
// c_za}.  Ck: 3 n^2 nhp complex in planes space; the others n^2 nhp.  Device array numbers for a canary return: 1 twiddles,
// then the non-null ones of Ck, q_in, p_in, g_in, q_out, p_out, g_out, wS, wM, guard_slot, stop, steps_done, guard_prev.
int fftp_step_boundary_x(int prec, int n, double box_len, int mode, int alpt, int two_tile, void *Ck, const void *q_in,
                         const void *p_in, const void *g_in, void *q_out, void *p_out, void *g_out, const double *wS,
                         const double *wM, const double *scal, double *guard_slot, int *stop,
                         unsigned long long *steps_done, const double *guard_prev, double guard_limit,
                         unsigned long long step_index) {
  const CtlArgs ca{stop, steps_done, guard_prev, guard_limit, step_index};
  if (!stop || !steps_done) return -1;
  return prec ? step_boundary_x<float>(n, box_len, mode, alpt, two_tile, Ck, q_in, p_in, g_in, q_out, p_out, g_out, wS, wM,
                                       scal, guard_slot, ca)
              : step_boundary_x<double>(n, box_len, mode, alpt, two_tile, Ck, q_in, p_in, g_in, q_out, p_out, g_out, wS, wM,
                                        scal, guard_slot, ca);
}

// fftp_step_boundary_x with the `vpair` flag (interior or last, Zel'dovich): Ck[0], Ck[1] hold V^_x | W of k_ypass_fwd_pair,
// Ck[2] is not read
int fftp_step_boundary_x_vpair(int prec, int n, double box_len, int mode, int alpt, int two_tile, void *Ck, const void *q_in,
                               const void *p_in, const void *g_in, void *q_out, void *p_out, void *g_out, const double *wS,
                               const double *wM, const double *scal, double *guard_slot, int *stop,
                               unsigned long long *steps_done, const double *guard_prev, double guard_limit,
                               unsigned long long step_index, int vpair) {
  const CtlArgs ca{stop, steps_done, guard_prev, guard_limit, step_index};
  if (!stop || !steps_done) return -1;
  return prec ? step_boundary_x<float>(n, box_len, mode, alpt, two_tile, Ck, q_in, p_in, g_in, q_out, p_out, g_out, wS, wM,
                                       scal, guard_slot, ca, vpair)
              : step_boundary_x<double>(n, box_len, mode, alpt, two_tile, Ck, q_in, p_in, g_in, q_out, p_out, g_out, wS, wM,
                                        scal, guard_slot, ca, vpair);
}

// fftp_step_boundary_x_vpair through the XT instantiations (Zel'dovich; wM required): wpair = n^2 nhp {wS, wM} in x-column
// tiles (xtile.hpp), and of the state arrays q_in, p_in (interior, last), q_out, p_out (interior, first) are tiled too -- Ck,
// g_in, g_out and the last boundary's p_out natural.  wS is not read.  wpair is the last device array of a canary return.
int fftp_step_boundary_x_xtile(int prec, int n, double box_len, int mode, int two_tile, void *Ck, const void *q_in,
                               const void *p_in, const void *g_in, void *q_out, void *p_out, void *g_out, const double *wS,
                               const double *wM, const double *scal, double *guard_slot, int *stop,
                               unsigned long long *steps_done, const double *guard_prev, double guard_limit,
                               unsigned long long step_index, int vpair, const void *wpair) {
  const CtlArgs ca{stop, steps_done, guard_prev, guard_limit, step_index};
  if (!stop || !steps_done || !wpair) return -1;
  return prec ? step_boundary_x<float>(n, box_len, mode, 0, two_tile, Ck, q_in, p_in, g_in, q_out, p_out, g_out, wS, wM,
                                       scal, guard_slot, ca, vpair, wpair)
              : step_boundary_x<double>(n, box_len, mode, 0, two_tile, Ck, q_in, p_in, g_in, q_out, p_out, g_out, wS, wM,
                                        scal, guard_slot, ca, vpair, wpair);
}

// k_xtile_weights as trajectory_fused launches it: wS, wM (n^2 nhp doubles, natural) -> pair (n^2 nhp {wS, wM}, tiled for
// the storage type's KB).  Device arrays: 1 wS, 2 wM, 3 pair.
int fftp_xtile_weights(int prec, int n, const double *wS, const double *wM, void *pair) {
  const int esz = prec ? 4 : 8;
  if (!x_shape(esz, n).nt || !wS || !wM || !pair) return -1;
  const Geo g = probe_geo(n, esz);
  if (g.nhp % pass_kb(esz)) return -1;
  Probe pr;
  const size_t db = (size_t)g.Nhp * sizeof(double);
  const double *d_ws = static_cast<const double *>(pr.alloc(db, wS)), *d_wm = static_cast<const double *>(pr.alloc(db, wM));
  double2 *d_pair = static_cast<double2 *>(pr.alloc(2 * db, pair));
  if (pr.err) return pr.err;
  k_xtile_weights<<<nblk_stride(g.Nhp), 256>>>(g, pass_kb(esz), d_ws, d_wm, d_pair);
  return pr.finish({{2, pair}});
}

// k_alpt_mix_x on Ck (3 n^2 nhp complex in planes space: A^, B^ in; the three displacement components out)
int fftp_alpt_mix_x(int prec, int n, double box_len, void *Ck, double smol, double inv_wtot, double inv_n) {
  return prec ? alpt_mix_x<float>(n, box_len, Ck, smol, inv_wtot, inv_n)
              : alpt_mix_x<double>(n, box_len, Ck, smol, inv_wtot, inv_n);
}

// k_kick_drift_za<T, DRIFT>, in place on qk, pk.  scal = {half_eps, eps, c_za}
int fftp_kick_drift_za(int prec, int n, double box_len, int drift, void *qk, void *pk, const void *gk, const double *wM,
                       const void *extra, void *Ck, const double *scal, int *stop, unsigned long long *steps_done,
                       const double *guard_prev, double guard_limit, unsigned long long step_index) {
  const CtlArgs ca{stop, steps_done, guard_prev, guard_limit, step_index};
  if (!stop || !steps_done) return -1;
  return prec ? kick_drift_za<float>(n, box_len, drift, qk, pk, gk, wM, extra, Ck, scal, ca)
              : kick_drift_za<double>(n, box_len, drift, qk, pk, gk, wM, extra, Ck, scal, ca);
}

// k_assemble<T, KICK>.  scal = {a, b, c_kick}
int fftp_assemble(int prec, int n, double box_len, int kick, const void *Ck, const void *qk, const double *wS, void *gk,
                  void *pk, const double *scal, int like_mode, double *guard_slot, int *stop) {
  return prec ? assemble<float>(n, box_len, kick, Ck, qk, wS, gk, pk, scal, like_mode, guard_slot, stop)
              : assemble<double>(n, box_len, kick, Ck, qk, wS, gk, pk, scal, like_mode, guard_slot, stop);
}

// k_step_boundary<T, LAST>.  scal = {a, b, half_eps, eps, c_za}
int fftp_step_boundary(int prec, int n, double box_len, int last, void *Ck, const void *q_in, const void *p_in, void *q_out,
                       void *p_out, void *gk, const double *wS, const double *wM, const double *scal, int like_mode,
                       double *guard_slot, int *stop, unsigned long long *steps_done, const double *guard_prev,
                       double guard_limit, unsigned long long step_index) {
  const CtlArgs ca{stop, steps_done, guard_prev, guard_limit, step_index};
  if (!stop || !steps_done) return -1;
  return prec ? step_boundary<float>(n, box_len, last, Ck, q_in, p_in, q_out, p_out, gk, wS, wM, scal, like_mode, guard_slot, ca)
              : step_boundary<double>(n, box_len, last, Ck, q_in, p_in, q_out, p_out, gk, wS, wM, scal, like_mode, guard_slot,
                                      ca);
}

int fftp_alpt_poisson(int prec, int n, double box_len, const void *qk, void *d1k, void *phik, double scale) {
  return prec ? alpt_poisson<float>(n, box_len, qk, d1k, phik, scale) : alpt_poisson<double>(n, box_len, qk, d1k, phik, scale);
}

int fftp_alpt_mix(int prec, int n, double box_len, void *Ck, double smol, double inv_wtot, double inv_n) {
  return prec ? alpt_mix<float>(n, box_len, Ck, smol, inv_wtot, inv_n) : alpt_mix<double>(n, box_len, Ck, smol, inv_wtot, inv_n);
}

// k_prepare_mult: corr (n^3 doubles) -> mult (n^2 nhp doubles, nhp that of `prec`)
int fftp_prepare_mult(int prec, int n, const double *corr, double *mult, double normFS) {
  return prepare_mult(n, prec ? 4 : 8, corr, mult, normFS);
}

// number of partials k_parseval writes
int fftp_parseval_blocks(void) { return kRedBlocks; }
int fftp_parseval(int prec, int n, const void *xk, const double *w, double *partials) {
  return prec ? parseval<float>(n, xk, w, partials) : parseval<double>(n, xk, w, partials);
}

int fftp_rollback(int prec, long long count, const int *stop, const unsigned long long *steps_done, const void *q0,
                  const void *p0, const void *q1, const void *p1, void *q_dst, void *p_dst) {
  return prec ? rollback<float>(count, stop, steps_done, q0, p0, q1, p1, q_dst, p_dst)
              : rollback<double>(count, stop, steps_done, q0, p0, q1, p1, q_dst, p_dst);
}

// ---- the real-space ALPT and calc_h 0 / 3 kernels.  Device array numbers for a canary return: the arrays in argument order.

// number of workgroups of the two stencil passes
int fftp_stencil_grid(int n) { return stencil_grid(n); }

int fftp_alpt_grad(int prec, int n, double box_len, const void *phi, void *g3) {
  return prec ? alpt_grad<float>(n, box_len, phi, g3) : alpt_grad<double>(n, box_len, phi, g3);
}

// layout 0: a_out == d1 (planes path), b_out = other;  layout 1: b_out == d1 (3-D path), a_out = other
int fftp_alpt_sources(int prec, int n, double box_len, int layout, const void *g3, void *d1, void *other, double D1, double D2) {
  return prec ? alpt_sources<float>(n, box_len, layout, g3, d1, other, D1, D2)
              : alpt_sources<double>(n, box_len, layout, g3, d1, other, D1, D2);
}

int fftp_alpt_kernel_table(int prec, int n, double box_len, void *tab, double smol) {
  return prec ? alpt_kernel_table<float>(n, box_len, tab, smol) : alpt_kernel_table<double>(n, box_len, tab, smol);
}

int fftp_findif_mul(int prec, int n, double box_len, int likelihood, double rho_c, double delta_min, const void *dX,
                    const void *plike, void *V) {
  return prec ? findif_mul<float>(n, box_len, likelihood, rho_c, delta_min, dX, plike, V)
              : findif_mul<double>(n, box_len, likelihood, rho_c, delta_min, dX, plike, V);
}

int fftp_gradfft_mult(int prec, int n, double box_len, const void *fk, void *Ck, double inv_n) {
  return prec ? gradfft_mult<float>(n, box_len, fk, Ck, inv_n) : gradfft_mult<double>(n, box_len, fk, Ck, inv_n);
}

// F: n^2 nhp doubles (nhp that of `prec`)
int fftp_conv_kernel(int prec, int n, double box_len, const void *pl, const double *F, void *Ck, double hh, double inv_n) {
  return prec ? conv_kernel<float>(n, box_len, pl, F, Ck, hh, inv_n) : conv_kernel<double>(n, box_len, pl, F, Ck, hh, inv_n);
}

int fftp_mul3(int prec, long long count, const void *a, const void *b3, void *out3) {
  return prec ? mul3<float>(count, a, b3, out3) : mul3<double>(count, a, b3, out3);
}

// pos = {cpecvel, v_norm}
int fftp_interp_tsc(int prec, int n, double box_len, int rsd, const double *pos, double f1, const void *psi,
                    const void *conv, void *V) {
  return prec ? interp_tsc<float>(n, box_len, rsd, pos, f1, psi, conv, V)
              : interp_tsc<double>(n, box_len, rsd, pos, f1, psi, conv, V);
}

// ---- the T-web's eigenvalue kernel on chosen tensors (tests/test_gpu_tweb.py)
int fftp_tweb_eigen(int prec, long long count, const void *t6, const double *x, double lambda_th, double *lam,
                    unsigned char *type, unsigned long long *res) {
  return prec ? tweb_eigen<float>(count, t6, x, lambda_th, lam, type, res)
              : tweb_eigen<double>(count, t6, x, lambda_th, lam, type, res);
}

// ---- the bispectrum's contraction kernel on chosen arrays (tests/test_gpu_bispec.py, scripts/bispec_bench.py)
int fftp_bispec_triple(int prec, int n_shell, long long count, const void *arrays, const unsigned char *s3_end, double *sums,
                       float *ms) {
  return prec ? bispec_triple<float>(n_shell, count, arrays, s3_end, sums, ms)
              : bispec_triple<double>(n_shell, count, arrays, s3_end, sums, ms);
}

// ---- the Philox momentum draw's two kernels (tests/test_gpu_draw.py).  Device arrays: the non-null ones in argument order.
int fftp_white_noise(int prec, long long n, unsigned seed_lo, unsigned seed_hi, unsigned attempt, unsigned stream,
                     const void *var, void *out) {
  return prec ? white_noise<float>(n, seed_lo, seed_hi, attempt, stream, var, out)
              : white_noise<double>(n, seed_lo, seed_hi, attempt, stream, var, out);
}

int fftp_color_momenta(int prec, long long nh, const void *wk, const double *wM, void *pk, int accumulate) {
  return prec ? color_momenta<float>(nh, wk, wM, pk, accumulate) : color_momenta<double>(nh, wk, wM, pk, accumulate);
}

// ---- the generic trajectory's real-space mass and GRF kernels (tests/test_gpu_massrs.py).  Device arrays: the arrays in
// argument order; output arrays go in as well.  `partials`: fftp_parseval_blocks() doubles.

// out == p runs the kernel in place, as the engine does on iop (device arrays then: 1 p and out, 2 mass_r)
int fftp_div_mass_r(int prec, long long count, const void *p, const void *mass_r, void *out) {
  return prec ? div_mass_r<float>(count, p, mass_r, out) : div_mass_r<double>(count, p, mass_r, out);
}

int fftp_kin_rs(int prec, long long count, const void *p, const void *mass_r, double *partials) {
  return prec ? kin_rs<float>(count, p, mass_r, partials) : kin_rs<double>(count, p, mass_r, partials);
}

int fftp_grf_grad(int prec, long long count, const void *q, const void *nobs, const void *noise, const void *window,
                  void *out) {
  return prec ? grf<float, false>(count, q, nobs, noise, window, out) : grf<double, false>(count, q, nobs, noise, window, out);
}

int fftp_grf_loglike(int prec, long long count, const void *q, const void *nobs, const void *noise, const void *window,
                     double *partials) {
  return prec ? grf<float, true>(count, q, nobs, noise, window, partials)
              : grf<double, true>(count, q, nobs, noise, window, partials);
}

// `count` complex elements
int fftp_scale_c(int prec, long long count, const void *in, void *out, double s) {
  return prec ? scale_c<float>(count, in, out, s) : scale_c<double>(count, in, out, s);
}

int fftp_add_r(int prec, long long count, const void *a, const void *b, void *out) {
  return prec ? add_r<float>(count, a, b, out) : add_r<double>(count, a, b, out);
}

}  // extern "C"
