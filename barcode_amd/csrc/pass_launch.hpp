// pass_launch.hpp -- the launch shapes of the engine's own FFT passes (step_boundary_x.hpp, alpt_x.hpp, zpass.hpp): for
// cells per axis n and a storage type of esz = 4 or 8 bytes, which instantiation, block size, dynamic LDS size and grid
// each pass gets.  The single statement of it: bchmc.hip launches the passes through here, and so does fft_probe.hip,
// whose test (tests/test_gpu_fft_passes.py) thereby runs the engine's launch code and not a copy of it.
//
// First part: the arithmetic, plain C++ (no HIP types; tests/host/pass_launch_check.cpp proves it against literals).
// Second part, for a HIP compile only: the launchers.  Which pass runs when is not in here: eval_plan.hpp decides that.
// The forward side of round 5 (k_zr2c from V records, k_ypass_fwd_pair, `vpair` of the boundary kernels) is launched from
// here like the rest: yfwd_pair_shape, launch_zr2c<T, REC>, launch_ypass_fwd_pair, BoundaryX::vpair.
#pragma once

#include <cstddef>

namespace bchmc {

// A column pass (x or y) gives each workgroup a tile of n x KB complex elements: KB neighbouring columns, one 128-byte
// line per row.  The kernels derive the same KB from their T.
constexpr int pass_kb(int esz) { return 128 / (2 * esz); }
constexpr int pass_nt_big(int esz) { return esz == 8 ? 256 : 512; }
constexpr int pass_nt_small(int esz) { return pass_nt_big(esz) / 4; }  // n = 32, 64 (tests)

struct PassShape {
  int nt = 0;   // threads per workgroup; 0: the pass is not available for this n
  int per = 0;  // template argument PER: elements of the tile per thread
};

// k_step_boundary_x, k_alpt_mix_x
constexpr PassShape x_shape(int esz, int n) {
  const int big = pass_nt_big(esz), small = pass_nt_small(esz);
  switch (n) {
    case 32: return {small, 4};
    case 64: return {small, 8};
    case 128: return {big, 4};
    case 256: return {2 * big, 4};  // 4 elements per thread: a little faster than 8 x NT_BIG
    case 512: return {2 * big, 8};
    default: return {};
  }
}
// k_step_boundary_x2 (two tiles per workgroup; PER <= 4 only)
constexpr PassShape x2_shape(int esz, int n) { return n == 128 || n == 256 ? x_shape(esz, n) : PassShape{}; }
// k_ypass
constexpr PassShape y_shape(int esz, int n) {
  const int nt = n == 128 ? 256 : 512;
  return n == 128 || n == 256 || n == 512 ? PassShape{nt, n * pass_kb(esz) / nt} : PassShape{};
}
// k_ypass_pair (the inverse y pass from the two arrays Psi^_x | B): k_ypass's tile and block; the workgroups of B make two
// transforms on the one tile, so the grid is that of two components (ypair_grid) and the LDS that of one tile
// (tests/host/two_array_check.cpp)
constexpr PassShape ypair_shape(int esz, int n) { return y_shape(esz, n); }
constexpr int ypair_comps = 2;
// k_ypass_fwd_pair (the forward y pass that leaves the two arrays V^_x | W = ky V^_y + kz V^_z): k_ypass_pair's shape, grid
// (ypair_grid) and one tile of LDS -- the workgroups of W make two transforms on the one tile too (tests/host/vpair_check.cpp)
constexpr PassShape yfwd_pair_shape(int esz, int n) { return ypair_shape(esz, n); }
// k_zr2c, k_zbin_direct: NZ = n, one lattice site along z per thread, over 6 interleaved rows
constexpr PassShape z_shape(int /*esz*/, int n) { return n == 128 || n == 256 || n == 512 ? PassShape{n, 6} : PassShape{}; }

// dynamic LDS: `tiles` column tiles, or the 6 rows of k_zr2c, and the n / 2 twiddles (k_zbin_direct: zbin_lds, zpass.hpp)
constexpr size_t col_lds(int esz, int n, int tiles = 1) { return ((size_t)tiles * n * pass_kb(esz) + n / 2) * 2 * esz; }
constexpr size_t zrow_lds(int esz, int n) { return ((size_t)n * 6 + n / 2) * 2 * esz; }

// workgroups: one per column tile of `comps` components with row stride nhp (fft_row_stride), one per 2 x 2 rows
constexpr int col_grid(int esz, int n, int nhp, int comps = 1) { return comps * n * (nhp / pass_kb(esz)); }
constexpr int row_grid(int n) { return (n / 2) * (n / 2); }
constexpr int ypair_grid(int esz, int n, int nhp) { return col_grid(esz, n, nhp, ypair_comps); }

}  // namespace bchmc

#ifdef __HIPCC__
#include "kernels.hpp"

#include <type_traits>

namespace bchmc {

// Launch with `lds` bytes of dynamic LDS: above the 48 KiB every kernel may use, the kernel's own limit is raised first.
template <typename... P, typename... A>
hipError_t launch_dyn_lds(hipStream_t stream, void (*kern)(P...), int grid, int threads, size_t lds, const A &...args) {
  if (lds > 48 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  kern<<<grid, threads, lds, stream>>>(args...);
  return hipGetLastError();
}

// Runtime n -> the compile-time row of a table: f(NT, PER) as std::integral_constant, for row N if that is n, or for the
// table's row of n.  hipErrorInvalidConfiguration where the table has none (callers ask the table first).
template <PassShape (*TABLE)(int, int), typename T, int N, typename F>
hipError_t pass_row(int n, F &f) {
  constexpr PassShape s = TABLE((int)sizeof(T), N);
  if constexpr (s.nt != 0) {
    if (n == N) return f(std::integral_constant<int, s.nt>{}, std::integral_constant<int, s.per>{});
  }
  return hipErrorInvalidConfiguration;
}
template <PassShape (*TABLE)(int, int), typename T, typename F>
hipError_t pass_dispatch(int n, F f) {
  switch (n) {
    case 32: return pass_row<TABLE, T, 32>(n, f);
    case 64: return pass_row<TABLE, T, 64>(n, f);
    case 128: return pass_row<TABLE, T, 128>(n, f);
    case 256: return pass_row<TABLE, T, 256>(n, f);
    case 512: return pass_row<TABLE, T, 512>(n, f);
    default: return hipErrorInvalidConfiguration;
  }
}

// what every pass is given: the stream, the geometry and the twiddle table (fft_twiddles)
template <typename T>
struct PassCtx {
  hipStream_t stream;
  Geo g;
  int log2n;
  const C2<T> *tw;
  int col_grid(int comps = 1) const { return bchmc::col_grid(sizeof(T), g.n, g.nhp, comps); }
  size_t col_lds(int tiles = 1) const { return bchmc::col_lds(sizeof(T), g.n, tiles); }
};

// k_ypass over the three components of ck, in place, inverse or forward (the engine launches the forward pass at n = 512
// only; 128 and 256 are the three-array reference of k_ypass_fwd_pair's test).
template <typename T, bool INV = true>
hipError_t launch_ypass(const PassCtx<T> &x, C2<T> *ck) {
  return pass_dispatch<y_shape, T>(x.g.n, [&](auto nt, auto per) {
    return launch_dyn_lds(x.stream, k_ypass<T, nt, per, BCHMC_YPASS_NT, INV>, x.col_grid(3), nt, x.col_lds(), x.g, x.log2n,
                          x.tw, ck);
  });
}

// k_ypass_fwd_pair: the three z-transformed components of V in ck -> ck[0] = V^_x, ck[1] = W for a boundary kernel with
// `vpair`; ck[2] is dead afterwards
template <typename T>
hipError_t launch_ypass_fwd_pair(const PassCtx<T> &x, C2<T> *ck) {
  return pass_dispatch<yfwd_pair_shape, T>(x.g.n, [&](auto nt, auto per) {
    return launch_dyn_lds(x.stream, k_ypass_fwd_pair<T, nt, per>, ypair_grid(sizeof(T), x.g.n, x.g.nhp),
                          nt, x.col_lds(), x.g, x.log2n, x.tw, ck);
  });
}

// k_ypass_pair: ck[0] = Psi^_x, ck[1] = B as a boundary kernel with `pair` left them -> the three y-transformed components
template <typename T>
hipError_t launch_ypass_pair(const PassCtx<T> &x, C2<T> *ck) {
  return pass_dispatch<ypair_shape, T>(x.g.n, [&](auto nt, auto per) {
    return launch_dyn_lds(x.stream, k_ypass_pair<T, nt, per, BCHMC_YPASS_NT>, ypair_grid(sizeof(T), x.g.n, x.g.nhp), nt,
                          x.col_lds(), x.g, x.log2n, x.tw, ck);
  });
}

// k_zr2c: V (3 n^3 real; REC: n^3 records of 4) -> ck
template <typename T, bool REC = false>
hipError_t launch_zr2c(const PassCtx<T> &x, const T *V, C2<T> *ck) {
  return pass_dispatch<z_shape, T>(x.g.n, [&](auto nz, auto) {
    return launch_dyn_lds(x.stream, k_zr2c<T, nz, REC>, row_grid(x.g.n), nz, zrow_lds(sizeof(T), x.g.n), x.g, x.log2n, x.tw, V,
                          ck);
  });
}

// k_zbin_direct: the z pass of ck ending in the binning, or (PSI_ONLY) in psi alone and only if *ovf is set.
// `out`: the kernel's arguments after ck (cnt, ovf, srec, V, zero_part, rho_zero, fix_zero, psi_out, vrec)
template <typename T, bool PSI_ONLY = false, typename... A>
hipError_t launch_zbin(const PassCtx<T> &x, const PosPar &pp, const SphPar &sp, const TilePar &tp, const C2<T> *ck,
                       const A &...out) {
  return pass_dispatch<z_shape, T>(x.g.n, [&](auto nz, auto) {
    return launch_dyn_lds(x.stream, k_zbin_direct<T, nz, PSI_ONLY>, row_grid(x.g.n), nz, zbin_lds<T>(x.g.n), x.g, pp, sp, tp,
                          x.log2n, x.tw, ck, out...);
  });
}

// k_alpt_mix_x on the two planes-space fields of Ck
template <typename T>
hipError_t launch_alpt_mix_x(const PassCtx<T> &x, C2<T> *Ck, double smol, double inv_wtot, double inv_n) {
  return pass_dispatch<x_shape, T>(x.g.n, [&](auto nt, auto per) {
    return launch_dyn_lds(x.stream, k_alpt_mix_x<T, nt, per>, x.col_grid(), nt, x.col_lds(), x.g, x.log2n, x.tw, Ck, smol,
                          inv_wtot, inv_n);
  });
}

// The step boundary's own arguments, by name (k_step_boundary_x): what a caller leaves out is null or zero, which is
// how the kernel is told "no momenta", "no kick", "no guard".
template <typename T>
struct BoundaryX {
  const C2<T> *qi = nullptr, *pi = nullptr;
  C2<T> *qo = nullptr, *po = nullptr;
  const double *wM = nullptr;
  double a = 0., b = 0., half_eps = 0., eps = 0., c_za = 0.;
  double *guard_slot = nullptr;
  StepCtl ctl{};
  const C2<T> *g_in = nullptr;
  C2<T> *g_out = nullptr;
  bool pair = false;  // the Zel'dovich inverse side leaves Psi^_x | B for k_ypass_pair instead of the three Psi^ components
  bool vpair = false;  // the Zel'dovich forward side reads V^_x | W as k_ypass_fwd_pair left them, not the three V^ components
  const double2 *wpair = nullptr;  // XT launches: {wS, wM} in x-column tiles (xtile.hpp); wS is not read then
};

// XT: the state (and a.wpair) in x-column tiles, as the kernel's comment says for each MODE; it needs a.wpair and, where
// the mode writes p, a p_out that is not p_in
template <typename T, int MODE, bool ALPT, bool XT = false>
hipError_t launch_step_boundary_x(const PassCtx<T> &x, C2<T> *Ck, const double *wS, const BoundaryX<T> &a) {
  if (XT && (!a.wpair || !a.wM || a.po == a.pi || a.qo == a.qi)) return hipErrorInvalidValue;
  return pass_dispatch<x_shape, T>(x.g.n, [&](auto nt, auto per) {
    return launch_dyn_lds(x.stream, k_step_boundary_x<T, nt, per, MODE, ALPT, XT>, x.col_grid(), nt, x.col_lds(), x.g,
                          x.log2n, x.tw, Ck, a.qi, a.pi, a.qo, a.po, wS, a.wM, a.a, a.b, a.half_eps, a.eps, a.c_za,
                          a.guard_slot, a.ctl, a.g_in, a.g_out, a.pair && !ALPT && MODE != BX_LAST,
                          a.vpair && !ALPT && MODE != BX_FIRST, a.wpair);
  });
}

// the two-tile formulation of the interior Zel'dovich boundary (no g_in / g_out)
template <typename T, bool XT = false>
hipError_t launch_step_boundary_x2(const PassCtx<T> &x, C2<T> *Ck, const double *wS, const BoundaryX<T> &a) {
  if (XT && (!a.wpair || !a.wM || a.po == a.pi || a.qo == a.qi)) return hipErrorInvalidValue;
  return pass_dispatch<x2_shape, T>(x.g.n, [&](auto nt, auto per) {
    return launch_dyn_lds(x.stream, k_step_boundary_x2<T, nt, per, XT>, x.col_grid(), nt, x.col_lds(2), x.g, x.log2n, x.tw,
                          Ck, a.qi, a.pi, a.qo, a.po, wS, a.wM, a.a, a.b, a.half_eps, a.eps, a.c_za, a.guard_slot, a.ctl,
                          a.pair, a.vpair, a.wpair);
  });
}

}  // namespace bchmc
#endif  // __HIPCC__
