// xtile.hpp -- the x-column tile layout of a fused trajectory's k-space state and weights: the single statement of it.
//
// A workgroup of the x pass (k_step_boundary_x, k_step_boundary_x2) owns column tile t = j (nhp / KB) + k0 / KB: the n rows
// of the KB = pass_kb(esz) complex elements k0 .. k0 + KB - 1 at one j.  In the natural (padded half-complex) layout the rows
// of a tile are 128-byte segments one plane apart; in the tiled layout element (i, j, k) of a component lives at
//   (t n + i) KB + k % KB,
// so that a tile is one contiguous run of n KB elements (32 KB at 256^3 fp64).  A permutation of the Nhp elements, padding
// columns included: array sizes do not change.  Only arrays that no transform reads may hold it: the ping-pong pairs
// (q^, p^) between the opening and the closing boundary of trajectory_fused, and the weight pair {wS, wM}.  Ck, gk and
// everything outside a trajectory stay natural.
//
// Three things: the index function, its inverse, and where the layout is on (x_tiles) with the bookkeeping of which pair
// holds which layout (XPairs), which bchmc.hip drives launch by launch and refuses to violate.  Plain C++: no HIP types, no
// getenv; tests/host/xtile_check.cpp proves the permutation against literals and sweeps the switches for the invariant.
#pragma once

#include "eval_plan.hpp"

#ifdef __HIPCC__
#define BCHMC_XTILE_FN __host__ __device__
#else
#define BCHMC_XTILE_FN
#endif

namespace bchmc {

// ---- the permutation ---------------------------------------------------------------------------------------------------
// n rows, row stride nhp (a multiple of kb), kb elements per row of a tile
BCHMC_XTILE_FN constexpr long long xtile_index(int n, int nhp, int kb, int i, int j, int k) {
  const long long t = (long long)j * (nhp / kb) + k / kb;
  return (t * n + i) * kb + k % kb;
}
// natural linear index (i n + j) nhp + k -> tiled index
BCHMC_XTILE_FN constexpr long long xtile_of(int n, int nhp, int kb, long long idx) {
  const int k = (int)(idx % nhp);
  const long long ij = idx / nhp;
  return xtile_index(n, nhp, kb, (int)(ij / n), (int)(ij % n), k);
}
// tiled index -> natural linear index
BCHMC_XTILE_FN constexpr long long xtile_inverse(int n, int nhp, int kb, long long e) {
  const int c = (int)(e % kb);
  const long long r = e / kb;
  const int i = (int)(r % n);
  const long long t = r / n;
  const int ntk = nhp / kb;
  const int j = (int)(t / ntk), k = (int)(t % ntk) * kb + c;
  return ((long long)i * n + j) * nhp + k;
}

// ---- where it is on ----------------------------------------------------------------------------------------------------
// Planes mode at the ends too (the opening is BX_FIRST and the closing BX_LAST: they convert), the fused Zel'dovich
// trajectory, a k-space mass (wM exists: the pair has both weights), n = 128 and 256.  n = 512 is not measured; ALPT's
// boundary shares the kernel but has no tiled instantiation.  BCHMC_NO_XTILE=1: the natural layout everywhere.
constexpr bool x_tiles(const PathFacts &f, const PathSwitches &s, const TrajPlan &tp) {
  return !s.no_xtile && planes_at_ends(f, s) && tp.fused && tp.fused_za && !tp.alpt_x && f.mass_fs &&
         (f.n == 128 || f.n == 256);
}

// ---- which pair holds which layout ---------------------------------------------------------------------------------------
// The two ping-pong pairs of trajectory_fused: pair 0 is (qk, pk) as the caller left it, pair 1 the private one.
//   natural layout throughout (xt = false): the opening updates pair 0 in place, boundary s reads pair s % 2 and writes the
//     other, the last boundary writes p in place, k_rollback leaves the result in the pair the last boundary read;
//   tiled (xt = true): no launch may write a buffer in one layout while other workgroups of it read it in the other, so the
//     opening reads pair 0 natural and writes pair 1 tiled, boundary s reads pair (s + 1) % 2 and writes the other (both
//     tiled), the last boundary reads its pair tiled and writes p natural into the OTHER pair, and the closing pass
//     (k_xtile_finish) un-tiles the final q there as well: the result is natural in the pair the last boundary did not read,
//     and what is left in the one it read is dead.
// kDead: nobody may read it.  Every method returns false where a kernel would read a pair in a layout it does not hold.
enum class XLayout : unsigned char { kNatural, kTiled, kDead };

constexpr bool closing_is_x(Closing c) {  // the boundaries that have a tiled instantiation
  return c == Closing::kBxLast || c == Closing::kBxInterior || c == Closing::kBxInteriorTwoTile;
}

struct XPairs {
  XLayout q[2] = {XLayout::kNatural, XLayout::kDead}, p[2] = {XLayout::kNatural, XLayout::kDead};
  int cur = 0;  // the pair the next boundary reads

  // the opening (BX_FIRST with g_in, or k_kick_drift_za) reads pair 0 natural; returns the pair it writes
  constexpr bool open(bool xt, bool opening_is_bx_first) {
    if (q[0] != XLayout::kNatural || p[0] != XLayout::kNatural) return false;
    if (xt && !opening_is_bx_first) return false;  // k_kick_drift_za has no tiled form
    cur = xt ? 1 : 0;
    q[cur] = p[cur] = xt ? XLayout::kTiled : XLayout::kNatural;
    return true;
  }
  // the pair boundary `c` writes p (and, interior, q) to
  constexpr int dst(bool xt, bool last) const { return last && !xt ? cur : cur ^ 1; }
  // boundary `c` of a step; last: the one after the final step
  constexpr bool close(bool xt, Closing c, bool last) {
    const XLayout want = xt && closing_is_x(c) ? XLayout::kTiled : XLayout::kNatural;
    if (xt && !closing_is_x(c)) return false;  // a 3-D boundary would read a tiled pair as natural
    if (q[cur] != want || p[cur] != want) return false;
    const int d = dst(xt, last);
    if (last) {
      p[d] = XLayout::kNatural;  // BX_LAST writes p natural, no q
    } else {
      q[d] = p[d] = want;
      cur ^= 1;
    }
    return true;
  }
  // the pair that holds the result after the closing pass (k_rollback / k_xtile_finish)
  constexpr int result(bool xt) const { return xt ? cur ^ 1 : cur; }
  constexpr bool finish(bool xt) {
    const int r = result(xt);
    if (xt) {
      if (q[cur] != XLayout::kTiled) return false;  // the closing pass reads the final q tiled
      q[r] = XLayout::kNatural;
      q[cur] = p[cur] = XLayout::kDead;
    } else {
      q[r ^ 1] = p[r ^ 1] = XLayout::kDead;
    }
    return q[r] == XLayout::kNatural && p[r] == XLayout::kNatural;
  }
};

}  // namespace bchmc
