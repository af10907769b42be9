// Stand-alone check, on the CPU, of barcode_amd/csrc/xtile.hpp (tests/test_xtile_cpu.py builds it with g++ under
// AddressSanitizer / UndefinedBehaviorSanitizer and runs it): the x-column tile layout of a fused trajectory's k-space
// state and weights.
//     The permutation, for n = 32 .. 512 in both precisions with the row strides the engine and the probe use (whole
//     128-byte lines: the engine pads from n = 128 on, the probe's small grids run under BCHMC_FFT_PAD=1): xtile_index is a
//     bijection on [0, Nhp), xtile_inverse inverts it, xtile_of is the same function of the natural linear index, every tile
//     t = j (nhp / KB) + k0 / KB is the contiguous run [t n KB, (t + 1) n KB) in row order, and a few elements worked out by
//     hand.
//     Where it is on (x_tiles), against literals.
//     The bookkeeping (XPairs), swept over the switches, the facts and 1 .. 4 steps: with the layout on, the opening is
//     BX_FIRST, every boundary has a tiled instantiation, reads the pair the previous one wrote and finds it tiled; a 3-D
//     boundary is refused; after the closing pass the result pair is natural and nothing tiled is left.  With the layout
//     off, the same walk is the parent's: in place, pair s % 2, result where the last boundary read.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../barcode_amd/csrc/fft_host.hpp"
#include "../../barcode_amd/csrc/xtile.hpp"

using namespace bchmc;

namespace {

int g_failures = 0;

void expect(const char *what, long long got, long long want) {
  if (got != want && g_failures++ < 40) std::printf("FAIL %s: %lld, expected %lld\n", what, got, want);
}

int stride(int n, int esz) {  // whole k-groups: the engine's own padding from 128 on, forced below (the probe's tests)
  if (n < 128) setenv("BCHMC_FFT_PAD", "1", 1);
  else unsetenv("BCHMC_FFT_PAD");
  const int s = fft_row_stride(n, esz);
  unsetenv("BCHMC_FFT_PAD");
  return s;
}

unsigned long long permutation() {
  unsigned long long checked = 0;
  for (int n : {32, 64, 128, 256, 512})
    for (int esz : {4, 8}) {
      const int kb = pass_kb(esz), nhp = stride(n, esz), ntk = nhp / kb;
      expect("rows are whole k-groups", nhp % kb, 0);
      expect("rows hold n / 2 + 1 elements", nhp >= n / 2 + 1 && nhp < n / 2 + 1 + kb, 1);
      const long long Nhp = (long long)n * n * nhp;
      std::vector<bool> hit((size_t)Nhp, false);
      long long bad = 0;
      for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++)
          for (int k = 0; k < nhp; k++) {
            const long long idx = ((long long)i * n + j) * nhp + k, e = xtile_index(n, nhp, kb, i, j, k);
            if (e < 0 || e >= Nhp || hit[(size_t)e]) {
              bad++;
              continue;
            }
            hit[(size_t)e] = true;
            const long long t = (long long)j * ntk + k / kb;
            bad += xtile_inverse(n, nhp, kb, e) != idx;
            bad += xtile_of(n, nhp, kb, idx) != e;
            bad += e != t * n * kb + (long long)i * kb + k % kb;  // the tile's run, rows in order, lanes in order
            bad += e / ((long long)n * kb) != t;
            checked += 4;
          }
      expect("bijection, inverse, tile runs", bad, 0);
      for (long long e = 0; e < Nhp; e += 4097) {  // ... and the inverse on its own domain
        const long long idx = xtile_inverse(n, nhp, kb, e);
        expect("inverse lands inside", idx >= 0 && idx < Nhp, 1);
        expect("index of inverse", xtile_of(n, nhp, kb, idx), e);
      }
    }
  // by hand.  256^3 fp64: KB 8, rows of 136, 17 tiles per j; (3, 5, 20) is lane 4 of row 3 of tile 5 * 17 + 2 = 87
  expect("stride 256 fp64", stride(256, 8), 136);
  expect("256 fp64 (3, 5, 20)", xtile_index(256, 136, 8, 3, 5, 20), (87LL * 256 + 3) * 8 + 4);
  expect("256 fp64 (3, 5, 20) literal", xtile_index(256, 136, 8, 3, 5, 20), 178204);
  expect("256 fp64 inverse", xtile_inverse(256, 136, 8, 178204), 105148);
  // 128^3 fp32: KB 16, rows of 80, 5 tiles per j; the last element stays the last
  expect("stride 128 fp32", stride(128, 4), 80);
  expect("128 fp32 last", xtile_index(128, 80, 16, 127, 127, 79), 1310719);
  // 32^3 fp64 (padded rows of 24, 3 tiles per j): one step along each axis from the origin
  expect("stride 32 fp64", stride(32, 8), 24);
  expect("32 fp64 (1, 0, 0): the next row of tile 0", xtile_index(32, 24, 8, 1, 0, 0), 8);
  expect("32 fp64 (0, 0, 7): the last lane of row 0", xtile_index(32, 24, 8, 0, 0, 7), 7);
  expect("32 fp64 (0, 0, 8): tile 1", xtile_index(32, 24, 8, 0, 0, 8), 256);
  expect("32 fp64 (0, 1, 0): tile 3", xtile_index(32, 24, 8, 0, 1, 0), 768);
  // 512^3 fp64: rows of 264, 33 tiles per j; a padding column: lane 7 of row 0 of tile 2 * 33 + 32 = 98
  expect("stride 512 fp64", stride(512, 8), 264);
  expect("512 fp64 (0, 2, 263)", xtile_index(512, 264, 8, 0, 2, 263), 401415);
  return checked;
}

PathFacts facts(int n, int esz) {  // the benchmark's: masskernel 3, calc_h 2, Gaussian likelihood, k-space mass, RSD
  PathFacts f;
  f.n = n, f.esz = esz, f.Nhp = (long long)n * n * stride(n, esz);
  f.planes_ok = f.tiled = f.sort_direct = f.std81 = f.mass_fs = true;
  f.rsd_model = 1;
  return f;
}
bool on(const PathFacts &f, const PathSwitches &s) { return x_tiles(f, s, traj_plan(f, s)); }

void decision() {
  const PathSwitches none;
  for (int esz : {8, 4}) {
    expect("256^3 is tiled", on(facts(256, esz), none), 1);
    expect("128^3 is tiled", on(facts(128, esz), none), 1);
    expect("512^3 is not", on(facts(512, esz), none), 0);
    expect("64^3 is not", on(facts(64, esz), none), 0);
    expect("32^3 is not", on(facts(32, esz), none), 0);
    PathSwitches nx, np, ne, nf, v2, v1;
    nx.no_xtile = true, np.no_planes = true, ne.no_planes_ends = true, nf.no_fuse = true, v2.bx_v2 = true, v1.bx_v1 = true;
    expect("NO_XTILE", on(facts(256, esz), nx), 0);
    expect("NO_PLANES", on(facts(256, esz), np), 0);
    expect("NO_PLANES_ENDS: the opening would not convert", on(facts(256, esz), ne), 0);
    expect("NO_FUSE", on(facts(256, esz), nf), 0);
    expect("BX_V2 keeps it", on(facts(256, esz), v2), 1);
    expect("BX_V1 keeps it", on(facts(256, esz), v1), 1);
    PathFacts fm = facts(256, esz), fr = facts(256, esz), fa = facts(256, esz), fl = facts(256, esz), fp = facts(256, esz);
    fm.mass_fs = false, fr.mass_rs = true, fl.likelihood = 3, fp.planes_ok = false;
    fa.rsd_model = 0, fa.sfmodel = 2, fa.alpt_plans = true;
    expect("no k-space mass: no wM for the pair", on(fm, none), 0);
    expect("a real-space mass: not the fused trajectory", on(fr, none), 0);
    expect("likelihood 3: not the fused trajectory", on(fl, none), 0);
    expect("the 3-D plans", on(fp, none), 0);
    expect("ALPT", on(fa, none), 0);
  }
}

PathSwitches switches(int bits) {
  PathSwitches s;
  s.no_planes = bits & 1, s.no_planes_ends = bits & 2, s.no_fuse = bits & 4, s.no_alpt_planes = bits & 8;
  s.no_zbin = bits & 16, s.zbin_128 = bits & 32, s.yfwd_f64 = bits & 64, s.bx_v1 = bits & 128, s.bx_v2 = bits & 256;
  s.no_pair = bits & 512, s.no_vpair = bits & 1024, s.no_vrec = bits & 2048, s.no_xtile = bits & 4096;
  return s;
}
constexpr int kSwitchSettings = 8192;

void fail_at(const char *what, const PathFacts &f, int bits, unsigned long long neps) {
  if (g_failures++ < 40)
    std::printf("FAIL invariant \"%s\" at n %d esz %d mk %d calc_h %d likelihood %d sfmodel %d rsd %d mass_rs %d mass_fs %d "
                "tiled %d planes_ok %d alpt_plans %d switches %d neps %llu\n", what, f.n, f.esz, f.mk, f.calc_h, f.likelihood,
                f.sfmodel, f.rsd_model, f.mass_rs, f.mass_fs, f.tiled, f.planes_ok, f.alpt_plans, bits, neps);
}

unsigned long long check_point(const PathFacts &f, int bits) {
  unsigned long long checked = 0, neps = 0;
#define hold(what, ok) do { checked++; if (!(ok)) fail_at(what, f, bits, neps); } while (0)
  const PathSwitches s = switches(bits);
  const TrajPlan tp = traj_plan(f, s);
  const bool xt = x_tiles(f, s, tp);
  hold("NO_XTILE means natural", !s.no_xtile || !xt);
  hold("tiled at 128 and 256 only", !xt || f.n == 128 || f.n == 256);
  hold("tiled needs the fused Zel'dovich trajectory in planes mode with a k-space mass",
       !xt || (tp.fused && tp.fused_za && !tp.alpt_x && planes_at_ends(f, s) && f.mass_fs && !f.mass_rs));
  hold("tiled needs the rows of the x pass", !xt || x_shape(f.esz, f.n).nt);
  if (!tp.fused) return checked;
  const Opening op = opening(f, s, tp);
  hold("a tiled trajectory opens with BX_FIRST", !xt || op == Opening::kBxFirst);
  for (neps = 1; neps <= 4; neps++) {
    XPairs xp;
    XLayout mine[2] = {XLayout::kNatural, XLayout::kDead};  // the same walk, followed here from what the kernels do
    hold("the opening finds pair 0 natural", xp.open(xt, op == Opening::kBxFirst));
    hold("the opening writes pair 1 tiled, or pair 0 in place", xp.cur == (xt ? 1 : 0));
    mine[xp.cur] = xt ? XLayout::kTiled : XLayout::kNatural;
    for (unsigned long long step = 0; step < neps; step++) {
      const bool last = step + 1 == neps;
      const Closing c = closing(f, s, tp, step, neps, 0);
      hold("every boundary of a tiled trajectory has a tiled instantiation", !xt || closing_is_x(c));
      const int src = xp.cur, dst = xp.dst(xt, last);
      hold("boundary s reads pair (s + xt) % 2", src == (int)((step + (xt ? 1 : 0)) % 2));
      hold("a tiled boundary never writes the pair it reads", !xt || dst != src);
      hold("the last boundary of the natural layout writes in place", xt || !last || dst == src);
      hold("the boundary reads what the one before wrote",
           mine[src] == (xt ? XLayout::kTiled : XLayout::kNatural) && xp.q[src] == mine[src] && xp.p[src] == mine[src]);
      if (xt) {  // a 3-D boundary (the likelihood's V is not three components) is refused, not run
        XPairs bad = xp;
        hold("a 3-D boundary on a tiled pair is refused", !bad.close(xt, last ? Closing::kStepBoundaryLast : Closing::kStepBoundary, last));
      }
      hold("the boundary is accepted", xp.close(xt, c, last));
      if (!last) mine[dst] = mine[src];
      hold("the pairs flip but after the last step", xp.cur == (last ? src : src ^ 1));
    }
    const int fin = xp.cur, res = xp.result(xt);
    hold("the closing pass is accepted", xp.finish(xt));
    hold("tiled: the result is in the pair the last boundary did not read", res == (xt ? fin ^ 1 : fin));
    hold("the result is natural", xp.q[res] == XLayout::kNatural && xp.p[res] == XLayout::kNatural);
    hold("nothing tiled is left", xp.q[0] != XLayout::kTiled && xp.q[1] != XLayout::kTiled && xp.p[0] != XLayout::kTiled &&
                                      xp.p[1] != XLayout::kTiled);
  }
  return checked;
#undef hold
}

unsigned long long sweep() {
  unsigned long long checked = 0;
  for (int n : {32, 64, 128, 256, 512})
    for (int esz : {4, 8})
      for (int cfg = 0; cfg < 128; cfg++)
        for (int have = 0; have < 8; have++) {
          PathFacts f;
          f.n = n, f.esz = esz, f.Nhp = (long long)n * n * stride(n, esz);
          f.mk = 2 + (cfg & 1), f.calc_h = 2 + ((cfg >> 1) & 1), f.likelihood = (cfg >> 2) & 1 ? 3 : 1;
          f.sfmodel = 1 + ((cfg >> 3) & 1), f.rsd_model = (cfg >> 4) & 1, f.mass_rs = (cfg >> 5) & 1, f.mass_fs = (cfg >> 6) & 1;
          f.tiled = f.sort_direct = f.std81 = have & 1, f.planes_ok = have & 2, f.alpt_plans = have & 4;
          for (int bits = 0; bits < kSwitchSettings; bits++) checked += check_point(f, bits);
        }
  return checked;
}

}  // namespace

int main() {
  unsigned long long checked = permutation();
  decision();
  checked += sweep();
  if (g_failures) {
    std::printf("xtile_check: %d failures\n", g_failures);
    return 1;
  }
  std::printf("xtile_check: ok (%llu checks held)\n", checked);
  return 0;
}
