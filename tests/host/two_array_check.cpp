// Stand-alone check, on the CPU, of what barcode_amd/csrc/pass_launch.hpp and eval_plan.hpp say about the two-array
// inverse side (tests/test_two_array_cpu.py builds it with g++ under AddressSanitizer / UndefinedBehaviorSanitizer and
// runs it): the launch shape of k_ypass_pair, and which boundary kernels leave Psi^_x | B instead of the three Psi^
// components (psi_pair).  Literals worked out by hand from the rules:
//     k_ypass_pair: k_ypass's block and PER (n = 128 -> 256 threads, 256 and 512 -> 512 threads, PER = n KB / NT), one
//         tile of LDS, a grid of TWO components' column tiles (the workgroups of B make two transforms);
//     psi_pair: NO_PAIR unset, a Zel'dovich boundary (never the ALPT one), planes mode (planes_ok, calc_h 2, mk 3, not
//         NO_PLANES) and the engine's own y pass after it (NO_ZBIN unset, n = 256, 512 or 128 with ZBIN_128, tiles with
//         the one-pass binning).
// Then the whole space is swept: wherever a boundary kernel leaves two arrays, the evaluation that reads Ck next runs the
// engine's own y pass, which has a k_ypass_pair for that n.
#include <cstdio>
#include <cstdlib>

#include "../../barcode_amd/csrc/eval_plan.hpp"
#include "../../barcode_amd/csrc/fft_host.hpp"

using namespace bchmc;

namespace {

int g_failures = 0;

void expect(const char *what, long long got, long long want) {
  if (got != want && g_failures++ < 40) std::printf("FAIL %s: %lld, expected %lld\n", what, got, want);
}

PathFacts facts(int n, int esz) {  // masskernel 3, calc_h 2, Gaussian likelihood, k-space mass, one-pass binning, RSD
  PathFacts f;
  f.n = n, f.esz = esz, f.Nhp = (long long)n * n * fft_row_stride(n, esz);
  f.planes_ok = f.tiled = f.sort_direct = true;
  f.rsd_model = 1;
  return f;
}
bool pair(const PathFacts &f, const PathSwitches &s) { return psi_pair(f, s, traj_plan(f, s)); }

struct Row {
  int n, nt, per, grid;
  long long lds;
};

void literals() {
  // ---- launch shapes ----
  const Row p64[] = {{128, 256, 4, 2304, 17408}, {256, 512, 4, 8704, 34816}, {512, 512, 8, 33792, 69632}};
  const Row p32[] = {{128, 256, 8, 1280, 16896}, {256, 512, 8, 4608, 33792}, {512, 512, 16, 17408, 67584}};
  for (int esz : {8, 4})
    for (const Row &r : esz == 8 ? p64 : p32) {
      expect("k_ypass_pair NT", ypair_shape(esz, r.n).nt, r.nt);
      expect("k_ypass_pair PER", ypair_shape(esz, r.n).per, r.per);
      expect("k_ypass_pair grid", ypair_grid(esz, r.n, fft_row_stride(r.n, esz)), r.grid);
      expect("k_ypass_pair LDS", (long long)col_lds(esz, r.n), r.lds);
      expect("k_ypass_pair grid is two thirds of k_ypass's", 3 * ypair_grid(esz, r.n, fft_row_stride(r.n, esz)),
             2 * col_grid(esz, r.n, fft_row_stride(r.n, esz), 3));
    }
  for (int esz : {8, 4})
    for (int n : {16, 32, 48, 64, 1024}) expect("k_ypass_pair not available", ypair_shape(esz, n).nt, 0);

  // ---- the path decision ----
  const PathSwitches none;
  for (int esz : {8, 4}) {
    expect("256^3 takes two arrays", pair(facts(256, esz), none), 1);
    expect("512^3 takes two arrays", pair(facts(512, esz), none), 1);
    expect("128^3 keeps three", pair(facts(128, esz), none), 0);
    expect("64^3 keeps three", pair(facts(64, esz), none), 0);
    expect("32^3 keeps three", pair(facts(32, esz), none), 0);
    PathSwitches z128, np, nplanes, nzbin, ends, both;
    z128.zbin_128 = true, np.no_pair = true, nplanes.no_planes = true, nzbin.no_zbin = true, ends.no_planes_ends = true;
    both.zbin_128 = both.no_pair = true;
    expect("128^3 with ZBIN_128 takes two", pair(facts(128, esz), z128), 1);
    expect("128^3 with ZBIN_128 and NO_PAIR keeps three", pair(facts(128, esz), both), 0);
    expect("64^3 with ZBIN_128 keeps three", pair(facts(64, esz), z128), 0);
    expect("NO_PAIR keeps three", pair(facts(256, esz), np), 0);
    expect("NO_PLANES keeps three", pair(facts(256, esz), nplanes), 0);
    expect("NO_ZBIN keeps three", pair(facts(256, esz), nzbin), 0);
    expect("NO_PLANES_ENDS: the interior boundaries still take two", pair(facts(256, esz), ends), 1);
    for (int calc_h : {0, 1, 3}) {
      PathFacts f = facts(256, esz);
      f.calc_h = calc_h;
      expect("calc_h != 2 keeps three", pair(f, none), 0);
    }
    for (int mk : {0, 1, 2}) {
      PathFacts f = facts(256, esz);
      f.mk = mk;
      expect("masskernel != 3 keeps three", pair(f, none), 0);
    }
    PathFacts fs = facts(256, esz), ft = facts(256, esz), fp = facts(256, esz), fa = facts(256, esz);
    fs.sort_direct = false, ft.tiled = false, fp.planes_ok = false;
    expect("the fallback sort keeps three", pair(fs, none), 0);
    expect("no tiles keeps three", pair(ft, none), 0);
    expect("the 3-D plans keep three", pair(fp, none), 0);
    fa.rsd_model = 0, fa.sfmodel = 2, fa.alpt_plans = true;
    expect("ALPT on the 2-D plans: its boundary's two arrays are other fields", traj_plan(fa, none).alpt_x * 2 + pair(fa, none), 2);
  }
}

PathSwitches switches(int bits) {
  PathSwitches s;
  s.no_planes = bits & 1, s.no_planes_ends = bits & 2, s.no_fuse = bits & 4, s.no_alpt_planes = bits & 8;
  s.no_zbin = bits & 16, s.zbin_128 = bits & 32, s.yfwd_f64 = bits & 64, s.bx_v1 = bits & 128, s.bx_v2 = bits & 256;
  s.no_pair = bits & 512;
  return s;
}

void fail_at(const char *what, const PathFacts &f, int bits) {
  if (g_failures++ < 40)
    std::printf("FAIL invariant \"%s\" at n %d esz %d mk %d calc_h %d likelihood %d sfmodel %d rsd %d mass_rs %d tiled %d "
                "sort_direct %d planes_ok %d alpt_plans %d switches %d\n", what, f.n, f.esz, f.mk, f.calc_h, f.likelihood,
                f.sfmodel, f.rsd_model, f.mass_rs, f.tiled, f.sort_direct, f.planes_ok, f.alpt_plans, bits);
}

unsigned long long check_point(const PathFacts f, int bits) {
  unsigned long long checked = 0;
#define hold(what, ok) do { checked++; if (!(ok)) fail_at(what, f, bits); } while (0)
  const PathSwitches s = switches(bits);
  const TrajPlan tp = traj_plan(f, s);
  const bool pr = psi_pair(f, s, tp);
  hold("NO_PAIR means three arrays", !s.no_pair || !pr);
  hold("two arrays need the engine's own y pass", !pr || zbin_ok(f, s));
  hold("two arrays need planes mode", !pr || planes_on(f, s));
  hold("two arrays need the rows of k_ypass_pair and k_zbin_direct", !pr || (ypair_shape(f.esz, f.n).nt && z_shape(f.esz, f.n).nt));
  hold("two arrays at 256 and 512 only, or 128 when asked", !pr || f.n == 256 || f.n == 512 || (f.n == 128 && s.zbin_128));
  hold("never the ALPT boundary", !pr || !tp.alpt_x);
  hold("the default path takes them wherever the y pass runs", pr || s.no_pair || tp.alpt_x || !planes_on(f, s) || !zbin_ok(f, s));
  if (!pr || !tp.fused) return checked;
  // every Zel'dovich boundary of a fused trajectory that writes Psi^ is followed by an evaluation with the y pass
  if (initial_eval(f, s, tp) == InitialEval::kBxFirst) {
    EvalMode m;
    m.planes_c2r = m.planes_r2c = true;
    hold("the force evaluation before the first step reads two arrays with the y pass", eval_zbin(f, s, m));
  }
  for (unsigned long long neps = 1; neps <= 4; neps++) {
    if (opening(f, s, tp) == Opening::kBxFirst)
      hold("step 0 reads the opening's two arrays with the y pass", eval_zbin(f, s, step_mode(f, s, tp, 0, neps)));
    for (unsigned long long step = 0; step + 1 < neps; step++) {
      const Closing c = closing(f, s, tp, step, neps, 0);
      if (c == Closing::kBxInterior || c == Closing::kBxInteriorTwoTile)
        hold("the next step reads an interior boundary's two arrays with the y pass",
             eval_zbin(f, s, step_mode(f, s, tp, step + 1, neps)));
    }
  }
  return checked;
#undef hold
}

unsigned long long sweep() {
  unsigned long long checked = 0;
  for (int n : {16, 32, 48, 64, 128, 256, 512, 1024})
    for (int esz : {4, 8})
      for (int cfg = 0; cfg < 4 * 4 * 4 * 2 * 2 * 2; cfg++)
        for (int have = 0; have < 16; have++) {
          PathFacts f;
          f.n = n, f.esz = esz, f.Nhp = (long long)n * n * fft_row_stride(n, esz);
          f.mk = cfg & 3, f.calc_h = (cfg >> 2) & 3, f.likelihood = (cfg >> 4) & 3, f.sfmodel = 1 + ((cfg >> 6) & 1);
          f.rsd_model = (cfg >> 7) & 1, f.mass_rs = (cfg >> 8) & 1;
          f.tiled = have & 1, f.sort_direct = have & 2, f.planes_ok = have & 4, f.alpt_plans = have & 8;
          for (int bits = 0; bits < 1024; bits++) checked += check_point(f, bits);
        }
  return checked;
}

}  // namespace

int main() {
  unsetenv("BCHMC_FFT_PAD");  // fft_row_stride's test switch: the literals are for the engine's default padding
  literals();
  const unsigned long long checked = sweep();
  if (g_failures) {
    std::printf("two_array_check: %d failures\n", g_failures);
    return 1;
  }
  std::printf("two_array_check: ok (%llu invariants held)\n", checked);
  return 0;
}
