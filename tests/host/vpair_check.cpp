// Stand-alone check, on the CPU, of what barcode_amd/csrc/pass_launch.hpp and eval_plan.hpp say about the forward side
// with V as records and two arrays into the forward x pass (tests/test_vpair_cpu.py builds it with g++ under
// AddressSanitizer / UndefinedBehaviorSanitizer and runs it): the launch shape of k_ypass_fwd_pair, and which evaluations
// leave V^_x | W (v_pair, eval_vpair) and gather V as records (v_rec).  Literals worked out by hand from the rules:
//     k_ypass_fwd_pair: k_ypass_pair's block, PER, grid (ypair_grid) and one tile of LDS (col_lds(.., 1));
//     v_pair: NO_VPAIR unset, a Zel'dovich boundary (never the ALPT one), planes mode (planes_ok, calc_h 2, mk 3, not
//         NO_PLANES), the tile-sorted standard-81 path with the one-pass binning (n = 256, or 128 with ZBIN_128; not
//         NO_ZBIN; not n = 512, where eval_yfwd keeps its measured choice), the y and z pass shapes; eval_vpair: an evaluation that wants V^ in planes space on such a handle;
//     v_rec: v_pair minus NO_VREC.
// Then the switch space is swept for the implications the engine relies on.
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

// masskernel 3, calc_h 2, Gaussian likelihood, k-space mass, one-pass binning, standard-81 hull, RSD
PathFacts facts(int n, int esz) {
  PathFacts f;
  f.n = n, f.esz = esz, f.Nhp = (long long)n * n * fft_row_stride(n, esz);
  f.planes_ok = f.tiled = f.sort_direct = f.std81 = true;
  f.rsd_model = 1;
  return f;
}
bool vp(const PathFacts &f, const PathSwitches &s) { return v_pair(f, s, traj_plan(f, s)); }
EvalMode interior() {
  EvalMode m;
  m.planes_c2r = m.planes_r2c = m.psi_unread = true;
  return m;
}

struct Row {
  int n, nt, per, grid;
  long long lds;
};

void literals() {
  // ---- launch shapes: those of k_ypass_pair (tests/host/two_array_check.cpp holds the same rows) ----
  const Row p64[] = {{128, 256, 4, 2304, 17408}, {256, 512, 4, 8704, 34816}, {512, 512, 8, 33792, 69632}};
  const Row p32[] = {{128, 256, 8, 1280, 16896}, {256, 512, 8, 4608, 33792}, {512, 512, 16, 17408, 67584}};
  for (int esz : {8, 4})
    for (const Row &r : esz == 8 ? p64 : p32) {
      const int nhp = fft_row_stride(r.n, esz);
      expect("k_ypass_fwd_pair NT", yfwd_pair_shape(esz, r.n).nt, r.nt);
      expect("k_ypass_fwd_pair PER", yfwd_pair_shape(esz, r.n).per, r.per);
      expect("k_ypass_fwd_pair grid", ypair_grid(esz, r.n, nhp), r.grid);
      expect("k_ypass_fwd_pair LDS", (long long)col_lds(esz, r.n, 1), r.lds);
      expect("k_ypass_fwd_pair NT is k_ypass_pair's", yfwd_pair_shape(esz, r.n).nt, ypair_shape(esz, r.n).nt);
      expect("k_ypass_fwd_pair PER is k_ypass_pair's", yfwd_pair_shape(esz, r.n).per, ypair_shape(esz, r.n).per);
      expect("k_ypass_fwd_pair tile is NT * PER elements", (long long)r.nt * r.per, (long long)r.n * pass_kb(esz));
    }
  for (int esz : {8, 4})
    for (int n : {16, 32, 48, 64, 1024}) expect("k_ypass_fwd_pair not available", yfwd_pair_shape(esz, n).nt, 0);

  // ---- the path decision ----
  const PathSwitches none;
  const EvalMode in = interior();
  for (int esz : {8, 4}) {
    expect("256^3 takes two arrays", vp(facts(256, esz), none), 1);
    expect("256^3 gathers records", v_rec(facts(256, esz), none), 1);
    expect("256^3: an interior evaluation", eval_vpair(facts(256, esz), none, in), 1);
    expect("256^3: an interior evaluation gathers records", eval_vrec(facts(256, esz), none, in), 1);
    expect("256^3: an evaluation on the 3-D plans", eval_vpair(facts(256, esz), none, EvalMode{}), 0);
    expect("256^3: an evaluation on the 3-D plans keeps the three arrays of V", eval_vrec(facts(256, esz), none, EvalMode{}), 0);
    expect("256^3: eval_yfwd stays off", eval_yfwd(facts(256, esz), none, in), 0);
    expect("512^3 keeps three: not measured there", vp(facts(512, esz), none), 0);
    expect("512^3 keeps the three arrays of V", v_rec(facts(512, esz), none), 0);
    expect("512^3: an interior evaluation", eval_vpair(facts(512, esz), none, in), 0);
    expect("512^3: eval_yfwd keeps its meaning", eval_yfwd(facts(512, esz), none, in), esz == 4);
    expect("128^3 keeps three", vp(facts(128, esz), none), 0);
    expect("128^3 keeps the three arrays of V", v_rec(facts(128, esz), none), 0);
    expect("64^3 keeps three", vp(facts(64, esz), none), 0);
    expect("32^3 keeps three", vp(facts(32, esz), none), 0);
    expect("32^3: an interior evaluation", eval_vpair(facts(32, esz), none, in), 0);
    PathSwitches z128, nvp, nvr, nplanes, nzbin, ends, both, npair;
    z128.zbin_128 = true, nvp.no_vpair = true, nvr.no_vrec = true, nplanes.no_planes = true, nzbin.no_zbin = true;
    ends.no_planes_ends = true, npair.no_pair = true;
    both.zbin_128 = both.no_vpair = true;
    expect("128^3 with ZBIN_128 takes two", vp(facts(128, esz), z128), 1);
    expect("128^3 with ZBIN_128 gathers records", v_rec(facts(128, esz), z128), 1);
    expect("128^3 with ZBIN_128 and NO_VPAIR keeps three", vp(facts(128, esz), both), 0);
    expect("64^3 with ZBIN_128 keeps three", vp(facts(64, esz), z128), 0);
    expect("NO_VPAIR keeps three", vp(facts(256, esz), nvp), 0);
    expect("NO_VPAIR keeps the three arrays of V", v_rec(facts(256, esz), nvp), 0);
    expect("NO_VPAIR: an interior evaluation", eval_vpair(facts(256, esz), nvp, in), 0);
    expect("NO_VREC takes two arrays", vp(facts(256, esz), nvr), 1);
    expect("NO_VREC keeps the three arrays of V", v_rec(facts(256, esz), nvr), 0);
    expect("NO_VREC: an interior evaluation takes two arrays", eval_vpair(facts(256, esz), nvr, in), 1);
    expect("NO_VREC: an interior evaluation keeps the three arrays of V", eval_vrec(facts(256, esz), nvr, in), 0);
    expect("NO_PLANES keeps three", vp(facts(256, esz), nplanes), 0);
    expect("NO_PLANES keeps the three arrays of V", v_rec(facts(256, esz), nplanes), 0);
    expect("NO_ZBIN keeps three", vp(facts(256, esz), nzbin), 0);
    expect("NO_PAIR is the inverse side's switch", vp(facts(256, esz), npair), 1);
    expect("NO_PLANES_ENDS: the interior evaluations still take two", vp(facts(256, esz), ends), 1);
    for (int calc_h : {0, 1, 3}) {
      PathFacts f = facts(256, esz);
      f.calc_h = calc_h;
      expect("calc_h != 2 keeps three", vp(f, none), 0);
      expect("calc_h != 2 keeps the three arrays of V", v_rec(f, none), 0);
    }
    for (int mk : {0, 1, 2}) {
      PathFacts f = facts(256, esz);
      f.mk = mk;
      expect("masskernel != 3 keeps three", vp(f, none), 0);
      expect("masskernel != 3 keeps the three arrays of V", v_rec(f, none), 0);
    }
    PathFacts fs = facts(256, esz), ft = facts(256, esz), fp = facts(256, esz), fh = facts(256, esz), fa = facts(256, esz);
    fs.sort_direct = false, ft.tiled = false, fp.planes_ok = false, fh.std81 = false;
    expect("the fallback sort from the start keeps three", vp(fs, none), 0);
    expect("no tiles keeps three", vp(ft, none), 0);
    expect("the 3-D plans keep three", vp(fp, none), 0);
    expect("the general hull keeps three", vp(fh, none), 0);
    expect("the general hull keeps the three arrays of V", v_rec(fh, none), 0);
    fa.rsd_model = 0, fa.sfmodel = 2, fa.alpt_plans = true;
    expect("ALPT on the 2-D plans keeps three", traj_plan(fa, none).alpt_x * 2 + vp(fa, none), 2);
    expect("ALPT on the 2-D plans: an interior evaluation", eval_vpair(fa, none, in), 0);
  }
}

PathSwitches switches(int bits) {
  PathSwitches s;
  s.no_planes = bits & 1, s.no_planes_ends = bits & 2, s.no_fuse = bits & 4, s.no_alpt_planes = bits & 8;
  s.no_zbin = bits & 16, s.zbin_128 = bits & 32, s.yfwd_f64 = bits & 64;  // NO_PAIR, BX_V1, BX_V2: not read on this side
  s.no_vpair = bits & 128, s.no_vrec = bits & 256;
  return s;
}

void fail_at(const char *what, const PathFacts &f, int bits) {
  if (g_failures++ < 40)
    std::printf("FAIL invariant \"%s\" at n %d esz %d mk %d calc_h %d likelihood %d sfmodel %d rsd %d mass_rs %d tiled %d "
                "sort_direct %d planes_ok %d alpt_plans %d std81 %d switches %d\n", what, f.n, f.esz, f.mk, f.calc_h,
                f.likelihood, f.sfmodel, f.rsd_model, f.mass_rs, f.tiled, f.sort_direct, f.planes_ok, f.alpt_plans, f.std81,
                bits);
}

unsigned long long check_point(const PathFacts f, int bits) {
  unsigned long long checked = 0;
#define hold(what, ok) do { checked++; if (!(ok)) fail_at(what, f, bits); } while (0)
  const PathSwitches s = switches(bits);
  const TrajPlan tp = traj_plan(f, s);
  const bool pr = v_pair(f, s, tp), rec = v_rec(f, s);
  hold("v_rec => v_pair", !rec || pr);
  hold("NO_VPAIR means three arrays", !s.no_vpair || !pr);
  hold("NO_VREC means the three arrays of V", !s.no_vrec || !rec);
  hold("v_pair => !alpt_x", !pr || !tp.alpt_x);
  hold("v_pair => planes mode", !pr || planes_on(f, s));
  hold("v_pair => the y and z pass shapes exist",
       !pr || (y_shape(f.esz, f.n).nt && z_shape(f.esz, f.n).nt && yfwd_pair_shape(f.esz, f.n).nt));
  hold("v_pair => the standard-81 tile path with records", !pr || (f.tiled && f.std81 && f.sort_direct));
  hold("v_pair at 256 only, or 128 when asked", !pr || f.n == 256 || (f.n == 128 && s.zbin_128));
  for (int r2c = 0; r2c < 2; r2c++) {
    EvalMode m;
    m.planes_r2c = r2c;
    hold("never eval_vpair and eval_yfwd at once", !(eval_vpair(f, s, m) && eval_yfwd(f, s, m)));
  }
  hold("v_pair => calc_h 2 and mk 3", !pr || (f.calc_h == 2 && f.mk == 3));
  for (int mode = 0; mode < 4; mode++) {  // alpt_pending and psi_unread are not read by these predicates
    EvalMode m;
    m.planes_c2r = mode & 1, m.planes_r2c = mode & 2, m.alpt_pending = tp.alpt_x, m.psi_unread = mode & 1;
    hold("eval_vpair => planes_r2c", !eval_vpair(f, s, m) || m.planes_r2c);
    hold("eval_vpair => v_pair", !eval_vpair(f, s, m) || pr);
    hold("eval_vrec => eval_vpair and v_rec", !eval_vrec(f, s, m) || (eval_vpair(f, s, m) && rec));
    hold("eval_vpair is v_pair of an evaluation with planes_r2c", eval_vpair(f, s, m) == (m.planes_r2c && pr));
    hold("eval_yfwd keeps its meaning", eval_yfwd(f, s, m) == (m.planes_r2c && yfwd_ok(f, s)));
  }
  // every evaluation of a fused trajectory that leaves two arrays is closed by a Zel'dovich boundary in planes space
  if (pr && tp.fused)
    for (unsigned long long neps = 1; neps <= 4; neps++)
      for (unsigned long long step = 0; step < neps; step++) {
        if (!eval_vpair(f, s, step_mode(f, s, tp, step, neps))) continue;
        const Closing c = closing(f, s, tp, step, neps, 0);
        hold("two arrays are read by a Zel'dovich k_step_boundary_x",
             c == Closing::kBxLast || c == Closing::kBxInterior || c == Closing::kBxInteriorTwoTile);
      }
  return checked;
#undef hold
}

unsigned long long sweep() {
  unsigned long long checked = 0;
  for (int n : {32, 48, 128, 256, 512, 1024})
    for (int esz : {4, 8})
      for (int cfg = 0; cfg < 4 * 4 * 2 * 2 * 2 * 2; cfg++)
        for (int have = 0; have < 32; have++) {
          PathFacts f;
          f.n = n, f.esz = esz, f.Nhp = (long long)n * n * fft_row_stride(n, esz);
          f.mk = cfg & 3, f.calc_h = (cfg >> 2) & 3, f.likelihood = ((cfg >> 4) & 1) ? 3 : 1, f.sfmodel = 1 + ((cfg >> 5) & 1);
          f.rsd_model = (cfg >> 6) & 1, f.mass_rs = (cfg >> 7) & 1;
          f.tiled = have & 1, f.sort_direct = have & 2, f.planes_ok = have & 4, f.alpt_plans = have & 8, f.std81 = have & 16;
          for (int bits = 0; bits < 512; bits++) checked += check_point(f, bits);
        }
  return checked;
}

}  // namespace

int main() {
  unsetenv("BCHMC_FFT_PAD");  // fft_row_stride's test switch: the literals are for the engine's default padding
  literals();
  const unsigned long long checked = sweep();
  if (g_failures) {
    std::printf("vpair_check: %d failures\n", g_failures);
    return 1;
  }
  std::printf("vpair_check: ok (%llu invariants held)\n", checked);
  return 0;
}
