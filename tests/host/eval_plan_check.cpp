// Stand-alone check of barcode_amd/csrc/eval_plan.hpp on the CPU (tests/test_eval_plan_cpu.py builds it with g++ under
// AddressSanitizer / UndefinedBehaviorSanitizer and runs it): which path a force evaluation takes, against literals
// worked out by hand from the rules bchmc.hip spelled out in Pipe<T> before the header existed:
//     planes mode: planes_ok, calc_h 2, mk 3, not NO_PLANES; at the trajectory's ends too unless NO_PLANES_ENDS;
//     ALPT: no RSD and sfmodel != 1; on the 2-D plans with planes mode at the ends, not NO_ALPT_PLANES, plans over 2 n planes;
//     fused: (Zel'dovich, or ALPT on the 2-D plans) and a forward-model likelihood, a k-space mass, not NO_FUSE;
//     step s of neps: planes_c2r = planes and (s > 0 or ends), planes_r2c = planes and (not last or ends),
//         alpt_pending = ALPT on the 2-D plans, psi_unread = not last;
//     closing: x kernels where planes_r2c and like_mode 0 -- BX_LAST | ALPT | two-tile | one-tile --, else k_step_boundary;
//     two-tile: a table row, (fp32 and not BX_V1) or (fp64, n <= 256, BX_V2), a field below 2^32 bytes;
//     z pass in the binning: planes_c2r and NO_ZBIN unset, n = 256, 512 (128 with ZBIN_128), mk 3, calc_h 2, one-pass
//         binning, planes_ok;   own forward passes: planes_r2c, n = 512, fp32 or YFWD_F64, planes_ok.
// Then the whole space is swept for the invariants that keep a launch off a kernel or a plan that is not there.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../barcode_amd/csrc/eval_plan.hpp"
#include "../../barcode_amd/csrc/fft_host.hpp"

using namespace bchmc;

namespace {

int g_failures = 0;

void expect(const char *what, long long got, long long want) {
  if (got != want && g_failures++ < 40) std::printf("FAIL %s: %lld, expected %lld\n", what, got, want);
}
template <typename E>
void expect_kind(const char *what, E got, E want) {
  expect(what, (long long)got, (long long)want);
}
void expect_text(const char *what, const char *got, const char *want) {
  const bool same = (!got && !want) || (got && want && !std::strcmp(got, want));
  if (!same && g_failures++ < 40) std::printf("FAIL %s: \"%s\", expected \"%s\"\n", what, got ? got : "(null)", want ? want : "(null)");
}
void expect_mode(const char *what, EvalMode m, bool c2r, bool r2c, bool pending, bool unread) {
  expect(what, m.planes_c2r * 8 + m.planes_r2c * 4 + m.alpt_pending * 2 + m.psi_unread, c2r * 8 + r2c * 4 + pending * 2 + unread);
}

// the defaults of the cases: masskernel 3, calc_h 2, likelihood 1, a k-space mass, tiles with one-pass binning, planes_ok,
// Zel'dovich with RSD
PathFacts facts(int n, int esz) {
  PathFacts f;
  f.n = n, f.esz = esz, f.Nhp = (long long)n * n * fft_row_stride(n, esz);
  f.planes_ok = f.tiled = f.sort_direct = true;
  f.rsd_model = 1;
  return f;
}
PathFacts alpt_facts(int n, int esz) {
  PathFacts f = facts(n, esz);
  f.rsd_model = 0, f.sfmodel = 2, f.alpt_plans = true;
  return f;
}
const char *why(const PathFacts &f, const PathSwitches &s) { return zbin_why_not_text(zbin_why_not(f, s)); }

void literals() {
  const PathSwitches none;
  // ---- A: 256^3 fp64, Zel'dovich with RSD, 4 steps ----
  {
    const PathFacts f = facts(256, 8);
    expect("A Nhp", f.Nhp, 256ll * 256 * 136);
    const TrajPlan tp = traj_plan(f, none);
    expect("A fused", tp.fused * 4 + tp.fused_za * 2 + tp.alpt_x, 6);
    expect_kind("A c_za", tp.c_za, CZa::kZeldovich);
    expect("A planes", planes_on(f, none) * 2 + planes_at_ends(f, none), 3);
    expect_kind("A initial", initial_eval(f, none, tp), InitialEval::kBxFirst);
    expect_kind("A opening", opening(f, none, tp), Opening::kBxFirst);
    for (int s = 0; s < 4; s++) {
      const EvalMode m = step_mode(f, none, tp, s, 4);
      expect_mode("A mode", m, true, true, false, s < 3);
      expect("A z pass inside the binning", eval_zbin(f, none, m), 1);
      expect("A rocFFT's forward passes", eval_yfwd(f, none, m), 0);
      expect_kind("A closing", closing(f, none, tp, s, 4, 0), s < 3 ? Closing::kBxInterior : Closing::kBxLast);
      expect("A flip", buffers_flip(s, 4), s < 3);
    }
    expect_text("A z pass runs", why(f, none), nullptr);
  }
  // ---- B: the same with fp32: the two-tile interior boundary ----
  {
    PathFacts f = facts(256, 4);
    expect("B Nhp", f.Nhp, 256ll * 256 * 144);
    const TrajPlan tp = traj_plan(f, none);
    for (int s = 0; s < 4; s++)
      expect_kind("B closing", closing(f, none, tp, s, 4, 0), s < 3 ? Closing::kBxInteriorTwoTile : Closing::kBxLast);
    PathSwitches v1, v2;
    v1.bx_v1 = true, v2.bx_v2 = true;
    expect_kind("B closing, BX_V1", closing(f, v1, tp, 1, 4, 0), Closing::kBxInterior);
    expect_kind("B closing, fp64", closing(facts(256, 8), none, tp, 1, 4, 0), Closing::kBxInterior);
    expect_kind("B closing, fp64 BX_V2", closing(facts(256, 8), v2, tp, 1, 4, 0), Closing::kBxInteriorTwoTile);
    expect_kind("B closing, like_mode 1", closing(f, none, tp, 1, 4, 1), Closing::kStepBoundary);
    f.Nhp = (1ll << 29) - 1;  // 8 bytes per element: one below 2^32 bytes
    expect("B two-tile below 2^32 bytes", interior_two_tile(f, none), 1);
    f.Nhp = 1ll << 29;
    expect("B one-tile at 2^32 bytes", interior_two_tile(f, none), 0);
    expect_kind("B closing at 2^32 bytes", closing(f, none, tp, 1, 4, 0), Closing::kBxInterior);
    PathFacts d = facts(256, 8);
    d.Nhp = 1ll << 28;  // 16 bytes per element
    expect("B one-tile at 2^32 bytes, fp64 BX_V2", interior_two_tile(d, v2), 0);
  }
  // ---- C: 512^3 ----
  {
    PathSwitches y, v2;
    y.yfwd_f64 = true, v2.bx_v2 = true;
    for (int esz : {4, 8}) {
      const PathFacts f = facts(512, esz);
      const TrajPlan tp = traj_plan(f, none);
      const EvalMode m = step_mode(f, none, tp, 1, 4);
      expect("C own forward passes", eval_yfwd(f, none, m), esz == 4);
      expect("C own forward passes, YFWD_F64", eval_yfwd(f, y, m), 1);
      expect("C z pass inside the binning", eval_zbin(f, none, m), 1);
      expect_kind("C closing", closing(f, none, tp, 1, 4, 0), Closing::kBxInterior);
      expect_kind("C closing, BX_V2", closing(f, v2, tp, 1, 4, 0), Closing::kBxInterior);
      EvalMode off = m;
      off.planes_r2c = false;
      expect("C no own forward passes on the 3-D plans", eval_yfwd(f, y, off), 0);
    }
  }
  // ---- D: 128^3 ----
  {
    PathSwitches z;
    z.zbin_128 = true;
    const PathFacts f = facts(128, 8);
    expect_text("D reason", why(f, none), "Nx = 128 takes it with BCHMC_ZBIN_128=1 only");
    expect("D runs", zbin_ok(f, none), 0);
    expect_text("D reason, ZBIN_128", why(f, z), nullptr);
    expect("D runs, ZBIN_128", zbin_ok(f, z), 1);
    expect_kind("D closing, fp32", closing(facts(128, 4), none, traj_plan(f, none), 0, 2, 0), Closing::kBxInteriorTwoTile);
    expect_kind("D closing, fp64", closing(f, none, traj_plan(f, none), 0, 2, 0), Closing::kBxInterior);
  }
  // ---- E: 32^3 with planes_ok ----
  for (int esz : {4, 8}) {
    const PathFacts f = facts(32, esz);
    const TrajPlan tp = traj_plan(f, none);
    expect("E planes", planes_on(f, none) * 2 + planes_at_ends(f, none), 3);
    expect_text("E reason", why(f, none), "it exists for Nx = 128, 256 and 512");
    const EvalMode m = step_mode(f, none, tp, 1, 3);
    expect_mode("E mode", m, true, true, false, true);
    expect("E z pass", eval_zbin(f, none, m), 0);
    expect("E forward passes", eval_yfwd(f, none, m), 0);
    expect_kind("E closing", closing(f, none, tp, 1, 3, 0), Closing::kBxInterior);
  }
  // ---- F: 16^3, no planes mode.  psi_unread is set on every step but the last whatever the path: only the z pass inside
  // the binning reads it, and that needs planes_c2r ----
  {
    PathFacts f = facts(16, 8);
    f.planes_ok = false;
    const TrajPlan tp = traj_plan(f, none);
    expect("F fused", tp.fused * 4 + tp.fused_za * 2 + tp.alpt_x, 6);
    expect_kind("F initial", initial_eval(f, none, tp), InitialEval::k3d);
    expect_kind("F opening", opening(f, none, tp), Opening::kKickDriftZa);
    for (int s = 0; s < 3; s++) {
      expect_mode("F mode", step_mode(f, none, tp, s, 3), false, false, false, s < 2);
      expect_kind("F closing", closing(f, none, tp, s, 3, 0), s < 2 ? Closing::kStepBoundary : Closing::kStepBoundaryLast);
      expect("F flip", buffers_flip(s, 3), s < 2);
    }
  }
  // ---- G: ALPT at 256^3 on the 2-D plans ----
  for (int esz : {4, 8}) {
    const PathFacts f = alpt_facts(256, esz);
    const TrajPlan tp = traj_plan(f, none);
    expect("G fused", tp.fused * 4 + tp.fused_za * 2 + tp.alpt_x, 5);
    expect_kind("G c_za", tp.c_za, CZa::kAlptInput);
    expect("G displacement", uses_alpt(f, 0) * 4 + alpt_planes_wanted(f, none, 0) * 2 + alpt_on_planes(f, none, 0), 7);
    expect("G displacement with RSD", uses_alpt(f, 1) * 4 + alpt_planes_wanted(f, none, 1) * 2 + alpt_on_planes(f, none, 1), 0);
    expect_kind("G initial", initial_eval(f, none, tp), InitialEval::kBxFirstAlpt);
    expect_kind("G opening", opening(f, none, tp), Opening::kBxFirstAlpt);
    for (int s = 0; s < 4; s++) {
      expect_mode("G mode", step_mode(f, none, tp, s, 4), true, true, true, s < 3);
      expect_kind("G closing", closing(f, none, tp, s, 4, 0), s < 3 ? Closing::kBxInteriorAlpt : Closing::kBxLast);
    }
    PathSwitches a, e;
    a.no_alpt_planes = true, e.no_planes_ends = true;
    PathFacts late = f;
    late.alpt_plans = false;
    expect("G NO_ALPT_PLANES", traj_plan(f, a).fused * 4 + alpt_planes_wanted(f, a, 0) * 2 + alpt_on_planes(f, a, 0), 0);
    expect("G NO_PLANES_ENDS", traj_plan(f, e).fused * 4 + alpt_planes_wanted(f, e, 0) * 2 + alpt_on_planes(f, e, 0), 0);
    expect("G no plans", traj_plan(late, none).fused * 4 + alpt_planes_wanted(late, none, 0) * 2 + alpt_on_planes(late, none, 0), 2);
    expect_kind("G no plans, c_za", traj_plan(late, none).c_za, CZa::kZeldovich);
    expect_kind("G no plans, initial", initial_eval(late, none, traj_plan(late, none)), InitialEval::k3d);
    expect("G no plans, uses ALPT", uses_alpt(late, 0), 1);
  }
  // ---- H, I: a real-space mass, the GRF likelihood ----
  {
    PathFacts hm = facts(256, 8), il = facts(256, 8);
    hm.mass_rs = true, il.likelihood = 3;
    expect("H fused", traj_plan(hm, none).fused * 2 + traj_plan(hm, none).fused_za, 1);
    expect_kind("H initial", initial_eval(hm, none, traj_plan(hm, none)), InitialEval::k3d);
    expect("I fused", traj_plan(il, none).fused * 2 + traj_plan(il, none).fused_za, 0);
    PathSwitches nf;
    nf.no_fuse = true;
    expect("NO_FUSE", traj_plan(facts(256, 8), nf).fused * 2 + traj_plan(facts(256, 8), nf).fused_za, 1);
  }
  // ---- J: A with NO_PLANES_ENDS ----
  {
    PathSwitches e;
    e.no_planes_ends = true;
    const PathFacts f = facts(256, 8);
    const TrajPlan tp = traj_plan(f, e);
    expect("J fused", tp.fused, 1);
    expect("J planes", planes_on(f, e) * 2 + planes_at_ends(f, e), 2);
    expect_kind("J initial", initial_eval(f, e, tp), InitialEval::k3d);
    expect_kind("J opening", opening(f, e, tp), Opening::kKickDriftZa);
    const EvalMode m0 = step_mode(f, e, tp, 0, 4), m1 = step_mode(f, e, tp, 1, 4), m3 = step_mode(f, e, tp, 3, 4);
    expect_mode("J step 0", m0, false, true, false, true);
    expect("J step 0, z pass", eval_zbin(f, e, m0), 0);
    expect_kind("J step 0, closing", closing(f, e, tp, 0, 4, 0), Closing::kBxInterior);
    expect_mode("J step 1", m1, true, true, false, true);
    expect("J step 1, z pass", eval_zbin(f, e, m1), 1);
    expect_mode("J step 3", m3, true, false, false, false);
    expect("J step 3, z pass", eval_zbin(f, e, m3), 1);
    expect_kind("J step 3, closing", closing(f, e, tp, 3, 4, 0), Closing::kStepBoundaryLast);
  }
  // ---- K: one step is first and last at once ----
  {
    PathSwitches e;
    e.no_planes_ends = true;
    const PathFacts f = facts(256, 8);
    expect_mode("K mode", step_mode(f, none, traj_plan(f, none), 0, 1), true, true, false, false);
    expect_kind("K closing", closing(f, none, traj_plan(f, none), 0, 1, 0), Closing::kBxLast);
    expect("K flip", buffers_flip(0, 1), 0);
    expect_mode("K mode, NO_PLANES_ENDS", step_mode(f, e, traj_plan(f, e), 0, 1), false, false, false, false);
    expect_kind("K closing, NO_PLANES_ENDS", closing(f, e, traj_plan(f, e), 0, 1, 0), Closing::kStepBoundaryLast);
    expect_kind("K opening, NO_PLANES_ENDS", opening(f, e, traj_plan(f, e)), Opening::kKickDriftZa);
  }
  // ---- L .. O: the z pass's reasons, in the order they are tested ----
  {
    PathFacts l = facts(256, 8), m = facts(256, 8), m2 = facts(256, 8), o = facts(256, 8);
    l.calc_h = 1;
    expect("L planes", planes_on(l, none), 0);
    expect_text("L reason", why(l, none), "it needs masskernel 3 with calc_h 2");
    m.sort_direct = false, m2.tiled = false;
    expect_text("M reason", why(m, none), "the one-pass tile binning is not in use");
    expect_text("M reason, no tiles", why(m2, none), "the one-pass tile binning is not in use");
    o.planes_ok = false;
    expect_text("O reason", why(o, none), "the planes-mode transforms are not available");
    PathSwitches nz;
    nz.no_zbin = true;
    PathFacts n = facts(128, 8);
    n.calc_h = 1, n.mk = 1, n.tiled = n.sort_direct = n.planes_ok = false;
    expect_text("N reason", why(n, nz), "BCHMC_NO_ZBIN is set");
    expect_text("N reason, all else in order", why(facts(256, 8), nz), "BCHMC_NO_ZBIN is set");
    expect_text("order: 128 before the configuration", why(n, none), "Nx = 128 takes it with BCHMC_ZBIN_128=1 only");
    n.n = 32;
    expect_text("order: size before the configuration", why(n, none), "it exists for Nx = 128, 256 and 512");
    n.n = 256;
    expect_text("order: configuration before the binning", why(n, none), "it needs masskernel 3 with calc_h 2");
    n.calc_h = 2, n.mk = 3;
    expect_text("order: binning before the planes", why(n, none), "the one-pass tile binning is not in use");
    PathSwitches np;
    np.no_planes = true;  // the z pass does not ask for planes mode, only for its transforms: its callers pass planes_c2r
    expect_text("NO_PLANES leaves the z pass itself alone", why(facts(256, 8), np), nullptr);
    expect("NO_PLANES: no planes_c2r", step_mode(facts(256, 8), np, traj_plan(facts(256, 8), np), 1, 3).planes_c2r, 0);
  }
}

PathSwitches switches(int bits) {
  PathSwitches s;
  s.no_planes = bits & 1, s.no_planes_ends = bits & 2, s.no_fuse = bits & 4, s.no_alpt_planes = bits & 8;
  s.no_zbin = bits & 16, s.zbin_128 = bits & 32, s.yfwd_f64 = bits & 64, s.bx_v1 = bits & 128, s.bx_v2 = bits & 256;
  return s;
}

bool is_bx(Closing c) { return c != Closing::kStepBoundary && c != Closing::kStepBoundaryLast; }

void fail_at(const char *what, const PathFacts &f) {
  if (g_failures++ < 40)
    std::printf("FAIL invariant \"%s\" at n %d esz %d mk %d calc_h %d likelihood %d sfmodel %d rsd %d mass_rs %d tiled %d "
                "sort_direct %d planes_ok %d alpt_plans %d\n", what, f.n, f.esz, f.mk, f.calc_h, f.likelihood, f.sfmodel,
                f.rsd_model, f.mass_rs, f.tiled, f.sort_direct, f.planes_ok, f.alpt_plans);
}

// One point of the space: every decision about it, held to the invariants.  Returns how many were checked.
// (facts, switches and the count are locals by value: the sanitizers then have no memory access to check per invariant)
unsigned long long check_point(const PathFacts f, const PathSwitches s) {
  unsigned long long checked = 0;  // (unsigned: no overflow check per invariant either)
#define hold(what, ok) do { checked++; if (!(ok)) fail_at(what, f); } while (0)
  const TrajPlan tp = traj_plan(f, s);
  const bool x_row = x_shape(f.esz, f.n).nt != 0, x2_row = x2_shape(f.esz, f.n).nt != 0, z_row = z_shape(f.esz, f.n).nt != 0;
  hold("alpt_x implies planes at the ends and fused", !tp.alpt_x || (planes_at_ends(f, s) && tp.fused));
  hold("alpt_x decides c_za", (tp.c_za == CZa::kAlptInput) == tp.alpt_x);
  hold("runs equals reason none", zbin_ok(f, s) == (zbin_why_not(f, s) == ZbinWhyNot::kNone));
  hold("reason none has no text", (zbin_why_not_text(zbin_why_not(f, s)) == nullptr) == zbin_ok(f, s));
  hold("z pass needs its row", !zbin_ok(f, s) || z_row);
  hold("own forward passes need the y and z rows", !yfwd_ok(f, s) || (z_row && y_shape(f.esz, f.n).nt));
  hold("two-tile needs its row", !interior_two_tile(f, s) || x2_row);
  for (int rsd = 0; rsd < 2; rsd++) {
    hold("ALPT on planes implies wanted and plans", !alpt_on_planes(f, s, rsd) || (alpt_planes_wanted(f, s, rsd) && f.alpt_plans));
    hold("ALPT planes wanted implies ALPT and planes at the ends", !alpt_planes_wanted(f, s, rsd) || (uses_alpt(f, rsd) && planes_at_ends(f, s)));
  }
  const InitialEval ie = initial_eval(f, s, tp);
  hold("BX_FIRST before the first step needs an x row and planes at the ends", ie == InitialEval::k3d || (x_row && planes_at_ends(f, s) && tp.fused));
  hold("BX_FIRST with ALPT before the first step iff alpt_x", (ie == InitialEval::kBxFirstAlpt) == (tp.alpt_x && ie != InitialEval::k3d));
  if (!tp.fused) return checked;
  const Opening op = opening(f, s, tp);
  hold("opening BX_FIRST needs an x row", op == Opening::kKickDriftZa || x_row);
  hold("opening with ALPT iff alpt_x", (op == Opening::kBxFirstAlpt) == tp.alpt_x);
  for (unsigned long long neps = 0; neps <= 4; neps++) {
    for (unsigned long long step = 0; step < neps; step++) {
      const bool last = step + 1 == neps;
      const EvalMode m = step_mode(f, s, tp, step, neps);
      hold("alpt_pending implies planes_c2r", !m.alpt_pending || m.planes_c2r);
      hold("psi_unread on every step but the last", m.psi_unread == !last);
      hold("planes_c2r of step 0 is what the opening left", step > 0 || m.planes_c2r == (op != Opening::kKickDriftZa));
      hold("z pass inside the binning needs planes_c2r and its row", !eval_zbin(f, s, m) || (m.planes_c2r && z_row));
      hold("own forward passes need planes_r2c", !eval_yfwd(f, s, m) || m.planes_r2c);
      hold("the buffers flip on every step but the last", buffers_flip(step, neps) == !last);
      const Closing c = closing(f, s, tp, step, neps, 0);
      hold("no BX kind without the three V components (like_mode 1)", !is_bx(closing(f, s, tp, step, neps, 1)));
      hold("every BX kind needs an x row", !is_bx(c) || x_row);
      hold("every BX kind needs planes_r2c", !is_bx(c) || m.planes_r2c);
      hold("two-tile needs its row", c != Closing::kBxInteriorTwoTile || (x2_row && interior_two_tile(f, s)));
      hold("two-tile never with ALPT", c != Closing::kBxInteriorTwoTile || !tp.alpt_x);
      hold("the last step closes with a last kind", last == (c == Closing::kBxLast || c == Closing::kStepBoundaryLast));
      hold("ALPT interior iff alpt_x", c != Closing::kBxInteriorAlpt || tp.alpt_x);
      hold("alpt_x never closes an interior step with a Zel'dovich x kernel",
           !tp.alpt_x || (c != Closing::kBxInterior && c != Closing::kBxInteriorTwoTile));
      // what the next step's evaluation finds in Ck is what this closing left there
      if (!last) hold("planes_c2r of the next step is what this closing left", step_mode(f, s, tp, step + 1, neps).planes_c2r == is_bx(c));
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
          for (int bits = 0; bits < 512; bits++) checked += check_point(f, switches(bits));
        }
  return checked;
}

}  // namespace

int main() {
  unsetenv("BCHMC_FFT_PAD");  // fft_row_stride's test switch: the literals are for the engine's default padding
  literals();
  const unsigned long long checked = sweep();
  if (g_failures) {
    std::printf("eval_plan_check: %d failures\n", g_failures);
    return 1;
  }
  std::printf("eval_plan_check: ok (%llu invariants held)\n", checked);
  return 0;
}
