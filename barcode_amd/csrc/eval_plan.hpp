// eval_plan.hpp -- which path a force evaluation takes: planes mode or the 3-D plans, the fused step boundary and its
// one-tile, two-tile or ALPT formulation, the ALPT pipeline on the 2-D plans, the z pass inside the binning, the engine's
// own forward y / z passes, V as records and as two arrays into the forward x pass.  The single statement of it, as pure
// functions of the path switches (PathSwitches: the environment as bchmc_create read it) and of what a handle is and holds
// at the moment of asking (PathFacts).  Plain C++: no HIP types, no getenv; tests/host/eval_plan_check.cpp proves it
// against literals and sweeps the whole space
// (psi_pair, the two arrays between the inverse x and y passes: tests/host/two_array_check.cpp; v_pair / v_rec, their
// mirror image on the forward side: tests/host/vpair_check.cpp).
// Whether a fused trajectory keeps its k-space state and weights in x-column tiles between its opening and its closing
// boundary (BCHMC_NO_XTILE=1: never) is decided next door, in xtile.hpp (x_tiles; tests/host/xtile_check.cpp), from the same
// switches and facts.
//
// Nothing here is cached and nothing should be: sort_direct changes when the record slots are given up, and the plans over
// 2 n planes can appear late.  bchmc.hip gathers the facts when it needs a decision, asks, and switches on the answer.
#pragma once

#include "pass_launch.hpp"

namespace bchmc {

struct PathSwitches {           // BCHMC_<NAME>=1, read once per handle
  bool no_planes = false;       // NO_PLANES: every transform on the 3-D plans
  bool no_planes_ends = false;  // NO_PLANES_ENDS: planes mode for interior steps only
  bool no_fuse = false;         // NO_FUSE: k_assemble + k_kick_drift_za instead of the fused step boundary
  bool no_alpt_planes = false;  // NO_ALPT_PLANES: the ALPT pipeline on the 3-D plans
  bool no_zbin = false;         // NO_ZBIN: rocFFT's 2-D C2R + k_bin_direct instead of k_ypass + k_zbin_direct
  bool zbin_128 = false;        // ZBIN_128: ... which n = 128 takes only when asked
  bool yfwd_f64 = false;        // YFWD_F64: the engine's own forward y / z passes at 512^3 for fp64 fields too
  bool bx_v1 = false;           // BX_V1: the one-tile interior boundary for fp32 fields
  bool bx_v2 = false;           // BX_V2: the two-tile interior boundary for fp64 fields
  bool no_pair = false;         // NO_PAIR: three arrays, not two, between the inverse x pass and the y pass
  bool no_vpair = false;        // NO_VPAIR: rocFFT's 2-D R2C of the three arrays of V and three arrays into the forward x pass
  bool no_vrec = false;         // NO_VREC: the gather's V as three arrays, not one record per particle
  bool no_xtile = false;        // NO_XTILE: the natural layout for the trajectory's k-space state and weights (xtile.hpp)
};

struct PathFacts {
  int n = 0, esz = 8;        // cells per axis, bytes of the storage type
  long long Nhp = 0;         // padded half-complex elements of one field
  bool planes_ok = false;    // the 2-D plans over 3 n planes, the x-pass table row and the twiddles exist
  bool tiled = false;        // tile-sorted particle-mesh path ...
  bool sort_direct = false;  // ... with the one-pass binning
  int mk = 3, calc_h = 2, likelihood = 1, sfmodel = 1, rsd_model = 0;
  bool mass_rs = false;      // the mass has a real-space part
  bool alpt_plans = false;   // the 2-D plans over 2 n planes exist
  bool std81 = false;        // ... the tile-sorted path gathers with the standard 81-cell hull (k_gather_tile81)
  bool mass_fs = false;      // the mass has a k-space part (wM exists)
};

struct EvalMode {             // how ONE force evaluation runs; decided by the caller
  bool planes_c2r = false;    // Psi^ in Ck is in planes space: only the (y, z) passes remain
  bool planes_r2c = false;    // V^ is wanted in planes space
  bool alpt_pending = false;  // Ck[0], Ck[1] hold delta(1)^ | Phi^ planes left by k_step_boundary_x<ALPT>
  bool psi_unread = false;    // interior step: nobody reads Psi / positions, the z pass may end in the binning
};

// ---- planes mode ------------------------------------------------------------------------------------------------------
// the SPH-adjoint path (three V components) with a supported grid (planes_ok says the x-pass table has the row; the table
// is asked all the same, so that no input at all leads to a k_step_boundary_x that does not exist)
constexpr bool planes_on(const PathFacts &f, const PathSwitches &s) {
  return f.planes_ok && x_shape(f.esz, f.n).nt && f.calc_h == 2 && f.mk == 3 && !s.no_planes;
}
// ... also for the force evaluation before the first step and for the first and the last step (BX_FIRST / BX_LAST
// variants of k_step_boundary_x)
constexpr bool planes_at_ends(const PathFacts &f, const PathSwitches &s) { return planes_on(f, s) && !s.no_planes_ends; }

// ---- the displacement of a forward evaluation ------------------------------------------------------------------------
// Which structure-formation model it uses (dispatcher Lag2Eul.cc:325-331; the RSD routine is Zel'dovich whatever sfmodel
// says, HMC_models.cc:395-405).
constexpr bool uses_alpt(const PathFacts &f, int rsd) { return !rsd && f.sfmodel != 1; }
// ALPT on the 2-D plans (alpt_x.hpp): the SPH-adjoint path's planes mode plus two plans over 2 n planes.  "Wanted" does
// not look at those plans: where it holds and they are missing, the engine tries to make them.
constexpr bool alpt_planes_wanted(const PathFacts &f, const PathSwitches &s, int rsd) {
  return uses_alpt(f, rsd) && planes_at_ends(f, s) && !s.no_alpt_planes;
}
constexpr bool alpt_on_planes(const PathFacts &f, const PathSwitches &s, int rsd) {
  return alpt_planes_wanted(f, s, rsd) && f.alpt_plans;
}

// ---- the fused z pass + binning (one lattice site along z per thread of k_zbin_direct) --------------------------------
enum class ZbinWhyNot { kNone, kSwitchedOff, kNeeds128Switch, kGridSize, kNotSphAdjoint, kNoOnePassBinning, kNoPlanes };

// The first condition that does not hold; kNone: it runs.
// (128^3: measured 2 % slower -- 4096 small workgroups, the binning part grows by more than rocFFT's row pass costs
// there -- so rocFFT keeps it unless BCHMC_ZBIN_128=1, which the tests use for the n = 128 instantiation.
// mk 3 + calc_h 2 on tiles: nothing but the fallback sort reads Psi after the binning.)
constexpr ZbinWhyNot zbin_why_not(const PathFacts &f, const PathSwitches &s) {
  if (s.no_zbin) return ZbinWhyNot::kSwitchedOff;
  if (f.n == 128 && !s.zbin_128) return ZbinWhyNot::kNeeds128Switch;
  if (!z_shape(f.esz, f.n).nt) return ZbinWhyNot::kGridSize;
  if (f.mk != 3 || f.calc_h != 2) return ZbinWhyNot::kNotSphAdjoint;
  if (!f.tiled || !f.sort_direct) return ZbinWhyNot::kNoOnePassBinning;
  if (!f.planes_ok) return ZbinWhyNot::kNoPlanes;
  return ZbinWhyNot::kNone;
}
constexpr const char *zbin_why_not_text(ZbinWhyNot w) {  // bchmc_probe_displacement_z's refusal
  switch (w) {
    case ZbinWhyNot::kNone: return nullptr;
    case ZbinWhyNot::kSwitchedOff: return "BCHMC_NO_ZBIN is set";
    case ZbinWhyNot::kNeeds128Switch: return "Nx = 128 takes it with BCHMC_ZBIN_128=1 only";
    case ZbinWhyNot::kGridSize: return "it exists for Nx = 128, 256 and 512";
    case ZbinWhyNot::kNotSphAdjoint: return "it needs masskernel 3 with calc_h 2";
    case ZbinWhyNot::kNoOnePassBinning: return "the one-pass tile binning is not in use";
    case ZbinWhyNot::kNoPlanes: break;
  }
  return "the planes-mode transforms are not available";
}
constexpr bool zbin_ok(const PathFacts &f, const PathSwitches &s) { return zbin_why_not(f, s) == ZbinWhyNot::kNone; }
// In an evaluation: the engine's own y pass, and the z pass inside the binning kernel -- Psi does not go through HBM
// (zpass.hpp).  Interior steps (m.psi_unread) skip the store of Psi; the other planes-space evaluations use the same
// kernels and store it on the way (0.385 against 0.45 ms at 256^3): their positions may be fetched.
constexpr bool eval_zbin(const PathFacts &f, const PathSwitches &s, const EvalMode &m) { return m.planes_c2r && zbin_ok(f, s); }

// ---- the engine's own row + column passes of the planes-mode R2C ------------------------------------------------------
// Where rocFFT's column kernel is the slower one (n = 512).  fp32 fields: R2C class 2.59 -> 1.85 ms per step (17.96 ->
// 17.35 ms, +3.5 %); fp64: rocFFT's double-precision column kernel is as fast as the pair (3.14 against 3.16 ms) and
// stays unless BCHMC_YFWD_F64=1.
constexpr bool yfwd_ok(const PathFacts &f, const PathSwitches &s) {
  return f.n == 512 && (f.esz == 4 || s.yfwd_f64) && f.planes_ok;
}
constexpr bool eval_yfwd(const PathFacts &f, const PathSwitches &s, const EvalMode &m) { return m.planes_r2c && yfwd_ok(f, s); }

// ---- the interior Zel'dovich boundary: one tile per workgroup or two --------------------------------------------------
// fp32 fields: the two-tile formulation (k_step_boundary_x2).  A 1024-thread workgroup is alone on its CU there and the
// first formulation leaves its memory phases exposed: 0.283 -> 0.231 ms at 256^3.  With fp64 fields (two 512-thread
// workgroups per CU) both formulations take the same 0.329 ms -- 4.7 TB/s is what this access pattern (128-byte segments,
// one per DRAM row) gets however much is in flight -- and the first one stays (BCHMC_BX_V2=1 selects the second for fp64
// too; profiles/r03_ab_bx2.txt).  512^3 fp32: no difference, and the table has no row.  The second formulation's lane
// offsets are 32-bit byte offsets into one field.
constexpr bool interior_two_tile(const PathFacts &f, const PathSwitches &s) {
  const bool want = (f.esz == 4 && !s.bx_v1) || (f.esz == 8 && f.n <= 256 && s.bx_v2);
  return x2_shape(f.esz, f.n).nt && want && (unsigned long long)f.Nhp * 2 * f.esz < (1ull << 32);
}

// ---- a trajectory ------------------------------------------------------------------------------------------------------
// Which model produces the displacement, whether the fused step boundary applies, and the constant that turns q^ into
// the model's k-space input.  The k-space kernels produce the Zel'dovich Psi^ as a by-product; the ALPT model needs its
// own pipeline, and on the 2-D plans the step boundary leaves that pipeline's two input fields instead of Psi^.
enum class CZa {
  kZeldovich,  // -D1 deltaQ_factor / N: q^ -> the Zel'dovich Psi^
  kAlptInput   // +deltaQ_factor / N: q^ -> delta(1)^ (D1 enters in k_alpt_sources)
};
struct TrajPlan {
  bool alpt_x = false, fused_za = false, fused = false;
  CZa c_za = CZa::kZeldovich;
};

// ---- two arrays, not three, between the inverse x pass and the y pass ---------------------------------------------------
// Psi^_y = ky B and Psi^_z = kz B with one B: a Zel'dovich k_step_boundary_x (BX_FIRST, interior, one tile or two) stores
// Psi^_x and B only, and k_ypass_pair makes the two products where it holds the column anyway: one complex array less
// written and one less read.  Only where the engine's own y pass is what follows a boundary in planes space -- rocFFT's
// 2-D C2R wants its three arrays, so NO_ZBIN, the fallback sort, 128^3 without ZBIN_128 and everything zbin_why_not lists
// keep them -- and never for the ALPT boundary, whose two arrays are other fields.  The boundary kernels exist only in
// planes mode (planes_on: calc_h 2, mk 3, not NO_PLANES).  bchmc.hip remembers what the last boundary left in Ck and
// refuses an evaluation that would read two arrays as three.
constexpr bool psi_pair(const PathFacts &f, const PathSwitches &s, const TrajPlan &tp) {
  return !s.no_pair && !tp.alpt_x && planes_on(f, s) && zbin_ok(f, s) && ypair_shape(f.esz, f.n).nt;
}
constexpr TrajPlan traj_plan(const PathFacts &f, const PathSwitches &s) {
  TrajPlan tp;
  const bool alpt = uses_alpt(f, f.rsd_model) && f.likelihood != 3;
  tp.alpt_x = alpt && !f.mass_rs && !s.no_fuse && alpt_on_planes(f, s, f.rsd_model);
  tp.fused_za = f.likelihood != 3 && !alpt;
  tp.c_za = tp.alpt_x ? CZa::kAlptInput : CZa::kZeldovich;
  tp.fused = (tp.fused_za || tp.alpt_x) && !f.mass_rs && !s.no_fuse;
  return tp;
}

// ---- V as records and two arrays, not three, into the forward x pass ----------------------------------------------------
// The mirror image on the forward side.  V^_y and V^_z enter the boundary kernel only as W = ky V^_y + kz V^_z, and ky, kz
// are constants of an element from the y pass on: k_zr2c makes the row pass, k_ypass_fwd_pair the column pass, storing V^_x
// and W only, and a Zel'dovich k_step_boundary_x (interior, BX_LAST, one tile or two) with `vpair` reads the two -- one
// complex array less written and one less read, in place of rocFFT's 2-D R2C.  Where planes mode is on and the boundary
// is not ALPT's (whose forward side this is too, but whose builds are not measured), on the tile-sorted standard-81
// path with the one-pass binning (zbin_ok: 128^3 follows BCHMC_ZBIN_128 as psi_pair does), where the y and z pass shapes
// exist.  bchmc.hip remembers what the last forward side left in Ck (ck_vpair) and refuses a boundary that would read
// two arrays as three or three as two.  BCHMC_NO_VPAIR=1: the three arrays through rocFFT.
// Not at n = 512: measured at 256^3 only (profiles/r05_ab_vpair.txt), and 512^3 has a measured choice of its own (yfwd_ok
// above), which stays as it is until this path is measured against it there.
constexpr bool v_pair(const PathFacts &f, const PathSwitches &s, const TrajPlan &tp) {
  return !s.no_vpair && !tp.alpt_x && f.n != 512 && planes_on(f, s) && zbin_ok(f, s) && f.std81 &&
         y_shape(f.esz, f.n).nt && z_shape(f.esz, f.n).nt && yfwd_pair_shape(f.esz, f.n).nt;
}
// ... in an evaluation: one that wants V^ in planes space.  Never where eval_yfwd holds (n = 512).
constexpr bool eval_vpair(const PathFacts &f, const PathSwitches &s, const EvalMode &m) {
  return m.planes_r2c && v_pair(f, s, traj_plan(f, s));
}
// ... and k_gather_tile81 then stores V as one record {vx, vy, vz, 0} per particle (a whole 32-byte write instead of three
// partial ones), which k_zr2c reads as records.  BCHMC_NO_VREC=1: the same transforms from the three arrays of V.
constexpr bool v_rec(const PathFacts &f, const PathSwitches &s) { return v_pair(f, s, traj_plan(f, s)) && !s.no_vrec; }
constexpr bool eval_vrec(const PathFacts &f, const PathSwitches &s, const EvalMode &m) {
  return eval_vpair(f, s, m) && !s.no_vrec;
}

// The force evaluation before the first step: on the 3-D plans from the displacement on, or on the 2-D plans between a
// BX_FIRST (Zel'dovich or ALPT) and a BX_LAST boundary.
enum class InitialEval { k3d, kBxFirst, kBxFirstAlpt };
constexpr InitialEval initial_eval(const PathFacts &f, const PathSwitches &s, const TrajPlan &tp) {
  if (!(tp.fused && planes_at_ends(f, s))) return InitialEval::k3d;
  return tp.alpt_x ? InitialEval::kBxFirstAlpt : InitialEval::kBxFirst;
}

// Step `step` of `neps` of a fused trajectory (tp.fused).  What opens the trajectory (before step 0):
enum class Opening { kKickDriftZa, kBxFirst, kBxFirstAlpt };
constexpr Opening opening(const PathFacts &f, const PathSwitches &s, const TrajPlan &tp) {
  if (!planes_at_ends(f, s)) return Opening::kKickDriftZa;
  return tp.alpt_x ? Opening::kBxFirstAlpt : Opening::kBxFirst;
}
// ... how the step's force evaluation runs:
constexpr EvalMode step_mode(const PathFacts &f, const PathSwitches &s, const TrajPlan &tp, unsigned long long step,
                             unsigned long long neps) {
  const bool planes = planes_on(f, s), ends = planes_at_ends(f, s), last = step + 1 == neps;
  EvalMode m;
  m.planes_c2r = planes && (step > 0 || ends);  // Psi^ left by k_step_boundary_x still needs only the (y, z) passes
  m.planes_r2c = planes && (!last || ends);     // ... and V^ for it gets only those
  m.alpt_pending = tp.alpt_x;                   // ... or delta(1)^ | Phi^ planes for the ALPT pipeline
  m.psi_unread = !last;
  return m;
}
// ... and what closes it, given the assemble mode the evaluation returned.  The last boundary writes p in place, no q, and
// leaves the gradient in gk; every other one moves the state to the other pair of the ping-pong buffers.
enum class Closing { kBxLast, kStepBoundaryLast, kBxInterior, kBxInteriorTwoTile, kBxInteriorAlpt, kStepBoundary };
constexpr Closing closing(const PathFacts &f, const PathSwitches &s, const TrajPlan &tp, unsigned long long step,
                          unsigned long long neps, int like_mode) {
  const bool last = step + 1 == neps, xmode = step_mode(f, s, tp, step, neps).planes_r2c && like_mode == 0;
  if (last) return xmode ? Closing::kBxLast : Closing::kStepBoundaryLast;
  if (!xmode) return Closing::kStepBoundary;
  if (tp.alpt_x) return Closing::kBxInteriorAlpt;
  return interior_two_tile(f, s) ? Closing::kBxInteriorTwoTile : Closing::kBxInterior;
}
constexpr bool buffers_flip(unsigned long long step, unsigned long long neps) { return step + 1 != neps; }

}  // namespace bchmc
