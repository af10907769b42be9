// bchmc.hip -- host side of libbarcode_hip.so: the C ABI of include/bchmc.h on top of the kernels in
// kernels.hpp and rocFFT R2C/C2R plans, all on one hipStream per handle.  gfx950 only.
//
// Trajectory layout: q and p live in Fourier space for the whole trajectory, so one
// leapfrog step costs 3 C2R (displacements) + 3 R2C (V components) instead of the reference's 12 FFTs
// (SURVEY.md 2.1 "FFT count per leapfrog step").
//
// The pipeline is a template on the storage type T of the field arrays (double: reference DOUBLE_PREC;
// float: BASELINE config 5, "fp32 field arrays"); the C ABI always exchanges double arrays.
#include "../../include/bchmc.h"
#include "kernels.hpp"
#include "fft_host.hpp"
#include "owned.hpp"
#include "pass_launch.hpp"
#include "launch_grid.hpp"
#include "eval_plan.hpp"
#include "xtile_kernels.hpp"
#include "interp_plan.hpp"

#include <rocfft/rocfft.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

using namespace bchmc;
using namespace owned;

namespace {

struct ProfRec {
  int cls;
  Event a, b;
};

}  // namespace

struct bchmc_handle {
  bchmc_config c{};
  Geo g{};
  bool f32 = false;   // storage type of the field arrays
  size_t esz = 8;     // sizeof(T)
  int mass_fs = 0, mass_rs = 0;
  PathSwitches sw;            // the path switches of eval_plan.hpp, as the environment had them at create (read_path_switches)
  bool no_tiles_low = false;  // BCHMC_NO_TILES_LOW, as make_tiles read it
  std::string err;
  // Every resource below is an owner of owned.hpp, and bchmc_destroy only deletes the handle: members are destroyed
  // in reverse declaration order, and three things depend on that order.  The stream is declared before every buffer
  // and event, so it outlives them; the rocFFT user before the stream, so rocfft_cleanup runs after the stream is
  // gone; the work buffer before the execution info and the plans that point at it, so they go first.
  RocfftUser fft_user;
  Stream stream;

  // rocFFT
  DevBytes work;  // shared by all plans; its capacity is what info was told
  FftInfo info;
  FftPlan r2c1, c2r1, r2c3, c2r3;

  // inputs (N elements of T each) + derived half-layout multipliers (always double)
  DevBytes in_arr[6];
  bool have[6] = {false, false, false, false, false, false};
  DevBuf<double> wS, wM;  // normFS / signal_PS, normFS / mass_f on the half-complex layout
  DevBuf<double2> wpair;  // Nhp: {wS, wM} in x-column tiles (xtile.hpp), made by trajectory_fused where x_tiles holds ...
  unsigned long long w_gen = 1, wpair_gen = 0;  // ... and made again when upload() has written wS or wM since (w_gen moved)

  // state and scratch (T / C2<T>)
  DevBytes qk, pk, gk;                               // Nhp complex each
  DevBytes qk2, pk2;                                 // ping-pong partners of (qk, pk) for the fused step boundary
  XLayout qk_layout = XLayout::kNatural;             // what (qk, pk) hold: tiled only between the opening and the closing
                                                     // boundary of trajectory_fused (XPairs, xtile.hpp), natural on every return
  DevBytes Ck;                                       // 3 Nhp: Psi^ / V^
  bool ck_pair = false;                              // Ck holds Psi^_x | B of a boundary kernel with `pair` (psi_pair, eval_plan.hpp)
  DevBytes tC;                                       // Nhp scratch
  DevBytes psi;                                      // 3 N: displacement components
  DevBytes V;                                        // 3 N: V components
  DevBytes vrec;                                     // 4 N: V as records {vx, vy, vz, 0}, where v_rec holds (eval_plan.hpp); made on first use
  bool ck_vpair = false;                             // Ck holds V^_x | W of k_ypass_fwd_pair (v_pair, eval_plan.hpp)
  bool vrec_eval = false;                            // this evaluation's binning zeroed V records: its gather writes records
  bool v_in_vrec = false;                            // the last evaluation's V is in vrec, not in V
  DevBytes rho, plike;                               // N each
  DevBuf<long long> rho_fix;                         // N: fixed-point density (deterministic mode only)
  DevBuf<int> fix_sat;                               // 1: set by k_fix_to_rho when a fixed-point cell came near wrapping
  long long fix_sat_limit = 1ll << 62;               // (BCHMC_FIX_SAT_LOG2 lowers it: test hook for the error path)
  bool fix = false;                                  // deterministic mode
  DevBytes ioq, iop;                                 // N each: staging / scratch
  DevBytes gprior, glike;                            // N each, lazily allocated by bchmc_gradient
  DevBytes conv;                                     // 3 N, lazily allocated for calc_h 0 / 3
  DevBuf<double> convF;                              // Nhp: SPH kernel transform table for calc_h = 3
  DevBuf<double> dstage;                             // 2 N doubles: ABI <-> T conversion staging
  // device-resident chain: current sample and momenta in k-space, energy partials
  DevBytes cq, cp;                                   // Nhp complex each
  DevBuf<double> part6;                              // 6 * kRedBlocks doubles
  bool have_cq = false, have_cp = false, have_prop = false;
  bool cp_draw_rs = false;  // cp is a draw for a real-space mass alone, and mass_r is still the array it was drawn with
  // Force carried along the chain: g^ = FFT-space gradient_psi at the chain state cq, with its -log L.  The end of an
  // accepted trajectory (or the start of a rejected one) IS the next trajectory's start, so the gradient HMC.cc:279
  // evaluates there is already known; only the fast attempt mode uses it.  Any new input or state invalidates it.
  DevBytes cg;
  bool cg_valid = false, prop_g_valid = false;
  double c_like = 0., prop_like = 0.;
  DevBuf<double> rho_part, partA;                    // kRedBlocks doubles each
  DevBuf<double> guard;                              // guard slots, one per step
  DevBuf<int> stop;
  DevBuf<unsigned long long> steps_done;
  PinnedBuf<double> h_part;                          // pinned host staging for partials
  // draw_momenta from a GSL mt19937 state (mt_draw.hpp), set up on the first such draw: S words per segment, B
  // segments, C = B S words per pass, G Gaussians per draw
  struct MtDraw {
    long long S = 0, C = 0, G = 0;
    int B = 0;
    DevBuf<uint32_t> poly, win, words, st;
    DevBuf<unsigned long long> nz, nzoff, acc, accoff, lastend;
    DevBuf<unsigned long long> res;      // 8 counters + the 624-word end state
    PinnedBuf<unsigned long long> h_io;  // pinned mirror of res (the input window goes out through its state words)
    DevBuf<double> gauss;                // grown by mt_reserve outside trajectories
    double setup_ms = 0.;
  } mt;
  // setup_random_test (mock.hpp): windowed cells per tile, their scan, {windowed cells, first noise == 0 index}
  struct Mock {
    DevBuf<unsigned long long> cnt, off, gsum, goff, res;
  } mock;
  DevBuf<double> spec_bins;                          // measure_spectrum's 3 * n_bin accumulators, the cross-spectrum's 5 * n_bin
  DevBytes cross_ak;                                 // Nhp complex: the first transform of bchmc_measure_cross_spectrum (the
                                                     // second is in tC), taken by its first call and kept like spec_bins
  // bchmc_ensemble_* (ensemble.hpp): the running accumulators.  A slot's arrays are taken by its first add or merge,
  // kept by bchmc_ensemble_reset, freed by bchmc_ensemble_release and bchmc_destroy.
  struct Ens {
    struct Slot {
      uint64_t count = 0;
      DevBuf<double> mean, m2;                       // N doubles each on every handle, cell order k + n (j + n i)
    } slot[BCHMC_ENS_SLOTS];
    int ncu = 0;                                     // compute units of the device (0: not asked yet)
  } ens;
  // bchmc_tweb_* (tweb.hpp): the six real arrays of the tensor, the type map, the partials and the result of the per-type
  // sums are taken by the first classify; the half-complex array by the first one whose source needs a transform (the
  // chain state's q^ is read where it is), the eigenvalue staging by the first that asks for lambda, the counters by the
  // first accumulating call or merge.  All kept until bchmc_tweb_release or bchmc_destroy.
  struct Tweb {
    DevBytes t[6];                       // N elements of T each: xx, xy, xz, yy, yz, zz of the last classify
    DevBytes xk;                         // Nhp complex: x^ of a host or deltaX source (the components go through tC)
    DevBuf<unsigned char> type;          // N
    DevBuf<double> lam;                  // 3 N
    DevBuf<unsigned long long> part;     // (workgroups + 1) * kTwebWords: partials, then the result
    DevBuf<unsigned int> cnt;            // 4 N, type-major: the posterior accumulator
    bool have_t = false;                 // t holds a tensor
    uint64_t samples = 0;
    bool have_par = false;               // R and lambda_th below are set (a merge brings counters, not their parameters)
    double R = 0., lambda_th = 0.;       // of the first sample accumulated by a classify since the last reset
  } tw;
  // bchmc_bispectrum (bispec.hpp): the n_shell real arrays (I_s while the table is built, D_s of the last call after
  // it), the partial sums with the results behind them, and the triangle sums of the shells in `key` (sum I1 I2 I3 per
  // triplet) are taken by the first call and replaced by a call with other shells; the half-complex array by the first
  // call whose source needs a transform.  All kept until bchmc_bispec_release or bchmc_destroy.
  struct Bispec {
    DevBytes d[kBispecMaxShell];         // N elements of T each
    DevBytes xk;                         // Nhp complex: x^ of a host or deltaX source (the shells go through tC)
    DevBuf<double> part;                 // bispec_part_words(): partials of either kernel, then 3 n_shell + T results
    DevBuf<double> tab;                  // T: sum over cells of I_s1 I_s2 I_s3
    bool have_tab = false;               // tab holds the sums of the shells below
    double k_min = 0., dk = 0.;
    int n_shell = 0;
  } bs;
  // measure_corr / measure_corr2d (corr.hpp): accumulators and the geometry of the last n_bin of each function, kept in
  // the handle like spec_bins (the driver measures after every sample with the same n_bin)
  struct Corr1 {
    uint64_t n_bin = 0;                // the geometry below is this bin count's (0: none yet)
    DevBuf<unsigned long long> acc;    // 5 n_bin + 1: { A limbs [2][n_bin], scale, rtot limbs [2][n_bin], counts }
    std::vector<double> rmode;
    std::vector<uint64_t> nmode;
  } corr1;
  struct Corr2 {
    uint64_t n_bin = 0;
    int n = 0;                 // the grid and the cut rpar, rperp < l_max (infinity: none) the tables were built for
    double l_max = 0.;
    DevBuf<int> idx;           // rows sorted by perp bin | par_start [npb + 1] | perp_slice [n_bin + 1]
    DevBuf<int2> slices;       // nsl: { first row, rows }
    DevBuf<double> part;       // nsl * npb
    DevBuf<double> out;        // [2][n_bin * npb]: rtot sums, A sums
    int nrows = 0, nsl = 0, npb = 0, max_rows = 0;
    std::vector<uint64_t> row_cnt, par_cnt;  // rows of a perp bin, cells along z of a populated par bin
    std::vector<int> par_bin;                // nbin_par of populated par bin c
    std::vector<double> rsum;                // n_bin * npb sums of rtot
  } corr2;
  // measure_spec2D (spec2d.hpp): the bin tables of the last n_bin and the sums of ktot on them, kept like corr2's
  struct Spec2 {
    uint64_t n_bin = 0;        // the tables below are this bin count's (0: none yet)
    DevBuf<int> idx;           // rows sorted by perp bin [n^2] | par_start [npb + 1] | perp_slice [n_bin + 1]
    DevBuf<int2> slices;       // nsl: { first row, rows }
    DevBuf<double> part;       // nsl * nh
    DevBuf<double> out;        // n_bin * npb
    int nsl = 0, npb = 0;
    std::vector<uint64_t> row_cnt, par_w;  // rows of a perp bin, sum of hw over the run of k of a populated par bin
    std::vector<int> par_bin;              // nbin_par of populated par bin c
    std::vector<double> ksum;              // n_bin * npb sums of ktot, filled by the first measurement
  } spec2;
  // bchmc_measure_*multipoles (multipoles.hpp): the class tables of the grid, the class sums of the last call (one table,
  // three once the cross form has run), the segment sums of the shell pass, a half-complex array once the cross form's
  // first source has needed a transform, and on the host the geometry of the last n_bin of each form.  Taken on first
  // use, kept until bchmc_multipoles_release or bchmc_destroy.
  struct Mp {
    DevBuf<int> rows;          // kMpRows per class
    DevBuf<int4> cls;          // { m_a, m_b, rows, 0 } per class
    DevBuf<double> part;       // tables * ncls * nh
    DevBuf<double> out;        // (n_bin + 1) * segments * sums
    DevBytes xk;               // Nhp complex
    int ncls = 0;              // 0: no tables yet
    struct Geom {
      uint64_t n_bin = 0;      // the arrays below are this bin count's (0: none yet)
      std::vector<double> tmode, leg;  // n_bin, [2][n_bin]
      std::vector<uint64_t> nmode;
    } fourier, real;
  } mp;
  // bchmc_interp_upres / bchmc_measure_corr2d_interp (upres.hpp): the fine grid of the last n_out, built on first use,
  // kept for the next call with the same n_out, replaced for another one, freed by bchmc_upres_release.  The work buffer
  // is declared before the execution info and the plans that point at it, like the handle's own.
  struct Upres {
    int n_out = 0;             // the grid everything below is for (0: nothing held)
    Geo g{};
    DevBytes real, half;       // N_out elements of T, Nhp_out of C2<T>
    DevBytes work;
    FftInfo info;
    FftPlan r2c, c2r;
    DevBuf<int> cell;          // interp_field's table: i0 [n_out] | i1 [n_out]
    DevBuf<double> dx;         // n_out
    Corr2 bins;                // the 2-D bin tables on the fine grid, keyed by (n_out, n_bin, l_max)
  } up;
  // bchmc_density_particles (catalogue.hpp): one batch of kCatBatch particles at a time -- the staged columns, the tile of
  // every particle, the tile-ordered records, the populations, offsets and fill cursors of the tiles, the work items and
  // the status words with their pinned mirror.  Built by the first call, kept for the next, freed by
  // bchmc_catalogue_release and bchmc_destroy.
  struct Cat {
    DevBuf<double> cols;                 // 4 kCatBatch: x | y | z | w
    DevBuf<int> tile_of;                 // kCatBatch
    DevBuf<CatRec> rec;                  // kCatBatch
    DevBuf<unsigned> cnt, off, cursor;   // ntiles, ntiles + 1, ntiles
    DevBuf<CatItem> items;               // ntiles + kCatBatch / chunk + 1
    DevBuf<unsigned long long> stat;     // kCatWords
    PinnedBuf<unsigned long long> h_stat;
  } cat;
  // bchmc_poisson_* (poisson.hpp): the resident sample is the exclusive scan of the counts and what a particle is
  // recomputed from; the rest is the scan's scratch, the status words and one batch of positions for
  // bchmc_poisson_positions (taken by its first call).  Built by bchmc_poisson_draw for its n_in, replaced by a draw
  // with another one, freed by bchmc_poisson_release and bchmc_destroy.  bchmc_setup_random_test_poisson takes the
  // status words only and leaves the sample alone.
  struct Pois {
    DevBuf<unsigned long long> off;                    // cells + 1
    DevBuf<unsigned long long> cnt, boff, gsum, goff;  // workgroups, workgroups, groups, groups
    DevBuf<unsigned long long> res, stat;              // 2, kPoisWords
    DevBuf<double> cols;                               // 3 kCatBatch: x | y | z
    long long cells = 0;                               // n_in^3 the scan buffers were built for (0: none)
    bool valid = false;                                // a sample is resident
    uint64_t seed = 0, n_part = 0;
    uint32_t stream = 0, n_in = 0;
    double d_in = 0.;
  } pois;
  // bchmc_interp_particles (interp_particles.hpp): the staged sources -- n_fields grid arrays of the storage type, grown
  // when a call asks for more fields -- and one batch of kCatBatch particles at a time: the columns, the results, and for
  // the tile kernel the tile of every particle, the indexed records, the tiles' populations, offsets and cursors and the
  // work items.  None of it is the catalogue's.  Built by the first call, kept for the next, freed by
  // bchmc_interp_release and bchmc_destroy.
  struct Itp {
    DevBytes src;                        // fields_held N elements of T
    int fields_held = 0;
    DevBuf<double> cols;                 // 3 kCatBatch: x | y | z
    DevBuf<double> out;                  // kItpMaxFields kCatBatch, field-major
    DevBuf<int> tile_of;                 // kCatBatch
    DevBuf<ItpRec> rec;                  // kCatBatch
    DevBuf<unsigned> cnt, off, cursor;   // ntiles, ntiles + 1, ntiles
    DevBuf<CatItem> items;               // ntiles + kCatBatch / chunk + 1
    DevBuf<unsigned long long> stat;     // kCatWords
    PinnedBuf<unsigned long long> h_stat;
  } itp;
  // host-array entry points: caller arrays are pageable, so they cross PCIe through two pinned staging chunks
  // (N-thread memcpy into one chunk while the DMA of the other is in flight)
  PinnedBuf<void> stg[2];
  Event stg_ev[2];
  size_t stg_chunk = 0;
  int stg_threads = 1;
  Stream copy_stream;                 // transfers that run beside compute (host-array trajectories: the momenta on their
                                      // way in beside the start-state force, the final q on its way out beside the last one)
  // Early download of a host-array trajectory's q1: the last step only kicks p, so the final q exists one force
  // evaluation before the trajectory ends.  Armed by the host entry points (early_q_dev = where its real-space copy
  // goes); trajectory_fused transforms it there before the last force evaluation and records ev_q; early_q_done says so.
  double *early_q_dev = nullptr;
  bool early_q_done = false;
  Event ev_q;

  DevBuf<int4> hull;
  // tile-sorted particle-mesh path: the partition (plan.tp is what the kernels take) and the state of the record-slot
  // policy, both decided in tile_plan.hpp
  TilePlan plan;
  // "planes" mode of the interior step boundary: 2-D (y, z) transforms by rocFFT, x passes inside k_step_boundary_x
  FftPlan r2c2d, c2r2d;                          // batch 3 n planes
  DevBytes xtw;                                  // n / 2 twiddles exp(-2 pi i r / n), C2<T>
  int log2n = 0;
  bool planes_ok = false;                        // plans + kernel available for this grid
  FftPlan r2c2d_2, c2r2d_2;  // 2-D plans over 2 n planes: delta(1) | Phi and A | B of the ALPT model
  bool alpt_plans_failed = false;
  double alpt_wtot = 0.;     // kernelcomp's normalisation (sum of the real-space kernel), computed on first use
  DevBuf<int> t_cnt, t_woff;                 // 9 ntiles + 2 (one-pass counts per (tile, octant), fallback counts per tile,
                                             // overflow flags), ntiles + 1
  DevBuf<int4> t_oct;                        // 2 ntiles: octant segment starts of every tile (k_scan_tiles)
  DevBuf<int> t_seg;                         // 1: slots per octant segment of the current sort, 0 = contiguous records
  DevBuf<long long> t_off, t_end;                // ntiles each: record range of every tile (ntiles * cap can pass 2^31)
  DevBuf<int2> t_rank;                                         // N
  DevBytes srec;         // tile-sorted particle records { x, y, z, original index | flags }: 4 * sizeof(T) bytes each
  bool sorted_valid = false;
  PinnedBuf<int> h_slots;   // pinned: two snapshots of {sticky overflow stamp, largest population} for those polls
  Event slot_ev[2];
  bool cnt_clean = false;   // t_cnt[0 .. 2 ntiles] was cleared by the last k_scatter_tile81 (no fill launch needed)
  bool have_eval = false;  // rho / psi hold a forward evaluation
  int last_rsd = 0;

  // profiling
  bool prof_on = false;
  std::vector<ProfRec> prof_recs;
  std::vector<Event> ev_pool;
  double prof_ms[BCHMC_K_COUNT] = {0};
  uint64_t prof_n[BCHMC_K_COUNT] = {0};

  int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
};

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return h->fail(BCHMC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define FFTCHK(expr)                                                                    \
  do {                                                                                  \
    rocfft_status s_ = (expr);                                                          \
    if (s_ != rocfft_status_success) return h->fail(BCHMC_ERR_ROCFFT, "%s: status %d", #expr, (int)s_); \
  } while (0)
#define CHK(expr)           \
  do {                      \
    int rc_ = (expr);       \
    if (rc_) return rc_;    \
  } while (0)

namespace {

// DevBuf::alloc / reserve on the handle's stream, zero-filled there (row padding of the half-complex arrays must hold
// finite values); count is in bytes for a DevBytes
int alloc_rc(bchmc_handle *h, hipError_t e, size_t bytes) {
  if (e == hipSuccess) return BCHMC_OK;
  return h->fail(e == hipErrorOutOfMemory ? BCHMC_ERR_NOMEM : BCHMC_ERR_HIP, "device buffer of %zu bytes: %s", bytes,
                 hipGetErrorString(e));
}
template <typename U>
int dev_alloc(bchmc_handle *h, DevBuf<U> &b, size_t count) {
  return alloc_rc(h, b.alloc(count, h->stream), count * b.kElem);
}
template <typename U>
int dev_reserve(bchmc_handle *h, DevBuf<U> &b, size_t count) {
  return alloc_rc(h, b.reserve(count, h->stream), count * b.kElem);
}

// Debug/A-B switches: set to 1 to enable (unset or 0 = off).
inline bool env_on(const char *name) {
  const char *v = std::getenv(name);
  return v && v[0] == '1';
}

// ---- profiling ------------------------------------------------------------------------------------
// roctx range names: the kernel ids of SURVEY.md 2.1 that each launch group replaces, so that a
// `rocprofv3 --marker-trace --kernel-trace` timeline maps onto the reference's kernel inventory.  A push/pop pair
// is a few nanoseconds when no tool is attached.
const char *roctx_name(int cls) {
  static const char *names[BCHMC_K_COUNT] = {
      "F:C2R (fftC2Rplanned)",
      "F:R2C (fftR2Cplanned)",
      "K1+K2+K3+K4+K5 kick|M^-1 p|drift|-D1 q|theta2vel",
      "K6+K7+K8 disp_part|calc_pos_rsd|getDensity",
      "K9+K10 overdens|partial_f_delta_x_log_like",
      "K11 likelihood_calc_V (K15 for calc_h=3)",
      "K12+K13+K1 grad_inv_lap_FS|gradient_psi|kick",
      "tile binning (no reference counterpart)",
      "other (K14 energies, ALPT stencils, state copies)"};
  return (cls >= 0 && cls < BCHMC_K_COUNT) ? names[cls] : "?";
}

struct ProfScope {
  bchmc_handle *h;
  int idx = -1;
  ProfScope(bchmc_handle *h_, int cls) : h(h_) {
    roctxRangePushA(roctx_name(cls));
    if (!h->prof_on) return;
    ProfRec r;
    r.cls = cls;
    for (Event *e : {&r.a, &r.b}) {
      if (!h->ev_pool.empty()) {
        *e = std::move(h->ev_pool.back());
        h->ev_pool.pop_back();
      } else {
        (void)e->create();
      }
    }
    (void)hipEventRecord(r.a, h->stream);
    h->prof_recs.push_back(std::move(r));
    idx = (int)h->prof_recs.size() - 1;
  }
  ~ProfScope() {
    if (idx >= 0) (void)hipEventRecord(h->prof_recs[idx].b, h->stream);
    roctxRangePop();
  }
};

void prof_collect(bchmc_handle *h) {
  for (auto &r : h->prof_recs) {
    float ms = 0.f;
    (void)hipEventSynchronize(r.b);
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    h->prof_ms[r.cls] += ms;
    h->prof_n[r.cls] += 1;
    h->ev_pool.push_back(std::move(r.a));
    h->ev_pool.push_back(std::move(r.b));
  }
  h->prof_recs.clear();
}

// ---- FFT wrapper (unnormalised both ways; callers fold 1/N into the preceding k-space kernel) -------
int fft_exec(bchmc_handle *h, rocfft_plan plan, void *in, void *out, int cls, rocfft_execution_info info = nullptr) {
  ProfScope ps(h, cls);
  void *ib[1] = {in}, *ob[1] = {out};
  FFTCHK(rocfft_execute(plan, ib, ob, info ? info : (rocfft_execution_info)h->info));
  return BCHMC_OK;
}

// ---- parameter packs --------------------------------------------------------------------------------
double E_Hubble_a(double a, double OM, double OL) {  // cosmo.cc:26-31
  const double OK = 1. - OM - OL;
  return std::sqrt(OM / (a * a * a) + OK / (a * a) + OL);
}
double fgrow1(double a, double OM, double OL) {  // cosmo.cc:182-217, term 1
  const double E = E_Hubble_a(a, OM, OL);
  const double Omega = OM / ((E * E) * (a * a * a));
  return std::pow(Omega, 5. / 9.);
}
double c_pecvel1(double a, double OM, double OL) {  // cosmo.cc:220-235
  return fgrow1(a, OM, OL) * 100. * E_Hubble_a(a, OM, OL) * a;
}

PosPar make_pos(const bchmc_handle *h, int rsd) {
  PosPar pp;
  pp.d = h->g.d;
  pp.L = h->g.L;
  pp.rsd = rsd;
  pp.periodic = 1;  // disp_part.cc:28 hard-codes periodic = true
  const double a = h->c.ascale, OM = h->c.OM, OL = h->c.OL;
  pp.cpecvel = c_pecvel1(a, OM, OL);
  const double Hub = 100. * std::sqrt(OM / a / a / a + OL + (1. - OM - OL) / a / a);  // rsd.cc:26-27
  pp.v_norm = 1. / Hub / a;
  return pp;
}

SphPar make_sph(const bchmc_handle *h) {
  SphPar sp;
  sp.h = h->c.particle_kernel_h;
  sp.h_inv = 1. / sp.h;
  sp.w_norm = 1. / M_PI / (sp.h * sp.h * sp.h);
  sp.r2_lim = 4. * sp.h * sp.h * (1. + (h->f32 ? 1e-5 : 1e-12));
  sp.min1 = h->c.min1;
  sp.min2 = h->c.min2;
  sp.min3 = h->c.min3;
  sp.reach = h->plan.reach;
  return sp;
}

LikePar make_like(const bchmc_handle *h) {
  LikePar lp;
  lp.rho_c = h->c.rho_c;
  lp.biasP = h->c.biasP;
  lp.biasE = h->c.biasE;
  lp.delta_min = h->c.delta_min;
  lp.likelihood = h->c.likelihood;
  lp.bias_is_identity = (h->c.biasE == 1.0);
  return lp;
}

HullPar make_hull(const bchmc_handle *h) {
  HullPar hp;
  const double hh = h->c.particle_kernel_h;
  hp.cols = h->hull;
  hp.ncol = h->plan.hull_n;
  hp.h_inv = 1. / hh;
  hp.d_h = h->g.d * hp.h_inv;
  hp.norm = 1. / (M_PI * (hh * hh) * (hh * hh));
  hp.normalize = h->c.rho_c * h->g.L * h->g.L * h->g.L / (double)h->g.N;
  hp.f1 = fgrow1(h->c.ascale, h->c.OM, h->c.OL);
  return hp;
}

int need_input(bchmc_handle *h, int f, const char *name) {
  if (!h->have[f]) return h->fail(BCHMC_ERR_STATE, "input array %s was never uploaded", name);
  return BCHMC_OK;
}

// Where bchmc_fetch takes a field from, or why it cannot: the one statement of it, for Pipe::fetch and for an entry point
// that must refuse before anything is queued.  A field that a kernel makes first lands in ioq.
struct FieldSource {
  enum Made { kAsHeld, kOverdens, kPositions, kVrec };
  void *base = nullptr;  // the buffer, in the storage type
  size_t offset = 0;     // elements into it
  Made made = kAsHeld;
};
int field_source(bchmc_handle *h, int field, FieldSource *fs) {
  const size_t N = (size_t)h->g.N;
  *fs = FieldSource{};
  switch (field) {
    case BCHMC_F_SIGNAL_PS: case BCHMC_F_MASS_F: case BCHMC_F_MASS_R:
    case BCHMC_F_NOBS: case BCHMC_F_NOISE: case BCHMC_F_WINDOW:
      fs->base = h->in_arr[field].get();
      break;
    case BCHMC_F_DELTAX: fs->base = h->ioq.get(), fs->made = FieldSource::kOverdens; break;
    case BCHMC_F_POSX: case BCHMC_F_POSY: case BCHMC_F_POSZ: fs->base = h->ioq.get(), fs->made = FieldSource::kPositions; break;
    case BCHMC_F_RHO: fs->base = h->rho.get(); break;
    case BCHMC_F_PART_LIKE: fs->base = h->plike.get(); break;
    case BCHMC_F_VX: case BCHMC_F_VY: case BCHMC_F_VZ:
      if (h->v_in_vrec) fs->base = h->ioq.get(), fs->made = FieldSource::kVrec;  // the gather left records: unpacked into ioq
      else fs->base = h->V.get(), fs->offset = (size_t)(field - BCHMC_F_VX) * N;
      break;
    case BCHMC_F_PSIX: case BCHMC_F_PSIY: case BCHMC_F_PSIZ:
      fs->base = h->psi.get(), fs->offset = (size_t)(field - BCHMC_F_PSIX) * N;
      break;
    case BCHMC_F_GRAD_PRIOR: fs->base = h->gprior.get(); break;
    case BCHMC_F_GRAD_LIKE: fs->base = h->glike.get(); break;
    default: return h->fail(BCHMC_ERR_ARG, "unknown field %d", field);
  }
  if (!fs->base) return h->fail(BCHMC_ERR_STATE, "field %d has not been computed", field);
  return BCHMC_OK;
}
// bchmc_fetch's refusals of a field, all of them: the outputs of a forward evaluation need one
int fetch_ready(bchmc_handle *h, int field) {
  if (field >= BCHMC_F_DELTAX && field <= BCHMC_F_PSIZ && !h->have_eval)
    return h->fail(BCHMC_ERR_STATE, "no forward evaluation to fetch from");
  FieldSource fs;
  return field_source(h, field, &fs);
}

int check_inputs(bchmc_handle *h) {
  CHK(need_input(h, BCHMC_F_SIGNAL_PS, "signal_PS"));
  if (h->mass_fs) CHK(need_input(h, BCHMC_F_MASS_F, "mass_f"));
  if (h->mass_rs) CHK(need_input(h, BCHMC_F_MASS_R, "mass_r"));
  CHK(need_input(h, BCHMC_F_NOBS, "nobs"));
  CHK(need_input(h, BCHMC_F_WINDOW, "window"));
  if (h->c.likelihood != 0) CHK(need_input(h, BCHMC_F_NOISE, "noise"));
  return BCHMC_OK;
}

// One-pass tile binning, sizing of the record slots: the rules are SlotPolicy's (tile_plan.hpp).  Here the slot words are
// read wherever the host synchronises anyway (read_ctl: bchmc_steps_done, bchmc_sync, bchmc_forward, the end of a chain
// attempt) and by a lagging poll inside a trajectory (poll_slots), and what the policy asks for is carried out.
RecQuad *recs(const bchmc_handle *h) { return static_cast<RecQuad *>(h->srec.get()); }  // the records, as the kernels take them
int *slot_words(bchmc_handle *h) { return h->t_cnt + (kOct + 1) * (size_t)h->plan.tp.ntiles + 1; }  // {sticky stamp, max}

void repartition(bchmc_handle *h) {
  h->plan.tp.cap = h->plan.slots.cap;
  h->sorted_valid = false;
}

int realloc_slots(bchmc_handle *h, long long want) {
  HIPCHK(hipStreamSynchronize(h->stream));  // rare path: the record slots are about to be replaced
  SlotPolicy &sl = h->plan.slots;
  const bool verbose = env_on("BCHMC_VERBOSE");
  const long long cap = sl.clamp_to_budget(want);
  if (!cap) {
    if (verbose) fprintf(stderr, "bchmc: record slots stay at %lld per tile (memory budget %lld): overflowing evaluations "
                                 "run the two-pass sort\n", sl.cap_alloc, sl.cap_budget);
    sl.after_realloc(SlotGot::kOldSize, cap);
    return BCHMC_OK;
  }
  // The old array goes first (its contents are rebuilt by the next binning anyway): at 512^3 fp64 it is 69 GB, and the
  // new one next to it would not fit.
  (void)h->srec.release();
  h->sorted_valid = false;
  for (SlotGot got : {SlotGot::kWanted, SlotGot::kOldSize, SlotGot::kRecordsOnly}) {
    const size_t nrec = record_count(h->g.N, sl.rung(got, cap), h->plan.tp.ntiles);
    if (h->srec.alloc(nrec * 4 * h->esz) == hipSuccess) {
      if (got == SlotGot::kWanted) {
        if (verbose) fprintf(stderr, "bchmc: record array reallocated for %lld slots per tile\n", cap);
      } else {
        if (verbose) fprintf(stderr, "bchmc: no memory for %lld record slots per tile: %s\n", cap,
                             got == SlotGot::kOldSize ? "kept the old size, overflowing steps run the two-pass sort"
                                                      : "one-pass binning given up");
      }
      sl.after_realloc(got, cap);
      return BCHMC_OK;
    }
    (void)hipGetLastError();
  }
  return h->fail(BCHMC_ERR_NOMEM, "no device memory for the particle records");
}

int adapt_slots(bchmc_handle *h, int sticky, int maxc, bool may_realloc) {
  if (!h->plan.tiled) return BCHMC_OK;
  SlotPolicy &sl = h->plan.slots;
  const int old = sl.cap;
  const SlotAction a = sl.observe(sticky, maxc, may_realloc);
  if (a.kind == SlotAction::kRealloc) CHK(realloc_slots(h, a.cap));  // the partition follows the array
  if (sl.cap == old) return BCHMC_OK;
  if (env_on("BCHMC_VERBOSE"))
    fprintf(stderr, "bchmc: record slots per tile %d -> %lld (largest (tile, octant) population %d%s)\n", old,
            (long long)sl.cap, maxc, a.overflowed ? ", a segment overflowed" : "");
  repartition(h);
  return BCHMC_OK;
}

// The host's view of the device-side trajectory control; synchronises the stream.  Also where the binning's slot words
// are read and acted upon (adapt_slots), while the host is waiting anyway.
int read_ctl(bchmc_handle *h, unsigned long long *steps_done) {
  unsigned long long sd = 0;
  int words[2] = {0, 0}, sat = 0;
  const bool slots = h->plan.tiled && h->plan.slots.sort_direct;
  if (steps_done) HIPCHK(hipMemcpyAsync(&sd, h->steps_done, sizeof sd, hipMemcpyDeviceToHost, h->stream));
  if (h->fix_sat) HIPCHK(hipMemcpyAsync(&sat, h->fix_sat, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (slots) HIPCHK(hipMemcpyAsync(words, slot_words(h), sizeof words, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (steps_done) *steps_done = sd;
  if (slots) {
    if (words[0] || words[1]) HIPCHK(hipMemsetAsync(slot_words(h), 0, sizeof words, h->stream));
    if (const long long want = h->plan.slots.pending()) {  // a poll inside a trajectory could not grow the array: do it now
      CHK(realloc_slots(h, want));
      repartition(h);
    }
    CHK(adapt_slots(h, words[0], words[1], true));
  }
  if (sat) {
    HIPCHK(hipMemsetAsync(h->fix_sat, 0, sizeof(int), h->stream));
    return h->fail(BCHMC_ERR_STATE,
                   "deterministic mode: a density cell exceeded the fixed-point range (more than 2^16 maximal "
                   "contributions in one cell); the results since the last read-back are not valid");
  }
  return BCHMC_OK;
}

// Inside a trajectory (slot_watch only): poll k enqueues snapshot k of the slot words and acts on snapshot k - 1, which
// the device finished at least kSlotPoll steps ago unless the host ran far ahead -- then the wait below throttles the
// host to at most 2 kSlotPoll queued steps, never the device.  Re-partitions within the allocation only.
constexpr uint64_t kSlotPoll = 4;
int poll_slots(bchmc_handle *h, uint64_t k) {
  if (!h->h_slots) {
    HIPCHK(h->h_slots.alloc(4));
    for (Event &e : h->slot_ev) HIPCHK(e.create(hipEventDisableTiming));
  }
  if (k >= 2) {
    const int b = (int)((k - 1) & 1);
    HIPCHK(hipEventSynchronize(h->slot_ev[b]));
    CHK(adapt_slots(h, h->h_slots[2 * b], h->h_slots[2 * b + 1], false));
  }
  const int b = (int)(k & 1);
  HIPCHK(hipMemcpyAsync(h->h_slots + 2 * b, slot_words(h), 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemsetAsync(slot_words(h), 0, 2 * sizeof(int), h->stream));
  HIPCHK(hipEventRecord(h->slot_ev[b], h->stream));
  return BCHMC_OK;
}

// Batched 2-D (y, z) real transforms over `batch` consecutive planes of the padded half-complex layout (planes mode).
// Optional fast path: on failure both plans are left null and the batched 3-D plans carry the work.
int make_plans_2d(bchmc_handle *h, size_t batch, FftPlan &r2c, FftPlan &c2r) {
  const Geo &g = h->g;
  const rocfft_precision prec = h->f32 ? rocfft_precision_single : rocfft_precision_double;
  const size_t len2[2] = {(size_t)g.n, (size_t)g.n};
  const size_t rs2[2] = {1, (size_t)g.n}, cs2[2] = {1, (size_t)g.nhp};
  rocfft_plan_description f2 = nullptr, i2 = nullptr;
  bool ok2 = rocfft_plan_description_create(&f2) == rocfft_status_success &&
             rocfft_plan_description_create(&i2) == rocfft_status_success;
  ok2 = ok2 && rocfft_plan_description_set_data_layout(f2, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved,
                                                       nullptr, nullptr, 2, rs2, (size_t)g.n * g.n, 2, cs2,
                                                       (size_t)g.n * g.nhp) == rocfft_status_success;
  ok2 = ok2 && rocfft_plan_description_set_data_layout(i2, rocfft_array_type_hermitian_interleaved, rocfft_array_type_real,
                                                       nullptr, nullptr, 2, cs2, (size_t)g.n * g.nhp, 2, rs2,
                                                       (size_t)g.n * g.n) == rocfft_status_success;
  ok2 = ok2 && r2c.create(rocfft_plan_create, rocfft_placement_notinplace, rocfft_transform_type_real_forward, prec, 2,
                          len2, batch, f2) == rocfft_status_success;
  ok2 = ok2 && c2r.create(rocfft_plan_create, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, prec, 2,
                          len2, batch, i2) == rocfft_status_success;
  if (f2) rocfft_plan_description_destroy(f2);
  if (i2) rocfft_plan_description_destroy(i2);
  if (ok2 && h->info) {
    // plans made after bchmc_create: the shared work buffer may have to grow
    size_t need = 0;
    for (const FftPlan *p : {&r2c, &c2r}) {
      size_t wb = 0;
      if (rocfft_plan_get_work_buffer_size(*p, &wb) != rocfft_status_success) ok2 = false;
      need = std::max(need, wb);
    }
    if (ok2 && need > h->work.capacity()) {
      // not DevBuf::reserve: the execution info points at the old buffer until it has been given the new one
      DevBytes nw;
      (void)hipStreamSynchronize(h->stream);
      if (nw.alloc(need) == hipSuccess &&
          rocfft_execution_info_set_work_buffer(h->info, nw, need) == rocfft_status_success) {
        h->work = std::move(nw);
      } else {
        (void)hipGetLastError();
        ok2 = false;
      }
    }
  }
  if (!ok2) {
    r2c.reset();
    c2r.reset();
    return BCHMC_ERR_ROCFFT;
  }
  return BCHMC_OK;
}

// The path switches of eval_plan.hpp from the environment: bchmc_create's, once per handle.
PathSwitches read_path_switches() {
  PathSwitches s;
  s.no_planes = env_on("BCHMC_NO_PLANES");
  s.no_planes_ends = env_on("BCHMC_NO_PLANES_ENDS");
  s.no_fuse = env_on("BCHMC_NO_FUSE");
  s.no_alpt_planes = env_on("BCHMC_NO_ALPT_PLANES");
  s.no_zbin = env_on("BCHMC_NO_ZBIN");
  s.zbin_128 = env_on("BCHMC_ZBIN_128");
  s.yfwd_f64 = env_on("BCHMC_YFWD_F64");
  s.bx_v1 = env_on("BCHMC_BX_V1");
  s.bx_v2 = env_on("BCHMC_BX_V2");
  s.no_pair = env_on("BCHMC_NO_PAIR");
  s.no_vpair = env_on("BCHMC_NO_VPAIR");
  s.no_vrec = env_on("BCHMC_NO_VREC");
  s.no_xtile = env_on("BCHMC_NO_XTILE");
  return s;
}

// What eval_plan.hpp's decisions read, as the handle is now; gathered for every decision, never kept.  rsd: of the forward
// evaluation the caller is deciding (a trajectory's and everything else's: the configuration's rsd_model).  The only place
// that makes the ALPT pipeline's plans over 2 n planes late: a forward evaluation that wants them and finds none --
// bchmc_forward or a log-likelihood without RSD on a handle configured with it; bchmc_create made them for rsd_model.
PathFacts path_facts(bchmc_handle *h, int rsd) {
  PathFacts f;
  f.n = h->g.n, f.esz = (int)h->esz, f.Nhp = h->g.Nhp;
  f.planes_ok = h->planes_ok && h->xtw;
  f.tiled = h->plan.tiled, f.sort_direct = h->plan.slots.sort_direct, f.std81 = h->plan.std81;
  f.mk = h->c.mk, f.calc_h = h->c.calc_h, f.likelihood = h->c.likelihood, f.sfmodel = h->c.sfmodel;
  f.rsd_model = h->c.rsd_model, f.mass_rs = h->mass_rs != 0, f.mass_fs = h->mass_fs != 0;
  if (alpt_planes_wanted(f, h->sw, rsd) && !h->c2r2d_2 && !h->alpt_plans_failed &&
      make_plans_2d(h, 2 * (size_t)h->g.n, h->r2c2d_2, h->c2r2d_2) != BCHMC_OK)
    h->alpt_plans_failed = true;
  f.alpt_plans = h->c2r2d_2 != nullptr;
  return f;
}

// Sum kRedBlocks device partials on the host (synchronises the stream).
int host_sum(bchmc_handle *h, const double *d_part, double *out) {
  HIPCHK(hipMemcpyAsync(h->h_part, d_part, kRedBlocks * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  double s = 0.;
  for (int i = 0; i < kRedBlocks; i++) s += h->h_part[i];
  *out = s;
  return BCHMC_OK;
}

// ---- host <-> device copies of the ABI's arrays ---------------------------------------------------------------
// The reference hands over plain heap arrays (fftw_array, call_hamil.cc:38 / HMC.cc:375).  hipMemcpy from pageable
// memory runs far below the link rate (profiles/r02_h2d_bench.txt), so both directions go through two pinned chunks:
// several host threads copy chunk c while the DMA engine moves chunk c - 1.
void par_memcpy(void *dst, const void *src, size_t bytes, int nt) {
  if (nt <= 1 || bytes < ((size_t)4 << 20)) {
    std::memcpy(dst, src, bytes);
    return;
  }
  std::vector<std::thread> th;
  const size_t per = ((bytes / (size_t)nt) + 4095) & ~(size_t)4095;
  for (int t = 1; t < nt; t++) {
    const size_t off = per * (size_t)t;
    if (off >= bytes) break;
    const size_t len = std::min(per, bytes - off);
    th.emplace_back([=] { std::memcpy((char *)dst + off, (const char *)src + off, len); });
  }
  std::memcpy(dst, src, std::min(per, bytes));
  for (auto &t : th) t.join();
}

int stg_init(bchmc_handle *h) {
  if (h->stg[0]) return BCHMC_OK;
  size_t chunk = (size_t)16 << 20;
  if (const char *ev = std::getenv("BCHMC_STAGE_MB")) chunk = (size_t)std::max(1, atoi(ev)) << 20;
  int nt = (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency() / 2));
  if (const char *ev = std::getenv("BCHMC_STAGE_THREADS")) nt = std::max(1, atoi(ev));
  for (int b = 0; b < 2; b++) {
    HIPCHK(h->stg[b].alloc(chunk));
    HIPCHK(h->stg_ev[b].create(hipEventDisableTiming));
  }
  h->stg_chunk = chunk;
  h->stg_threads = nt;
  return BCHMC_OK;
}

// host -> device, enqueued on the handle's stream; returns once the host array has been read completely (the caller
// may reuse it), the last DMA chunks may still be in flight on the stream
int h2d(bchmc_handle *h, void *dst, const void *src, size_t bytes, hipStream_t stream = nullptr) {
  if (!stream) stream = h->stream;
  if (bytes <= ((size_t)1 << 20)) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return BCHMC_OK;
  }
  CHK(stg_init(h));
  const size_t chunk = h->stg_chunk;
  const size_t nch = (bytes + chunk - 1) / chunk;
  for (size_t c = 0; c < nch; c++) {
    const int b = (int)(c & 1);
    const size_t off = c * chunk, len = std::min(chunk, bytes - off);
    if (c >= 2) HIPCHK(hipEventSynchronize(h->stg_ev[b]));  // DMA of chunk c - 2 has left this buffer
    par_memcpy(h->stg[b], (const char *)src + off, len, h->stg_threads);
    HIPCHK(hipMemcpyAsync((char *)dst + off, h->stg[b], len, hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(h->stg_ev[b], stream));
  }
  // the staging buffers are reused by the next call: wait for the two DMAs still in flight
  HIPCHK(hipEventSynchronize(h->stg_ev[0]));
  if (nch > 1) HIPCHK(hipEventSynchronize(h->stg_ev[1]));
  return BCHMC_OK;
}

// device -> host after everything enqueued so far on the handle's stream; returns when `dst` is complete
// (stream: the transfers go there instead, after `after` has happened -- the early download of q1)
int d2h(bchmc_handle *h, void *dst, const void *src, size_t bytes, hipStream_t stream = nullptr,
        hipEvent_t after = nullptr) {
  if (!stream) stream = h->stream;
  if (after) HIPCHK(hipStreamWaitEvent(stream, after, 0));
  if (bytes <= ((size_t)1 << 20)) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return BCHMC_OK;
  }
  CHK(stg_init(h));
  const size_t chunk = h->stg_chunk;
  const size_t nch = (bytes + chunk - 1) / chunk;
  for (size_t c = 0; c <= nch; c++) {
    const int b = (int)(c & 1);
    if (c < nch) {
      const size_t off = c * chunk, len = std::min(chunk, bytes - off);
      HIPCHK(hipMemcpyAsync(h->stg[b], (const char *)src + off, len, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipEventRecord(h->stg_ev[b], stream));
    }
    if (c >= 1) {
      const size_t off = (c - 1) * chunk, len = std::min(chunk, bytes - off);
      HIPCHK(hipEventSynchronize(h->stg_ev[b ^ 1]));
      par_memcpy((char *)dst + off, h->stg[b ^ 1], len, h->stg_threads);
    }
  }
  return BCHMC_OK;
}

// Fourier transform of the SPH kernel on the half-complex grid (HMC_models_testing.cpp:96-111), host libm.
int build_conv_table(bchmc_handle *h) {
  const Geo &g = h->g;
  const double hh = h->c.particle_kernel_h;
  const double norm = (24. / (hh * hh * hh)) * (h->c.rho_c * g.L * g.L * g.L / (double)((size_t)g.n * g.n * g.n));
  std::vector<double> F((size_t)g.Nhp);
  auto kv = [&](int i) { return (i <= g.n / 2) ? g.kfac * (double)i : -g.kfac * (double)(g.n - i); };
  for (int i = 0; i < g.n; ++i) {
    const double kx = kv(i);
    for (int j = 0; j < g.n; ++j) {
      const double ky = kv(j);
      for (int k = 0; k < g.nh; ++k) {
        const double kz = kv(k);
        const double k_sq = kx * kx + ky * ky + kz * kz;
        double f;
        if (k_sq == 0.) {
          f = 1. / (hh * hh * hh);
        } else {
          const double kk = std::sqrt(k_sq);
          const double ksink = kk * std::sin(kk);
          f = norm * (3 + std::cos(2 * kk) - ksink + std::cos(kk) * (ksink - 4)) / (k_sq * k_sq * k_sq);
        }
        F[k + (size_t)g.nhp * (j + (size_t)g.n * i)] = f;
      }
    }
  }
  CHK(dev_alloc(h, h->convF, (size_t)g.Nhp));
  HIPCHK(hipMemcpyAsync(h->convF, F.data(), F.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // F is a local vector
  return BCHMC_OK;
}

// measure_spectrum's bin width |k|_max / n_bin (field_statistics.cpp:37-39)
double spectrum_dk(const Geo &g, uint64_t n_bin) {
  const double knyq = g.kfac * (double)(g.n / 2);
  const double kmax = std::sqrt(knyq * knyq + knyq * knyq + knyq * knyq);
  return kmax / (double)n_bin;
}

// measure_spectrum (field_statistics.cpp:20-90) of a half-complex transform xk in the handle's storage type: n_bin
// bins, Hermitian mode weights (k_spectrum); kmode / power on the host, empty bins 0.  Synchronises.
int spectrum_bins(bchmc_handle *h, const void *xk, uint64_t n_bin, double *kmode, double *power) {
  CHK(dev_reserve(h, h->spec_bins, 3 * (size_t)n_bin));  // kept in the handle: barcoderunner measures after every sample
  double *bins = h->spec_bins;
  HIPCHK(hipMemsetAsync(bins, 0, 3 * (size_t)n_bin * sizeof(double), h->stream));
  const Geo &g = h->g;
  const double dk = spectrum_dk(g, n_bin);
  const int grid = std::min(nblk_stride(g.Nhp), 512);
  if (h->f32)
    k_spectrum<float><<<grid, 256, 3 * n_bin * sizeof(double), h->stream>>>(
        g, reinterpret_cast<const float2 *>(xk), (int)n_bin, dk, bins);
  else
    k_spectrum<double><<<grid, 256, 3 * n_bin * sizeof(double), h->stream>>>(
        g, reinterpret_cast<const double2 *>(xk), (int)n_bin, dk, bins);
  std::vector<double> hb(3 * n_bin);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), bins, hb.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return h->fail(BCHMC_ERR_HIP, "measure_spectrum: %s", hipGetErrorString(e));
  const double N = (double)g.N, NORM = g.L * g.L * g.L / N / N;  // FOURIER_DEF_2, field_statistics.cpp:73-75
  for (uint64_t l = 0; l < n_bin; l++) {
    const double cnt = hb[2 * n_bin + l];
    kmode[l] = cnt > 0. ? hb[l] / cnt : 0.;
    power[l] = cnt > 0. ? hb[n_bin + l] / cnt * NORM : 0.;
  }
  return BCHMC_OK;
}

// The cross-spectrum of two half-complex transforms in measure_spectrum's bins (k_cross_spectrum): per bin kmode, nmode
// (may be null), both auto powers normalised as spectrum_bins normalises its one, cross = the same of Re(A conj B), and
// coeff = cross / sqrt(power_a power_b) from those three (0 for an empty bin or a zero product, NaN for a NaN one).
// Synchronises.
int cross_bins(bchmc_handle *h, const void *ak, const void *bk, uint64_t n_bin, double *kmode, uint64_t *nmode,
               double *power_a, double *power_b, double *cross, double *coeff) {
#pragma clang fp contract(off)
  CHK(dev_reserve(h, h->spec_bins, kCrossSums * (size_t)n_bin));
  double *bins = h->spec_bins;
  const size_t lds = kCrossSums * (size_t)n_bin * sizeof(double);
  HIPCHK(hipMemsetAsync(bins, 0, lds, h->stream));
  const Geo &g = h->g;
  const double dk = spectrum_dk(g, n_bin);
  const int grid = std::min(nblk_stride(g.Nhp), 512);
  if (h->f32) {
    if (lds > ((size_t)48 << 10))  // 2048 bins are 80 KiB of the CU's 160
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cross_spectrum<float>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k_cross_spectrum<float><<<grid, 256, lds, h->stream>>>(g, reinterpret_cast<const float2 *>(ak),
                                                           reinterpret_cast<const float2 *>(bk), (int)n_bin, dk, bins);
  } else {
    if (lds > ((size_t)48 << 10))
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cross_spectrum<double>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k_cross_spectrum<double><<<grid, 256, lds, h->stream>>>(g, reinterpret_cast<const double2 *>(ak),
                                                            reinterpret_cast<const double2 *>(bk), (int)n_bin, dk, bins);
  }
  std::vector<double> hb(kCrossSums * n_bin);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), bins, hb.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return h->fail(BCHMC_ERR_HIP, "measure_cross_spectrum: %s", hipGetErrorString(e));
  const double N = (double)g.N, NORM = g.L * g.L * g.L / N / N;  // FOURIER_DEF_2, field_statistics.cpp:73-75
  for (uint64_t l = 0; l < n_bin; l++) {
    const double cnt = hb[4 * n_bin + l];
    const bool pop = cnt > 0.;
    kmode[l] = pop ? hb[l] / cnt : 0.;
    if (nmode) nmode[l] = pop ? (uint64_t)cnt : 0;
    power_a[l] = pop ? hb[n_bin + l] / cnt * NORM : 0.;
    power_b[l] = pop ? hb[2 * n_bin + l] / cnt * NORM : 0.;
    cross[l] = pop ? hb[3 * n_bin + l] / cnt * NORM : 0.;
    const double pp = power_a[l] * power_b[l];
    coeff[l] = (pop && pp != 0.) ? cross[l] / std::sqrt(pp) : 0.;
  }
  return BCHMC_OK;
}

// The correlation tools' bin width rmax / n_bin, rmax = L/2 sqrt(3) (2D_corr_fct.cc:35-39), in this order on the host
double corr_dr(const Geo &g, uint64_t n_bin) {
  const double rmax = g.L / 2 * std::sqrt(3.);
  return rmax / (double)n_bin;
}

// measure_corr2D's geometry for n_bin, built when n_bin changes: the rows (i, j) sorted by nbin_perp and cut into slices,
// the runs of |z| that make up the populated par bins, the counts (products of the two), and on the device the sums of
// rtot.  The bin indices are computed here exactly as the tool does (IEEE sqrt and divide, no FMA contraction).
// `c`, `g`: the handle's own tables and grid, or those of the fine grid of 2D_corr_fct_interp.cc, whose measure_corr2D
// bins a cell only if rpar < L_max && rperp < L_max (:123, both strict): rows with rperp >= l_max leave the row list and
// the par runs stop at the first kk with rpar >= l_max (rpar grows with kk).  l_max = infinity: no cut.
// Synchronises (the tables are uploaded from local vectors).
int corr2d_setup(bchmc_handle *h, bchmc_handle::Corr2 &c, const Geo &g, uint64_t n_bin, double l_max) {
#pragma clang fp contract(off)
  if (c.n_bin == n_bin && c.n == g.n && c.l_max == l_max) return BCHMC_OK;
  const int n = g.n;
  const double dr = corr_dr(g, n_bin);
  HIPCHK(hipStreamSynchronize(h->stream));
  c.n_bin = 0;
  // rows by perp bin: a counting sort that keeps the row order inside a bin
  std::vector<int> perp((size_t)n * n);
  c.row_cnt.assign(n_bin, 0);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      const double x = corr_pos(i, n, g.d), y = corr_pos(j, n, g.d);
      const double rperp = std::sqrt(x * x + y * y);
      const unsigned long long b = (unsigned long long)(rperp / dr);
      const bool in = rperp < l_max && b < n_bin;
      perp[(size_t)i * n + j] = in ? (int)b : -1;
      if (in) c.row_cnt[b]++;
    }
  std::vector<int> first(n_bin + 1, 0);
  for (uint64_t p = 0; p < n_bin; p++) first[p + 1] = first[p] + (int)c.row_cnt[p];
  c.nrows = first[n_bin];
  std::vector<int> rows((size_t)std::max(c.nrows, 1)), fill(first.begin(), first.end() - 1);
  for (int r = 0; r < n * n; r++)
    if (perp[r] >= 0) rows[fill[perp[r]]++] = r;
  // slices of one perp bin: enough of them to fill the device, few enough that a slice amortises its combine step
  const int per = std::max(8, std::min(64, n * n / 2048));
  std::vector<int2> slices;
  std::vector<int> perp_slice(n_bin + 1, 0);
  c.max_rows = 0;
  for (uint64_t p = 0; p < n_bin; p++) {
    perp_slice[p] = (int)slices.size();
    for (int o = 0; o < (int)c.row_cnt[p]; o += per) slices.push_back(make_int2(first[p] + o, std::min(per, (int)c.row_cnt[p] - o)));
    c.max_rows = std::max(c.max_rows, (int)c.row_cnt[p]);
  }
  perp_slice[n_bin] = (int)slices.size();
  c.nsl = (int)slices.size();
  // populated par bins: nbin_par is monotone in kk = min(k, n - k), so every bin is one run of kk
  std::vector<int> par_start;
  c.par_bin.clear();
  c.par_cnt.clear();
  int kk = 0;
  for (; kk <= n / 2; kk++) {
    const double z = corr_pos(kk, n, g.d);
    const double rpar = std::sqrt(z * z);
    const unsigned long long b = (unsigned long long)(rpar / dr);
    if (!(rpar < l_max) || b >= n_bin) break;
    if (c.par_bin.empty() || c.par_bin.back() != (int)b) {
      par_start.push_back(kk);
      c.par_bin.push_back((int)b);
      c.par_cnt.push_back(0);
    }
    c.par_cnt.back() += (kk == 0 || kk == n - kk) ? 1 : 2;
  }
  par_start.push_back(kk);
  c.npb = (int)c.par_bin.size();
  if (c.nsl == 0 || c.npb == 0) return h->fail(BCHMC_ERR_STATE, "measure_corr2d: no populated bin");
  std::vector<int> idx(rows.begin(), rows.begin() + c.nrows);
  idx.insert(idx.end(), par_start.begin(), par_start.end());
  idx.insert(idx.end(), perp_slice.begin(), perp_slice.end());
  CHK(dev_alloc(h, c.idx, idx.size()));
  CHK(dev_alloc(h, c.slices, slices.size()));
  CHK(dev_alloc(h, c.part, (size_t)c.nsl * c.npb));
  CHK(dev_alloc(h, c.out, 2 * (size_t)n_bin * c.npb));
  HIPCHK(hipMemcpyAsync(c.idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(c.slices, slices.data(), slices.size() * sizeof(int2), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // idx and slices are local vectors
  c.rsum.clear();  // filled by the first measurement
  c.n_bin = n_bin;
  c.n = n;
  c.l_max = l_max;
  return BCHMC_OK;
}

// measure_spec2D's bin width (2D_powspec.cc:40-43): |k|_max / (N_bin - 1), +infinity for N_bin = 1 (property S2)
double spec2d_dk(const Geo &g, uint64_t n_bin) {
#pragma clang fp contract(off)
  const double knyq = g.kfac * (double)(g.n / 2);
  const double kmax = std::sqrt(knyq * knyq + knyq * knyq + knyq * knyq);
  return kmax / (double)(n_bin - 1);
}

// measure_spec2D's tables for n_bin on the handle's half-complex layout, built when n_bin changes: the rows (i, j) sorted
// by nbin_perp and cut into slices, the runs of k <= n / 2 that make up the populated par bins, and the mode counts
// (rows of the perp bin times the Hermitian weights of the run).  The bin indices are computed here exactly as the tool
// does (IEEE sqrt and divide, no FMA contraction).  Every mode is binned (S2), so every row is in the list and the runs
// cover 0 .. n / 2.  Synchronises (the tables are uploaded from local vectors).
int spec2d_setup(bchmc_handle *h, uint64_t n_bin) {
#pragma clang fp contract(off)
  auto &c = h->spec2;
  if (c.n_bin == n_bin) return BCHMC_OK;
  const Geo &g = h->g;
  const int n = g.n;
  const double dk = spec2d_dk(g, n_bin);
  auto kv = [&](int i) { return (i <= n / 2) ? g.kfac * (double)i : -g.kfac * (double)(n - i); };  // calc_ki
  HIPCHK(hipStreamSynchronize(h->stream));
  c.n_bin = 0;
  // rows by perp bin: a counting sort that keeps the row order inside a bin
  std::vector<int> perp((size_t)n * n);
  c.row_cnt.assign(n_bin, 0);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      const double kx = kv(i), ky = kv(j);
      const double kperp = std::sqrt(kx * kx + ky * ky);
      const unsigned long long b = (unsigned long long)(kperp / dk);
      if (b >= n_bin) return h->fail(BCHMC_ERR_STATE, "measure_spectrum2d: perp bin %llu of row (%d, %d) >= n_bin", b, i, j);
      perp[(size_t)i * n + j] = (int)b;
      c.row_cnt[b]++;
    }
  std::vector<int> first(n_bin + 1, 0);
  for (uint64_t p = 0; p < n_bin; p++) first[p + 1] = first[p] + (int)c.row_cnt[p];
  std::vector<int> idx((size_t)n * n), fill(first.begin(), first.end() - 1);
  for (int r = 0; r < n * n; r++) idx[fill[perp[r]]++] = r;
  // slices of one perp bin: enough workgroups to fill the device, few enough partial rows to keep the reduce short, and
  // at least kSpecUnroll rows for every wave of a full slice
  const int per = std::max(kSpecWaves * kSpecUnroll, std::min(256, n * n / 2048));
  std::vector<int2> slices;
  std::vector<int> perp_slice(n_bin + 1, 0);
  for (uint64_t p = 0; p < n_bin; p++) {
    perp_slice[p] = (int)slices.size();
    for (int o = 0; o < (int)c.row_cnt[p]; o += per) slices.push_back(make_int2(first[p] + o, std::min(per, (int)c.row_cnt[p] - o)));
  }
  perp_slice[n_bin] = (int)slices.size();
  c.nsl = (int)slices.size();
  // populated par bins: nbin_par is monotone in k <= n / 2, so every bin is one run of k
  std::vector<int> par_start;
  c.par_bin.clear();
  c.par_w.clear();
  for (int k = 0; k < g.nh; k++) {
    const double kz = kv(k);
    const double kpar = std::sqrt(kz * kz);
    const unsigned long long b = (unsigned long long)(kpar / dk);
    if (b >= n_bin) return h->fail(BCHMC_ERR_STATE, "measure_spectrum2d: par bin %llu of k = %d >= n_bin", b, k);
    if (c.par_bin.empty() || c.par_bin.back() != (int)b) {
      par_start.push_back(k);
      c.par_bin.push_back((int)b);
      c.par_w.push_back(0);
    }
    c.par_w.back() += (k == 0 || ((n & 1) == 0 && k == n / 2)) ? 1 : 2;
  }
  par_start.push_back(g.nh);
  c.npb = (int)c.par_bin.size();
  idx.insert(idx.end(), par_start.begin(), par_start.end());
  idx.insert(idx.end(), perp_slice.begin(), perp_slice.end());
  CHK(dev_alloc(h, c.idx, idx.size()));
  CHK(dev_alloc(h, c.slices, slices.size()));
  CHK(dev_alloc(h, c.part, (size_t)c.nsl * g.nh));
  CHK(dev_alloc(h, c.out, (size_t)n_bin * c.npb));
  HIPCHK(hipMemcpyAsync(c.idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(c.slices, slices.data(), slices.size() * sizeof(int2), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // idx and slices are local vectors
  c.ksum.clear();  // filled by the first measurement
  c.n_bin = n_bin;
  return BCHMC_OK;
}

// ---- bchmc_measure_*multipoles (multipoles.hpp) --------------------------------------------------------------------------
void mp_drop(bchmc_handle *h) {
  auto &w = h->mp;
  (void)w.rows.release();
  (void)w.cls.release();
  (void)w.part.release();
  (void)w.out.release();
  (void)w.xk.release();
  w.ncls = 0;
}

// doubles of the segment sums: the widest pass is the cross form's nine sums
size_t mp_out_words(uint64_t n_bin) { return ((size_t)n_bin + 1) * mp_segments((int)n_bin) * 9; }

// The buffers a call needs, each on its first use or when it has to grow: the class tables of the grid (the rows (i, j)
// by class {min(i, n - i), min(j, n - j)}, ascending inside a class), `tables` class-sum tables, the segment sums for
// n_bin and, `xk`, a half-complex array.  If one cannot be had, every buffer of the feature goes back and the handle stays
// usable.  Synchronises when it builds the tables (they are uploaded from local vectors).
int mp_take(bchmc_handle *h, int tables, uint64_t n_bin, bool xk) {
  auto &w = h->mp;
  const Geo &g = h->g;
  const int n = g.n, m = n / 2, ncls = mp_classes(n);
  int rc = BCHMC_OK;
  if (!w.ncls) {
    std::vector<int> rows((size_t)ncls * kMpRows, -1);
    std::vector<int4> cls((size_t)ncls);
    auto id = [&](int a, int b) { return a * (m + 1) - a * (a - 1) / 2 + (b - a); };  // a <= b <= m
    for (int a = 0; a <= m; a++)
      for (int b = a; b <= m; b++) cls[id(a, b)] = make_int4(a, b, 0, 0);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) {
        const int mi = std::min(i, n - i), mj = std::min(j, n - j);
        int4 &c = cls[id(std::min(mi, mj), std::max(mi, mj))];
        rows[(size_t)id(c.x, c.y) * kMpRows + c.z++] = i * n + j;
      }
    rc = dev_alloc(h, w.rows, rows.size());
    if (!rc) rc = dev_alloc(h, w.cls, cls.size());
    if (!rc) {
      hipError_t e = hipMemcpyAsync(w.rows, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, h->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(w.cls, cls.data(), cls.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      if (e != hipSuccess) rc = h->fail(BCHMC_ERR_HIP, "multipoles: class tables: %s", hipGetErrorString(e));
    }
    if (!rc) w.ncls = ncls;
  }
  if (!rc) rc = dev_reserve(h, w.part, (size_t)tables * ncls * g.nh);
  if (!rc) rc = dev_reserve(h, w.out, mp_out_words(n_bin));
  if (!rc && xk && !w.xk) rc = dev_alloc(h, w.xk, 2 * (size_t)g.Nhp * h->esz);
  if (rc) {
    (void)hipStreamSynchronize(h->stream);  // the zero fills of what goes back
    mp_drop(h);
  }
  return rc;
}

// The segment sums hs[(n_bin + 1) * nseg * nacc] added per bin in ascending segment order: sums[(n_bin + 1) * nacc]
std::vector<double> mp_bins(const std::vector<double> &hs, uint64_t n_bin, int nacc) {
  const int nseg = mp_segments((int)n_bin);
  std::vector<double> sums(((size_t)n_bin + 1) * nacc, 0.);
  for (size_t b = 0; b <= n_bin; b++)
    for (int a = 0; a < nacc; a++) {
      double v = 0.;
      for (int s = 0; s < nseg; s++) v += hs[(b * nseg + s) * nacc + a];
      sums[b * nacc + a] = v;
    }
  return sums;
}

// nmode, the mean of t = |k| or r and the means of L_2 and L_4 per bin from the GEOM pass's segment sums
void mp_geometry(bchmc_handle::Mp::Geom &c, const std::vector<double> &hg, uint64_t n_bin) {
  const std::vector<double> s = mp_bins(hg, n_bin, kMpGeom);
  c.tmode.assign(n_bin, 0.);
  c.leg.assign(2 * n_bin, 0.);
  c.nmode.assign(n_bin, 0);
  for (size_t b = 0; b < n_bin; b++) {
    const double cnt = s[b * kMpGeom];  // a sum of integers below 2^53: exact
    c.nmode[b] = (uint64_t)cnt;
    if (!(cnt > 0.)) continue;
    c.tmode[b] = s[b * kMpGeom + 1] / cnt;
    c.leg[b] = s[b * kMpGeom + 2] / cnt;
    c.leg[n_bin + b] = s[b * kMpGeom + 3] / cnt;
  }
  c.n_bin = n_bin;
}

// out[l][b] = (2 l + 1) * norm * sum_l[b] / nmode[b] for table `tab` of `ntab`; 0 in an empty bin; NaN in every populated
// one if the table's total (the elements past the last bin included) is not finite
void mp_normalise(const bchmc_handle::Mp::Geom &c, const std::vector<double> &sums, uint64_t n_bin, int ntab, int tab,
                  double norm, double *out) {
#pragma clang fp contract(off)
  const int nacc = 3 * ntab;
  double total = 0.;
  for (size_t b = 0; b <= n_bin; b++) total += sums[b * nacc + 3 * tab];
  const bool finite = total - total == 0.;
  for (int l = 0; l < 3; l++)
    for (size_t b = 0; b < n_bin; b++) {
      double v = 0.;
      if (c.nmode[b]) v = finite ? (double)(4 * l + 1) * norm * sums[b * nacc + 3 * tab + l] / (double)c.nmode[b] : total - total;
      out[(size_t)l * n_bin + b] = v;
    }
}

// ---- the fine grid of bchmc_interp_upres / bchmc_measure_corr2d_interp (upres.hpp) ------------------------------------
// Releases everything the fine grid holds: the plans and the execution info before the work buffer they point at.
void upres_drop(bchmc_handle *h) {
  auto &u = h->up;
  u.r2c.reset();
  u.c2r.reset();
  u.info.reset();
  (void)u.work.release();
  (void)u.real.release();
  (void)u.half.release();
  (void)u.cell.release();
  (void)u.dx.release();
  u.bins = bchmc_handle::Corr2{};
  u.n_out = 0;
}

// The fine grid for n_out: the two arrays, the plans at n_out in the handle's precision with a work buffer of their own,
// and interp_field's table.  Nothing to do when the last call had the same n_out; another n_out replaces what is held.
// A failure releases what was taken and leaves the handle as it was before its first fine-grid call.
// The table holds getCICcells / getCICweights (interpolate_grid.cpp:27-79) of the centre of fine cell m, in the
// reference's expressions and order, IEEE divide, no FMA contraction: the cell pair depends on the rounding of xpos / d.
int upres_setup(bchmc_handle *h, int n_out) {
#pragma clang fp contract(off)
  auto &u = h->up;
  if (u.n_out == n_out) return BCHMC_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  upres_drop(h);
  auto build = [&]() -> int {
    Geo &f = u.g;
    f.n = n_out;
    f.nh = n_out / 2 + 1;
    f.N = (long long)n_out * n_out * n_out;
    f.Nh = (long long)n_out * n_out * f.nh;
    f.nhp = fft_row_stride(n_out, (int)h->esz);
    f.Nhp = (long long)n_out * n_out * f.nhp;
    f.L = h->g.L;
    f.d = h->g.L / (double)n_out;
    f.kfac = h->g.kfac;
    const size_t e = h->esz;
    CHK(dev_alloc(h, u.real, (size_t)f.N * e));
    CHK(dev_alloc(h, u.half, 2 * (size_t)f.Nhp * e));
    const size_t len[3] = {(size_t)n_out, (size_t)n_out, (size_t)n_out};
    const rocfft_precision prec = h->f32 ? rocfft_precision_single : rocfft_precision_double;
    const size_t rs[3] = {1, (size_t)n_out, (size_t)n_out * n_out}, cs[3] = {1, (size_t)f.nhp, (size_t)f.nhp * n_out};
    rocfft_plan_description fwd = nullptr, inv = nullptr;
    rocfft_status st = rocfft_plan_description_create(&fwd);
    if (st == rocfft_status_success) st = rocfft_plan_description_create(&inv);
    if (st == rocfft_status_success)
      st = rocfft_plan_description_set_data_layout(fwd, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved,
                                                   nullptr, nullptr, 3, rs, (size_t)f.N, 3, cs, (size_t)f.Nhp);
    if (st == rocfft_status_success)
      st = rocfft_plan_description_set_data_layout(inv, rocfft_array_type_hermitian_interleaved, rocfft_array_type_real,
                                                   nullptr, nullptr, 3, cs, (size_t)f.Nhp, 3, rs, (size_t)f.N);
    if (st == rocfft_status_success)
      st = u.r2c.create(rocfft_plan_create, rocfft_placement_notinplace, rocfft_transform_type_real_forward, prec, 3, len, 1,
                        fwd);
    if (st == rocfft_status_success)
      st = u.c2r.create(rocfft_plan_create, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, prec, 3, len, 1,
                        inv);
    if (fwd) rocfft_plan_description_destroy(fwd);
    if (inv) rocfft_plan_description_destroy(inv);
    if (st != rocfft_status_success) return h->fail(BCHMC_ERR_ROCFFT, "plans at n_out = %d: status %d", n_out, (int)st);
    size_t wb = 0, wb2 = 0;
    FFTCHK(rocfft_plan_get_work_buffer_size(u.r2c, &wb));
    FFTCHK(rocfft_plan_get_work_buffer_size(u.c2r, &wb2));
    wb = std::max(wb, wb2);
    FFTCHK(u.info.create(rocfft_execution_info_create));
    FFTCHK(rocfft_execution_info_set_stream(u.info, h->stream));
    if (wb) {
      CHK(alloc_rc(h, u.work.alloc(wb), wb));
      FFTCHK(rocfft_execution_info_set_work_buffer(u.info, u.work, wb));
    }
    const int n = h->g.n;
    const double L = h->g.L, d = h->g.d, d_out = f.d;
    std::vector<int> cell(2 * (size_t)n_out);
    std::vector<double> dx((size_t)n_out);
    for (int m = 0; m < n_out; m++) {
      const double pos = d_out * (0.5 + (double)m);  // interp_upres.cc:79
      double xpos = pos - 0.5 * d;
      if (xpos < 0.) {  // pacman_coordinate, pacman.cpp:20-28
        xpos = std::fmod(xpos, L);
        xpos += L;
      }
      if (xpos >= L) xpos = std::fmod(xpos, L);
      unsigned long long c = (unsigned long long)(xpos / d);
      c = (c + (unsigned long long)n) % (unsigned long long)n;
      cell[m] = (int)c;
      cell[n_out + m] = (int)((c + 1) % (unsigned long long)n);
      dx[m] = xpos / d - (double)c;
    }
    CHK(dev_alloc(h, u.cell, cell.size()));
    CHK(dev_alloc(h, u.dx, dx.size()));
    HIPCHK(hipMemcpyAsync(u.cell, cell.data(), cell.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(u.dx, dx.data(), dx.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // cell and dx are local vectors
    return BCHMC_OK;
  };
  const int rc = build();
  if (rc) upres_drop(h);
  else u.n_out = n_out;
  return rc;
}

// ======================================================================================================
// The pipeline, for storage type T
// ======================================================================================================
// What bchmc_density_particles asks of the pipe, after its checks: the source, the kernel and scale length in force, the
// largest |w| (1 without weights), the caller's columns
// A source beside the two of bchmc_part_source that only bchmc_poisson_density sets (bchmc_density_particles refuses it):
// the resident Poisson sample, whose batches k_pois_positions writes into the staged columns
constexpr int kCatSrcPoisson = 2;

struct CatCall {
  int src, mk, weighted, dest;
  double hh, max_w;
  const double *x, *y, *z, *w;
  uint64_t n_part;
};

// What bchmc_interp_particles asks of the pipe, after its checks: the position source, the kernel, the path decided by
// interp_plan.hpp, the fields and the columns.
struct ItpCall {
  int psrc, kernel, tiled, n_fields;
  const bchmc_interp_field *fields;
  const double *x, *y, *z;
  uint64_t n_part;
};

template <typename T>
struct Pipe {
  using CT = C2<T>;
  static constexpr bool kDouble = std::is_same<T, double>::value;

  static T *R(void *p) { return reinterpret_cast<T *>(p); }
  static CT *C(void *p) { return reinterpret_cast<CT *>(p); }
  static const CT *C(const void *p) { return reinterpret_cast<const CT *>(p); }

  static size_t tile_lds(const bchmc_handle *h, int ncol, size_t cell_bytes) {
    const size_t ncell = (size_t)h->plan.tp.lx * h->plan.tp.ly * h->plan.tp.lz;
    return ((ncell * cell_bytes + 15) & ~(size_t)15) + (size_t)ncol * sizeof(int4);
  }
  // upper bound on the (tile, chunk) work items of the tile kernels
  static int tile_grid(const bchmc_handle *h) { return h->plan.tp.ntiles + (int)(h->g.N / h->plan.tp.chunk) + 1; }
  // the engine's own FFT passes (pass_launch.hpp) on this handle
  static PassCtx<T> pass_ctx(const bchmc_handle *h) { return {h->stream, h->g, h->log2n, C(h->xtw)}; }

  // ---- ABI (double) <-> storage (T) on the device ----
  static int load_real(bchmc_handle *h, const double *d_src, T *dst) {
    if (kDouble) {
      if ((const void *)d_src != (const void *)dst)
        HIPCHK(hipMemcpyAsync(dst, d_src, h->g.N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    } else {
      k_convert<double, T><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g.N, d_src, dst);
      HIPCHK(hipGetLastError());
    }
    return BCHMC_OK;
  }
  static int store_real(bchmc_handle *h, const T *src, double *d_dst) {
    if (kDouble) {
      if ((const void *)src != (const void *)d_dst)
        HIPCHK(hipMemcpyAsync(d_dst, src, h->g.N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    } else {
      k_convert<T, double><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g.N, src, d_dst);
      HIPCHK(hipGetLastError());
    }
    return BCHMC_OK;
  }

  // ---- building blocks of one force / energy evaluation ----

  // Psi^ from the current q^ (no kick, no drift), Zel'dovich: Lag2Eul.cc:88-89 + theta2vel
  static int launch_za(bchmc_handle *h, double dq_factor) {
    ProfScope ps(h, BCHMC_K_KSPACE_DRIFT_ZA);
    StepCtl ctl{h->stop, h->steps_done, nullptr, 0., 0};
    const double c_za = -h->c.D1 * dq_factor / (double)h->g.N;
    k_kick_drift_za<T, false><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, C(h->qk), C(h->pk), C(h->gk), nullptr,
                                                                          nullptr, C(h->Ck), 0., 0., c_za, ctl);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // Psi^ of the forward model selected by (sfmodel, rsd) from the current q^; *psi_planes: it is left in planes space
  // (EvalMode::planes_c2r of the forward_rest that follows)
  static int displacement(bchmc_handle *h, double dq_factor, int rsd, bool *psi_planes) {
    const PathFacts f = path_facts(h, rsd);
    *psi_planes = alpt_on_planes(f, h->sw, rsd);
    h->ck_pair = false;  // three components of Psi^, whichever model
    return uses_alpt(f, rsd) ? launch_alpt(h, dq_factor, *psi_planes) : launch_za(h, dq_factor);
  }

  // kernelcomp: wtot = sum over the box of the inverse transform of the kernel table (= K(0) up to round-off)
  static int alpt_norm(bchmc_handle *h) {
    if (h->alpt_wtot != 0.) return BCHMC_OK;
    return kernel_norm(h, h->c.kth, h->rho, &h->alpt_wtot);
  }
  // the same for any scale; `scratch`: N elements of T
  static int kernel_norm(bchmc_handle *h, double smol, void *scratch, double *wtot) {
    ProfScope ps(h, BCHMC_K_OTHER);
    k_alpt_kernel_table<T><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, C(h->tC), smol);
    HIPCHK(hipGetLastError());
    CHK(fft_exec(h, h->c2r1, h->tC, scratch, BCHMC_K_FFT_C2R));
    k_sum<T><<<kRedBlocks, 256, 0, h->stream>>>(R(scratch), h->g.N, h->partA);
    HIPCHK(hipGetLastError());
    double v;
    CHK(host_sum(h, h->partA, &v));
    *wtot = v / (double)h->g.N;
    return BCHMC_OK;
  }

  // ALPT displacement (Lag2Eul_non_zeldovich, Lag2Eul.cc:160-267), second part: from delta(1)^ and Phi^ in Ck[0], Ck[1]
  // (full k-space, or planes space when `planes`) to Psi^ of the three components in Ck, in the same space, cell-boundary
  // average included.  Scratch: V, psi (planes) / plike, rho, V (3-D).
  static int alpt_middle(bchmc_handle *h, bool planes) {
    const long long N = h->g.N, Nhp = h->g.Nhp;
    CT *Ck = C(h->Ck);
    CHK(alpt_norm(h));
    T *d1, *phi, *g3, *a_out, *b_out;
    if (planes) {
      // both transforms batched over 2 n planes: delta(1) -> V[0, N), Phi(1) -> V[N, 2N); first derivatives in psi
      CHK(fft_exec(h, h->c2r2d_2, Ck, h->V, BCHMC_K_FFT_C2R));
      d1 = R(h->V), phi = R(h->V) + N, g3 = R(h->psi), a_out = R(h->V), b_out = R(h->V) + N;
    } else {
      CHK(fft_exec(h, h->c2r1, Ck, h->plike, BCHMC_K_FFT_C2R));        // delta(1)
      CHK(fft_exec(h, h->c2r1, Ck + Nhp, h->rho, BCHMC_K_FFT_C2R));    // Phi(1)
      d1 = R(h->plike), phi = R(h->rho), g3 = R(h->V), a_out = R(h->rho), b_out = R(h->plike);
    }
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_alpt_grad<T><<<stencil_grid(h->g.n), 256, 0, h->stream>>>(h->g, phi, g3);
      k_alpt_sources<T><<<stencil_grid(h->g.n), 256, 0, h->stream>>>(h->g, g3, d1, a_out, b_out, h->c.D1, h->c.D2);
      HIPCHK(hipGetLastError());
    }
    if (planes) {
      CHK(fft_exec(h, h->r2c2d_2, h->V, Ck, BCHMC_K_FFT_R2C));         // A^, B^ of every (y, z) plane
      ProfScope ps(h, BCHMC_K_KSPACE_DRIFT_ZA);
      HIPCHK(launch_alpt_mix_x<T>(pass_ctx(h), Ck, h->c.kth, 1. / h->alpt_wtot, 1. / (double)N));
    } else {
      CHK(fft_exec(h, h->r2c1, a_out, Ck, BCHMC_K_FFT_R2C));           // A^ = FFT[D1 delta(1) - D2 delta(2)]
      CHK(fft_exec(h, h->r2c1, b_out, Ck + Nhp, BCHMC_K_FFT_R2C));     // B^ = FFT[spherical-collapse source]
      ProfScope ps(h, BCHMC_K_KSPACE_DRIFT_ZA);
      k_alpt_mix<T><<<nblk_stride(Nhp), 256, 0, h->stream>>>(h->g, Ck, h->c.kth, 1. / h->alpt_wtot, 1. / (double)N);
      HIPCHK(hipGetLastError());
    }
    return BCHMC_OK;
  }

  // ALPT displacement from the current q^, on the 2-D plans (`planes`: alpt_on_planes, eval_plan.hpp) or the 3-D ones.
  static int launch_alpt(bchmc_handle *h, double dq_factor, bool planes) {
    const double scale = dq_factor / (double)h->g.N;
    if (planes) {
      {
        ProfScope ps(h, BCHMC_K_KSPACE_DRIFT_ZA);
        StepCtl nc{h->stop, h->steps_done, nullptr, 0., 0};
        BoundaryX<T> bx;
        bx.qi = C(h->qk), bx.c_za = scale, bx.ctl = nc;
        CHK((launch_boundary_x<BX_FIRST, true>(h, bx)));
      }
      return alpt_middle(h, true);
    }
    {
      ProfScope ps(h, BCHMC_K_KSPACE_DRIFT_ZA);
      k_alpt_poisson<T><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, C(h->qk), C(h->Ck), C(h->Ck) + h->g.Nhp, scale);
      HIPCHK(hipGetLastError());
    }
    return alpt_middle(h, false);
  }

  // C2R of the three displacement components, mass assignment, sum of rho.  Lag2Eul.cc:90-131 / 363-423.
  // Reads m.planes_c2r (where the caller or `displacement` left Psi^) and m.psi_unread.
  static int forward_rest(bchmc_handle *h, int rsd, EvalMode m) {
    if (rsd && !h->c.planepar) return h->fail(BCHMC_ERR_RSD_NOT_PLANEPAR, "non-plane-parallel RSD is not implemented");
    const bool zbin = eval_zbin(path_facts(h, rsd), h->sw, m);  // the z pass of Psi^ is particle_stage's
    const bool pair = h->ck_pair;  // what the boundary kernel left: Psi^_x | B (k_ypass_pair makes ky B and kz B)
    h->ck_pair = false;
    if (pair && !zbin) return h->fail(BCHMC_ERR_STATE, "two arrays between the x and y passes, and no y pass of the engine's own");
    if (zbin) {
      ProfScope ps(h, BCHMC_K_FFT_C2R);
      HIPCHK(pair ? launch_ypass_pair<T>(pass_ctx(h), C(h->Ck)) : launch_ypass<T>(pass_ctx(h), C(h->Ck)));
    } else {
      CHK(fft_exec(h, m.planes_c2r ? h->c2r2d : h->c2r3, h->Ck, h->psi, BCHMC_K_FFT_C2R));
    }
    return particle_stage(h, rsd, m, zbin);
  }

  // Everything of the forward model after the C2R of Psi: binning (one-pass, or the two-pass sort + subsort after an
  // overflow), mass assignment, fixed-point conversion, sum of rho.  Reads Psi from h->psi -- unless `zbin`, where
  // k_zbin_direct takes the z pass of Psi^ (Ck) on its way (forward_rest, and bchmc_probe_displacement_z, which makes
  // that Psi^ from a real-space displacement with k_zr2c; bchmc_probe_displacement has no Psi^ to give it).
  static int particle_stage(bchmc_handle *h, int rsd, EvalMode m, bool zbin) {
    h->sorted_valid = false;
    bool rho_cleared = false;  // by k_bin_direct, on its way through the lattice
    const PosPar pp = make_pos(h, rsd);
    const SphPar sp = make_sph(h);
    // this evaluation's gather will store V as records (like_force): the binning zeroes the record, not the three arrays,
    // of a particle without a usable position
    h->vrec_eval = eval_vrec(path_facts(h, h->c.rsd_model), h->sw, m);
    if (h->vrec_eval && !h->vrec) CHK(dev_alloc(h, h->vrec, 4 * (size_t)h->g.N * sizeof(T)));
    T *const vrec = h->vrec_eval ? R(h->vrec) : nullptr;
    if (h->plan.tiled) {
      // counting sort of the particles by the Eulerian tile of their home cell
      ProfScope ps(h, BCHMC_K_SORT);
      // one-pass binning into fixed slots per tile; the two-pass kernels run only if a tile overflowed
      const int nt = h->plan.tp.ntiles, nbricks = nblk_full(h->g.N);
      int *cnt1 = h->t_cnt, *cnt2 = h->t_cnt + kOct * nt, *ovf = h->t_cnt + (kOct + 1) * nt;  // ovf[1], ovf[2]: the host's slot words, see adapt_slots
      if (!h->cnt_clean) HIPCHK(hipMemsetAsync(h->t_cnt, 0, ((kOct + 1) * (size_t)nt + 1) * sizeof(int), h->stream));
      h->cnt_clean = false;
      // the two fallback kernels return at once unless a tile overflowed; when one did (every step until the slots are
      // doubled at the next trajectory start) they must still fill the chip, so the grid is capped, not tiny: with 512
      // workgroups a 512^3 step in fallback mode took 69 ms instead of 22 (and the no-op launches cost 18-20 us either way)
      const int fb_grid = h->plan.slots.sort_direct ? std::min(nbricks, 4096) : nbricks;
      if (zbin) {
        HIPCHK(launch_zbin<T>(pass_ctx(h), pp, sp, h->plan.tp, C(h->Ck), cnt1, ovf, recs(h), R(h->V), h->rho_part,
                              h->fix ? nullptr : R(h->rho), h->fix ? h->rho_fix : nullptr,
                              m.psi_unread ? nullptr : R(h->psi), vrec));
        // second launch (interior steps, where Psi is not stored on the way): a segment overflowed -> the two-pass sort
        // below needs Psi after all (returns at once otherwise)
        if (m.psi_unread)
          HIPCHK((launch_zbin<T, true>(pass_ctx(h), pp, sp, h->plan.tp, C(h->Ck), cnt1, ovf, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, R(h->psi), nullptr)));
        rho_cleared = true;
      } else if (h->plan.slots.sort_direct) {
        const int nsuper = (nbricks + kBinPer - 1) / kBinPer;
        k_bin_direct<T><<<nsuper, BCHMC_BIN_THREADS, 0, h->stream>>>(h->g, pp, sp, h->plan.tp, nsuper, R(h->psi), cnt1, ovf,
                                                       recs(h), R(h->V), h->rho_part,
                                                       h->fix ? nullptr : R(h->rho),
                                                       h->fix ? h->rho_fix : nullptr, vrec);
        rho_cleared = true;
      } else {
        HIPCHK(hipMemsetAsync(ovf, 1, 1, h->stream));  // non-zero flag: two-pass sort only
      }
      k_bin<T><<<fb_grid, 256, 0, h->stream>>>(h->g, pp, sp, h->plan.tp, nbricks, R(h->psi), cnt2, ovf, h->t_rank, R(h->V),
                                             vrec);
      k_scan_tiles<<<(nt + 1023) / 1024, 1024, 0, h->stream>>>(h->plan.tp, cnt1, cnt2, ovf, h->t_off, h->t_end, h->t_woff,
                                                               h->t_oct, h->t_seg, ovf + 2);
      k_reorder<T><<<fb_grid, 256, 0, h->stream>>>(h->g, pp, nbricks, R(h->psi), h->t_rank, h->t_off, ovf,
                                                   recs(h));
      HIPCHK(hipGetLastError());
      h->sorted_valid = true;
    }
    {
      ProfScope ps(h, BCHMC_K_SCATTER);
      const bool tile_path = (h->c.mk == 3 && h->plan.tiled), tile_low = (h->c.mk >= 0 && h->c.mk <= 2 && h->plan.tiled);
      // fixed point (deterministic mode): scale = 2^46 / largest single contribution (W(0) = 1/(pi h^3) for the SPH
      // kernel, 1 for NGP / CIC / TSC weights)
      const double fix_scale = h->c.mk == 3 ? 70368744177664. / sp.w_norm : 70368744177664.;
      if (rho_cleared) {
      } else if (h->fix) {
        HIPCHK(hipMemsetAsync(h->rho_fix, 0, h->g.N * sizeof(long long), h->stream));
      } else {
        HIPCHK(hipMemsetAsync(h->rho, 0, h->g.N * sizeof(T), h->stream));
      }
      if (tile_path) {
        // the tile kernels also leave sum(rho) in rho_part (partial sums of what they flush): no pass over rho
        // (k_bin<DIRECT> has cleared the partials; without the one-pass binning a fill does)
        if (!h->plan.slots.sort_direct && !h->fix) HIPCHK(hipMemsetAsync(h->rho_part, 0, kRedBlocks * sizeof(double), h->stream));
        const int grid = tile_grid(h);
        const int ncol = h->plan.hull_exact ? h->plan.hull_n : 0;
        // sub-cell ordering inside each work item: two binary digits per axis
        const int reorder = (h->plan.tp.chunk > 2048) ? 0 : 2;
        if (reorder) {  // orders the records only after a fallback sort; returns at once otherwise
          k_subsort<T><<<std::min(grid, 8192), 256, 0, h->stream>>>(h->g, h->plan.tp, reorder, recs(h), h->t_off, h->t_end, h->t_woff,
                                                   h->t_oct, h->t_seg);
          HIPCHK(hipGetLastError());
        }
        if (h->plan.std81) {
          if (h->fix)
            k_scatter_tile81<T, 12, 20, true><<<grid, kTile81Threads, tile_lds(h, 0, sizeof(double)), h->stream>>>(
                h->g, sp, h->plan.tp, recs(h), h->t_off, h->t_end, h->t_woff,
                h->t_oct, h->t_seg, h->rho_fix, h->rho_part, h->t_cnt,
                (kOct + 1) * h->plan.tp.ntiles + 1, fix_scale);
          else
            k_scatter_tile81<T, 12, 20, false><<<grid, kTile81Threads, tile_lds(h, 0, sizeof(double)), h->stream>>>(
                h->g, sp, h->plan.tp, recs(h), h->t_off, h->t_end, h->t_woff,
                h->t_oct, h->t_seg, R(h->rho), h->rho_part, h->t_cnt,
                (kOct + 1) * h->plan.tp.ntiles + 1, fix_scale);
          h->cnt_clean = true;
        } else if (h->fix) {
          k_scatter_tile<T, true><<<grid, 256, tile_lds(h, ncol, sizeof(double)), h->stream>>>(
              h->g, sp, h->plan.tp, h->hull, ncol, recs(h), h->t_off, h->t_end,
              h->t_woff, h->t_oct, h->t_seg, h->rho_fix, h->rho_part, fix_scale);
        } else {
          k_scatter_tile<T, false><<<grid, 256, tile_lds(h, ncol, sizeof(double)), h->stream>>>(
              h->g, sp, h->plan.tp, h->hull, ncol, recs(h), h->t_off, h->t_end,
              h->t_woff, h->t_oct, h->t_seg, R(h->rho), h->rho_part, fix_scale);
        }
      } else if (tile_low) {
        // NGP / CIC / TSC on the (tile, octant) records: LDS image of the tile + a one-cell halo, one flush
        if (!h->plan.slots.sort_direct && !h->fix) HIPCHK(hipMemsetAsync(h->rho_part, 0, kRedBlocks * sizeof(double), h->stream));
        const int grid = tile_grid(h);
        const size_t lds = (size_t)(h->plan.tp.tx + 2) * (h->plan.tp.ty + 2) * (h->plan.tp.tz + 2) * sizeof(double);
        const int ncnt = (kOct + 1) * h->plan.tp.ntiles + 1;
        if (h->fix)
          k_scatter_tile_low<T, true><<<grid, 256, lds, h->stream>>>(h->g, h->plan.tp, h->c.mk, recs(h), h->t_off,
                                                                     h->t_end, h->t_woff, h->t_oct, h->t_seg, h->rho_fix,
                                                                     h->rho_part, h->t_cnt, ncnt, fix_scale);
        else
          k_scatter_tile_low<T, false><<<grid, 256, lds, h->stream>>>(h->g, h->plan.tp, h->c.mk, recs(h), h->t_off,
                                                                      h->t_end, h->t_woff, h->t_oct, h->t_seg, R(h->rho),
                                                                      h->rho_part, h->t_cnt, ncnt, fix_scale);
        h->cnt_clean = true;
      } else if (h->c.mk == 3) {
        if (h->fix)
          k_scatter_sph<T, true><<<nblk_full(h->g.N), 256, 0, h->stream>>>(h->g, pp, sp, R(h->psi), h->rho_fix, fix_scale);
        else
          k_scatter_sph<T, false><<<nblk_full(h->g.N), 256, 0, h->stream>>>(h->g, pp, sp, R(h->psi), R(h->rho), fix_scale);
      } else if (h->c.mk >= 0 && h->c.mk <= 2) {
        if (h->fix)
          k_scatter_low_order<T, true><<<nblk_full(h->g.N), 256, 0, h->stream>>>(h->g, pp, sp, h->c.mk, R(h->psi),
                                                                                 h->rho_fix, fix_scale);
        else
          k_scatter_low_order<T, false><<<nblk_full(h->g.N), 256, 0, h->stream>>>(h->g, pp, sp, h->c.mk, R(h->psi),
                                                                                  R(h->rho), fix_scale);
      } else {
        return h->fail(BCHMC_ERR_ARG, "masskernel %d is not a valid value (0..3)", h->c.mk);
      }
      HIPCHK(hipGetLastError());
      if (h->fix) {
        k_fix_to_rho<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g.N, h->rho_fix, 1. / fix_scale, R(h->rho), h->rho_part,
                                                           h->fix_sat, h->fix_sat_limit);
        HIPCHK(hipGetLastError());
      }
    }
    if (!h->plan.tiled && !h->fix) {
      ProfScope ps(h, BCHMC_K_MEAN_PARTIAL);
      k_sum<T><<<kRedBlocks, 256, 0, h->stream>>>(R(h->rho), h->g.N, h->rho_part);
      HIPCHK(hipGetLastError());
    }
    h->have_eval = true;
    h->last_rsd = rsd;
    return BCHMC_OK;
  }

  static int ensure_conv(bchmc_handle *h) {
    if (!h->conv) CHK(dev_alloc(h, h->conv, 3 * (size_t)h->g.N * sizeof(T)));
    return BCHMC_OK;
  }

  // After forward_rest: leaves the k-space likelihood source in Ck and returns the assemble mode.
  // transform = false (bchmc_probe_displacement): stops before the R2C that ends each branch; part_like and V stay.
  static int like_force(bchmc_handle *h, EvalMode m, int *like_mode, bool transform = true) {
    if (h->c.calc_h == 2 || h->c.calc_h == 3) {
      if (h->c.mk != 3)
        return h->fail(BCHMC_ERR_MK_NOT_SPH, "Must use SPH mass kernel (masskernel = 3) with calc_h = 2 or 3");
    } else if (h->c.calc_h != 1 && h->c.calc_h != 0) {
      return h->fail(BCHMC_ERR_ARG, "calc_h = %d is not a valid value (0..3)", h->c.calc_h);
    }
    const long long N = h->g.N, Nh = h->g.Nhp;
    const bool vrec = h->vrec_eval;  // as particle_stage decided for this evaluation
    h->vrec_eval = h->v_in_vrec = h->ck_vpair = false;
    {
      ProfScope ps(h, BCHMC_K_MEAN_PARTIAL);
      k_partial_like<T><<<nblk_stride(N), 256, 0, h->stream>>>(h->g, make_like(h), R(h->rho), h->rho_part,
                                                               R(h->in_arr[BCHMC_F_NOBS]), R(h->in_arr[BCHMC_F_NOISE]),
                                                               R(h->in_arr[BCHMC_F_WINDOW]), R(h->plike));
      HIPCHK(hipGetLastError());
    }
    if (h->c.calc_h == 1) {
      if (transform) CHK(fft_exec(h, h->r2c1, h->plike, h->Ck, BCHMC_K_FFT_R2C));
      *like_mode = 1;
      return BCHMC_OK;
    }
    if (h->c.calc_h == 0) {
      // likelihood_calc_h (HMC_models_testing.cpp:25-50)
      {
        ProfScope ps(h, BCHMC_K_OTHER);
        k_overdens<T><<<nblk_stride(N), 256, 0, h->stream>>>(h->g, R(h->rho), h->rho_part, R(h->ioq));
        HIPCHK(hipGetLastError());
      }
      if (h->c.likelihood == 1) {
        CHK(ensure_conv(h));
        CHK(fft_exec(h, h->r2c1, h->ioq, h->tC, BCHMC_K_FFT_R2C));
        {
          ProfScope ps(h, BCHMC_K_OTHER);
          k_gradfft_mult<T><<<nblk_stride(Nh), 256, 0, h->stream>>>(h->g, C(h->tC), C(h->Ck), 1. / (double)N);
          HIPCHK(hipGetLastError());
        }
        CHK(fft_exec(h, h->c2r3, h->Ck, h->conv, BCHMC_K_FFT_C2R));
        ProfScope ps(h, BCHMC_K_OTHER);
        k_mul3<T><<<nblk_stride(N), 256, 0, h->stream>>>(N, R(h->plike), R(h->conv), R(h->V));
        HIPCHK(hipGetLastError());
      } else {
        ProfScope ps(h, BCHMC_K_OTHER);
        k_findif_mul<T><<<nblk_stride(N), 256, 0, h->stream>>>(h->g, make_like(h), R(h->ioq), R(h->plike), R(h->V));
        HIPCHK(hipGetLastError());
      }
      if (transform) CHK(fft_exec(h, h->r2c3, h->V, h->Ck, BCHMC_K_FFT_R2C));
      *like_mode = 0;
      return BCHMC_OK;
    }
    if (h->c.calc_h == 3) {
      // likelihood_calc_V_SPH_fourier_TSC (HMC_models_testing.cpp:54-188)
      if (h->last_rsd && !h->c.planepar)
        return h->fail(BCHMC_ERR_RSD_NOT_PLANEPAR, "non-plane-parallel RSD is not implemented in calc_V");
      CHK(ensure_conv(h));
      if (!h->convF) CHK(build_conv_table(h));
      CHK(fft_exec(h, h->r2c1, h->plike, h->tC, BCHMC_K_FFT_R2C));
      const double hh = h->c.particle_kernel_h;
      {
        ProfScope ps(h, BCHMC_K_OTHER);
        k_conv_kernel<T><<<nblk_stride(Nh), 256, 0, h->stream>>>(h->g, C(h->tC), h->convF, C(h->Ck), hh, 1. / (double)N);
        HIPCHK(hipGetLastError());
      }
      CHK(fft_exec(h, h->c2r3, h->Ck, h->conv, BCHMC_K_FFT_C2R));
      {
        ProfScope ps(h, BCHMC_K_GATHER);
        if (h->plan.tiled && h->sorted_valid && !h->no_tiles_low) {
          const int grid = tile_grid(h);
          const size_t lds = 3 * (size_t)(h->plan.tp.tx + 2) * (h->plan.tp.ty + 2) * (h->plan.tp.tz + 2) * sizeof(T);
          k_interp_tsc_tile<T><<<grid, 256, lds, h->stream>>>(h->g, h->plan.tp, h->last_rsd, fgrow1(h->c.ascale, h->c.OM, h->c.OL),
                                                              recs(h), h->t_off, h->t_end, h->t_woff,
                                                              h->t_oct, h->t_seg, R(h->conv), R(h->V));
        } else {
          k_interp_tsc<T><<<nblk_full(N), 256, 0, h->stream>>>(h->g, make_pos(h, h->last_rsd),
                                                               fgrow1(h->c.ascale, h->c.OM, h->c.OL), R(h->psi),
                                                               R(h->conv), R(h->V));
        }
        HIPCHK(hipGetLastError());
      }
    } else {
      ProfScope ps(h, BCHMC_K_GATHER);
      HullPar hp = make_hull(h);
      if (h->plan.tiled && h->sorted_valid) {
        const int grid = tile_grid(h);
        if (h->plan.std81 && vrec) {
          k_gather_tile81<T, 12, 20, true><<<grid, kTile81Threads, tile_lds(h, 0, sizeof(T)), h->stream>>>(
              h->g, hp, h->plan.tp, h->last_rsd, recs(h), h->t_off, h->t_end, h->t_woff,
              h->t_oct, h->t_seg, R(h->plike), R(h->vrec));
          h->v_in_vrec = true;
        } else if (h->plan.std81)
          k_gather_tile81<T, 12, 20><<<grid, kTile81Threads, tile_lds(h, 0, sizeof(T)), h->stream>>>(
              h->g, hp, h->plan.tp, h->last_rsd, recs(h), h->t_off, h->t_end, h->t_woff,
              h->t_oct, h->t_seg, R(h->plike), R(h->V));
        else
          k_gather_tile<T><<<grid, 256, tile_lds(h, hp.ncol, sizeof(T)), h->stream>>>(
              h->g, hp, h->plan.tp, h->last_rsd, recs(h), h->t_off, h->t_end, h->t_woff,
              h->t_oct, h->t_seg, R(h->plike), R(h->V));
      } else {
        k_gather_sph<T><<<nblk_full(N), 256, hp.ncol * sizeof(int4), h->stream>>>(h->g, make_pos(h, h->last_rsd), hp,
                                                                                  R(h->psi), R(h->plike), R(h->V));
      }
      HIPCHK(hipGetLastError());
      if (vrec && !h->v_in_vrec) return h->fail(BCHMC_ERR_STATE, "V records were zeroed and no gather writes records");
    }
    const bool vpair = eval_vpair(path_facts(h, h->c.rsd_model), h->sw, m);
    if (transform && h->v_in_vrec && !vpair)
      return h->fail(BCHMC_ERR_STATE, "V was gathered as records, and a transform that reads three arrays");
    if (!transform) {
    } else if (vpair) {
      // the engine's own row pass (from the V records, or the three arrays with BCHMC_NO_VREC) and the column pass that
      // leaves V^_x | W = ky V^_y + kz V^_z for the boundary kernel (zpass.hpp)
      ProfScope ps(h, BCHMC_K_FFT_R2C);
      if (h->v_in_vrec) HIPCHK((launch_zr2c<T, true>(pass_ctx(h), R(h->vrec), C(h->Ck))));
      else HIPCHK(launch_zr2c<T>(pass_ctx(h), R(h->V), C(h->Ck)));
      HIPCHK(launch_ypass_fwd_pair<T>(pass_ctx(h), C(h->Ck)));
      h->ck_vpair = true;
    } else if (eval_yfwd(path_facts(h, h->c.rsd_model), h->sw, m)) {
      // 512^3: the engine's own row and column passes (rocFFT's length-512 column kernel runs at 2.3 TB/s, its 1-D row
      // plan alone at half the speed of the same pass inside the 2-D plan: k_zr2c + k_ypass<forward>, zpass.hpp)
      ProfScope ps(h, BCHMC_K_FFT_R2C);
      HIPCHK(launch_zr2c<T>(pass_ctx(h), R(h->V), C(h->Ck)));
      HIPCHK((launch_ypass<T, false>(pass_ctx(h), C(h->Ck))));
    } else {
      CHK(fft_exec(h, m.planes_r2c ? h->r2c2d : h->r2c3, h->V, h->Ck, BCHMC_K_FFT_R2C));
    }
    *like_mode = 0;
    return BCHMC_OK;
  }

  // GRF likelihood force (gaussian_random_field.cpp:25-37): needs q in real space.
  static int grf_force(bchmc_handle *h) {
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_scale_c<T><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g.Nhp, C(h->qk), C(h->tC), 1. / (double)h->g.N);
      HIPCHK(hipGetLastError());
    }
    CHK(fft_exec(h, h->c2r1, h->tC, h->plike, BCHMC_K_FFT_C2R));
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_grf_grad<T><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g.N, R(h->plike), R(h->in_arr[BCHMC_F_NOBS]),
                                                                R(h->in_arr[BCHMC_F_NOISE]),
                                                                R(h->in_arr[BCHMC_F_WINDOW]), R(h->rho));
      HIPCHK(hipGetLastError());
    }
    CHK(fft_exec(h, h->r2c1, h->rho, h->Ck, BCHMC_K_FFT_R2C));
    h->have_eval = false;
    return BCHMC_OK;
  }

  // Likelihood part of gradient_psi from the current q^: fills Ck, returns (like_mode, b).
  // pre_za: Psi^ is already in Ck (the fused kick+drift+ZA kernel ran), or with m.alpt_pending the ALPT model's inputs.
  static int force_sources(bchmc_handle *h, bool pre_za, EvalMode m, int *like_mode, double *b) {
    if (h->c.likelihood == 3) {
      CHK(grf_force(h));
      *like_mode = 1;
      *b = h->c.grad_psi_likeli_factor;
      return BCHMC_OK;
    }
    if (!pre_za) {
      CHK(displacement(h, h->c.deltaQ_factor, h->c.rsd_model, &m.planes_c2r));
    } else if (m.alpt_pending) {
      CHK(alpt_middle(h, true));  // delta(1)^ | Phi^ planes left by k_step_boundary_x<ALPT> -> Psi^ planes
      m.planes_c2r = true;
    }
    CHK(forward_rest(h, h->c.rsd_model, m));
    CHK(like_force(h, m, like_mode));
    double norm = -1.;  // zeldovich_norm, HMC_models.cc:458-461
    norm *= h->c.deltaQ_factor;
    if (h->c.correct_delta) norm *= h->c.D1;
    *b = h->c.grad_psi_likeli_factor * norm;
    return BCHMC_OK;
  }

  template <bool KICK>
  static int launch_assemble(bchmc_handle *h, double a, double b, int like_mode, double c_kick, double *guard_slot) {
    h->prop_g_valid = false;  // gk is rewritten: whatever gradient a chain proposal left there is gone
    if (h->ck_vpair) return h->fail(BCHMC_ERR_STATE, "two arrays of V^ in Ck, and a kernel that reads three");
    ProfScope ps(h, BCHMC_K_KSPACE_FORCE_KICK);
    k_assemble<T, KICK><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, C(h->Ck), C(h->qk), h->wS, C(h->gk), C(h->pk),
                                                                     a, b, like_mode, c_kick, guard_slot, h->stop);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // R2C of a real-space state given as an ABI (double) device array; `staging` receives the T copy that is
  // transformed (rocFFT may use its input as scratch, and the caller's array must stay intact).
  static int r2c_state(bchmc_handle *h, const double *d_real, void *staging, void *out) {
    CHK(load_real(h, d_real, R(staging)));
    return fft_exec(h, h->r2c1, staging, out, BCHMC_K_FFT_R2C);
  }

  // xk / N -> C2R -> T array.  xtiled: xk is in x-column tiles (the early q of a tiled trajectory); the scaling pass
  // un-tiles it on the way.
  static int c2r_scaled(bchmc_handle *h, const void *xk, void *out_T, bool xtiled = false) {
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      if (xtiled)
        k_xtile_scale_c<T><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, reinterpret_cast<const CT *>(xk), C(h->tC),
                                                                        1. / (double)h->g.N);
      else
        k_scale_c<T><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g.Nhp, reinterpret_cast<const CT *>(xk), C(h->tC),
                                                                  1. / (double)h->g.N);
      HIPCHK(hipGetLastError());
    }
    return fft_exec(h, h->c2r1, h->tC, out_T, BCHMC_K_FFT_C2R);
  }

  // C2R of a k-space state into an ABI (double) device array; `scratch_T` is used when T != double.
  static int c2r_state(bchmc_handle *h, const void *xk, void *scratch_T, double *d_out, bool xtiled = false) {
    if (kDouble) return c2r_scaled(h, xk, d_out, xtiled);
    CHK(c2r_scaled(h, xk, scratch_T, xtiled));
    return store_real(h, R(scratch_T), d_out);
  }

  // extra = R2C[ C2R[p^]/N / mass_r ]  (real-space mass term of the drift, HMC.cc:317-327)
  static int mass_rs_term(bchmc_handle *h) {
    CHK(c2r_scaled(h, h->pk, h->iop));
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_div_mass_r<T><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g.N, R(h->iop), R(h->in_arr[BCHMC_F_MASS_R]),
                                                                  R(h->iop));
      HIPCHK(hipGetLastError());
    }
    return fft_exec(h, h->r2c1, h->iop, h->tC, BCHMC_K_FFT_R2C);
  }

  // Optional taps for the resident-chain path: -log L partials of the forward model at the first and the last
  // force evaluation of a trajectory (the same forward models delta_Hamiltonian would recompute, HMC.cc:214-225).
  struct Tap {
    double *like_i, *like_f;
  };

  static int tap_loglike(bchmc_handle *h, double *partials) {
    k_loglike<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g, make_like(h), R(h->rho), h->rho_part,
                                                    R(h->in_arr[BCHMC_F_NOBS]), R(h->in_arr[BCHMC_F_NOISE]),
                                                    R(h->in_arr[BCHMC_F_WINDOW]), partials);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // How a trajectory runs on this handle now (eval_plan.hpp), and the two constants its kernels take: a, the prior
  // factor, and c_za, which turns q^ into the displacement model's k-space input.  Lives for one call: nothing that opening,
  // step_mode and closing read changes inside a trajectory (sort_direct may: forward_rest gathers the facts again).
  struct Traj {
    PathFacts f;
    TrajPlan p;
    double a, c_za;
    bool pair;  // the Zel'dovich boundaries leave Psi^_x | B (psi_pair)
    bool xt;    // a fused trajectory keeps its state and weights in x-column tiles (x_tiles, xtile.hpp)
  };
  static Traj traj(bchmc_handle *h) {
    Traj t;
    t.f = path_facts(h, h->c.rsd_model);
    t.p = traj_plan(t.f, h->sw);
    t.a = h->c.grad_psi_prior_factor;
    t.c_za = (t.p.c_za == CZa::kAlptInput ? 1. : -h->c.D1) * h->c.deltaQ_factor / (double)h->g.N;
    t.pair = psi_pair(t.f, h->sw, t.p);
    t.xt = x_tiles(t.f, h->sw, t.p);
    return t;
  }

  // k_step_boundary_x for this grid, one tile per workgroup
  template <int MODE, bool ALPT = false, bool XT = false>
  static int launch_boundary_x(bchmc_handle *h, BoundaryX<T> bx) {
    // the forward side of this boundary reads what the last forward transform left in Ck: V^_x | W, or three arrays
    if (MODE != BX_FIRST) {
      if (ALPT && h->ck_vpair) return h->fail(BCHMC_ERR_STATE, "two arrays of V^ in Ck, and a boundary that reads three");
      bx.vpair = h->ck_vpair;
      h->ck_vpair = false;
    }
    HIPCHK((launch_step_boundary_x<T, MODE, ALPT, XT>(pass_ctx(h), C(h->Ck), h->wS, bx)));
    h->ck_pair = bx.pair && !ALPT && MODE != BX_LAST;  // as launch_step_boundary_x told the kernel
    return BCHMC_OK;
  }

  // gradient_psi at the trajectory's start state q^ = qk (HMC.cc:279-280) into gk; needs nothing of the momenta.
  // like_i: where to leave the -log L partials of this evaluation's forward model (may be null).
  static int initial_force(bchmc_handle *h, const Traj &t, double *like_i, void *g0_out) {
    int like_mode = 2;
    double b = 0.;
    const InitialEval kind = initial_eval(t.f, h->sw, t.p);
    if (kind == InitialEval::k3d) {
      CHK(force_sources(h, false, EvalMode{}, &like_mode, &b));
      if (like_i) CHK(tap_loglike(h, like_i));
      CHK(launch_assemble<false>(h, t.a, b, like_mode, 0., nullptr));
    } else {
      // the same evaluation on the 2-D plans: Psi^ with its inverse x passes, V^ assembled after forward x passes
      StepCtl nc{h->stop, h->steps_done, nullptr, 0., 0};
      {
        ProfScope ps(h, BCHMC_K_KSPACE_DRIFT_ZA);
        BoundaryX<T> bx;
        bx.qi = C(h->qk), bx.c_za = t.c_za, bx.ctl = nc, bx.pair = t.pair;
        if (kind == InitialEval::kBxFirstAlpt) CHK((launch_boundary_x<BX_FIRST, true>(h, bx)));
        else CHK(launch_boundary_x<BX_FIRST>(h, bx));
      }
      EvalMode m;
      m.planes_c2r = m.planes_r2c = true;
      m.alpt_pending = t.p.alpt_x;
      CHK(force_sources(h, true, m, &like_mode, &b));
      if (like_mode != 0) return h->fail(BCHMC_ERR_STATE, "planes mode without the three V components");
      if (like_i) CHK(tap_loglike(h, like_i));
      h->prop_g_valid = false;
      ProfScope ps(h, BCHMC_K_KSPACE_FORCE_KICK);
      BoundaryX<T> bx;
      bx.qi = C(h->qk), bx.a = t.a, bx.b = b, bx.ctl = nc, bx.g_out = C(h->gk);
      CHK(launch_boundary_x<BX_LAST>(h, bx));
    }
    if (g0_out)
      HIPCHK(hipMemcpyAsync(g0_out, h->gk, 2 * (size_t)h->g.Nhp * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    return BCHMC_OK;
  }

  // Hamiltonian_EoM (HMC.cc:275-365) on the k-space state already in (qk, pk).
  // g0_in: the gradient at the start state if the caller has it (the evaluation of HMC.cc:279 is skipped);
  // g0_out: where to keep a copy of it when it is evaluated here.
  static int trajectory(bchmc_handle *h, double eps, uint64_t neps, const Tap *tap, const void *g0_in = nullptr,
                        void *g0_out = nullptr) {
    h->prop_g_valid = false;
    if (neps + 1 > h->guard.capacity())  // generous: a reallocation synchronises the device
      CHK(dev_reserve(h, h->guard, std::max<size_t>(4096, 2 * (neps + 1))));
    HIPCHK(hipMemsetAsync(h->guard, 0, (neps + 1) * sizeof(double), h->stream));
    k_init_ctl<<<1, 1, 0, h->stream>>>(h->stop, h->steps_done, (unsigned long long)neps);
    HIPCHK(hipGetLastError());

    const Traj t = traj(h);
    int like_mode = 2;
    double b = 0.;
    // 0) gradient at t = 0 (HMC.cc:279-280)
    if (!g0_in) CHK(initial_force(h, t, tap ? tap->like_i : nullptr, g0_out));
    const void *g_first = g0_in ? g0_in : h->gk;
    if (neps == 0) return BCHMC_OK;  // HMC.cc:284 loops zero times: the state is returned as it came

    if (t.p.fused) return trajectory_fused(h, eps, neps, tap, t, g_first);
    const double *wM = h->mass_fs ? h->wM : nullptr;
    const double guard_limit = 1e50 * (double)h->g.N;
    for (uint64_t s = 0; s < neps; s++) {
      StepCtl ctl{h->stop, h->steps_done, s > 0 ? h->guard + (s - 1) : nullptr, guard_limit, s};
      if (!h->mass_rs) {
        ProfScope ps(h, BCHMC_K_KSPACE_DRIFT_ZA);
        k_kick_drift_za<T, true><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(
            h->g, C(h->qk), C(h->pk), C(s == 0 ? g_first : h->gk), wM, nullptr, C(h->Ck), 0.5 * eps, eps, t.c_za, ctl);
        HIPCHK(hipGetLastError());
      } else {
        // kick first (needs p in real space for the mass_r term), then drift with the extra term
        {
          ProfScope ps(h, BCHMC_K_KSPACE_DRIFT_ZA);
          k_kick_drift_za<T, true><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(
              h->g, C(h->qk), C(h->pk), C(s == 0 ? g_first : h->gk), nullptr, nullptr, C(h->Ck), 0.5 * eps, 0., t.c_za,
              ctl);
          HIPCHK(hipGetLastError());
        }
        CHK(mass_rs_term(h));
        StepCtl ctl2{h->stop, h->steps_done, nullptr, 0., s};
        ProfScope ps(h, BCHMC_K_KSPACE_DRIFT_ZA);
        k_kick_drift_za<T, true><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, C(h->qk), C(h->pk), C(h->gk), wM,
                                                                             C(h->tC), C(h->Ck), 0., eps, t.c_za, ctl2);
        HIPCHK(hipGetLastError());
      }
      CHK(force_sources(h, t.p.fused_za, EvalMode{}, &like_mode, &b));
      if (tap && tap->like_f && s + 1 == neps) CHK(tap_loglike(h, tap->like_f));
      CHK(launch_assemble<true>(h, t.a, b, like_mode, 0.5 * eps, h->guard + s));
    }
    return BCHMC_OK;
  }

  // The same trajectory with every interior "second half kick | first half kick + drift + Zel'dovich" pair done by
  // one kernel (k_step_boundary) on ping-pong state buffers.  Used for k-space masses and forward-model likelihoods.
  // Which kernel opens it, how each step's force evaluation runs and which kernel closes the step: eval_plan.hpp.
  static int trajectory_fused(bchmc_handle *h, double eps, uint64_t neps, const Tap *tap, const Traj &t,
                              const void *g_first) {
    const double *wM = h->mass_fs ? h->wM : nullptr;
    const double guard_limit = 1e50 * (double)h->g.N, a = t.a, c_za = t.c_za;
    if (!h->qk2) {
      CHK(dev_alloc(h, h->qk2, 2 * (size_t)h->g.Nhp * sizeof(T)));
      CHK(dev_alloc(h, h->pk2, 2 * (size_t)h->g.Nhp * sizeof(T)));
    }
    // Between the opening and the closing boundary the pairs may hold the x-column tile layout (xtile.hpp): `xp` follows
    // which pair holds what, launch by launch, and a kernel that would read one layout as the other is refused.
    const bool xt = t.xt;
    const char *const wrong_layout = "a k-space state pair in one layout, and a kernel that reads the other";
    if (h->qk_layout != XLayout::kNatural) return h->fail(BCHMC_ERR_STATE, wrong_layout);
    if (xt) CHK(tiled_weights(h));
    XPairs xp;
    void *const qb[2] = {h->qk, h->qk2}, *const pb[2] = {h->pk, h->pk2};
    int like_mode = 2;
    double b = 0.;
    {
      const Opening op = opening(t.f, h->sw, t.p);
      if (!xp.open(xt, op == Opening::kBxFirst)) return h->fail(BCHMC_ERR_STATE, wrong_layout);
      StepCtl ctl{h->stop, h->steps_done, nullptr, guard_limit, 0};
      ProfScope ps(h, BCHMC_K_KSPACE_DRIFT_ZA);
      BoundaryX<T> bx;  // natural: in place; tiled: pair 0 natural -> pair 1 tiled
      bx.qi = C(qb[0]), bx.pi = C(pb[0]), bx.qo = C(qb[xp.cur]), bx.po = C(pb[xp.cur]), bx.wM = wM, bx.wpair = h->wpair;
      bx.half_eps = 0.5 * eps, bx.eps = eps, bx.c_za = c_za;
      bx.ctl = ctl, bx.g_in = C(g_first), bx.pair = t.pair;
      switch (op) {
        case Opening::kBxFirstAlpt: CHK((launch_boundary_x<BX_FIRST, true>(h, bx))); break;
        case Opening::kBxFirst:
          if (xt) CHK((launch_boundary_x<BX_FIRST, false, true>(h, bx)));
          else CHK(launch_boundary_x<BX_FIRST>(h, bx));
          break;
        case Opening::kKickDriftZa:
          h->ck_pair = false;
          k_kick_drift_za<T, true><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, C(qb[0]), C(pb[0]), C(g_first), wM,
                                                                               nullptr, C(h->Ck), 0.5 * eps, eps, c_za, ctl);
          break;
      }
      HIPCHK(hipGetLastError());
    }
    for (uint64_t s = 0; s < neps; s++) {
      const bool last = (s + 1 == neps);
      if (last && h->early_q_dev && h->ev_q) {
        // the last boundary only kicks p: this is the final q (unless the runaway guard stops the trajectory, which the
        // caller checks).  Its real-space copy is made now, so that its transfer to the host runs beside the force
        // evaluation that follows.
        CHK(c2r_state(h, qb[xp.cur], h->ioq, h->early_q_dev, xp.q[xp.cur] == XLayout::kTiled));
        HIPCHK(hipEventRecord(h->ev_q, h->stream));
        h->early_q_done = true;
      }
      if (h->plan.slots.slot_watch && h->plan.tiled && h->plan.slots.sort_direct && s > 0 && s % kSlotPoll == 0)
        CHK(poll_slots(h, s / kSlotPoll));
      CHK(force_sources(h, true, step_mode(t.f, h->sw, t.p, s, neps), &like_mode, &b));
      if (tap && tap->like_f && last) CHK(tap_loglike(h, tap->like_f));
      StepCtl ctl{h->stop, h->steps_done, s > 0 ? h->guard + (s - 1) : nullptr, guard_limit, s};
      const Closing cl = closing(t.f, h->sw, t.p, s, neps, like_mode);
      const int src = xp.cur, dst = xp.dst(xt, last);
      if (!xp.close(xt, cl, last)) return h->fail(BCHMC_ERR_STATE, wrong_layout);
      void *qi = qb[src], *pi = pb[src], *qo = qb[src ^ 1], *po = pb[src ^ 1];
      ProfScope ps(h, BCHMC_K_KSPACE_FORCE_KICK);
      BoundaryX<T> bx;  // the interior boundary; the last one writes p (natural: in place), no q, and leaves the gradient in gk
      bx.qi = C(qi), bx.pi = C(pi), bx.qo = C(qo), bx.po = C(po), bx.wM = wM, bx.a = a, bx.b = b, bx.half_eps = 0.5 * eps;
      bx.eps = eps, bx.c_za = c_za, bx.guard_slot = h->guard + s, bx.ctl = ctl, bx.pair = t.pair, bx.wpair = h->wpair;
      switch (cl) {
        case Closing::kBxLast:
          bx.qo = nullptr, bx.po = C(pb[dst]), bx.g_out = C(h->gk);
          if (xt) CHK((launch_boundary_x<BX_LAST, false, true>(h, bx)));
          else CHK(launch_boundary_x<BX_LAST>(h, bx));
          break;
        case Closing::kStepBoundaryLast:
          if (h->ck_vpair) return h->fail(BCHMC_ERR_STATE, "two arrays of V^ in Ck, and a boundary that reads three");
          k_step_boundary<T, true><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(
              h->g, C(h->Ck), C(qi), C(pi), C(qi), C(pi), C(h->gk), h->wS, wM, a, b, like_mode, 0.5 * eps, eps, c_za,
              h->guard + s, ctl);
          break;
        case Closing::kBxInteriorAlpt: CHK((launch_boundary_x<BX_INTERIOR, true>(h, bx))); break;
        case Closing::kBxInterior:
          if (xt) CHK((launch_boundary_x<BX_INTERIOR, false, true>(h, bx)));
          else CHK(launch_boundary_x<BX_INTERIOR>(h, bx));
          break;
        case Closing::kBxInteriorTwoTile:
          bx.vpair = h->ck_vpair;
          h->ck_vpair = false;
          if (xt) HIPCHK((launch_step_boundary_x2<T, true>(pass_ctx(h), C(h->Ck), h->wS, bx)));
          else HIPCHK(launch_step_boundary_x2<T>(pass_ctx(h), C(h->Ck), h->wS, bx));
          h->ck_pair = bx.pair;
          break;
        case Closing::kStepBoundary:
          if (h->ck_vpair) return h->fail(BCHMC_ERR_STATE, "two arrays of V^ in Ck, and a boundary that reads three");
          k_step_boundary<T, false><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(
              h->g, C(h->Ck), C(qi), C(pi), C(qo), C(po), C(h->gk), h->wS, wM, a, b, like_mode, 0.5 * eps, eps, c_za,
              h->guard + s, ctl);
          break;
      }
      HIPCHK(hipGetLastError());
    }
    const int fin = xp.cur, res = xp.result(xt);
    if (!xp.finish(xt)) return h->fail(BCHMC_ERR_STATE, wrong_layout);
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      if (xt) {
        // the final q, or the state a guard stop rolls back to, out of the tiles: natural in pair `res`.  Ck is dead after
        // the last boundary; its first two components are the stop path's scratch.
        CT *const sq = C(h->Ck), *const sp = C(h->Ck) + h->g.Nhp;
        k_xtile_finish<T><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, h->stop, h->steps_done, C(qb[0]), C(pb[0]),
                                                                       C(qb[1]), C(pb[1]), fin, C(qb[res]), sq, sp);
        HIPCHK(hipGetLastError());
        k_xtile_restore<T><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g.Nhp, h->stop, sq, sp, C(qb[res]), C(pb[res]));
      } else {
        k_rollback<T><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g.Nhp, h->stop, h->steps_done, C(qb[0]), C(pb[0]),
                                                                   C(qb[1]), C(pb[1]), C(qb[res]), C(pb[res]));
      }
      HIPCHK(hipGetLastError());
    }
    h->qk_layout = xp.q[res];  // natural: finish() has checked it
    if (res) {
      std::swap(h->qk, h->qk2);
      std::swap(h->pk, h->pk2);
    }
    return BCHMC_OK;
  }

  // {wS, wM} in x-column tiles for the tiled boundary kernels: made on first use and again after an upload of either
  static int tiled_weights(bchmc_handle *h) {
    if (!h->wpair) CHK(dev_alloc(h, h->wpair, (size_t)h->g.Nhp));
    else if (h->wpair_gen == h->w_gen) return BCHMC_OK;
    ProfScope ps(h, BCHMC_K_OTHER);
    k_xtile_weights<<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, pass_kb((int)sizeof(T)), h->wS, h->wM, h->wpair);
    HIPCHK(hipGetLastError());
    h->wpair_gen = h->w_gen;
    return BCHMC_OK;
  }

  // prologue_done: plain_prologue has run (FFT[q0] is in qk and gk holds the gradient at the start state)
  static int leapfrog_core(bchmc_handle *h, const double *d_q0, const double *d_p0, double *d_q1, double *d_p1,
                           double eps, uint64_t neps, bool prologue_done = false) {
    CHK(check_inputs(h));
    if (eps > 2.) eps = 2.;  // HMC.cc:263-264
    if (!prologue_done) CHK(r2c_state(h, d_q0, h->ioq, h->qk));
    CHK(r2c_state(h, d_p0, h->iop, h->pk));
    CHK(trajectory(h, eps, neps, nullptr, prologue_done ? h->gk : nullptr));
    if (!h->early_q_done) CHK(c2r_state(h, h->qk, h->ioq, d_q1));  // else: made before the last force evaluation
    CHK(c2r_state(h, h->pk, h->iop, d_p1));
    return BCHMC_OK;
  }
  // the runaway guard stopped a trajectory whose q had been sent early: transform the state it stopped in
  static int requeue_q(bchmc_handle *h, double *d_q1) { return c2r_state(h, h->qk, h->ioq, d_q1); }

  // ---- device-resident chain --------------------------------------------------------------------------------
  static int chain_alloc(bchmc_handle *h) {
    if (!h->cq) {
      CHK(dev_alloc(h, h->cq, 2 * (size_t)h->g.Nhp * sizeof(T)));
      CHK(dev_alloc(h, h->cp, 2 * (size_t)h->g.Nhp * sizeof(T)));
      CHK(dev_alloc(h, h->part6, (size_t)6 * kRedBlocks));
    }
    return BCHMC_OK;
  }

  // p ~ N(0, M): coloured white noise, entirely on the device.
  static int chain_draw(bchmc_handle *h, uint64_t seed, uint64_t attempt) {
    const long long N = h->g.N, Nh = h->g.Nhp;
    const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32));
    ProfScope ps(h, BCHMC_K_OTHER);
    if (h->mass_fs) {
      k_white_noise<T><<<nblk_stride((N + 1) / 2), 256, 0, h->stream>>>(N, key, (unsigned)attempt, 0u, nullptr, R(h->iop));
      HIPCHK(hipGetLastError());
      CHK(fft_exec(h, h->r2c1, h->iop, h->tC, BCHMC_K_FFT_R2C));
      k_color_momenta<T><<<nblk_stride(Nh), 256, 0, h->stream>>>(Nh, C(h->tC), h->wM, C(h->cp), 0);
      HIPCHK(hipGetLastError());
    } else {
      HIPCHK(hipMemsetAsync(h->cp, 0, 2 * (size_t)Nh * sizeof(T), h->stream));
    }
    if (h->mass_rs) {
      k_white_noise<T><<<nblk_stride((N + 1) / 2), 256, 0, h->stream>>>(N, key, (unsigned)attempt, 1u,
                                                                        R(h->in_arr[BCHMC_F_MASS_R]), R(h->iop));
      HIPCHK(hipGetLastError());
      CHK(fft_exec(h, h->r2c1, h->iop, h->tC, BCHMC_K_FFT_R2C));
      k_color_momenta<T><<<nblk_stride(Nh), 256, 0, h->stream>>>(Nh, C(h->tC), nullptr, C(h->cp), 1);
      HIPCHK(hipGetLastError());
    }
    return BCHMC_OK;
  }

  // dstage = the real-space copy of the resident momenta; after a draw for a real-space mass alone, exactly 0 where that
  // mass is not positive, as the draw itself was (the resident form is k-space, and the way back leaves round-off there)
  static int momenta_to_stage(bchmc_handle *h) {
    CHK(c2r_state(h, h->cp, h->ioq, h->dstage));
    if (h->cp_draw_rs) {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_zero_closed<T><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g.N, R(h->in_arr[BCHMC_F_MASS_R]), h->dstage);
      HIPCHK(hipGetLastError());
    }
    return BCHMC_OK;
  }

  // log_like's forward model equals the force's one iff these hold (gaussian_independent.cpp:57-76 vs
  // poissonian.cpp:54-56, lognormal_independent.cpp:105-107); then the -log L of both trajectory ends can be tapped
  // from the trajectory's own first and last force evaluation, and K, psi_prior are Parseval sums of the k-space
  // state.  Otherwise, and for the real-space terms (GRF likelihood, mass_r kinetic term): generic energy evaluation.
  static bool attempt_is_fast(const bchmc_handle *h, uint64_t neps) {
    const bool like_shared = h->c.likelihood == 1 || ((h->c.likelihood == 0 || h->c.likelihood == 2) &&
                                                       h->c.deltaQ_factor == 1. && !h->c.rsd_model);
    return like_shared && !h->mass_rs && neps >= 1;
  }

  // Hamiltonian_EoM + delta_Hamiltonian in one pass.  Start state: fast mode -> (qk, pk) in k-space, set by the caller;
  // generic mode -> (d_q0, d_p0), ABI doubles in real space, optionally with the exact k-space state to restart from
  // in (src_qk, src_pk).  The proposal stays in (qk, pk); with want_real the generic mode's real-space copy of it is
  // left in dstage (fast mode: the caller transforms).
  // Fast mode only: g0_in / like0 = the gradient and -log L at the start state when the caller carries them;
  // g0_out = where to keep the gradient at the start state otherwise.
  // g0_ready (fast mode): gk already holds the gradient at the start state and the partials of its -log L are in
  // part6's third slot (host_prologue evaluated them while the momenta were still on their way).
  static int attempt_core(bchmc_handle *h, double eps, uint64_t neps, const double *d_q0, const double *d_p0,
                          const void *src_qk, const void *src_pk, double terms[6], uint64_t *steps_done,
                          const void *g0_in = nullptr, double like0 = 0., void *g0_out = nullptr, bool g0_ready = false,
                          double *host_q1 = nullptr) {
    CHK(check_inputs(h));
    if (eps > 2.) eps = 2.;
    const size_t cbytes = 2 * (size_t)h->g.Nhp * sizeof(T);
    const double N = (double)h->g.N;
    const bool fast = attempt_is_fast(h, neps);
    if (!h->part6) CHK(dev_alloc(h, h->part6, (size_t)6 * kRedBlocks));
    double *P = h->part6;
    if (!fast) {
      CHK(energies_core(h, d_q0, d_p0, terms));  // leaves FFT[q0], FFT[p0] in (qk, pk)
      if (src_qk) {
        HIPCHK(hipMemcpyAsync(h->qk, src_qk, cbytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->pk, src_pk, cbytes, hipMemcpyDeviceToDevice, h->stream));
      }
    } else {
      k_parseval<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g, C(h->pk), h->wM, P);
      k_parseval<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g, C(h->qk), h->wS, P + kRedBlocks);
      HIPCHK(hipGetLastError());
    }
    if (g0_ready && fast) g0_in = h->gk;
    Tap tap{g0_in ? nullptr : P + 2 * kRedBlocks, P + 5 * kRedBlocks};
    if (g0_in && !g0_ready) HIPCHK(hipMemsetAsync(P + 2 * kRedBlocks, 0, kRedBlocks * sizeof(double), h->stream));
    CHK(trajectory(h, eps, neps, fast ? &tap : nullptr, fast ? g0_in : nullptr, fast ? g0_out : nullptr));
    uint64_t done = 0;
    if (fast) {
      k_parseval<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g, C(h->pk), h->wM, P + 3 * kRedBlocks);
      k_parseval<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g, C(h->qk), h->wS, P + 4 * kRedBlocks);
      HIPCHK(hipGetLastError());
      if (host_q1) {
        // host-array trajectory: the proposal's real-space copies go to dstage (q, unless the trajectory made it
        // early) and dstage + N (p); everything is enqueued before this thread starts moving q1 across PCIe
        if (!h->early_q_done) CHK(c2r_state(h, h->qk, h->ioq, h->dstage));
        CHK(c2r_state(h, h->pk, h->iop, h->dstage + h->g.N));
      }
      // (before the copy of the partials below: a device-to-host copy into pageable memory returns when it is done)
      if (host_q1 && h->early_q_done)
        CHK(d2h(h, host_q1, h->dstage, (size_t)h->g.N * sizeof(double), h->copy_stream, h->ev_q));
      std::vector<double> hp(6 * kRedBlocks);
      unsigned long long sd = 0;
      HIPCHK(hipMemcpyAsync(hp.data(), P, hp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      CHK(read_ctl(h, &sd));
      done = sd;
      for (int t = 0; t < 6; t++) {
        double s = 0.;
        for (int i = 0; i < kRedBlocks; i++) s += hp[(size_t)t * kRedBlocks + i];
        terms[t] = (t == 0 || t == 1 || t == 3 || t == 4) ? s / (2. * N) : s;
      }
      if (g0_in && !g0_ready) terms[2] = like0;
      if (done < neps) {
        if (host_q1 && h->early_q_done) {  // ... and the q sent early is not the state the trajectory stopped in
          h->early_q_done = false;
          CHK(c2r_state(h, h->qk, h->ioq, h->dstage));
        }
        // runaway guard fired (HMC.cc:360-364): the tapped forward model is not the final state's; redo it
        EvalMode m;
        CHK(displacement(h, h->c.likelihood == 1 ? h->c.deltaQ_factor : 1., h->c.likelihood == 1 ? h->c.rsd_model : 0,
                         &m.planes_c2r));
        CHK(forward_rest(h, h->c.likelihood == 1 ? h->c.rsd_model : 0, m));
        CHK(tap_loglike(h, P));
        CHK(host_sum(h, P, &terms[5]));
      }
    } else {
      unsigned long long sd = 0;
      CHK(read_ctl(h, &sd));
      done = sd;
      // keep the proposal: energies_core re-transforms into (qk, pk), which reproduces it to round-off
      CHK(c2r_state(h, h->qk, h->ioq, h->dstage));
      CHK(c2r_state(h, h->pk, h->iop, h->dstage + h->g.N));
      CHK(energies_core(h, h->dstage, h->dstage + h->g.N, terms + 3));
    }
    if (steps_done) *steps_done = done;
    return BCHMC_OK;
  }

  // The resident chain's attempt: from (cq, cp).
  static int chain_attempt(bchmc_handle *h, double eps, uint64_t neps, double terms[6], uint64_t *steps_done) {
    const size_t cbytes = 2 * (size_t)h->g.Nhp * sizeof(T);
    if (attempt_is_fast(h, neps)) {
      HIPCHK(hipMemcpyAsync(h->qk, h->cq, cbytes, hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(hipMemcpyAsync(h->pk, h->cp, cbytes, hipMemcpyDeviceToDevice, h->stream));
      const bool use = !env_on("BCHMC_NO_FORCE_CARRY"), carry = use && h->cg_valid;
      if (use && !h->cg) CHK(dev_alloc(h, h->cg, cbytes));
      uint64_t done = 0;
      CHK(attempt_core(h, eps, neps, nullptr, nullptr, nullptr, nullptr, terms, &done, carry ? h->cg : nullptr,
                       h->c_like, (use && !carry) ? h->cg : nullptr));
      if (steps_done) *steps_done = done;
      if (use && !carry) {
        h->cg_valid = true;
        h->c_like = terms[2];
      }
      // gk holds the gradient at the proposal (the last step's evaluation) unless the runaway guard cut the trajectory
      h->prop_g_valid = use && done == neps;
      h->prop_like = terms[5];
    } else {
      h->cg_valid = h->prop_g_valid = false;
      CHK(c2r_state(h, h->cq, h->ioq, h->dstage));
      CHK(c2r_state(h, h->cp, h->iop, h->dstage + h->g.N));
      CHK(attempt_core(h, eps, neps, h->dstage, h->dstage + h->g.N, h->cq, h->cp, terms, steps_done));
    }
    h->have_prop = true;
    return BCHMC_OK;
  }

  // Hamiltonian_EoM for host arrays already staged in dstage (q0) and dstage + N (p0): the same single pass, so the
  // energies of both ends come with it (bchmc_leapfrog_dh hands them to the caller, who asks for them next,
  // HMC.cc:455-459).  Leaves (q1, p1) in dstage, dstage + N.
  // prologue_done: host_prologue has run (FFT[q0] is in qk, gk and the -log L partials are the start state's).
  // host_q1: the caller's q1 array.  With the early download armed (early_q_dev) it is filled here, beside the last
  // force evaluation, and h->early_q_done stays set; otherwise the caller copies it from dstage as before.
  static int leapfrog_host_core(bchmc_handle *h, double eps, uint64_t neps, double terms[6], uint64_t *steps_done,
                                bool prologue_done, double *host_q1) {
    double *dq = h->dstage, *dp = h->dstage + h->g.N;
    if (attempt_is_fast(h, neps)) {
      if (!prologue_done) CHK(r2c_state(h, dq, h->ioq, h->qk));
      CHK(r2c_state(h, dp, h->iop, h->pk));
      CHK(attempt_core(h, eps, neps, nullptr, nullptr, nullptr, nullptr, terms, steps_done, nullptr, 0., nullptr,
                       prologue_done, host_q1));
    } else {
      // generic mode: energies_core transforms the staged arrays itself (it only reads dstage), and after the
      // trajectory attempt_core leaves the proposal's real-space copy there
      CHK(attempt_core(h, eps, neps, dq, dp, nullptr, nullptr, terms, steps_done));
    }
    return BCHMC_OK;
  }

  // Everything of a host-array trajectory that needs q0 only -- its transform and the force evaluation of HMC.cc:279 --
  // enqueued before the momenta are uploaded, so that their PCIe transfer (3 ms per 134 MB array) runs beside it.
  static int host_prologue(bchmc_handle *h) {
    CHK(check_inputs(h));
    if (!h->part6) CHK(dev_alloc(h, h->part6, (size_t)6 * kRedBlocks));
    k_init_ctl<<<1, 1, 0, h->stream>>>(h->stop, h->steps_done, 0ull);  // a stop flag left by an earlier trajectory
    HIPCHK(hipGetLastError());
    CHK(r2c_state(h, h->dstage, h->ioq, h->qk));
    return initial_force(h, traj(h), h->part6 + 2 * kRedBlocks, nullptr);
  }
  // the same for the plain trajectory (bchmc_leapfrog): no energies, so no -log L partials to keep
  static int plain_prologue(bchmc_handle *h) {
    CHK(check_inputs(h));
    k_init_ctl<<<1, 1, 0, h->stream>>>(h->stop, h->steps_done, 0ull);
    HIPCHK(hipGetLastError());
    CHK(r2c_state(h, h->dstage, h->ioq, h->qk));
    return initial_force(h, traj(h), nullptr, nullptr);
  }
  static bool host_prologue_applies(const bchmc_handle *h, uint64_t neps) {
    return attempt_is_fast(h, neps) && !env_on("BCHMC_NO_UPLOAD_OVERLAP");
  }

  // kinetic_term (HMC.cc:64-121) of the momenta in the ABI (double) device array d_p: 1/2 p^T M^-1 p.
  // Leaves FFT[p] in pk and the T copy of p in iop.  Needs mass_f / mass_r only.
  static int kinetic_core(bchmc_handle *h, const double *d_p, double *out) {
    if (h->mass_fs) CHK(need_input(h, BCHMC_F_MASS_F, "mass_f"));
    if (h->mass_rs) CHK(need_input(h, BCHMC_F_MASS_R, "mass_r"));
    const double N = (double)h->g.N;
    // rocFFT may clobber its input: transform a scratch copy, keep iop intact for the real-space term
    CHK(load_real(h, d_p, R(h->iop)));
    T *scratch = R(h->psi);
    HIPCHK(hipMemcpyAsync(scratch, h->iop, h->g.N * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    CHK(fft_exec(h, h->r2c1, scratch, h->pk, BCHMC_K_FFT_R2C));
    double kin = 0., v;
    if (h->mass_fs) {
      k_parseval<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g, C(h->pk), h->wM, h->partA);
      HIPCHK(hipGetLastError());
      CHK(host_sum(h, h->partA, &v));
      kin += v / (2. * N);
    }
    if (h->mass_rs) {
      k_kin_rs<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g.N, R(h->iop), R(h->in_arr[BCHMC_F_MASS_R]), h->partA);
      HIPCHK(hipGetLastError());
      CHK(host_sum(h, h->partA, &v));
      kin += v;
    }
    *out = kin;
    return BCHMC_OK;
  }

  // psi (HMC.cc:124-143) of the signal in the ABI (double) device array d_q: out = { log_prior, log_like }.
  // Leaves FFT[q] in qk and this evaluation's forward model in rho / psi (hd->deltaX, hd->pos*).
  static int psi_core(bchmc_handle *h, const double *d_q, double out[2]) {
    CHK(need_input(h, BCHMC_F_SIGNAL_PS, "signal_PS"));
    CHK(need_input(h, BCHMC_F_NOBS, "nobs"));
    CHK(need_input(h, BCHMC_F_WINDOW, "window"));
    if (h->c.likelihood != 0) CHK(need_input(h, BCHMC_F_NOISE, "noise"));
    const double N = (double)h->g.N;
    CHK(load_real(h, d_q, R(h->ioq)));
    T *scratch = R(h->psi);
    HIPCHK(hipMemcpyAsync(scratch, h->ioq, h->g.N * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    CHK(fft_exec(h, h->r2c1, scratch, h->qk, BCHMC_K_FFT_R2C));
    double v;
    k_parseval<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g, C(h->qk), h->wS, h->partA);
    HIPCHK(hipGetLastError());
    CHK(host_sum(h, h->partA, &v));
    const double prior = v / (2. * N);
    double like = 0.;
    if (h->c.likelihood == 3) {
      k_grf_loglike<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g.N, R(h->ioq), R(h->in_arr[BCHMC_F_NOBS]),
                                                          R(h->in_arr[BCHMC_F_NOISE]), R(h->in_arr[BCHMC_F_WINDOW]),
                                                          h->partA);
      HIPCHK(hipGetLastError());
      CHK(host_sum(h, h->partA, &like));
    } else {
      // gaussian log_like applies deltaQ_factor and honours rsd_model (gaussian_independent.cpp:57-76);
      // poissonian / log-normal log_like do neither (poissonian.cpp:54-56, lognormal_independent.cpp:105-107)
      const bool gauss = (h->c.likelihood == 1);
      EvalMode m;
      CHK(displacement(h, gauss ? h->c.deltaQ_factor : 1., gauss ? h->c.rsd_model : 0, &m.planes_c2r));
      CHK(forward_rest(h, gauss ? h->c.rsd_model : 0, m));
      k_loglike<T><<<kRedBlocks, 256, 0, h->stream>>>(h->g, make_like(h), R(h->rho), h->rho_part,
                                                      R(h->in_arr[BCHMC_F_NOBS]), R(h->in_arr[BCHMC_F_NOISE]),
                                                      R(h->in_arr[BCHMC_F_WINDOW]), h->partA);
      HIPCHK(hipGetLastError());
      CHK(host_sum(h, h->partA, &like));
    }
    out[0] = prior;
    out[1] = like;
    return BCHMC_OK;
  }

  static int energies_core(bchmc_handle *h, const double *d_q, const double *d_p, double out[3]) {
    CHK(check_inputs(h));
    CHK(kinetic_core(h, d_p, &out[0]));  // first: psi_core's forward model uses the psi scratch afterwards
    return psi_core(h, d_q, &out[1]);
  }

  static int forward(bchmc_handle *h, const double *d_q, int rsd) {
    CHK(r2c_state(h, d_q, h->ioq, h->qk));
    EvalMode m;
    CHK(displacement(h, 1., rsd, &m.planes_c2r));
    return forward_rest(h, rsd, m);
  }

  // Lag2Eul of the resident chain state, from its q^ directly (no transform pair through real space)
  static int chain_forward(bchmc_handle *h, int rsd) {
    HIPCHK(hipMemcpyAsync(h->qk, h->cq, 2 * (size_t)h->g.Nhp * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    EvalMode m;
    CHK(displacement(h, 1., rsd, &m.planes_c2r));
    return forward_rest(h, rsd, m);
  }

  // bchmc_probe_displacement: the particle stage (and the likelihood force up to V) of a displacement given in real
  // space; component c of it is staged in dstage
  static int probe_load(bchmc_handle *h, int c) { return load_real(h, h->dstage, R(h->psi) + (size_t)c * h->g.N); }
  static int probe(bchmc_handle *h, int rsd, bool with_force) {
    EvalMode m;
    CHK(particle_stage(h, rsd, m, false));
    int like_mode = 0;
    if (with_force) CHK(like_force(h, m, &like_mode, false));
    return BCHMC_OK;
  }
  // bchmc_probe_displacement_z: the same through the fused z pass + binning.  Psi / n (exact: n is a power of two) goes
  // through k_zr2c into Ck, in the layout k_ypass leaves there; particle_stage then runs its own launch_zbin.
  static int probe_z(bchmc_handle *h, int rsd, bool with_force, bool store_psi) {
    const int n = h->g.n;
    k_scale_r<T><<<nblk_stride(3 * h->g.N), 256, 0, h->stream>>>(3 * h->g.N, R(h->psi), T(1) / T(n));
    HIPCHK(hipGetLastError());
    HIPCHK(launch_zr2c<T>(pass_ctx(h), R(h->psi), C(h->Ck)));
    EvalMode m;
    m.planes_c2r = m.planes_r2c = true;  // as an interior step: its gather leaves V where the handle's trajectories do
    m.psi_unread = !store_psi;
    CHK(particle_stage(h, rsd, m, true));
    int like_mode = 0;
    if (with_force) CHK(like_force(h, m, &like_mode, false));
    return BCHMC_OK;
  }

  // ---- measure_corr_grid / measure_corr2D (corr.hpp) ----------------------------------------------------------------
  // A(r) = C2R[|x^|^2] / N of the source into ioq.  Scratch: tC, ioq (and dstage for a host signal, already there);
  // qk / pk / gk, the chain's arrays, the inputs and rho / psi are not touched.  C2R destroys its input, so |x^|^2
  // always goes to tC, never back into cq.
  static int corr_field(bchmc_handle *h, int src) {
    const void *xk = h->tC;
    if (src == BCHMC_CORR_HOST) {
      CHK(r2c_state(h, h->dstage, h->ioq, h->tC));
    } else if (src == BCHMC_CORR_CHAIN_STATE) {
      xk = h->cq;
    } else {  // deltaX exactly as bchmc_fetch makes it
      k_overdens<T><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g, R(h->rho), h->rho_part, R(h->ioq));
      HIPCHK(hipGetLastError());
      CHK(fft_exec(h, h->r2c1, h->ioq, h->tC, BCHMC_K_FFT_R2C));
    }
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_corr_abs2<T><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g.Nhp, C(xk), C(h->tC), 1. / (double)h->g.N);
      HIPCHK(hipGetLastError());
    }
    return fft_exec(h, h->c2r1, h->tC, h->ioq, BCHMC_K_FFT_C2R);
  }

  // The 1-D bin sums of A in ioq; the first call for an n_bin also builds rmode / nmode.  One synchronise.
  static int corr1d_bins(bchmc_handle *h, uint64_t n_bin, double *rmode, uint64_t *nmode, double *corr) {
    auto &c = h->corr1;
    const Geo &g = h->g;
    const size_t nb = (size_t)n_bin, words = 5 * nb + 1;
    if (c.acc.capacity() < words) {
      c.n_bin = 0;
      CHK(dev_reserve(h, c.acc, words));
    }
    const bool geom = c.n_bin != n_bin;
    const double dr = corr_dr(g, n_bin);
    const int grid = std::min(nblk_full(g.N), 1024);
    unsigned long long *d_geo = c.acc + 2 * nb + 1;
    std::vector<unsigned long long> hb(words);
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      HIPCHK(hipMemsetAsync(c.acc, 0, (geom ? words : 2 * nb + 1) * sizeof(unsigned long long), h->stream));
      if (geom) {
        // rtot < 2 rmax < 2^(e + 1) and a multiple of ulp(d) >= 2^(e - 62) for n <= 1024: rtot 2^(62 - e) is an integer
        const double rscale = std::ldexp(1., 62 - std::ilogb(g.L / 2 * std::sqrt(3.)));
        k_corr1d<T, true><<<grid, 256, 3 * nb * sizeof(unsigned long long), h->stream>>>(g, nullptr, (int)n_bin, dr,
                                                                                      rscale, d_geo);
      }
      k_corr1d<T, false><<<grid, 256, 2 * nb * sizeof(unsigned long long), h->stream>>>(g, R(h->ioq), (int)n_bin, dr, 0.,
                                                                                     c.acc);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(hb.data(), c.acc, (geom ? words : 2 * nb + 1) * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    const long double limb = (long double)(1ull << kCorrLimb);
    if (geom) {
      const long double rscale = std::ldexp(1.L, 62 - std::ilogb(g.L / 2 * std::sqrt(3.)));
      const unsigned long long *hg = hb.data() + 2 * nb + 1;
      c.rmode.assign(nb, 0.);
      c.nmode.assign(nb, 0);
      for (size_t l = 0; l < nb; l++) {
        c.nmode[l] = hg[2 * nb + l];
        if (c.nmode[l]) {
          const double rsum = (double)(((long double)hg[l] * limb + (long double)hg[nb + l]) / rscale);
          c.rmode[l] = rsum / (double)c.nmode[l];
        }
      }
      c.n_bin = n_bin;
    }
    double sc;
    std::memcpy(&sc, &hb[2 * nb], sizeof sc);
    const double N = (double)g.N;
    for (size_t l = 0; l < nb; l++) {
      rmode[l] = c.rmode[l];
      nmode[l] = c.nmode[l];
      corr[l] = 0.;
      if (c.nmode[l] && sc != sc) corr[l] = sc;  // a non-finite field: NaN, like the host tool's sums
      if (c.nmode[l] && sc > 0.) {
        const double asum = (double)(((long double)(long long)hb[l] * limb + (long double)hb[nb + l]) / (long double)sc);
        corr[l] = asum / ((double)c.nmode[l] * N);
      }
    }
    return BCHMC_OK;
  }

  template <bool GEOM>
  static int launch_corr2d_slices(bchmc_handle *h, bchmc_handle::Corr2 &c, const Geo &g, const T *A) {
    const int n = g.n, bd = std::min(256, (n + 63) / 64 * 64), kpt = (n + bd - 1) / bd;
    const size_t lds = ((size_t)n + n / 2 + 1) * sizeof(double);
    const int *par_start = c.idx + c.nrows;
#define BCHMC_LAUNCH_C2(KPT) \
  k_corr2d_slices<T, KPT, GEOM><<<c.nsl, bd, lds, h->stream>>>(g, A, c.idx, c.slices, par_start, c.npb, c.part)
    if (kpt == 1) BCHMC_LAUNCH_C2(1);
    else if (kpt == 2) BCHMC_LAUNCH_C2(2);
    else BCHMC_LAUNCH_C2(4);
#undef BCHMC_LAUNCH_C2
    const int *perp_slice = par_start + c.npb + 1;
    k_corr2d_reduce<<<nblk_stride((long long)c.n_bin * c.npb), 256, 0, h->stream>>>(
        c.part, perp_slice, (int)c.n_bin, c.npb, c.out + (GEOM ? 0 : (size_t)c.n_bin * c.npb));
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // The 2-D bin sums of A on grid g (corr2d_setup has run for c and g).  One synchronise.
  static int corr2d_bins(bchmc_handle *h, bchmc_handle::Corr2 &c, const Geo &g, const void *A_T, uint64_t n_bin,
                         double *rmode, uint64_t *nmode, double *corr) {
    const T *A = reinterpret_cast<const T *>(A_T);
    const size_t nb = (size_t)n_bin, cells = nb * c.npb;
    const bool geom = c.rsum.empty();
    std::vector<double> hb(cells), hr(geom ? cells : 0);
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      if (geom) {
        CHK(launch_corr2d_slices<true>(h, c, g, A));
        HIPCHK(hipMemcpyAsync(hr.data(), c.out, cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      }
      CHK(launch_corr2d_slices<false>(h, c, g, A));
      HIPCHK(hipMemcpyAsync(hb.data(), c.out + cells, cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (geom) c.rsum.swap(hr);
    std::memset(rmode, 0, nb * nb * sizeof(double));
    std::memset(corr, 0, nb * nb * sizeof(double));
    std::memset(nmode, 0, nb * nb * sizeof(uint64_t));
    const double N = (double)g.N;
    for (size_t p = 0; p < nb; p++) {
      if (!c.row_cnt[p]) continue;
      for (int q = 0; q < c.npb; q++) {
        const uint64_t nm = c.row_cnt[p] * c.par_cnt[q];
        const size_t ii = (size_t)c.par_bin[q] + nb * p;  // 2D_corr_fct.cc:87
        nmode[ii] = nm;
        rmode[ii] = c.rsum[p * c.npb + q] / (double)nm;
        corr[ii] = hb[p * c.npb + q] / ((double)nm * N);
      }
    }
    return BCHMC_OK;
  }

  // ---- interp_field and tools/2D_corr_fct_interp.cc on the fine grid (upres.hpp; upres_setup has run) -----------------
  // The source as a real field of T in ioq, as corr_field takes it (a host signal is in dstage; the chain state goes
  // through tC like chain_fetch's c2r_state).  Scratch only: tC, ioq.
  static int upres_real(bchmc_handle *h, int src) {
    if (src == BCHMC_CORR_HOST) return load_real(h, h->dstage, R(h->ioq));
    if (src == BCHMC_CORR_CHAIN_STATE) return c2r_scaled(h, h->cq, h->ioq);
    k_overdens<T><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g, R(h->rho), h->rho_part, R(h->ioq));
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // interp_field of the source onto the fine grid's real array
  static int upres_interp(bchmc_handle *h, int src) {
    auto &u = h->up;
    CHK(upres_real(h, src));
    ProfScope ps(h, BCHMC_K_OTHER);
    const int n = h->g.n, no = u.n_out, bd = std::min(256, (no + 63) / 64 * 64);
    k_interp_cic<T><<<no * no, bd, 4 * (size_t)n * sizeof(T), h->stream>>>(n, no, R(h->ioq), R(u.real), u.cell, u.cell + no,
                                                                            u.dx);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // the fine real array -> n_out^3 host doubles; returns when `out` is complete
  static int upres_fetch(bchmc_handle *h, double *out) {
    auto &u = h->up;
    const size_t N = (size_t)u.g.N;
    if (kDouble) return d2h(h, out, u.real, N * sizeof(double));
    std::vector<T> tmp(N);
    CHK(d2h(h, tmp.data(), u.real, N * sizeof(T)));
    for (size_t i = 0; i < N; i++) out[i] = (double)tmp[i];
    return BCHMC_OK;
  }

  // mode 0: A = C2R[|R2C interp_field(source)|^2 / N_out] into the fine real array
  static int upres_corr_cic(bchmc_handle *h, int src) {
    auto &u = h->up;
    CHK(upres_interp(h, src));
    CHK(fft_exec(h, u.r2c, u.real, u.half, BCHMC_K_FFT_R2C, u.info));
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_corr_abs2<T><<<nblk_stride(u.g.Nhp), 256, 0, h->stream>>>(u.g.Nhp, C(u.half), C(u.half), 1. / (double)u.g.N);
      HIPCHK(hipGetLastError());
    }
    return fft_exec(h, u.c2r, u.half, u.real, BCHMC_K_FFT_C2R, u.info);
  }

  // mode 1: A = C2R[zero-padded |x^|^2 / N_out] into the fine real array; x^ as corr_field takes it (no transform for the
  // chain state)
  static int upres_corr_zeropad(bchmc_handle *h, int src) {
    auto &u = h->up;
    const void *xk = h->tC;
    if (src == BCHMC_CORR_HOST) {
      CHK(r2c_state(h, h->dstage, h->ioq, h->tC));
    } else if (src == BCHMC_CORR_CHAIN_STATE) {
      xk = h->cq;
    } else {
      CHK(upres_real(h, src));
      CHK(fft_exec(h, h->r2c1, h->ioq, h->tC, BCHMC_K_FFT_R2C));
    }
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_zeropad_embed<T><<<nblk_stride(u.g.Nhp), 256, 0, h->stream>>>(h->g, u.g, C(xk), C(u.half), 1. / (double)u.g.N);
      HIPCHK(hipGetLastError());
    }
    return fft_exec(h, u.c2r, u.half, u.real, BCHMC_K_FFT_C2R, u.info);
  }

  // the transform of the source for bchmc_measure_spectrum_src, as corr_field takes it
  static int spectrum_source(bchmc_handle *h, int src, const void **xk) {
    *xk = h->tC;
    if (src == BCHMC_CORR_HOST) return r2c_state(h, h->dstage, h->ioq, h->tC);
    if (src == BCHMC_CORR_CHAIN_STATE) {
      *xk = h->cq;
      return BCHMC_OK;
    }
    CHK(upres_real(h, src));
    return fft_exec(h, h->r2c1, h->ioq, h->tC, BCHMC_K_FFT_R2C);
  }

  // One source of bchmc_measure_cross_spectrum: its transform as spectrum_source obtains it, a host signal staged here
  // (the two sources share dstage and ioq, one after the other on the stream), a fresh R2C landing in `out`.
  static int cross_source(bchmc_handle *h, int src, const double *signal, void *out, const void **xk) {
    *xk = out;
    if (src == BCHMC_CORR_HOST) {
      CHK(h2d(h, h->dstage, signal, h->g.N * sizeof(double)));
      return r2c_state(h, h->dstage, h->ioq, out);
    }
    if (src == BCHMC_CORR_CHAIN_STATE) {
      *xk = h->cq;
      return BCHMC_OK;
    }
    CHK(upres_real(h, src));
    return fft_exec(h, h->r2c1, h->ioq, out, BCHMC_K_FFT_R2C);
  }

  // ---- bchmc_ensemble_add (ensemble.hpp) -------------------------------------------------------------------------------
  // One Welford step of a slot from the source: a host signal from its staged doubles in dstage (an fp32 handle loses
  // nothing of it), the chain state and deltaX as a real field of T in ioq, widened on load -- the chain state through
  // c2r_scaled like chain_fetch's c2r_state, deltaX by k_overdens like Pipe::fetch.  Scratch only: tC, ioq.
  static int ens_add(bchmc_handle *h, int src, double *mean, double *m2, double c, int blocks) {
    const long long N = h->g.N;
    if (src != BCHMC_CORR_HOST) CHK(upres_real(h, src));
    ProfScope ps(h, BCHMC_K_OTHER);
    if (src == BCHMC_CORR_HOST)
      k_ens_add<double><<<blocks, kEnsBlock, 0, h->stream>>>(N, h->dstage.get(), mean, m2, c);
    else
      k_ens_add<T><<<blocks, kEnsBlock, 0, h->stream>>>(N, R(h->ioq), mean, m2, c);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // ---- bchmc_tweb_classify (tweb.hpp; tweb_take has run) ----------------------------------------------------------------
  // The six components of the tensor of the source into h->tw.t: x^ as spectrum_source obtains it (a host signal is in
  // dstage; a fresh transform lands in the feature's own half-complex array, because tC is the scratch of the
  // components), then per component one element-wise pass into tC and one C2R.  One k-space array beyond x^ at any time.
  static int tweb_tensor(bchmc_handle *h, int src, double half_r2) {
    auto &w = h->tw;
    const void *xk = w.xk;
    if (src == BCHMC_CORR_HOST) {
      CHK(r2c_state(h, h->dstage, h->ioq, w.xk));
    } else if (src == BCHMC_CORR_CHAIN_STATE) {
      xk = h->cq;
    } else {
      CHK(upres_real(h, src));
      CHK(fft_exec(h, h->r2c1, h->ioq, w.xk, BCHMC_K_FFT_R2C));
    }
    static const int ab[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    for (int c = 0; c < 6; c++) {
      {
        ProfScope ps(h, BCHMC_K_OTHER);
        k_tweb_component<T><<<nblk_stride(h->g.Nhp), kTwebBlock, 0, h->stream>>>(h->g, C(xk), C(h->tC), ab[c][0], ab[c][1],
                                                                                half_r2, 1. / (double)h->g.N);
        HIPCHK(hipGetLastError());
      }
      CHK(fft_exec(h, h->c2r1, h->tC, w.t[c], BCHMC_K_FFT_C2R));
    }
    return BCHMC_OK;
  }

  // Eigenvalues, types and the per-type sums of the tensor in h->tw.t.  The mass weights 1 + x come from the unsmoothed
  // source in real space: the staged doubles of a host signal, else the field of T that upres_real leaves in ioq (tC is
  // free again by now).  lam: h->tw.lam or null.  The result lands in the last kTwebWords of h->tw.part.
  static int tweb_eigen(bchmc_handle *h, int src, double lambda_th, double *lam, int nblk) {
    auto &w = h->tw;
    if (src != BCHMC_CORR_HOST) CHK(upres_real(h, src));
    TwebTensor t;
    for (int c = 0; c < 6; c++) t.c[c] = w.t[c];
    ProfScope ps(h, BCHMC_K_OTHER);
    if (src == BCHMC_CORR_HOST)
      k_tweb_eigen<T, double><<<nblk, kTwebBlock, 0, h->stream>>>(h->g.N, t, h->dstage.get(), lambda_th, lam, w.type, w.part);
    else
      k_tweb_eigen<T, T><<<nblk, kTwebBlock, 0, h->stream>>>(h->g.N, t, R(h->ioq), lambda_th, lam, w.type, w.part);
    k_tweb_reduce<<<kTwebWords, kWave, 0, h->stream>>>(nblk, w.part, w.part + (size_t)nblk * kTwebWords);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // one component of the tensor -> N host doubles
  static int tweb_component_fetch(bchmc_handle *h, int c, double *out) {
    const size_t bytes = (size_t)h->g.N * sizeof(double);
    if (kDouble) return d2h(h, out, h->tw.t[c], bytes);
    CHK(store_real(h, R(h->tw.t[c]), h->dstage));
    return d2h(h, out, h->dstage, bytes);
  }

  // ---- bchmc_bispectrum (bispec.hpp; bispec_take has run) ------------------------------------------------------------------
  // x^ of the source as spectrum_source obtains it, but a fresh transform lands in the feature's own half-complex array:
  // tC is the scratch of the shells.
  static int bispec_source(bchmc_handle *h, int src, const void **xk) {
    auto &w = h->bs;
    *xk = w.xk;
    if (src == BCHMC_CORR_HOST) return r2c_state(h, h->dstage, h->ioq, w.xk);
    if (src == BCHMC_CORR_CHAIN_STATE) {
      *xk = h->cq;
      return BCHMC_OK;
    }
    CHK(upres_real(h, src));
    return fft_exec(h, h->r2c1, h->ioq, w.xk, BCHMC_K_FFT_R2C);
  }

  // The n_shell shell fields into h->bs.d: per shell one filter pass into tC and one C2R.  xk null: I_s.
  static int bispec_shells(bchmc_handle *h, const void *xk, double k_min, double dk, int n_shell) {
    auto &w = h->bs;
    for (int s = 0; s < n_shell; s++) {
      {
        ProfScope ps(h, BCHMC_K_OTHER);
        if (xk)
          k_bispec_filter<T, false><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, C(xk), C(h->tC), k_min, dk, n_shell, s);
        else
          k_bispec_filter<T, true><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, nullptr, C(h->tC), k_min, dk, n_shell, s);
        HIPCHK(hipGetLastError());
      }
      CHK(fft_exec(h, h->c2r1, h->tC, w.d[s], BCHMC_K_FFT_C2R));
    }
    return BCHMC_OK;
  }

  // the contraction of the arrays in h->bs.d -> res (T doubles on the device)
  static int bispec_triple(bchmc_handle *h, int n_shell, const BispecPlan &plan, double *res) {
    auto &w = h->bs;
    BispecArrays arr{};
    for (int s = 0; s < n_shell; s++) arr.a[s] = w.d[s];
    ProfScope ps(h, BCHMC_K_OTHER);
    HIPCHK(launch_bispec_triple<T>(h->stream, h->g.N, n_shell, arr, plan, w.part, res));
    return BCHMC_OK;
  }

  // the per-shell sums of x^ -> res (3 n_shell doubles on the device: sum hw, sum hw |k|, sum hw |x^|^2)
  static int bispec_stats(bchmc_handle *h, const void *xk, double k_min, double dk, int n_shell, double *res) {
    auto &w = h->bs;
    const int grid = (int)std::min<long long>((h->g.Nhp + kBispecStatBlock - 1) / kBispecStatBlock, kBispecStatGrid);
    ProfScope ps(h, BCHMC_K_OTHER);
    k_bispec_stats<T><<<grid, kBispecStatBlock, (size_t)3 * n_shell * kWave * sizeof(double), h->stream>>>(
        h->g, C(xk), k_min, dk, n_shell, w.part);
    k_bispec_reduce<<<(3 * n_shell + kWave - 1) / kWave, 256, 0, h->stream>>>(grid, 3 * n_shell, w.part, res);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // ---- measure_spec2D (spec2d.hpp; spec2d_setup has run for n_bin) ----------------------------------------------------
  template <bool GEOM>
  static int launch_spec2d(bchmc_handle *h, const CT *xk) {
    auto &c = h->spec2;
    const Geo &g = h->g;
    const int *par_start = c.idx + (size_t)g.n * g.n, *perp_slice = par_start + c.npb + 1;
    const dim3 grid((unsigned)c.nsl, (unsigned)((g.nh + kSpecChunk - 1) / kSpecChunk));
    k_spec2d_slices<T, GEOM><<<grid, kSpecChunk * kSpecWaves, 0, h->stream>>>(g, xk, c.idx, c.slices, c.part);
    k_spec2d_reduce<<<(unsigned)c.n_bin, 256, (size_t)g.nh * sizeof(double), h->stream>>>(g.n, g.nh, c.part, perp_slice,
                                                                                          par_start, c.npb, c.out);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // kmode, nmode (may be null) and power of the half-complex transform xk_T: arrays of n_bin^2, element
  // par + n_bin * perp (2D_powspec.cc:94), normalised like :102-109.  One synchronise.
  static int spec2d_bins(bchmc_handle *h, const void *xk_T, uint64_t n_bin, double *kmode, uint64_t *nmode, double *power) {
    auto &c = h->spec2;
    const Geo &g = h->g;
    const CT *xk = reinterpret_cast<const CT *>(xk_T);
    const size_t nb = (size_t)n_bin, cells = nb * c.npb;
    const bool geom = c.ksum.empty();
    std::vector<double> hb(cells), hk(geom ? cells : 0);
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      if (geom) {
        CHK(launch_spec2d<true>(h, xk));
        HIPCHK(hipMemcpyAsync(hk.data(), c.out, cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      }
      CHK(launch_spec2d<false>(h, xk));
      HIPCHK(hipMemcpyAsync(hb.data(), c.out, cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (geom) c.ksum.swap(hk);
    std::memset(kmode, 0, nb * nb * sizeof(double));
    std::memset(power, 0, nb * nb * sizeof(double));
    if (nmode) std::memset(nmode, 0, nb * nb * sizeof(uint64_t));
    const double N = (double)g.N;
    const double NORM = g.L * g.L * g.L / (4. * M_PI) / (N * N);  // 2D_powspec.cc:32, the 1 / (4 pi) included (S1)
    for (size_t p = 0; p < nb; p++) {
      if (!c.row_cnt[p]) continue;
      for (int q = 0; q < c.npb; q++) {
        const uint64_t nm = c.row_cnt[p] * c.par_w[q];
        const size_t ii = (size_t)c.par_bin[q] + nb * p;
        if (nmode) nmode[ii] = nm;
        kmode[ii] = c.ksum[p * c.npb + q] / (double)nm;
        power[ii] = NORM * hb[p * c.npb + q] / (double)nm;
      }
    }
    return BCHMC_OK;
  }

  // ---- bchmc_measure_*multipoles (multipoles.hpp; mp_take has run) -----------------------------------------------------
  // The segment sums of the shell pass over the class sums of a (and b, NS = 3): hs[(n_bin + 1) * segments * 3 NS], and,
  // `hg` not null, those of the GEOM pass: hg[(n_bin + 1) * segments * kMpGeom].  REAL: a is the real grid A(r) of T and
  // the bins are measure_corr's; else a, b are half-complex transforms and the bins measure_spectrum's.  One synchronise.
  template <int NS, bool REAL>
  static int mp_sums(bchmc_handle *h, const void *a, const void *b, uint64_t n_bin, double *hg, double *hs) {
    auto &w = h->mp;
    const Geo &g = h->g;
    const int nseg = mp_segments((int)n_bin);
    const double u = REAL ? g.d : g.kfac, dt = REAL ? corr_dr(g, n_bin) : spectrum_dk(g, n_bin);
    const long long stride = (long long)w.ncls * g.nh;
    const size_t cells = ((size_t)n_bin + 1) * nseg;
    const dim3 g1((unsigned)((w.ncls + kMpWaves - 1) / kMpWaves), (unsigned)((g.nh + kSpecChunk - 1) / kSpecChunk));
    const dim3 g2((unsigned)n_bin + 1, (unsigned)nseg);
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_mp_classes<T, NS, REAL><<<g1, kSpecChunk * kMpWaves, 0, h->stream>>>(g, a, b, w.rows, w.ncls, w.part, stride);
      if (hg) {
        k_mp_shells<1, true><<<g2, kMpBlock, 0, h->stream>>>(g.n, g.nh, u, dt, (int)n_bin, w.ncls, w.cls, w.part, stride, REAL ? 0 : 1, w.out);
        HIPCHK(hipMemcpyAsync(hg, w.out, cells * kMpGeom * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      }
      k_mp_shells<NS, false><<<g2, kMpBlock, 0, h->stream>>>(g.n, g.nh, u, dt, (int)n_bin, w.ncls, w.cls, w.part, stride, REAL ? 0 : 1, w.out);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(hs, w.out, cells * 3 * NS * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return BCHMC_OK;
  }
  static int mp_auto(bchmc_handle *h, const void *xk, uint64_t n_bin, double *hg, double *hs) {
    return mp_sums<1, false>(h, xk, nullptr, n_bin, hg, hs);
  }
  static int mp_cross(bchmc_handle *h, const void *ak, const void *bk, uint64_t n_bin, double *hg, double *hs) {
    return mp_sums<3, false>(h, ak, bk, n_bin, hg, hs);
  }
  static int mp_corr(bchmc_handle *h, uint64_t n_bin, double *hg, double *hs) {  // A(r) is in ioq (corr_field)
    return mp_sums<1, true>(h, h->ioq, nullptr, n_bin, hg, hs);
  }

  static int gradient(bchmc_handle *h, const double *d_q, double *d_g) {
    const size_t N = (size_t)h->g.N;
    if (!h->gprior) {
      CHK(dev_alloc(h, h->gprior, N * sizeof(T)));
      CHK(dev_alloc(h, h->glike, N * sizeof(T)));
    }
    CHK(r2c_state(h, d_q, h->ioq, h->qk));
    int like_mode = 2;
    double b = 0.;
    CHK(force_sources(h, false, EvalMode{}, &like_mode, &b));
    CHK(launch_assemble<false>(h, h->c.grad_psi_prior_factor, 0., 2, 0., nullptr));
    CHK(c2r_scaled(h, h->gk, h->gprior));
    CHK(launch_assemble<false>(h, 0., b, like_mode, 0., nullptr));
    CHK(c2r_scaled(h, h->gk, h->glike));
    k_add_r<T><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g.N, R(h->gprior), R(h->glike), R(h->iop));
    HIPCHK(hipGetLastError());
    return store_real(h, R(h->iop), d_g);
  }

  // Fill the double staging array with one output field.
  static int fetch(bchmc_handle *h, bchmc_field field, double *d_out) {
    FieldSource fs;
    CHK(field_source(h, (int)field, &fs));
    if (fs.made == FieldSource::kOverdens)
      k_overdens<T><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g, R(h->rho), h->rho_part, R(h->ioq));
    if (fs.made == FieldSource::kPositions)
      k_positions<T><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g, make_pos(h, h->last_rsd), R(h->psi), R(h->ioq),
                                                                 (int)field - (int)BCHMC_F_POSX);
    if (fs.made == FieldSource::kVrec)
      k_vrec_unpack<T><<<nblk_stride(h->g.N), 256, 0, h->stream>>>(h->g.N, R(h->vrec), (int)field - (int)BCHMC_F_VX, R(h->ioq));
    if (fs.made != FieldSource::kAsHeld) HIPCHK(hipGetLastError());
    return store_real(h, R(fs.base) + fs.offset, d_out);
  }

  // Momenta from the Gaussians of an exact draw (mt_draw.hpp): cp = G of create_GARFIELD placed directly (the R2C of
  // its C2R / N), plus R2C[sqrt(mass_r) g] for a real-space mass -- what bchmc_chain_set_momenta makes of
  // draw_momenta's array.
  static int mt_place(bchmc_handle *h) {
    const long long N = h->g.N, Nh = h->g.Nhp;
    const int n = h->g.n;
    ProfScope ps(h, BCHMC_K_OTHER);
    HIPCHK(hipMemsetAsync(h->cp, 0, 2 * (size_t)Nh * sizeof(T), h->stream));
    if (h->mass_fs) {
      const long long cells = (long long)(n / 2 + 1) * (n / 2 + 1) * (n / 2 + 1);
      const double amp = (double)N * (double)N / (h->g.L * h->g.L * h->g.L);  // random.cpp:88-90
      k_mt_place<T><<<nblk_stride(cells), 256, 0, h->stream>>>(n, h->g.nhp, h->mt.gauss, R(h->in_arr[BCHMC_F_MASS_F]),
                                                               amp, C(h->cp));
      HIPCHK(hipGetLastError());
    }
    if (h->mass_rs) {
      k_mt_real_space<T><<<nblk_stride(N), 256, 0, h->stream>>>(N, h->mt.gauss + (h->mass_fs ? 2 * N : 0),
                                                                R(h->in_arr[BCHMC_F_MASS_R]), R(h->iop));
      HIPCHK(hipGetLastError());
      CHK(fft_exec(h, h->r2c1, h->iop, h->tC, BCHMC_K_FFT_R2C));
      k_color_momenta<T><<<nblk_stride(Nh), 256, 0, h->stream>>>(Nh, C(h->tC), nullptr, C(h->cp), 1);
      HIPCHK(hipGetLastError());
    }
    return BCHMC_OK;
  }

  // ---- setup_random_test / make_initial_guess (barcoderunner.cc:42-247; mock.hpp) ----------------------------------
  // create_GARFIELD(signal_PS) from the 2 N unit Gaussians of the draw, placed in k-space into dst (qk or cq): the
  // R2C of upstream's real-space field, like the momenta of mt_place.
  static int mock_place(bchmc_handle *h, void *dst) {
    const long long N = h->g.N;
    const int n = h->g.n;
    ProfScope ps(h, BCHMC_K_OTHER);
    HIPCHK(hipMemsetAsync(dst, 0, 2 * (size_t)h->g.Nhp * sizeof(T), h->stream));
    const long long cells = (long long)(n / 2 + 1) * (n / 2 + 1) * (n / 2 + 1);
    const double amp = (double)N * (double)N / (h->g.L * h->g.L * h->g.L);  // random.cpp:88-90
    k_mt_place<T><<<nblk_stride(cells), 256, 0, h->stream>>>(n, h->g.nhp, h->mt.gauss, R(h->in_arr[BCHMC_F_SIGNAL_PS]),
                                                             amp, C(dst));
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  static long long mock_tiles(const bchmc_handle *h) { return (h->g.N + kMockTile - 1) / kMockTile; }
  static long long mock_groups(const bchmc_handle *h) { return (mock_tiles(h) + kMtThreads - 1) / kMtThreads; }

  static int mock_alloc(bchmc_handle *h) {
    auto &k = h->mock;
    if (k.cnt) return BCHMC_OK;
    CHK(dev_alloc(h, k.cnt, (size_t)mock_tiles(h)));
    CHK(dev_alloc(h, k.off, (size_t)mock_tiles(h)));
    CHK(dev_alloc(h, k.gsum, (size_t)mock_groups(h)));
    CHK(dev_alloc(h, k.goff, (size_t)mock_groups(h)));
    CHK(dev_alloc(h, k.res, (size_t)2));
    return BCHMC_OK;
  }

  // From the truth's k-space form in qk: delta_lag -> dstage[0, N), its forward model (left in the handle) with
  // delta_eul -> dstage[N, 2N), the window into the handle's input array, the ranks of its cells; res[0] = their count.
  static int mock_window(bchmc_handle *h, int rsd, int window_type) {
    const long long N = h->g.N;
    auto &k = h->mock;
    CHK(c2r_state(h, h->qk, h->ioq, h->dstage));
    EvalMode m;
    CHK(displacement(h, 1., rsd, &m.planes_c2r));
    CHK(forward_rest(h, rsd, m));
    CHK(fetch(h, BCHMC_F_DELTAX, h->dstage + N));
    ProfScope ps(h, BCHMC_K_OTHER);
    HIPCHK(hipMemsetAsync(k.res, 0xff, 2 * sizeof(unsigned long long), h->stream));
    k_mock_window<T><<<(int)mock_tiles(h), kMockThreads, 0, h->stream>>>(N, window_type, h->dstage + N,
                                                                         R(h->in_arr[BCHMC_F_WINDOW]), k.cnt);
    k_mock_scan<<<(int)mock_groups(h), kMtThreads, 0, h->stream>>>(k.cnt, mock_tiles(h), k.off, k.gsum);
    k_mt_scan<<<1, kMtThreads, 0, h->stream>>>(k.gsum, (int)mock_groups(h), k.goff, k.res, 0, nullptr);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // nobs and noise into the handle's input arrays from the split Gaussians of the second draw
  static int mock_noise(bchmc_handle *h, const MockPar &mp) {
    const long long N = h->g.N;
    auto &k = h->mock;
    ProfScope ps(h, BCHMC_K_OTHER);
    k_mock_noise<T><<<(int)mock_tiles(h), kMockThreads, 0, h->stream>>>(
        N, mp, h->dstage, h->dstage + N, R(h->in_arr[BCHMC_F_WINDOW]), k.off, k.goff,
        reinterpret_cast<const double2 *>(h->mt.gauss.get()), R(h->in_arr[BCHMC_F_NOBS]), R(h->in_arr[BCHMC_F_NOISE]), k.res);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // initial_guess 3: the placed field in cq times kernelcomp's table
  static int mock_smooth(bchmc_handle *h, double smol) {
    double wtot = 0.;
    CHK(kernel_norm(h, smol, h->ioq, &wtot));
    ProfScope ps(h, BCHMC_K_OTHER);
    k_mock_smooth<T><<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, C(h->cq), smol, 1. / wtot);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // initial_guess 4: N draws gsl_ran_gaussian(sigma) in cell order, taken in like bchmc_chain_set_state takes an array
  static int mock_guess_noise(bchmc_handle *h, double sigma) {
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_mock_guess_noise<<<nblk_stride(h->g.N), kMockThreads, 0, h->stream>>>(
          h->g.N, sigma, reinterpret_cast<const double2 *>(h->mt.gauss.get()), h->dstage);
      HIPCHK(hipGetLastError());
    }
    return r2c_state(h, h->dstage, h->ioq, h->cq);
  }

  static int upload(bchmc_handle *h, bchmc_field field, const double *d_src) {
    CHK(load_real(h, d_src, R(h->in_arr[field])));
    const double normFS = h->g.L * h->g.L * h->g.L / (double)h->g.N;  // FOURIER_DEF_2, HMC_help.cc:25-27
    if (field == BCHMC_F_SIGNAL_PS || field == BCHMC_F_MASS_F) {
      double *w = field == BCHMC_F_SIGNAL_PS ? h->wS : h->wM;
      k_prepare_mult<<<nblk_stride(h->g.Nhp), 256, 0, h->stream>>>(h->g, d_src, w, normFS);
      HIPCHK(hipGetLastError());
      h->w_gen++;  // the tiled pair {wS, wM} is stale (trajectory_fused makes it again)
    }
    return BCHMC_OK;
  }

  // ---- Hamiltonian_mass (HMC_mass.cc:315-368) ---------------------------------------------------------------------
  // measure_spectrum of likelihood_grad_log_like at the state in qk (likeli_force_power, 39-50): the likelihood force
  // before grad_psi_likeli_factor, binned from its k-space form in gk (the R2C of the real force up to round-off:
  // grad_inv_lap_FS keeps it Hermitian).  Leaves the force's forward model in the handle.
  static int mass_force_spectrum(bchmc_handle *h, uint64_t n_bin, double *kmode, double *power) {
    int like_mode = 2;
    double b = 0.;
    CHK(force_sources(h, false, EvalMode{}, &like_mode, &b));
    double norm = -1.;  // zeldovich_norm, HMC_models.cc:458-461, without the test factor
    norm *= h->c.deltaQ_factor;
    if (h->c.correct_delta) norm *= h->c.D1;
    CHK(launch_assemble<false>(h, 0., norm, like_mode, 0., nullptr));
    return spectrum_bins(h, h->gk, n_bin, kmode, power);
  }

  // (pairs + cells) x outputs of one k_jasche_accum launch, so that no kernel holds a shared device long: measured
  // 5.4-6.5 ms per launch at 64^3 (profiles/mass_kernel_stats_64.csv)
  static constexpr long long kJascheWork = 1ll << 32;

  // likeli_force_1st_order_diagonal_mass (230-306) at the state in qk into d_r (N doubles).  G first (its transform
  // uses Ck / psi), then Lag2Eul(signal) as bchmc_forward runs it, the (particle, cell) pairs, the sums in slices.
  static int mass_jasche(bchmc_handle *h, double *d_r) {
    const Geo &g = h->g;
    const long long N = g.N;
    DevBuf<double> G, acc;
    DevBuf<int> cnt, off;
    DevBuf<long long> total;
    DevBuf<JRec> rec;
    struct Drain {  // declared after the scratch buffers: they are released after the stream has drained
      hipStream_t stream;
      ~Drain() { (void)hipStreamSynchronize(stream); }
    } drain{h->stream};
    CHK(dev_alloc(h, G, 3 * (size_t)N));
    CHK(dev_alloc(h, acc, (size_t)N));
    CHK(dev_alloc(h, cnt, (size_t)N));
    CHK(dev_alloc(h, off, (size_t)N + 1));
    CHK(dev_alloc(h, total, (size_t)1));
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_glap_impulse<T><<<nblk_stride(g.Nhp), 256, 0, h->stream>>>(g, C(h->Ck));
      HIPCHK(hipGetLastError());
    }
    CHK(fft_exec(h, h->c2r3, h->Ck, h->psi, BCHMC_K_FFT_C2R));
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_convert<T, double><<<nblk_stride(3 * N), 256, 0, h->stream>>>(3 * N, R(h->psi), G);
      HIPCHK(hipGetLastError());
    }
    // Lag2Eul(signal) (HMC_mass.cc:242-257): no deltaQ_factor, rsd_model as configured
    const int rsd = h->c.rsd_model;
    EvalMode mode;
    CHK(displacement(h, 1., rsd, &mode.planes_c2r));
    CHK(forward_rest(h, rsd, mode));
    const PosPar pp = make_pos(h, rsd);
    JaschePar jp;
    jp.h = h->c.particle_kernel_h;
    const double h2 = jp.h * jp.h;
    jp.norm = 1. / (M_PI * (h2 * h2 * jp.h));  // gsl_pow_5
    jp.reach = (int)(2. * jp.h / g.d) + 1;
    const T *window = R(h->in_arr[BCHMC_F_WINDOW]), *noise = R(h->in_arr[BCHMC_F_NOISE]);
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_jasche_pairs<T, false><<<nblk_stride(N), 256, 0, h->stream>>>(g, pp, jp, R(h->psi), window, cnt, nullptr, nullptr);
      k_jasche_scan<<<1, 1024, 0, h->stream>>>(N, cnt, total, off);
      HIPCHK(hipGetLastError());
    }
    long long npairs = 0;
    HIPCHK(hipMemcpyAsync(&npairs, total, sizeof npairs, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (npairs >= 0x7fffffffLL)
      return h->fail(BCHMC_ERR_UNSUPPORTED, "Jasche mass: %lld (particle, cell) pairs exceed the 32-bit offsets", npairs);
    CHK(dev_alloc(h, rec, (size_t)std::max(npairs, 1ll)));
    HIPCHK(hipMemsetAsync(cnt, 0, (size_t)N * sizeof(int), h->stream));
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      k_jasche_pairs<T, true><<<nblk_stride(N), 256, 0, h->stream>>>(g, pp, jp, R(h->psi), window, cnt, off, rec);
      k_jasche_sort<<<nblk_stride(N), 256, 0, h->stream>>>(N, off, rec);
      HIPCHK(hipGetLastError());
    }
    std::vector<int> hoff((size_t)N + 1);
    HIPCHK(hipMemcpyAsync(hoff.data(), off, hoff.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const long long budget = std::max(kJascheWork / N, 1ll);
    for (long long l0 = 0; l0 < N;) {
      long long l1 = l0 + 1;
      while (l1 < N && (long long)(hoff[l1 + 1] - hoff[l0]) + (l1 + 1 - l0) <= budget) l1++;
      ProfScope ps(h, BCHMC_K_OTHER);
      k_jasche_accum<<<nblk_full(N), 256, 0, h->stream>>>(g, rec, off, l0, l1, G, acc);
      HIPCHK(hipGetLastError());
      l0 = l1;
    }
    const double m = h->c.rho_c * (g.L * g.L * g.L) / (double)N;  // rho_c vol / N
    ProfScope ps(h, BCHMC_K_OTHER);
    k_jasche_final<T><<<nblk_stride(N), 256, 0, h->stream>>>(N, acc, window, noise, m * m, d_r);
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // The whole of Hamiltonian_mass for the handle's mass_type.  The state is the R2C of dstage[0, N) (a host signal) or
  // the resident chain state (from_chain).  mass_f goes to dstage[0, N), mass_r to dstage[N, 2N), both then taken in
  // exactly like bchmc_upload takes an array (load_real + k_prepare_mult).
  static int mass_build(bchmc_handle *h, bool from_chain, const bchmc_mass_opts &o, bool force, bool jasche) {
    const int t = h->c.mass_type;
    const long long N = h->g.N;
    double *d_f = h->dstage, *d_r = h->dstage + N;
    if (force || jasche) {
      if (from_chain)
        HIPCHK(hipMemcpyAsync(h->qk, h->cq, 2 * (size_t)h->g.Nhp * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
      else
        CHK(r2c_state(h, h->dstage, h->ioq, h->qk));
    }
    double dk = 0., fbar = 0.;
    std::vector<double> kmode, power;
    if (force) {
      kmode.resize(o.n_bin);
      power.resize(o.n_bin);
      CHK(mass_force_spectrum(h, o.n_bin, kmode.data(), power.data()));
      dk = spectrum_dk(h->g, o.n_bin);
      if (t == 3) {  // Hamiltonian_mass_mean_likeli_force (86-114)
        double fm = 0., kv = 0.;
        for (uint64_t i = 0; i < o.n_bin; i++) fm += 4. * M_PI * kmode[i] * kmode[i] * dk * power[i];
        for (uint64_t i = 0; i < o.n_bin; i++) kv += 4. * M_PI * kmode[i] * kmode[i] * dk;
        fbar = fm / kv;
      } else {  // the binned force power, read by k_mass_elementwise (spectrum_bins left room for 3 n_bin doubles)
        HIPCHK(hipMemcpyAsync(h->spec_bins, power.data(), o.n_bin * sizeof(double), hipMemcpyHostToDevice, h->stream));
      }
    }
    if (h->mass_fs) {
      const int mode = (t == 1 || t == 5) ? MASS_INVP : t == 2 ? MASS_FORCE : t == 3 ? MASS_MEAN : MASS_PS;
      ProfScope ps(h, BCHMC_K_OTHER);
      k_mass_elementwise<T><<<nblk_stride(N), 256, 0, h->stream>>>(h->g, mode, R(h->in_arr[BCHMC_F_SIGNAL_PS]),
                                                                   h->spec_bins, (int)o.n_bin, dk, fbar, o.mass_factor,
                                                                   d_f);
      HIPCHK(hipGetLastError());
    }
    if (h->mass_rs) {
      if (jasche) {
        CHK(mass_jasche(h, d_r));
      } else {  // fill_one: type 0, type 60 before its switch
        ProfScope ps(h, BCHMC_K_OTHER);
        k_mass_elementwise<T><<<nblk_stride(N), 256, 0, h->stream>>>(h->g, MASS_ONE, nullptr, nullptr, 0, 0., 0., 1., d_r);
        HIPCHK(hipGetLastError());
      }
    }
    if (h->mass_fs) CHK(upload(h, BCHMC_F_MASS_F, d_f));
    if (h->mass_rs) CHK(upload(h, BCHMC_F_MASS_R, d_r));
    HIPCHK(hipStreamSynchronize(h->stream));  // `power` is a local vector
    return BCHMC_OK;
  }

  // ---- bchmc_poisson_* (poisson.hpp) ----------------------------------------------------------------------------------
  // The counts of an n_in^3 rate grid of `cells` cells.  The field: doubles at xd, or (xd null) the source in ioq as
  // upres_real leaves it, read in the storage type.  cd: the counts as doubles.  resident: the scan into h->pois.off,
  // the total in h->pois.res[0]; otherwise the counts and the status words only.
  static int pois_counts(bchmc_handle *h, int src, long long cells, const double *xd, const bchmc_poisson_opts &o,
                         double *cd, bool resident) {
    auto &k = h->pois;
    if (!xd) CHK(upres_real(h, src));
    const long long nb = (cells + kPoisThreads - 1) / kPoisThreads, ng = (nb + kMtThreads - 1) / kMtThreads;
    const uint2 key = make_uint2((unsigned)o.seed, (unsigned)(o.seed >> 32));
    const T *win = o.use_window ? R(h->in_arr[BCHMC_F_WINDOW]) : nullptr;
    unsigned long long *off = resident ? k.off.get() : nullptr, *cnt = resident ? k.cnt.get() : nullptr;
    ProfScope ps(h, BCHMC_K_OTHER);
    HIPCHK(hipMemsetAsync(k.stat, 0, kPoisWords * sizeof(unsigned long long), h->stream));
    HIPCHK(hipMemsetAsync(k.stat + kPoisBad, 0xff, sizeof(unsigned long long), h->stream));
    if (xd)
      k_pois_counts<double, T><<<(int)nb, kPoisThreads, 0, h->stream>>>(cells, key, o.stream, o.rate_mode, o.scale, xd, win,
                                                                        cd, off, cnt, k.stat);
    else
      k_pois_counts<T, T><<<(int)nb, kPoisThreads, 0, h->stream>>>(cells, key, o.stream, o.rate_mode, o.scale, R(h->ioq),
                                                                   win, cd, off, cnt, k.stat);
    if (resident) {
      k_mock_scan<<<(int)ng, kMtThreads, 0, h->stream>>>(k.cnt, nb, k.boff, k.gsum);
      k_mt_scan<<<1, kMtThreads, 0, h->stream>>>(k.gsum, (int)ng, k.goff, k.res, 0, nullptr);
      k_pois_offsets<<<(int)nb, kPoisThreads, 0, h->stream>>>(cells, k.boff, k.goff, k.res, k.off);
    }
    HIPCHK(hipGetLastError());
    return BCHMC_OK;
  }

  // particles p0 .. p0 + m - 1 of the resident sample into three device columns (m >= 1, p0 + m <= n_part)
  static void pois_positions(bchmc_handle *h, uint64_t p0, int m, double *x, double *y, double *z) {
    const auto &k = h->pois;
    const uint2 key = make_uint2((unsigned)k.seed, (unsigned)(k.seed >> 32));
    k_pois_positions<<<nblk_full(m), 256, 0, h->stream>>>(k.cells, (int)k.n_in, k.d_in, key, k.stream, k.off,
                                                          (unsigned long long)p0, m, x, y, z);
  }

  // ---- bchmc_density_particles (catalogue.hpp) ---------------------------------------------------------------------
  template <int MK, bool FIX>
  static void cat_launch(bchmc_handle *h, const SphPar &sp, bool tiled, int H, size_t lds, int m, const double *w,
                         double fix_scale) {
    using Cell = typename CatCell<FIX>::type;
    auto &c = h->cat;
    Cell *acc = reinterpret_cast<Cell *>(h->dstage + h->g.N);
    const double *x = c.cols, *y = x + kCatBatch, *z = y + kCatBatch;
    if (tiled) {
      const int grid = h->plan.tp.ntiles + m / h->plan.tp.chunk + 1;  // upper bound on the work items of this batch
      k_cat_scatter<T, MK, FIX><<<grid, 256, lds, h->stream>>>(h->g, sp, h->plan.tp, H, c.items, c.stat, c.rec, acc, fix_scale);
    } else {
      k_cat_direct<T, MK, FIX><<<nblk_full(m), 256, 0, h->stream>>>(h->g, sp, m, x, y, z, w, acc, fix_scale, c.stat);
    }
  }

  // The whole call after its arguments were checked: batches of kCatBatch particles through count / scan / fill /
  // scatter (or the direct kernel) into an accumulator in the upper half of the transfer staging, then the ABI's doubles
  // in its lower half, from where they go to the host and, for dest = nobs, through upload() like a host array.
  static int density_particles(bchmc_handle *h, const CatCall &cc, double *out, bchmc_density_stats *stats) {
    auto &c = h->cat;
    const Geo &g = h->g;
    const TilePar &tp = h->plan.tp;
    SphPar sp = make_sph(h);
    sp.h = cc.hh;
    sp.h_inv = 1. / sp.h;
    sp.w_norm = 1. / M_PI / (sp.h * sp.h * sp.h);
    sp.r2_lim = 4. * sp.h * sp.h * (1. + (h->f32 ? 1e-5 : 1e-12));
    sp.reach = (int)(2. * sp.h / g.d) + 1;
    // tiles: the handle's partition, where the home cells are those the partition was made for (origin 0) and the image
    // of the tile and this kernel's halo leaves two workgroups per CU well inside the 160 KiB (64 KiB at most)
    // SPH: where the stencil hull of this scale length is the standard 81-cell one and exact (h = d and its
    // neighbourhood down to the 0.8661 d of plan_tiles) the unrolled hull kernel with the hull's halo, 2; else the cube
    bool hull81 = false;
    if (cc.mk == 3) {
      const Hull hull = build_hull(sp.h, g.d);
      hull81 = hull.exact && hull.cols.size() == 21 && hull.max_offset() == 2 && sp.h >= 0.8661 * g.d;
      for (auto &col : hull.cols) {
        const int zw = (std::abs(col.x) <= 2 && std::abs(col.y) <= 2) ? hull81_zw(col.x + 2, col.y + 2) : -1;
        if (zw < 0 || col.z != -zw || col.w != zw) hull81 = false;
      }
    }
    const int H = cc.mk == 0 ? 0 : (cc.mk == 3 ? (hull81 ? 2 : sp.reach) : 1);
    const bool origin0 = h->c.min1 == 0. && h->c.min2 == 0. && h->c.min3 == 0.;
    size_t lds = 0;
    bool tiled = h->plan.tiled && origin0 && H <= g.n;
    if (tiled) {
      lds = (size_t)(tp.tx + 2 * H) * (tp.ty + 2 * H) * (tp.tz + 2 * H) * 8;
      tiled = lds <= 64 * 1024;
    }
    // built with the first call, whichever path it takes, so that a later call allocates nothing; all or nothing: a
    // failed allocation leaves no half-built set behind for the next call to trust
    if (!c.cols) {
      auto build = [&]() -> int {
        CHK(dev_alloc(h, c.cols, 4 * (size_t)kCatBatch));
        CHK(dev_alloc(h, c.stat, kCatWords));
        HIPCHK(c.h_stat.alloc(kCatWords));
        if (!h->plan.tiled) return BCHMC_OK;
        CHK(dev_alloc(h, c.tile_of, kCatBatch));
        CHK(dev_alloc(h, c.rec, kCatBatch));
        CHK(dev_alloc(h, c.cnt, tp.ntiles));
        CHK(dev_alloc(h, c.off, tp.ntiles + 1));
        CHK(dev_alloc(h, c.cursor, tp.ntiles));
        return dev_alloc(h, c.items, (size_t)tp.ntiles + kCatBatch / tp.chunk + 1);
      };
      if (const int rc = build()) {
        h->cat = bchmc_handle::Cat{};
        return rc;
      }
    }
    const double k_max = cc.mk == 3 ? sp.w_norm : 1.;
    const double fix_scale = 70368744177664. / ((cc.max_w > 0. ? cc.max_w : 1.) * k_max);  // 2^46 / largest contribution
    double *acc = h->dstage + g.N;
    // profiling: per batch the binning (positions, count, scan, fill) is a scope of the sort class and the scatter one of
    // the scatter class; clearing and conversion go to "other".  The catalogue's way to the device (h2d synchronises on
    // the host) lies between the scopes
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      HIPCHK(hipMemsetAsync(acc, 0, g.N * sizeof(double), h->stream));
      HIPCHK(hipMemsetAsync(c.stat, 0, kCatWords * sizeof(unsigned long long), h->stream));
    }
    double *x = c.cols, *y = x + kCatBatch, *z = y + kCatBatch, *w = cc.weighted ? z + kCatBatch : nullptr;
    const PosPar pp = make_pos(h, h->last_rsd);
    for (uint64_t p0 = 0; p0 < cc.n_part; p0 += kCatBatch) {
      const int m = (int)std::min<uint64_t>(kCatBatch, cc.n_part - p0);
      if (cc.src == BCHMC_PART_HOST) {
        CHK(h2d(h, x, cc.x + p0, m * sizeof(double)));
        CHK(h2d(h, y, cc.y + p0, m * sizeof(double)));
        CHK(h2d(h, z, cc.z + p0, m * sizeof(double)));
        if (w) CHK(h2d(h, w, cc.w + p0, m * sizeof(double)));
      }
      if (cc.src != BCHMC_PART_HOST || tiled) {
        ProfScope ps(h, BCHMC_K_SORT);
        if (cc.src == BCHMC_PART_FORWARD)
          k_cat_positions<T><<<nblk_full(m), 256, 0, h->stream>>>(g, pp, R(h->psi), (long long)p0, m, x, y, z);
        if (cc.src == kCatSrcPoisson) pois_positions(h, p0, m, x, y, z);
        if (tiled) {
          HIPCHK(hipMemsetAsync(c.cnt, 0, tp.ntiles * sizeof(unsigned), h->stream));
          k_cat_count<T><<<nblk_full(m), 256, 0, h->stream>>>(g, sp, tp, cc.mk, m, x, y, z, c.tile_of, c.cnt, c.stat);
          k_cat_scan<<<1, 1024, 0, h->stream>>>(tp.ntiles, tp.chunk, c.cnt, c.off, c.cursor, c.items, c.stat);
          k_cat_fill<T><<<nblk_full(m), 256, 0, h->stream>>>(m, x, y, z, w, c.tile_of, c.off, c.cursor, c.rec);
        }
        HIPCHK(hipGetLastError());
      }
      ProfScope ps(h, BCHMC_K_SCATTER);
#define BCHMC_CAT_MK(MK)                                                          \
  if (h->fix) cat_launch<MK, true>(h, sp, tiled, H, lds, m, w, fix_scale);       \
  else cat_launch<MK, false>(h, sp, tiled, H, lds, m, w, fix_scale)
      switch (cc.mk) {
        case 0: BCHMC_CAT_MK(0); break;
        case 1: BCHMC_CAT_MK(1); break;
        case 2: BCHMC_CAT_MK(2); break;
        default:
          if (hull81) { BCHMC_CAT_MK(kCatSph81); }
          else { BCHMC_CAT_MK(3); }
          break;
      }
#undef BCHMC_CAT_MK
      HIPCHK(hipGetLastError());
    }
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      if (h->fix)
        k_cat_finish<true><<<nblk_stride(g.N), 256, 0, h->stream>>>(g.N, reinterpret_cast<long long *>(acc), 1. / fix_scale,
                                                                    h->fix_sat_limit, h->dstage, c.stat);
      else
        k_cat_finish<false><<<nblk_stride(g.N), 256, 0, h->stream>>>(g.N, acc, 1., 0, h->dstage, c.stat);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(c.h_stat, c.stat, kCatWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (c.h_stat[kCatSat])
      return h->fail(BCHMC_ERR_STATE, "density_particles: a fixed-point cell passed 2^16 maximal contributions "
                                      "(deterministic mode); nothing was written");
    if (stats) {
      stats->n_in = c.h_stat[kCatIn];
      stats->n_lost = cc.n_part - c.h_stat[kCatIn];
      stats->max_per_tile = c.h_stat[kCatMaxTile];
    }
    if (out) CHK(d2h(h, out, h->dstage, g.N * sizeof(double)));
    if (cc.dest == BCHMC_F_NOBS) {
      CHK(upload(h, BCHMC_F_NOBS, h->dstage));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
    return BCHMC_OK;
  }
  // ---- bchmc_interp_particles (interp_particles.hpp) ----------------------------------------------------------------
  template <int MK, int K>
  static void itp_launch(bchmc_handle *h, bool tiled, size_t lds, int m) {
    auto &c = h->itp;
    const double *x = c.cols, *y = x + kCatBatch, *z = y + kCatBatch;
    if (tiled) {
      const int grid = h->plan.tp.ntiles + m / h->plan.tp.chunk + 1;  // upper bound on the work items of this batch
      k_itp_gather_tile<T, MK, K><<<grid, 256, lds, h->stream>>>(h->g, h->plan.tp, c.items, c.stat, c.rec, R(c.src), c.out);
    } else {
      k_itp_gather_direct<T, MK, K><<<nblk_full(m), 256, 0, h->stream>>>(h->g, m, x, y, z, R(c.src), c.out, c.stat);
    }
  }
  template <int MK>
  static void itp_launch_k(bchmc_handle *h, int K, bool tiled, size_t lds, int m) {
    switch (K) {
      case 1: itp_launch<MK, 1>(h, tiled, lds, m); break;
      case 2: itp_launch<MK, 2>(h, tiled, lds, m); break;
      case 3: itp_launch<MK, 3>(h, tiled, lds, m); break;
      default: itp_launch<MK, 4>(h, tiled, lds, m); break;
    }
  }

  // The whole call after its arguments were checked.  The sources are staged once, each as bchmc_upload /
  // bchmc_chain_get_state / bchmc_fetch would hold or return it, into the feature's own grid arrays; then batches of
  // kCatBatch particles go through count / scan / fill / gather (or the direct kernel) into a batch-ordered result array
  // that crosses PCIe as one contiguous copy per field.
  static int interp_particles(bchmc_handle *h, const ItpCall &ic, double *out, bchmc_interp_stats *stats) {
    auto &c = h->itp;
    const Geo &g = h->g;
    const TilePar &tp = h->plan.tp;
    const size_t N = (size_t)g.N;
    const int K = ic.n_fields;
    const bool tiled = ic.tiled != 0;
    // all or nothing, like the catalogue's: a failed allocation leaves no half-built set behind
    if (!c.cols || (tiled && !c.tile_of)) {
      auto build = [&]() -> int {
        if (!c.cols) {
          CHK(dev_alloc(h, c.cols, 3 * (size_t)kCatBatch));
          CHK(dev_alloc(h, c.out, kItpMaxFields * (size_t)kCatBatch));
          CHK(dev_alloc(h, c.stat, kCatWords));
          HIPCHK(c.h_stat.alloc(kCatWords));
        }
        if (!h->plan.tiled) return BCHMC_OK;
        CHK(dev_alloc(h, c.tile_of, kCatBatch));
        CHK(dev_alloc(h, c.rec, kCatBatch));
        CHK(dev_alloc(h, c.cnt, tp.ntiles));
        CHK(dev_alloc(h, c.off, tp.ntiles + 1));
        CHK(dev_alloc(h, c.cursor, tp.ntiles));
        return dev_alloc(h, c.items, (size_t)tp.ntiles + kCatBatch / tp.chunk + 1);
      };
      if (const int rc = build()) {
        h->itp = bchmc_handle::Itp{};
        return rc;
      }
    }
    if (c.fields_held < K) {
      c.fields_held = 0;
      CHK(dev_reserve(h, c.src, (size_t)K * N * sizeof(T)));
      c.fields_held = K;
    }
    for (int f = 0; f < K; f++) {
      const bchmc_interp_field &fd = ic.fields[f];
      T *dst = R(c.src) + (size_t)f * N;
      if (fd.source == BCHMC_CORR_HOST) {
        CHK(h2d(h, h->dstage, fd.host, N * sizeof(double)));
        CHK(load_real(h, h->dstage, dst));
      } else if (fd.source == BCHMC_CORR_CHAIN_STATE) {
        CHK(c2r_scaled(h, h->cq, dst));
      } else {
        ProfScope ps(h, BCHMC_K_OTHER);
        CHK(fetch(h, fd.source == BCHMC_CORR_DELTAX ? BCHMC_F_DELTAX : (bchmc_field)fd.field, h->dstage));
        CHK(load_real(h, h->dstage, dst));
      }
    }
    HIPCHK(hipMemsetAsync(c.stat, 0, kCatWords * sizeof(unsigned long long), h->stream));
    double *x = c.cols, *y = x + kCatBatch, *z = y + kCatBatch;
    const PosPar pp = make_pos(h, h->last_rsd);
    const size_t lds = tiled ? (size_t)(tp.tx + 2 * kItpHalo) * (tp.ty + 2 * kItpHalo) * (tp.tz + 2 * kItpHalo) * sizeof(T) * K : 0;
    for (uint64_t p0 = 0; p0 < ic.n_part; p0 += kCatBatch) {
      const int m = (int)std::min<uint64_t>(kCatBatch, ic.n_part - p0);
      if (ic.psrc != BCHMC_PART_FORWARD) {
        CHK(h2d(h, x, ic.x + p0, m * sizeof(double)));
        CHK(h2d(h, y, ic.y + p0, m * sizeof(double)));
        CHK(h2d(h, z, ic.z + p0, m * sizeof(double)));
      }
      if (ic.psrc == BCHMC_PART_FORWARD || tiled) {
        ProfScope ps(h, BCHMC_K_SORT);
        if (ic.psrc == BCHMC_PART_FORWARD)
          k_cat_positions<T><<<nblk_full(m), 256, 0, h->stream>>>(g, pp, R(h->psi), (long long)p0, m, x, y, z);
        if (tiled) {
          HIPCHK(hipMemsetAsync(c.cnt, 0, tp.ntiles * sizeof(unsigned), h->stream));
          if (ic.kernel == 1)
            k_itp_count<T, 1><<<nblk_full(m), 256, 0, h->stream>>>(g, tp, m, K, x, y, z, c.tile_of, c.cnt, c.out, c.stat);
          else
            k_itp_count<T, 2><<<nblk_full(m), 256, 0, h->stream>>>(g, tp, m, K, x, y, z, c.tile_of, c.cnt, c.out, c.stat);
          k_cat_scan<<<1, 1024, 0, h->stream>>>(tp.ntiles, tp.chunk, c.cnt, c.off, c.cursor, c.items, c.stat);
          k_itp_fill<T><<<nblk_full(m), 256, 0, h->stream>>>(m, x, y, z, c.tile_of, c.off, c.cursor, c.rec);
        }
        HIPCHK(hipGetLastError());
      }
      {
        ProfScope ps(h, BCHMC_K_GATHER);
        if (ic.kernel == 1) itp_launch_k<1>(h, K, tiled, lds, m);
        else itp_launch_k<2>(h, K, tiled, lds, m);
        HIPCHK(hipGetLastError());
      }
      for (int f = 0; f < K; f++)
        CHK(d2h(h, out + (size_t)f * ic.n_part + p0, c.out + (size_t)f * kCatBatch, m * sizeof(double)));
    }
    HIPCHK(hipMemcpyAsync(c.h_stat, c.stat, kCatWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (stats) {
      stats->n_in = c.h_stat[kCatIn];
      stats->n_lost = ic.n_part - c.h_stat[kCatIn];
      stats->max_per_tile = tiled ? c.h_stat[kCatMaxTile] : 0;
      stats->path_used = tiled ? kInterpTile : kInterpDirect;
      stats->reserved = 0;
    }
    return BCHMC_OK;
  }
};

#define DISPATCH(h, call) ((h)->f32 ? Pipe<float>::call : Pipe<double>::call)

// Every entry point makes the handle's device current first: handles on different GPUs may be driven from one
// process (one host thread per chain), and HIP launches use the calling thread's current device.
#define ENTER(h)                                                                                  \
  do {                                                                                            \
    hipError_t e_ = hipSetDevice((h)->c.device);                                                  \
    if (e_ != hipSuccess) return (h)->fail(BCHMC_ERR_HIP, "hipSetDevice(%d): %s", (h)->c.device, hipGetErrorString(e_)); \
  } while (0)

// A host entry point is about to overwrite (qk, pk, gk): a resident-chain proposal left there by bchmc_chain_attempt
// is gone, and bchmc_chain_accept / bchmc_chain_get_proposal must say so instead of committing the wrong arrays.
void clobber_proposal(bchmc_handle *h) { h->have_prop = h->prop_g_valid = false; }

int validate_config(const bchmc_config *c, std::string &why) {
  char buf[256];
  if (c->abi_version != BCHMC_ABI_VERSION) {
    snprintf(buf, sizeof buf, "abi_version %u != %u", c->abi_version, BCHMC_ABI_VERSION);
    why = buf;
    return BCHMC_ERR_ARG;
  }
  if (c->Nx < 4 || !(c->L > 0) || !(c->particle_kernel_h > 0)) {
    why = "Nx >= 4, L > 0 and particle_kernel_h > 0 are required";
    return BCHMC_ERR_ARG;
  }
  if (c->precision != 0 && c->precision != 1) {
    why = "precision must be 0 (fp64 fields) or 1 (fp32 fields)";
    return BCHMC_ERR_ARG;
  }
  if (c->likelihood < 0 || c->likelihood > 3) {
    why = "likelihood must be 0..3";
    return BCHMC_ERR_ARG;
  }
  if (!c->rsd_model && c->sfmodel != 1 && !(c->kth > 0.)) {
    why = "sfmodel != 1 (ALPT) needs the split scale kth = slength > 0";
    return BCHMC_ERR_ARG;
  }
  if (c->particle_kernel_h > c->L / 4) {
    why = "particle_kernel_h of more than Nx/4 cells (init_par.cc:373-375)";
    return BCHMC_ERR_ARG;
  }
  return BCHMC_OK;
}

// ---- draw_momenta from a GSL mt19937 state (mt_draw.hpp) ------------------------------------------------------------
const mt_host::Phi &mt_phi() {
  static std::once_flag once;
  static mt_host::Phi phi;
  std::call_once(once, [] { phi = mt_host::make_phi(); });
  return phi;
}

// GSL state `steps` outputs later.  mti = (Q - 1) mod 624 + 1 for the position Q = mti_in + steps: GSL regenerates a
// block when the next output needs it, so after any output 1 <= mti <= 624; mt[] = the 624 words from Q - mti on.
int mt_jump_gsl(const uint32_t *mt_in, int32_t mti_in, uint64_t steps, uint32_t *mt_out, int32_t *mti_out) {
  if (mti_in < 0 || mti_in > kMtN) return BCHMC_ERR_ARG;
  if (steps == 0) {
    std::memmove(mt_out, mt_in, kMtN * sizeof(uint32_t));
    *mti_out = mti_in;
    return BCHMC_OK;
  }
  const unsigned long long Q = (unsigned long long)mti_in + steps, mo = (Q - 1) % kMtN + 1, base = Q - mo;
  if (base == 0) {
    std::memmove(mt_out, mt_in, kMtN * sizeof(uint32_t));
  } else {
    const mt_host::Phi &phi = mt_phi();
    if (!phi.ok) return BCHMC_ERR_STATE;
    uint32_t tmp[kMtN];
    mt_host::window_ahead(phi, mt_in, base, tmp);  // mt_in is the window at position 0
    std::memcpy(mt_out, tmp, sizeof tmp);
  }
  *mti_out = (int32_t)mo;
  return BCHMC_OK;
}

// Once per handle: segment length S, segments B, the jump polynomials x^(b S - 1) mod phi (b = 1 .. B-1), buffers.
// Capacity per pass: 2.546 words per Gaussian (4/pi pairs of 2 words per accepted one) + 12 sigma + 4 blocks.
// BCHMC_MT_SEGMENT_WORDS / BCHMC_MT_CAPACITY (tests) set S and the capacity.
int mt_setup(bchmc_handle *h) {
  auto &m = h->mt;
  if (m.words) return BCHMC_OK;
  const auto t0 = std::chrono::steady_clock::now();
  const mt_host::Phi &phi = mt_phi();
  if (!phi.ok) return h->fail(BCHMC_ERR_STATE, "MT19937 characteristic polynomial: Berlekamp-Massey did not give degree 19937");
  const long long N = h->g.N;
  m.G = (h->mass_fs ? 2 * N : 0) + (h->mass_rs ? N : 0);
  double cap = std::ceil(2.546 * (double)m.G + 12. * 1.18 * std::sqrt((double)m.G)) + 4. * kMtN;
  if (const char *v = std::getenv("BCHMC_MT_CAPACITY")) cap = std::max(2. * kMtN, std::atof(v));
  int ncu = 256;
  HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->c.device));
  auto round624 = [](double w) { return (long long)std::ceil(w / kMtN) * kMtN; };
  long long S = std::max(round624(cap / std::max(ncu, 1)), 4LL * kMtN);
  if (const char *v = std::getenv("BCHMC_MT_SEGMENT_WORDS")) S = std::max(round624(std::atof(v)), (long long)kMtN);
  const long long B = (long long)std::ceil(cap / (double)S);
  if (B * S >= (1LL << 32) || B > (1 << 20))
    return h->fail(BCHMC_ERR_UNSUPPORTED, "exact momentum draw: %lld words per pass exceed 32-bit positions", B * S);
  m.S = S, m.B = (int)B, m.C = B * S;
  std::vector<uint32_t> polys((size_t)std::max<long long>(B - 1, 1) * kMtPolyWords, 0);
  if (B > 1) {
    mt_host::Poly p = mt_host::xpow(phi, (unsigned long long)S - 1);
    const mt_host::Poly J = B > 2 ? mt_host::xpow(phi, (unsigned long long)S) : p;
    for (long long b = 1; b < B; b++) {
      mt_host::to_words(p, polys.data() + (size_t)(b - 1) * kMtPolyWords);
      if (b + 1 < B) p = mt_host::mulmod(phi, p, J);
    }
  }
  CHK(dev_alloc(h, m.poly, polys.size()));
  CHK(dev_alloc(h, m.win, (size_t)34 * kMtN));
  CHK(dev_alloc(h, m.words, (size_t)m.C));
  CHK(dev_alloc(h, m.st, (size_t)kMtN));
  for (DevBuf<unsigned long long> *p : {&m.nz, &m.nzoff, &m.acc, &m.accoff, &m.lastend}) CHK(dev_alloc(h, *p, (size_t)B));
  CHK(dev_alloc(h, m.res, (size_t)8 + kMtN / 2));
  CHK(dev_alloc(h, m.gauss, (size_t)std::max(m.G, 1LL)));
  HIPCHK(m.h_io.alloc(8 + kMtN / 2));
  HIPCHK(hipMemcpyAsync(m.poly, polys.data(), polys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mt_segments), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)kMtSegLds));
  HIPCHK(hipStreamSynchronize(h->stream));
  m.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return BCHMC_OK;
}

// The Gaussian buffer was sized for the momenta (m.G); a request of another size (the mock data: 2 N for the truth,
// 2 doubles per windowed cell in split form) grows it.  Only called between trajectories.
int mt_reserve(bchmc_handle *h, long long doubles) {
  auto &m = h->mt;
  if (doubles <= (long long)m.gauss.capacity()) return BCHMC_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  return dev_reserve(h, m.gauss, (size_t)doubles);
}

// One pass: C words from the window at position P (counted from mt[0] of the caller's state), Gaussians
// done .. G of the request into gauss (split: two doubles each, k_mt_pairs).  Leaves res on the host in m.h_io.
int mt_pass(bchmc_handle *h, const uint32_t *win, unsigned long long P, long long done, long long G, bool split) {
  auto &m = h->mt;
  ProfScope ps(h, BCHMC_K_OTHER);
  uint32_t *io_st = reinterpret_cast<uint32_t *>(m.h_io + 8);
  std::memcpy(io_st, win, kMtN * sizeof(uint32_t));
  HIPCHK(hipMemcpyAsync(m.st, io_st, kMtN * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(m.res, 0, 8 * sizeof(unsigned long long), h->stream));
  k_mt_window<<<1, kMtThreads, 0, h->stream>>>(m.st, m.win, 34);
  k_mt_segments<<<m.B, kMtThreads, kMtSegLds, h->stream>>>(m.win, m.poly, m.S, m.words, m.nz);
  k_mt_scan<<<1, kMtThreads, 0, h->stream>>>(m.nz, m.B, m.nzoff, m.res, 4, nullptr);
  k_mt_pairs<false><<<m.B, kMtThreads, 0, h->stream>>>(m.words, m.C, m.S, m.nzoff, nullptr, m.acc, m.lastend, 0,
                                                        nullptr, m.res);
  k_mt_scan<<<1, kMtThreads, 0, h->stream>>>(m.acc, m.B, m.accoff, m.res, 0, m.lastend);
  if (split)
    k_mt_pairs<true, true><<<m.B, kMtThreads, 0, h->stream>>>(m.words, m.C, m.S, m.nzoff, m.accoff, nullptr, nullptr,
                                                               G - done, m.gauss + 2 * done, m.res);
  else
    k_mt_pairs<true><<<m.B, kMtThreads, 0, h->stream>>>(m.words, m.C, m.S, m.nzoff, m.accoff, nullptr, nullptr,
                                                         G - done, m.gauss + done, m.res);
  k_mt_final<<<1, 640, 0, h->stream>>>(m.words, m.C, P, m.res, reinterpret_cast<uint32_t *>(m.res + 8));
  HIPCHK(hipGetLastError());
  return BCHMC_OK;
}

int mt_place_momenta(bchmc_handle *h);

// G Gaussians of the stream from the GSL state (mt, mti) into m.gauss, unit or split; `place` (may be null) is what the
// caller makes of them, queued while the host still waits for the pass.
int mt_draw(bchmc_handle *h, uint32_t *mt, int32_t *mti, uint64_t *words_used, long long G, bool split,
            int (*place)(bchmc_handle *)) {
  CHK(mt_setup(h));
  auto &m = h->mt;
  CHK(mt_reserve(h, (split ? 2 : 1) * G));
  const int32_t mti_in = *mti;
  uint32_t win[kMtN];
  mt_host::gsl_to_window(mt, mti_in, win);
  unsigned long long P = (unsigned long long)mti_in;
  long long done = 0;
  for (int pass = 0;; pass++) {
    CHK(mt_pass(h, win, P, done, G, split));
    // placed now, so that it runs while the host waits; a continuation pass places again
    if (pass == 0 && place) CHK(place(h));
    HIPCHK(hipMemcpyAsync(m.h_io, m.res, (8 + kMtN / 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const unsigned long long got = m.h_io[0];
    if ((long long)got >= G - done) {
      const unsigned long long used = P + m.h_io[2] - (unsigned long long)mti_in;
      if (m.h_io[3]) {
        const unsigned long long Q = P + m.h_io[2];
        std::memcpy(mt, m.h_io + 8, kMtN * sizeof(uint32_t));
        *mti = (int32_t)((Q - 1) % kMtN + 1);
      } else {  // end state outside the last pass's buffer: jump there from the caller's state
        uint32_t out[kMtN];
        int32_t mo = 0;
        if (mt_jump_gsl(mt, mti_in, used, out, &mo)) return h->fail(BCHMC_ERR_STATE, "MT19937 jump failed");
        std::memcpy(mt, out, sizeof out);
        *mti = mo;
      }
      if (words_used) *words_used = used;
      if (pass > 0 && place) CHK(place(h));
      return BCHMC_OK;
    }
    // the pass ran out of words (a far statistical tail, or a capacity set small on purpose): continue the stream
    // after its last complete pair
    const unsigned long long E = m.h_io[1];
    if (E == 0) return h->fail(BCHMC_ERR_STATE, "exact momentum draw: a pass of %lld words held no complete pair", m.C);
    done += (long long)got;
    uint32_t next[kMtN];
    mt_host::window_ahead(mt_phi(), win, E, next);
    std::memcpy(win, next, sizeof next);
    P += E;
  }
}

int mt_place_momenta(bchmc_handle *h) { return DISPATCH(h, mt_place(h)); }
int mock_place_truth(bchmc_handle *h) { return DISPATCH(h, mock_place(h, h->qk)); }
int mock_place_guess(bchmc_handle *h) { return DISPATCH(h, mock_place(h, h->cq)); }

// The handle's stream; BCHMC_CU_MASK restricts it to a subset of the CUs
int create_stream(bchmc_handle *h) {
  if (const char *cm = std::getenv("BCHMC_CU_MASK")) {
    // experiment: restrict this handle's stream to a subset of the CUs (two chains per GPU on disjoint halves).
    // "lo" / "hi": first / second half of the mask bits; "even" / "odd": alternating groups of 32 bits (XCD-sized)
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, h->c.device));
    const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32;
    std::vector<uint32_t> mask(words, 0u);
    const std::string mode(cm);
    for (int cu = 0; cu < ncu; cu++) {
      bool on = true;
      if (mode == "lo") on = cu < ncu / 2;
      else if (mode == "hi") on = cu >= ncu / 2;
      else if (mode == "even") on = ((cu / 32) & 1) == 0;
      else if (mode == "odd") on = ((cu / 32) & 1) == 1;
      else if (mode == "evencu") on = (cu & 1) == 0;
      else if (mode == "oddcu") on = (cu & 1) == 1;
      if (on) mask[cu / 32] |= 1u << (cu % 32);
    }
    hipStream_t masked = nullptr;
    HIPCHK(hipExtStreamCreateWithCUMask(&masked, (uint32_t)words, mask.data()));
    h->stream.reset(masked);
  } else {
    HIPCHK(h->stream.create(hipStreamNonBlocking));
  }
  return BCHMC_OK;
}

// The 3-D real transforms of the whole grid, one field and three fields at a time
int make_plans_3d(bchmc_handle *h) {
  const Geo &g = h->g;
  const size_t len[3] = {(size_t)g.n, (size_t)g.n, (size_t)g.n};  // fastest first; cubic
  const rocfft_precision prec = h->f32 ? rocfft_precision_single : rocfft_precision_double;
  // real side contiguous (n, n^2), half-complex side with row stride nhp
  const size_t rs[3] = {1, (size_t)g.n, (size_t)g.n * g.n}, cs[3] = {1, (size_t)g.nhp, (size_t)g.nhp * g.n};
  rocfft_plan_description fwd = nullptr, inv = nullptr;
  FFTCHK(rocfft_plan_description_create(&fwd));
  FFTCHK(rocfft_plan_description_create(&inv));
  FFTCHK(rocfft_plan_description_set_data_layout(fwd, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved,
                                                 nullptr, nullptr, 3, rs, (size_t)g.N, 3, cs, (size_t)g.Nhp));
  FFTCHK(rocfft_plan_description_set_data_layout(inv, rocfft_array_type_hermitian_interleaved, rocfft_array_type_real,
                                                 nullptr, nullptr, 3, cs, (size_t)g.Nhp, 3, rs, (size_t)g.N));
  FFTCHK(h->r2c1.create(rocfft_plan_create, rocfft_placement_notinplace, rocfft_transform_type_real_forward, prec, 3, len,
                        1, fwd));
  FFTCHK(h->c2r1.create(rocfft_plan_create, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, prec, 3, len,
                        1, inv));
  FFTCHK(h->r2c3.create(rocfft_plan_create, rocfft_placement_notinplace, rocfft_transform_type_real_forward, prec, 3, len,
                        3, fwd));
  FFTCHK(h->c2r3.create(rocfft_plan_create, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, prec, 3, len,
                        3, inv));
  rocfft_plan_description_destroy(fwd);
  rocfft_plan_description_destroy(inv);
  return BCHMC_OK;
}

// The SPH hull and the tile partition (tile_plan.hpp decides both), and the buffers of the tile-sorted path
int make_tiles(bchmc_handle *h) {
  const bchmc_config &c = h->c;
  const size_t N = (size_t)h->g.N;
  const Hull hull = build_hull(c.particle_kernel_h, h->g.d);
  CHK(dev_alloc(h, h->hull, hull.cols.size()));
  HIPCHK(hipMemcpyAsync(h->hull, hull.cols.data(), hull.cols.size() * sizeof(HullCol), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  TileSwitches sw;
  sw.no_tiles = env_on("BCHMC_NO_TILES");
  sw.no_tiles_low = h->no_tiles_low = env_on("BCHMC_NO_TILES_LOW");
  if (const char *ev = std::getenv("BCHMC_CHUNK")) sw.chunk = std::max(atoi(ev), 1);  // set: the plan clamps it to 64..2048
  if (const char *ev = std::getenv("BCHMC_SORT_CAP")) {
    sw.has_cap = true;
    sw.cap = atoll(ev);
  }
  sw.cap_fixed = env_on("BCHMC_SORT_CAP_FIXED");
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  h->plan = plan_tiles(h->g.n, c.mk, c.min1, c.min2, c.min3, c.particle_kernel_h, h->g.d, h->g.N, h->esz, hull, sw, total_b);
  if (!h->plan.tiled) return BCHMC_OK;
  const size_t nt = (size_t)h->plan.tp.ntiles;
  CHK(dev_alloc(h, h->t_cnt, (kOct + 1) * nt + 3));
  CHK(dev_alloc(h, h->t_oct, 2 * nt));
  CHK(dev_alloc(h, h->t_seg, (size_t)1));
  CHK(dev_alloc(h, h->t_off, nt));
  CHK(dev_alloc(h, h->t_end, nt));
  CHK(dev_alloc(h, h->t_woff, nt + 1));
  CHK(dev_alloc(h, h->t_rank, N));
  CHK(dev_alloc(h, h->srec, h->plan.nrec * 4 * h->esz));
  return BCHMC_OK;
}

}  // namespace

// ======================================================================================================
// C ABI
// ======================================================================================================
extern "C" {

const char *bchmc_strerror(int code) {
  switch (code) {
    case BCHMC_OK: return "ok";
    case BCHMC_ERR_ARG: return "invalid argument";
    case BCHMC_ERR_MK_NOT_SPH: return "Must use SPH mass kernel (masskernel = 3) when using calc_h = 2 or 3";
    case BCHMC_ERR_RSD_NOT_PLANEPAR: return "Non-plane-parallel RSD model is not implemented; use planepar = true";
    case BCHMC_ERR_MASS_TYPE: return "mass_type is not a valid value";
    case BCHMC_ERR_UNSUPPORTED: return "configuration not supported by this build";
    case BCHMC_ERR_HIP: return "HIP runtime error";
    case BCHMC_ERR_ROCFFT: return "rocFFT error";
    case BCHMC_ERR_NOMEM: return "out of device memory";
    case BCHMC_ERR_STATE: return "engine state error (missing input?)";
  }
  return "unknown error";
}

const char *bchmc_last_error(const bchmc_handle *h) { return h ? h->err.c_str() : ""; }

const char *bchmc_kernel_name(int cls) {
  static const char *names[BCHMC_K_COUNT] = {"rocfft_c2r",   "rocfft_r2c",           "k_kick_drift_za",
                                            "k_scatter_sph", "k_sum+k_partial_like", "k_gather_sph",
                                            "k_assemble",    "k_bin+k_scan_tiles+k_reorder", "other"};
  return (cls >= 0 && cls < BCHMC_K_COUNT) ? names[cls] : "?";
}

int bchmc_create(const bchmc_config *cfg, bchmc_handle **out) {
  if (!cfg || !out) return BCHMC_ERR_ARG;
  *out = nullptr;
  bchmc_handle *h = new bchmc_handle();
  auto bail = [&](int rc) {
    // keep the handle alive so the caller can read bchmc_last_error; it is freed by bchmc_destroy
    *out = h;
    return rc;
  };
  int rc = validate_config(cfg, h->err);
  if (rc) return bail(rc);
  h->c = *cfg;
  h->f32 = (cfg->precision == 1);
  h->fix = cfg->deterministic != 0 || env_on("BCHMC_DETERMINISTIC");
  h->esz = h->f32 ? sizeof(float) : sizeof(double);
  switch (cfg->mass_type) {  // struct_hamil.h:272-313
    case 0: case 6: case 60: h->mass_rs = 1; h->mass_fs = 0; break;
    case 1: case 2: case 3: case 4: h->mass_rs = 0; h->mass_fs = 1; break;
    case 5: h->mass_rs = 1; h->mass_fs = 1; break;
    default: return bail(h->fail(BCHMC_ERR_MASS_TYPE, "mass_type %d is not a valid value!", cfg->mass_type));
  }
  Geo &g = h->g;
  g.n = (int)cfg->Nx;
  g.nh = g.n / 2 + 1;
  g.N = (long long)g.n * g.n * g.n;
  g.Nh = (long long)g.n * g.n * g.nh;
  g.nhp = fft_row_stride(g.n, (int)h->esz);  // whole 128-byte lines per row for n >= 128 (fft_host.hpp)
  g.Nhp = (long long)g.n * g.n * g.nhp;
  g.L = cfg->L;
  g.d = cfg->L / (double)cfg->Nx;
  g.kfac = 2. * M_PI / cfg->L;

  auto run = [&]() -> int {
    HIPCHK(hipSetDevice(cfg->device));
    CHK(create_stream(h));
    FFTCHK(h->fft_user.acquire());
    CHK(make_plans_3d(h));
    {
      // planes mode (k_step_boundary_x): an n its table has (powers of two), whole 128-byte k-groups per row
      int l2 = 0;
      while ((1 << l2) < g.n) l2++;
      if (x_shape((int)h->esz, g.n).nt && g.nhp % pass_kb((int)h->esz) == 0) {
        h->log2n = l2;
        const bool ok2 = make_plans_2d(h, 3 * (size_t)g.n, h->r2c2d, h->c2r2d) == BCHMC_OK;
        // twiddles exp(-2 pi i r / n), r < n / 2, from the host's libm (fft_host.hpp)
        CHK(dev_alloc(h, h->xtw, (size_t)g.n * h->esz));
        if (h->f32) {
          const std::vector<float> twf = fft_twiddles<float>(g.n);
          HIPCHK(hipMemcpyAsync(h->xtw, twf.data(), twf.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
          HIPCHK(hipStreamSynchronize(h->stream));
        } else {
          const std::vector<double> tw = fft_twiddles<double>(g.n);
          HIPCHK(hipMemcpyAsync(h->xtw, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
          HIPCHK(hipStreamSynchronize(h->stream));
        }
        h->planes_ok = ok2;
        // the ALPT model's planes pipeline transforms two fields at a time (alpt_x.hpp): plans made here, not inside
        // the first trajectory
        if (ok2 && !cfg->rsd_model && cfg->sfmodel != 1 && cfg->calc_h == 2 && cfg->mk == 3 &&
            make_plans_2d(h, 2 * (size_t)g.n, h->r2c2d_2, h->c2r2d_2) != BCHMC_OK)
          h->alpt_plans_failed = true;
      }
    }
    size_t work_bytes = 0;
    for (const FftPlan *p : {&h->r2c1, &h->c2r1, &h->r2c3, &h->c2r3, &h->r2c2d, &h->c2r2d, &h->r2c2d_2, &h->c2r2d_2}) {
      if (!*p) continue;
      size_t wb = 0;
      FFTCHK(rocfft_plan_get_work_buffer_size(*p, &wb));
      work_bytes = std::max(work_bytes, wb);
    }
    FFTCHK(h->info.create(rocfft_execution_info_create));
    FFTCHK(rocfft_execution_info_set_stream(h->info, h->stream));
    if (work_bytes) {
      HIPCHK(h->work.alloc(work_bytes));
      FFTCHK(rocfft_execution_info_set_work_buffer(h->info, h->work, work_bytes));
    }
    const size_t N = (size_t)g.N, Nh = (size_t)g.Nhp, e = h->esz;
    for (int f = 0; f < 6; f++) CHK(dev_alloc(h, h->in_arr[f], N * e));
    CHK(dev_alloc(h, h->wS, Nh));
    CHK(dev_alloc(h, h->wM, Nh));
    CHK(dev_alloc(h, h->qk, 2 * Nh * e));
    CHK(dev_alloc(h, h->pk, 2 * Nh * e));
    CHK(dev_alloc(h, h->gk, 2 * Nh * e));
    CHK(dev_alloc(h, h->Ck, 3 * 2 * (size_t)g.Nhp * e));
    CHK(dev_alloc(h, h->tC, 2 * Nh * e));
    CHK(dev_alloc(h, h->psi, 3 * N * e));
    CHK(dev_alloc(h, h->V, 3 * N * e));
    CHK(dev_alloc(h, h->rho, N * e));
    CHK(dev_alloc(h, h->plike, N * e));
    if (h->fix) CHK(dev_alloc(h, h->rho_fix, N));
    if (h->fix) CHK(dev_alloc(h, h->fix_sat, (size_t)1));
    if (const char *ev = std::getenv("BCHMC_FIX_SAT_LOG2")) h->fix_sat_limit = 1ll << std::min(std::max(atoi(ev), 1), 62);
    CHK(dev_alloc(h, h->ioq, N * e));
    CHK(dev_alloc(h, h->iop, N * e));
    CHK(dev_alloc(h, h->dstage, 2 * N));
    CHK(dev_alloc(h, h->rho_part, (size_t)kRedBlocks));
    CHK(dev_alloc(h, h->partA, (size_t)kRedBlocks));
    CHK(dev_alloc(h, h->stop, (size_t)1));
    CHK(dev_alloc(h, h->steps_done, (size_t)1));
    HIPCHK(hipMemsetAsync(h->stop, 0, sizeof(int), h->stream));
    HIPCHK(h->h_part.alloc(kRedBlocks));
    CHK(make_tiles(h));            // reads the tile switches ...
    h->sw = read_path_switches();  // ... and this the path switches: from here on the environment's do not matter
    HIPCHK(hipStreamSynchronize(h->stream));
    return BCHMC_OK;
  };
  rc = run();
  *out = h;
  return rc;
}

void bchmc_destroy(bchmc_handle *h) {
  if (!h) return;
  (void)hipSetDevice(h->c.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  prof_collect(h);
  delete h;  // the owners release everything, in the order the handle declares
}

int bchmc_upload(bchmc_handle *h, bchmc_field field, const double *host, size_t n) {
  if (!h || !host) return BCHMC_ERR_ARG;
  ENTER(h);
  if ((int)field < 0 || (int)field > BCHMC_F_WINDOW) return h->fail(BCHMC_ERR_ARG, "field %d is not an input", (int)field);
  if (n != (size_t)h->g.N) return h->fail(BCHMC_ERR_ARG, "upload size %zu != N = %lld", n, h->g.N);
  CHK(h2d(h, h->dstage, host, n * sizeof(double)));
  CHK(DISPATCH(h, upload(h, field, h->dstage)));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->have[field] = true;
  if (field == BCHMC_F_MASS_R) h->cp_draw_rs = false;
  // gradient_psi and -log L do not involve the mass (it enters the kinetic term and the drift only)
  if (field != BCHMC_F_MASS_F && field != BCHMC_F_MASS_R) h->cg_valid = h->prop_g_valid = false;
  return BCHMC_OK;
}

int bchmc_sync(bchmc_handle *h) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  return read_ctl(h, nullptr);  // synchronises; also picks up the binning's overflow flag
}

void *bchmc_stream(bchmc_handle *h) { return h ? (void *)h->stream : nullptr; }

int bchmc_leapfrog_device(bchmc_handle *h, const double *d_q0, const double *d_p0, double *d_q1, double *d_p1,
                          double eps, uint64_t neps) {
  if (!h || !d_q0 || !d_p0 || !d_q1 || !d_p1) return BCHMC_ERR_ARG;
  ENTER(h);
  clobber_proposal(h);
  return DISPATCH(h, leapfrog_core(h, d_q0, d_p0, d_q1, d_p1, eps, neps));
}

int bchmc_steps_done(bchmc_handle *h, uint64_t *steps_done) {
  if (!h || !steps_done) return BCHMC_ERR_ARG;
  ENTER(h);
  unsigned long long v = 0;
  CHK(read_ctl(h, &v));
  *steps_done = v;
  return BCHMC_OK;
}

// Arms the early download of q1 for the duration of one host-array trajectory (BCHMC_NO_DOWNLOAD_OVERLAP=1: never).
struct EarlyQ {
  bchmc_handle *h;
  EarlyQ(bchmc_handle *h_, double *dev) : h(h_) {
    h->early_q_done = false;
    h->early_q_dev = nullptr;
    if (!dev || !h->copy_stream || env_on("BCHMC_NO_DOWNLOAD_OVERLAP")) return;
    if (!h->ev_q && h->ev_q.create(hipEventDisableTiming) != hipSuccess) return;
    h->early_q_dev = dev;
  }
  ~EarlyQ() {
    h->early_q_dev = nullptr;
    h->early_q_done = false;
  }
};

int bchmc_leapfrog(bchmc_handle *h, const double *q0, const double *p0, double *q1, double *p1, double eps,
                   uint64_t neps, uint64_t *steps_done) {
  if (!h || !q0 || !p0 || !q1 || !p1) return BCHMC_ERR_ARG;
  ENTER(h);
  clobber_proposal(h);
  const size_t N = (size_t)h->g.N, bytes = N * sizeof(double);
  double *dq = h->dstage, *dp = h->dstage + N;
  CHK(h2d(h, dq, q0, bytes));
  // as in bchmc_leapfrog_dh: the start-state force evaluation is enqueued before the momenta are uploaded beside it
  // (any configuration: the force never involves p; HMC.cc:284 with neps = 0 evaluates it too)
  const bool prologue = !env_on("BCHMC_NO_UPLOAD_OVERLAP");
  if (prologue) {
    CHK(DISPATCH(h, plain_prologue(h)));
    if (!h->copy_stream) HIPCHK(h->copy_stream.create(hipStreamNonBlocking));
    CHK(h2d(h, dp, p0, bytes, h->copy_stream));
  } else {
    CHK(h2d(h, dp, p0, bytes));
  }
  EarlyQ early(h, prologue ? dq : nullptr);
  CHK(DISPATCH(h, leapfrog_core(h, dq, dp, dq, dp, eps, neps, prologue)));
  const bool sent = h->early_q_done;
  CHK(sent ? d2h(h, q1, dq, bytes, h->copy_stream, h->ev_q) : d2h(h, q1, dq, bytes));
  CHK(d2h(h, p1, dp, bytes));
  uint64_t done = 0;
  CHK(bchmc_steps_done(h, &done));
  if (sent && done < neps) {  // runaway guard: the q sent early is not the state the trajectory stopped in
    CHK(DISPATCH(h, requeue_q(h, dq)));
    CHK(d2h(h, q1, dq, bytes));
  }
  if (steps_done) *steps_done = done;
  return BCHMC_OK;
}

int bchmc_leapfrog_dh(bchmc_handle *h, const double *q0, const double *p0, double *q1, double *p1, double eps,
                      uint64_t neps, uint64_t *steps_done, double *dH, double terms[6]) {
  if (!h || !q0 || !p0 || !q1 || !p1 || !dH || !terms) return BCHMC_ERR_ARG;
  ENTER(h);
  clobber_proposal(h);
  const size_t N = (size_t)h->g.N, bytes = N * sizeof(double);
  double *dq = h->dstage, *dp = h->dstage + N;
  CHK(h2d(h, dq, q0, bytes));
  // The force evaluation at the start state (HMC.cc:279) needs q0 only: it is enqueued now, and the momenta cross PCIe
  // on a second stream while it runs (h2d returns when its last chunk has arrived, so no event is needed afterwards).
  const bool prologue = DISPATCH(h, host_prologue_applies(h, neps));
  if (prologue) {
    CHK(DISPATCH(h, host_prologue(h)));
    if (!h->copy_stream) HIPCHK(h->copy_stream.create(hipStreamNonBlocking));
    CHK(h2d(h, dp, p0, bytes, h->copy_stream));
  } else {
    CHK(h2d(h, dp, p0, bytes));
  }
  uint64_t done = 0;
  // one pass: the trajectory's own first and last force evaluation carry -log L of both ends, K and psi_prior are
  // Parseval sums of the k-space state (the resident chain's attempt_core); generic configurations evaluate the
  // energies around the trajectory without further transfers
  EarlyQ early(h, prologue ? dq : nullptr);
  CHK(DISPATCH(h, leapfrog_host_core(h, eps, neps, terms, &done, prologue, q1)));
  if (!h->early_q_done) CHK(d2h(h, q1, dq, bytes));  // else: q1 crossed PCIe beside the last force evaluation
  CHK(d2h(h, p1, dp, bytes));
  if (steps_done) *steps_done = done;
  const double Hami = terms[0] + (terms[1] + terms[2]);
  const double Hamf = terms[3] + (terms[4] + terms[5]);
  double d = Hamf - Hami;
  if (h->c.div_dH_by_N) d /= (double)h->g.N;  // HMC.cc:234-237
  *dH = d;
  return BCHMC_OK;
}

int bchmc_energies_device(bchmc_handle *h, const double *d_q, const double *d_p, double out[3]) {
  if (!h || !d_q || !d_p || !out) return BCHMC_ERR_ARG;
  ENTER(h);
  clobber_proposal(h);
  return DISPATCH(h, energies_core(h, d_q, d_p, out));
}

int bchmc_energies(bchmc_handle *h, const double *q, const double *p, double out[3]) {
  if (!h || !q || !p || !out) return BCHMC_ERR_ARG;
  ENTER(h);
  clobber_proposal(h);
  const size_t N = (size_t)h->g.N, bytes = N * sizeof(double);
  CHK(h2d(h, h->dstage, q, bytes));
  CHK(h2d(h, h->dstage + N, p, bytes));
  CHK(DISPATCH(h, energies_core(h, h->dstage, h->dstage + N, out)));
  return read_ctl(h, nullptr);
}

int bchmc_kinetic_term(bchmc_handle *h, const double *p, double *out) {
  if (!h || !p || !out) return BCHMC_ERR_ARG;
  ENTER(h);
  clobber_proposal(h);
  CHK(h2d(h, h->dstage + (size_t)h->g.N, p, (size_t)h->g.N * sizeof(double)));
  return DISPATCH(h, kinetic_core(h, h->dstage + (size_t)h->g.N, out));
}

int bchmc_psi(bchmc_handle *h, const double *q, double out[2]) {
  if (!h || !q || !out) return BCHMC_ERR_ARG;
  ENTER(h);
  clobber_proposal(h);
  CHK(h2d(h, h->dstage, q, (size_t)h->g.N * sizeof(double)));
  CHK(DISPATCH(h, psi_core(h, h->dstage, out)));
  return read_ctl(h, nullptr);
}

int bchmc_delta_hamiltonian(bchmc_handle *h, const double *qi, const double *pi, const double *qf, const double *pf,
                            double *dH, double terms[6]) {
  if (!h || !dH || !terms || !qi || !pi || !qf || !pf) return BCHMC_ERR_ARG;
  // always evaluated: kinetic_term + psi at both ends, HMC.cc:214-225, psi(signalf) last.  A caller that has just run
  // the trajectory on these arrays gets the same six terms from bchmc_leapfrog_dh without the four uploads.
  CHK(bchmc_energies(h, qi, pi, terms));
  CHK(bchmc_energies(h, qf, pf, terms + 3));
  const double Hami = terms[0] + (terms[1] + terms[2]);
  const double Hamf = terms[3] + (terms[4] + terms[5]);
  double d = Hamf - Hami;
  if (h->c.div_dH_by_N) d /= (double)h->g.N;  // HMC.cc:234-237
  *dH = d;
  return BCHMC_OK;
}

int bchmc_forward(bchmc_handle *h, const double *q, int use_rsd) {
  if (!h || !q) return BCHMC_ERR_ARG;
  ENTER(h);
  clobber_proposal(h);
  CHK(h2d(h, h->dstage, q, h->g.N * sizeof(double)));
  CHK(DISPATCH(h, forward(h, h->dstage, use_rsd < 0 ? h->c.rsd_model : (use_rsd ? 1 : 0))));
  return read_ctl(h, nullptr);  // synchronises; enlarges the binning's record slots if this field overflowed them
}

int bchmc_probe_displacement(bchmc_handle *h, const double *psi, int use_rsd, int with_force) {
  if (!h || !psi) return BCHMC_ERR_ARG;
  ENTER(h);
  const int rsd = use_rsd < 0 ? h->c.rsd_model : (use_rsd ? 1 : 0);
  if (rsd && !h->c.planepar) return h->fail(BCHMC_ERR_RSD_NOT_PLANEPAR, "non-plane-parallel RSD is not implemented");
  if (with_force) {
    if (h->c.likelihood == 3)
      return h->fail(BCHMC_ERR_UNSUPPORTED, "the GRF likelihood's force has no particle stage to probe");
    CHK(check_inputs(h));
  }
  clobber_proposal(h);
  h->cg_valid = false;
  const size_t N = (size_t)h->g.N;
  for (int c = 0; c < 3; c++) {
    CHK(h2d(h, h->dstage, psi + c * N, N * sizeof(double)));
    CHK(DISPATCH(h, probe_load(h, c)));
  }
  CHK(DISPATCH(h, probe(h, rsd, with_force != 0)));
  return read_ctl(h, nullptr);  // synchronises; adapts the binning's record slots like bchmc_forward
}

int bchmc_probe_displacement_z(bchmc_handle *h, const double *psi, int use_rsd, int with_force, int store_psi) {
  if (!h || !psi) return BCHMC_ERR_ARG;
  ENTER(h);
  const int rsd = use_rsd < 0 ? h->c.rsd_model : (use_rsd ? 1 : 0);
  if (const char *why = zbin_why_not_text(zbin_why_not(path_facts(h, h->c.rsd_model), h->sw)))
    return h->fail(BCHMC_ERR_UNSUPPORTED, "the fused z pass + binning does not run on this handle: %s", why);
  if (rsd && !h->c.planepar) return h->fail(BCHMC_ERR_RSD_NOT_PLANEPAR, "non-plane-parallel RSD is not implemented");
  if (with_force) {
    if (h->c.likelihood == 3)
      return h->fail(BCHMC_ERR_UNSUPPORTED, "the GRF likelihood's force has no particle stage to probe");
    CHK(check_inputs(h));
  }
  clobber_proposal(h);
  h->cg_valid = false;
  const size_t N = (size_t)h->g.N;
  for (int c = 0; c < 3; c++) {
    CHK(h2d(h, h->dstage, psi + c * N, N * sizeof(double)));
    CHK(DISPATCH(h, probe_load(h, c)));
  }
  CHK(DISPATCH(h, probe_z(h, rsd, with_force != 0, store_psi != 0)));
  return read_ctl(h, nullptr);  // synchronises; adapts the binning's record slots like bchmc_forward
}

int bchmc_gradient(bchmc_handle *h, const double *q, double *gout) {
  if (!h || !q || !gout) return BCHMC_ERR_ARG;
  ENTER(h);
  clobber_proposal(h);
  CHK(check_inputs(h));
  const size_t N = (size_t)h->g.N;
  CHK(h2d(h, h->dstage, q, N * sizeof(double)));
  CHK(DISPATCH(h, gradient(h, h->dstage, h->dstage + N)));
  CHK(d2h(h, gout, h->dstage + N, N * sizeof(double)));
  return read_ctl(h, nullptr);
}

int bchmc_fetch(bchmc_handle *h, bchmc_field field, double *host, size_t n) {
  if (!h || !host) return BCHMC_ERR_ARG;
  ENTER(h);
  if (n != (size_t)h->g.N) return h->fail(BCHMC_ERR_ARG, "fetch size %zu != N = %lld", n, h->g.N);
  CHK(fetch_ready(h, (int)field));
  CHK(DISPATCH(h, fetch(h, field, h->dstage)));
  CHK(d2h(h, host, h->dstage, n * sizeof(double)));
  return BCHMC_OK;
}

// ---- device-resident chain ------------------------------------------------------------------------------------
int bchmc_chain_set_state(bchmc_handle *h, const double *q) {
  if (!h || !q) return BCHMC_ERR_ARG;
  ENTER(h);
  CHK(DISPATCH(h, chain_alloc(h)));
  CHK(h2d(h, h->dstage, q, h->g.N * sizeof(double)));
  CHK(DISPATCH(h, r2c_state(h, h->dstage, h->ioq, h->cq)));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->have_cq = true;
  h->have_prop = false;
  h->cg_valid = h->prop_g_valid = false;
  return BCHMC_OK;
}

int bchmc_chain_set_momenta(bchmc_handle *h, const double *p) {
  if (!h || !p) return BCHMC_ERR_ARG;
  ENTER(h);
  CHK(DISPATCH(h, chain_alloc(h)));
  CHK(h2d(h, h->dstage, p, h->g.N * sizeof(double)));
  CHK(DISPATCH(h, r2c_state(h, h->dstage, h->iop, h->cp)));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->have_cp = true;
  h->cp_draw_rs = false;
  return BCHMC_OK;
}

int bchmc_chain_draw_momenta(bchmc_handle *h, uint64_t seed, uint64_t attempt) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  // the attempt is one 32-bit word of the Philox counter: refuse what would wrap onto an earlier attempt's values
  if (attempt >> 32)
    return h->fail(BCHMC_ERR_ARG, "attempt = %llu does not fit the counter's 32-bit word", (unsigned long long)attempt);
  if (h->mass_fs && !h->have[BCHMC_F_MASS_F]) return h->fail(BCHMC_ERR_STATE, "mass_f was never uploaded");
  if (h->mass_rs && !h->have[BCHMC_F_MASS_R]) return h->fail(BCHMC_ERR_STATE, "mass_r was never uploaded");
  CHK(DISPATCH(h, chain_alloc(h)));
  CHK(DISPATCH(h, chain_draw(h, seed, attempt)));
  h->have_cp = true;
  h->cp_draw_rs = h->mass_rs && !h->mass_fs;
  return BCHMC_OK;
}

int bchmc_chain_draw_momenta_mt19937(bchmc_handle *h, uint32_t mt[624], int32_t *mti, uint64_t *words_used) {
  if (!h || !mt || !mti) return BCHMC_ERR_ARG;
  if (*mti < 0 || *mti > 624) return h->fail(BCHMC_ERR_ARG, "mti = %d outside [0, 624]", (int)*mti);
  ENTER(h);
  // the Fourier-space part is placed by create_GARFIELD's walk (mt_walk_index), which pairs i with n - i around i = n / 2;
  // the real-space part (mass_type 0, 6, 60) is white noise per cell and has no such condition
  if (h->mass_fs && (h->g.n & 1))
    return h->fail(BCHMC_ERR_UNSUPPORTED, "create_GARFIELD's placement needs an even Nx (%d)", h->g.n);
  if (h->mass_fs && !h->have[BCHMC_F_MASS_F]) return h->fail(BCHMC_ERR_STATE, "mass_f was never uploaded");
  if (h->mass_rs && !h->have[BCHMC_F_MASS_R]) return h->fail(BCHMC_ERR_STATE, "mass_r was never uploaded");
  CHK(DISPATCH(h, chain_alloc(h)));
  CHK(mt_setup(h));
  CHK(mt_draw(h, mt, mti, words_used, h->mt.G, false, mt_place_momenta));
  h->have_cp = true;
  h->cp_draw_rs = h->mass_rs && !h->mass_fs;
  return BCHMC_OK;
}

int bchmc_mt19937_jump(const uint32_t mt_in[624], int32_t mti_in, uint64_t steps, uint32_t mt_out[624],
                       int32_t *mti_out) {
  if (!mt_in || !mt_out || !mti_out) return BCHMC_ERR_ARG;
  return mt_jump_gsl(mt_in, mti_in, steps, mt_out, mti_out);
}

int bchmc_garfield_walk_index(uint32_t n, uint32_t i, uint32_t j, uint32_t k, uint64_t *index) {
  if (!index || n < 2 || (n & 1) || n > (1u << 20) || i >= n || j >= n || k >= n) return BCHMC_ERR_ARG;
  *index = mt_walk_index((int)n, (int)i, (int)j, (int)k);
  return BCHMC_OK;
}

static int chain_fetch(bchmc_handle *h, const void *xk, double *host) {
  CHK(DISPATCH(h, c2r_state(h, xk, h->ioq, h->dstage)));
  return d2h(h, host, h->dstage, h->g.N * sizeof(double));
}

int bchmc_chain_get_state(bchmc_handle *h, double *q) {
  if (!h || !q) return BCHMC_ERR_ARG;
  ENTER(h);
  if (!h->have_cq) return h->fail(BCHMC_ERR_STATE, "no chain state set");
  return chain_fetch(h, h->cq, q);
}

int bchmc_chain_get_momenta(bchmc_handle *h, double *p) {
  if (!h || !p) return BCHMC_ERR_ARG;
  ENTER(h);
  if (!h->have_cp) return h->fail(BCHMC_ERR_STATE, "no momenta set or drawn");
  CHK(DISPATCH(h, momenta_to_stage(h)));
  return d2h(h, p, h->dstage, h->g.N * sizeof(double));
}

int bchmc_chain_get_proposal(bchmc_handle *h, double *q1, double *p1) {
  if (!h || !q1 || !p1) return BCHMC_ERR_ARG;
  ENTER(h);
  if (!h->have_prop) return h->fail(BCHMC_ERR_STATE, "no proposal: call bchmc_chain_attempt first");
  CHK(chain_fetch(h, h->qk, q1));
  return chain_fetch(h, h->pk, p1);
}

int bchmc_chain_attempt(bchmc_handle *h, double eps, uint64_t neps, double *dH, double terms[6],
                        uint64_t *steps_done) {
  if (!h || !dH || !terms) return BCHMC_ERR_ARG;
  ENTER(h);
  if (!h->have_cq || !h->have_cp) return h->fail(BCHMC_ERR_STATE, "chain state and momenta must be set first");
  CHK(DISPATCH(h, chain_attempt(h, eps, neps, terms, steps_done)));
  const double Hami = terms[0] + (terms[1] + terms[2]);
  const double Hamf = terms[3] + (terms[4] + terms[5]);
  double d = Hamf - Hami;
  if (h->c.div_dH_by_N) d /= (double)h->g.N;  // HMC.cc:234-237
  *dH = d;
  return BCHMC_OK;
}

int bchmc_chain_accept(bchmc_handle *h, int accepted) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  if (!h->have_prop) return h->fail(BCHMC_ERR_STATE, "no proposal: call bchmc_chain_attempt first");
  if (accepted) {  // HMC.cc:497-498: copyArray(signalf, hd->x)
    HIPCHK(hipMemcpyAsync(h->cq, h->qk, 2 * (size_t)h->g.Nhp * h->esz, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->prop_g_valid) {  // the proposal's gradient and -log L become the chain state's
      std::swap(h->gk, h->cg);
      h->c_like = h->prop_like;
      h->cg_valid = true;
    } else {
      h->cg_valid = false;
    }
  }
  h->prop_g_valid = false;
  h->have_prop = false;
  return BCHMC_OK;
}

int bchmc_measure_spectrum(bchmc_handle *h, const double *signal, uint64_t n_bin, double *kmode, double *power) {
  if (!h || !kmode || !power || n_bin == 0 || n_bin > 2048) return BCHMC_ERR_ARG;
  ENTER(h);
  const void *xk = nullptr;
  if (signal) {
    CHK(h2d(h, h->dstage, signal, h->g.N * sizeof(double)));
    CHK(DISPATCH(h, r2c_state(h, h->dstage, h->ioq, h->tC)));
    xk = h->tC;
  } else {
    if (!h->have_cq) return h->fail(BCHMC_ERR_STATE, "no chain state: call bchmc_chain_set_state first");
    xk = h->cq;
  }
  return spectrum_bins(h, xk, n_bin, kmode, power);
}

static int corr_measure(bchmc_handle *h, bool two_d, bchmc_corr_source src, const double *signal, uint64_t n_bin,
                        double *rmode, uint64_t *nmode, double *corr) {
  if (!h || !rmode || !nmode || !corr) return BCHMC_ERR_ARG;
  const char *name = two_d ? "measure_corr2d" : "measure_corr";
  if (n_bin == 0 || n_bin > 2048) return h->fail(BCHMC_ERR_ARG, "%s: n_bin = %llu outside 1..2048", name, (unsigned long long)n_bin);
  if (src != BCHMC_CORR_HOST && src != BCHMC_CORR_CHAIN_STATE && src != BCHMC_CORR_DELTAX)
    return h->fail(BCHMC_ERR_ARG, "%s: unknown source %d", name, (int)src);
  if ((src == BCHMC_CORR_HOST) != (signal != nullptr))
    return h->fail(BCHMC_ERR_ARG, "%s: signal must be given for BCHMC_CORR_HOST and NULL otherwise", name);
  ENTER(h);
  if (src == BCHMC_CORR_CHAIN_STATE && !h->have_cq)
    return h->fail(BCHMC_ERR_STATE, "no chain state: call bchmc_chain_set_state first");
  if (src == BCHMC_CORR_DELTAX && !h->have_eval) return h->fail(BCHMC_ERR_STATE, "no forward evaluation to take deltaX from");
  // both kernels are laid out for n <= 1024: the 1-D limb sums hold N <= 2^30 cells, the 2-D slices 4 k per thread of 256
  if (h->g.n > 1024) return h->fail(BCHMC_ERR_UNSUPPORTED, "%s: n = %d > 1024", name, h->g.n);
  if (two_d) CHK(corr2d_setup(h, h->corr2, h->g, n_bin, INFINITY));
  if (signal) CHK(h2d(h, h->dstage, signal, h->g.N * sizeof(double)));
  CHK(DISPATCH(h, corr_field(h, (int)src)));
  return two_d ? DISPATCH(h, corr2d_bins(h, h->corr2, h->g, h->ioq, n_bin, rmode, nmode, corr)) : DISPATCH(h, corr1d_bins(h, n_bin, rmode, nmode, corr));
}

int bchmc_measure_corr(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *rmode,
                       uint64_t *nmode, double *corr) {
  return corr_measure(h, false, src, signal, n_bin, rmode, nmode, corr);
}

int bchmc_measure_corr2d(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *rmode,
                         uint64_t *nmode, double *corr) {
  return corr_measure(h, true, src, signal, n_bin, rmode, nmode, corr);
}

// What the entry points with a bchmc_corr_source check before anything is queued (bchmc_measure_corr2d's rules)
static int source_args(bchmc_handle *h, const char *name, bchmc_corr_source src, const double *signal) {
  if (src != BCHMC_CORR_HOST && src != BCHMC_CORR_CHAIN_STATE && src != BCHMC_CORR_DELTAX)
    return h->fail(BCHMC_ERR_ARG, "%s: unknown source %d", name, (int)src);
  if ((src == BCHMC_CORR_HOST) != (signal != nullptr))
    return h->fail(BCHMC_ERR_ARG, "%s: signal must be given for BCHMC_CORR_HOST and NULL otherwise", name);
  return BCHMC_OK;
}
static int source_state(bchmc_handle *h, bchmc_corr_source src) {
  if (src == BCHMC_CORR_CHAIN_STATE && !h->have_cq)
    return h->fail(BCHMC_ERR_STATE, "no chain state: call bchmc_chain_set_state first");
  if (src == BCHMC_CORR_DELTAX && !h->have_eval) return h->fail(BCHMC_ERR_STATE, "no forward evaluation to take deltaX from");
  return BCHMC_OK;
}
static int upres_n_out(bchmc_handle *h, const char *name, uint32_t n_out) {
  // the 2-D slice kernel holds 4 k per thread of 256, interp_field's rows 4 n elements of LDS
  if (n_out < 4 || n_out > 1024) return h->fail(BCHMC_ERR_ARG, "%s: n_out = %u outside 4..1024", name, n_out);
  return BCHMC_OK;
}

int bchmc_interp_upres(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint32_t n_out, double *out) {
  if (!h || !out) return BCHMC_ERR_ARG;
  const char *name = "interp_upres";
  CHK(source_args(h, name, src, signal));
  CHK(upres_n_out(h, name, n_out));
  ENTER(h);
  CHK(source_state(h, src));
  if (h->g.n > 1024) return h->fail(BCHMC_ERR_UNSUPPORTED, "%s: n = %d > 1024", name, h->g.n);
  CHK(upres_setup(h, (int)n_out));
  if (signal) CHK(h2d(h, h->dstage, signal, h->g.N * sizeof(double)));
  CHK(DISPATCH(h, upres_interp(h, (int)src)));
  return DISPATCH(h, upres_fetch(h, out));
}

int bchmc_measure_corr2d_interp(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint32_t n_out, int32_t mode,
                                double l_max, uint64_t n_bin, double *rmode, uint64_t *nmode, double *corr) {
  if (!h || !rmode || !nmode || !corr) return BCHMC_ERR_ARG;
  const char *name = "measure_corr2d_interp";
  if (n_bin == 0 || n_bin > 2048) return h->fail(BCHMC_ERR_ARG, "%s: n_bin = %llu outside 1..2048", name, (unsigned long long)n_bin);
  CHK(source_args(h, name, src, signal));
  CHK(upres_n_out(h, name, n_out));
  if (mode != 0 && mode != 1) return h->fail(BCHMC_ERR_ARG, "%s: mode %d is neither 0 (CIC) nor 1 (zero padding)", name, (int)mode);
  if (mode == 1 && (int)n_out < h->g.n)
    return h->fail(BCHMC_ERR_ARG, "%s: zero padding needs n_out = %u >= n = %d", name, n_out, h->g.n);
  if (mode == 0 && !(l_max > 0.)) return h->fail(BCHMC_ERR_ARG, "%s: l_max = %g is not > 0", name, l_max);
  ENTER(h);
  CHK(source_state(h, src));
  if (h->g.n > 1024) return h->fail(BCHMC_ERR_UNSUPPORTED, "%s: n = %d > 1024", name, h->g.n);
  CHK(upres_setup(h, (int)n_out));
  auto &u = h->up;
  if (const int rc = corr2d_setup(h, u.bins, u.g, n_bin, mode == 0 ? l_max : (double)INFINITY)) {
    upres_drop(h);  // the tables did not fit: the fine grid goes too, the handle stays usable
    return rc;
  }
  if (signal) CHK(h2d(h, h->dstage, signal, h->g.N * sizeof(double)));
  CHK(mode == 0 ? DISPATCH(h, upres_corr_cic(h, (int)src)) : DISPATCH(h, upres_corr_zeropad(h, (int)src)));
  return DISPATCH(h, corr2d_bins(h, u.bins, u.g, u.real, n_bin, rmode, nmode, corr));
}

int bchmc_upres_release(bchmc_handle *h) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  upres_drop(h);
  return BCHMC_OK;
}

int bchmc_measure_spectrum_src(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *kmode,
                               double *power) {
  if (!h || !kmode || !power) return BCHMC_ERR_ARG;
  const char *name = "measure_spectrum_src";
  if (n_bin == 0 || n_bin > 2048) return h->fail(BCHMC_ERR_ARG, "%s: n_bin = %llu outside 1..2048", name, (unsigned long long)n_bin);
  CHK(source_args(h, name, src, signal));
  ENTER(h);
  CHK(source_state(h, src));
  if (signal) CHK(h2d(h, h->dstage, signal, h->g.N * sizeof(double)));
  const void *xk = nullptr;
  CHK(DISPATCH(h, spectrum_source(h, (int)src, &xk)));
  return spectrum_bins(h, xk, n_bin, kmode, power);
}

int bchmc_measure_spectrum2d(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *kmode,
                             uint64_t *nmode, double *power) {
  if (!h || !kmode || !power) return BCHMC_ERR_ARG;
  const char *name = "measure_spectrum2d";
  if (n_bin == 0 || n_bin > 2048) return h->fail(BCHMC_ERR_ARG, "%s: n_bin = %llu outside 1..2048", name, (unsigned long long)n_bin);
  CHK(source_args(h, name, src, signal));
  ENTER(h);
  CHK(source_state(h, src));
  // the reduce kernel keeps a row's nh column sums in LDS and the tables are sized like the correlation functions'
  if (h->g.n > 1024) return h->fail(BCHMC_ERR_UNSUPPORTED, "%s: n = %d > 1024", name, h->g.n);
  CHK(spec2d_setup(h, n_bin));
  if (signal) CHK(h2d(h, h->dstage, signal, h->g.N * sizeof(double)));
  const void *xk = nullptr;
  CHK(DISPATCH(h, spectrum_source(h, (int)src, &xk)));
  return DISPATCH(h, spec2d_bins(h, xk, n_bin, kmode, nmode, power));
}

int bchmc_measure_cross_spectrum(bchmc_handle *h, bchmc_corr_source src_a, const double *signal_a, bchmc_corr_source src_b,
                                 const double *signal_b, uint64_t n_bin, double *kmode, uint64_t *nmode, double *power_a,
                                 double *power_b, double *cross, double *coeff) {
  if (!h || !kmode || !power_a || !power_b || !cross || !coeff) return BCHMC_ERR_ARG;
  const char *name = "measure_cross_spectrum";
  if (n_bin == 0 || n_bin > 2048) return h->fail(BCHMC_ERR_ARG, "%s: n_bin = %llu outside 1..2048", name, (unsigned long long)n_bin);
  CHK(source_args(h, name, src_a, signal_a));
  CHK(source_args(h, name, src_b, signal_b));
  ENTER(h);
  CHK(source_state(h, src_a));
  CHK(source_state(h, src_b));
  if (!h->cross_ak) CHK(dev_alloc(h, h->cross_ak, 2 * (size_t)h->g.Nhp * h->esz));
  const void *ak = nullptr, *bk = nullptr;
  CHK(DISPATCH(h, cross_source(h, (int)src_a, signal_a, h->cross_ak, &ak)));
  CHK(DISPATCH(h, cross_source(h, (int)src_b, signal_b, h->tC, &bk)));
  return cross_bins(h, ak, bk, n_bin, kmode, nmode, power_a, power_b, cross, coeff);
}

// ---- bchmc_ensemble_* (ensemble.hpp) -----------------------------------------------------------------------------------
static int ens_slot(bchmc_handle *h, const char *name, int32_t slot) {
  if (slot < 0 || slot >= BCHMC_ENS_SLOTS)
    return h->fail(BCHMC_ERR_ARG, "%s: slot %d outside 0..%d", name, (int)slot, BCHMC_ENS_SLOTS - 1);
  return BCHMC_OK;
}
// Workgroups of the ensemble kernels: enough to cover the pairs of cells, at most kEnsBlocksPerCu per compute unit
static int ens_blocks(bchmc_handle *h, int *blocks) {
  if (!h->ens.ncu) {
    int ncu = 0;
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->c.device));
    h->ens.ncu = std::max(ncu, 1);
  }
  const long long pairs = h->g.N >> 1;
  *blocks = (int)std::min<long long>((pairs + kEnsBlock - 1) / kEnsBlock, (long long)h->ens.ncu * kEnsBlocksPerCu);
  return BCHMC_OK;
}
// The slot's two arrays, zeroed on the handle's stream, on its first add or merge; a failed allocation leaves the slot
// empty and the handle usable.
static int ens_take(bchmc_handle *h, bchmc_handle::Ens::Slot &s) {
  if (s.mean && s.m2) return BCHMC_OK;
  int rc = dev_alloc(h, s.mean, (size_t)h->g.N);
  if (!rc) rc = dev_alloc(h, s.m2, (size_t)h->g.N);
  if (rc) {
    (void)s.mean.release();
    (void)s.m2.release();
    s.count = 0;
  }
  return rc;
}

int bchmc_ensemble_add(bchmc_handle *h, int32_t slot, bchmc_corr_source src, const double *signal) {
  if (!h) return BCHMC_ERR_ARG;
  const char *name = "ensemble_add";
  CHK(ens_slot(h, name, slot));
  CHK(source_args(h, name, src, signal));
  ENTER(h);
  CHK(source_state(h, src));
  auto &s = h->ens.slot[slot];
  if (s.count == UINT64_MAX) return h->fail(BCHMC_ERR_STATE, "%s: the count of slot %d is full", name, (int)slot);
  int blocks = 0;
  CHK(ens_blocks(h, &blocks));
  CHK(ens_take(h, s));
  if (signal) CHK(h2d(h, h->dstage, signal, h->g.N * sizeof(double)));
  CHK(DISPATCH(h, ens_add(h, (int)src, s.mean, s.m2, (double)(s.count + 1), blocks)));
  HIPCHK(hipStreamSynchronize(h->stream));
  s.count++;
  return BCHMC_OK;
}

int bchmc_ensemble_count(bchmc_handle *h, int32_t slot, uint64_t *count) {
  if (!h || !count) return BCHMC_ERR_ARG;
  CHK(ens_slot(h, "ensemble_count", slot));
  *count = h->ens.slot[slot].count;
  return BCHMC_OK;
}

int bchmc_ensemble_fetch(bchmc_handle *h, int32_t slot, bchmc_ens_what what, double *out) {
  if (!h || !out) return BCHMC_ERR_ARG;
  const char *name = "ensemble_fetch";
  CHK(ens_slot(h, name, slot));
  if (what != BCHMC_ENS_MEAN && what != BCHMC_ENS_VARIANCE && what != BCHMC_ENS_STD && what != BCHMC_ENS_M2)
    return h->fail(BCHMC_ERR_ARG, "%s: unknown quantity %d", name, (int)what);
  ENTER(h);
  auto &s = h->ens.slot[slot];
  const uint64_t need = (what == BCHMC_ENS_VARIANCE || what == BCHMC_ENS_STD) ? 2 : 1;
  if (s.count < need)
    return h->fail(BCHMC_ERR_STATE, "%s: slot %d holds %llu samples, this needs %llu", name, (int)slot,
                   (unsigned long long)s.count, (unsigned long long)need);
  const size_t bytes = (size_t)h->g.N * sizeof(double);
  if (what == BCHMC_ENS_MEAN) return d2h(h, out, s.mean, bytes);
  if (what == BCHMC_ENS_M2) return d2h(h, out, s.m2, bytes);
  int blocks = 0;
  CHK(ens_blocks(h, &blocks));
  {
    ProfScope ps(h, BCHMC_K_OTHER);
    const double cm1 = (double)(s.count - 1);
    if (what == BCHMC_ENS_STD)
      k_ens_moment<true><<<blocks, kEnsBlock, 0, h->stream>>>(h->g.N, s.m2.get(), h->dstage.get(), cm1);
    else
      k_ens_moment<false><<<blocks, kEnsBlock, 0, h->stream>>>(h->g.N, s.m2.get(), h->dstage.get(), cm1);
    HIPCHK(hipGetLastError());
  }
  return d2h(h, out, h->dstage, bytes);
}

int bchmc_ensemble_merge(bchmc_handle *h, int32_t slot, uint64_t count_b, const double *mean_b, const double *m2_b) {
  if (!h) return BCHMC_ERR_ARG;
  const char *name = "ensemble_merge";
  CHK(ens_slot(h, name, slot));
  if (count_b == 0) return BCHMC_OK;  // nothing to fold in: the arrays are not looked at
  if (!mean_b || !m2_b) return h->fail(BCHMC_ERR_ARG, "%s: mean_b and m2_b must be given with count_b > 0", name);
  ENTER(h);
  auto &s = h->ens.slot[slot];
  if (count_b > UINT64_MAX - s.count) return h->fail(BCHMC_ERR_ARG, "%s: the two counts do not fit 64 bits", name);
  int blocks = 0;
  CHK(ens_blocks(h, &blocks));
  CHK(ens_take(h, s));
  const size_t N = (size_t)h->g.N, bytes = N * sizeof(double);
  if (s.count == 0) {  // into an empty slot: a copy, bit for bit
    int rc = h2d(h, s.mean, mean_b, bytes);
    if (!rc) rc = h2d(h, s.m2, m2_b, bytes);
    if (rc) {  // half a copy must not pass for an empty slot: the next add or merge takes zeroed arrays again
      (void)hipStreamSynchronize(h->stream);
      (void)s.mean.release();
      (void)s.m2.release();
      return rc;
    }
  } else {
    CHK(h2d(h, h->dstage, mean_b, bytes));
    CHK(h2d(h, h->dstage + N, m2_b, bytes));
    const double na = (double)s.count, nb = (double)count_b, nab = (double)(s.count + count_b);
    const double w = nb / nab, c = na * nb / nab;
    ProfScope ps(h, BCHMC_K_OTHER);
    k_ens_merge<<<blocks, kEnsBlock, 0, h->stream>>>(h->g.N, h->dstage.get(), h->dstage.get() + N, s.mean.get(), s.m2.get(), w, c);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  s.count += count_b;
  return BCHMC_OK;
}

int bchmc_ensemble_reset(bchmc_handle *h, int32_t slot) {
  if (!h) return BCHMC_ERR_ARG;
  CHK(ens_slot(h, "ensemble_reset", slot));
  ENTER(h);
  auto &s = h->ens.slot[slot];
  s.count = 0;
  if (s.mean) HIPCHK(hipMemsetAsync(s.mean, 0, (size_t)h->g.N * sizeof(double), h->stream));
  if (s.m2) HIPCHK(hipMemsetAsync(s.m2, 0, (size_t)h->g.N * sizeof(double), h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BCHMC_OK;
}

int bchmc_ensemble_release(bchmc_handle *h) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  for (auto &s : h->ens.slot) {
    (void)s.mean.release();
    (void)s.m2.release();
    s.count = 0;
  }
  return BCHMC_OK;
}

// ---- bchmc_tweb_* (tweb.hpp) -------------------------------------------------------------------------------------------
// Workgroups of k_tweb_eigen: a function of the grid alone, so that the order of the per-type sums, and with it every
// bit of the masses, is the same on every handle of a kind.
static int tweb_blocks(const bchmc_handle *h) { return nblk_stride(h->g.N); }

static void tweb_drop(bchmc_handle *h) {
  auto &w = h->tw;
  for (auto &b : w.t) (void)b.release();
  (void)w.xk.release();
  (void)w.type.release();
  (void)w.lam.release();
  (void)w.part.release();
  (void)w.cnt.release();
  w.have_t = false;
  w.samples = 0;
  w.have_par = false;
}

// The buffers a call needs, zeroed on the handle's stream, each on its first use.  If one cannot be had the call gives
// back those it took itself and the handle is as it was before it (the ens_take pattern).
static int tweb_take(bchmc_handle *h, bool tensor, bool xk, bool lam, bool cnt) {
  auto &w = h->tw;
  const size_t N = (size_t)h->g.N;
  bool took_t[6] = {false, false, false, false, false, false}, took_type = false, took_part = false, took_xk = false,
       took_lam = false, took_cnt = false;
  int rc = BCHMC_OK;
  if (tensor) {
    for (int c = 0; c < 6 && !rc; c++)
      if (!w.t[c]) rc = dev_alloc(h, w.t[c], N * h->esz), took_t[c] = !rc;
    if (!rc && !w.type) rc = dev_alloc(h, w.type, N), took_type = !rc;
    if (!rc && !w.part) rc = dev_alloc(h, w.part, ((size_t)tweb_blocks(h) + 1) * kTwebWords), took_part = !rc;
  }
  if (!rc && xk && !w.xk) rc = dev_alloc(h, w.xk, 2 * (size_t)h->g.Nhp * h->esz), took_xk = !rc;
  if (!rc && lam && !w.lam) rc = dev_alloc(h, w.lam, 3 * N), took_lam = !rc;
  if (!rc && cnt && !w.cnt) rc = dev_alloc(h, w.cnt, 4 * N), took_cnt = !rc;
  if (rc) {
    (void)hipStreamSynchronize(h->stream);  // the zero fills of what goes back
    for (int c = 0; c < 6; c++)
      if (took_t[c]) (void)w.t[c].release();
    if (took_type) (void)w.type.release();
    if (took_part) (void)w.part.release();
    if (took_xk) (void)w.xk.release();
    if (took_lam) (void)w.lam.release();
    if (took_cnt) (void)w.cnt.release();
    if (took_t[0] || took_t[1] || took_t[2] || took_t[3] || took_t[4] || took_t[5]) w.have_t = false;
  }
  return rc;
}

int bchmc_tweb_classify(bchmc_handle *h, bchmc_corr_source src, const double *signal, const bchmc_tweb_opts *opts,
                        double *lambda, uint8_t *type, bchmc_tweb_stats *stats) {
  if (!h) return BCHMC_ERR_ARG;
  const char *name = "tweb_classify";
  if (!opts) return h->fail(BCHMC_ERR_ARG, "%s: opts is NULL", name);
  const double Rs = opts->smoothing_scale, lth = opts->lambda_th;
  if (!(Rs >= 0.) || !(Rs <= DBL_MAX))
    return h->fail(BCHMC_ERR_ARG, "%s: smoothing_scale = %g is negative or not finite", name, Rs);
  if (!(std::fabs(lth) <= DBL_MAX)) return h->fail(BCHMC_ERR_ARG, "%s: lambda_th = %g is not finite", name, lth);
  if (opts->accumulate != 0 && opts->accumulate != 1)
    return h->fail(BCHMC_ERR_ARG, "%s: accumulate = %d is neither 0 nor 1", name, (int)opts->accumulate);
  CHK(source_args(h, name, src, signal));
  ENTER(h);
  CHK(source_state(h, src));
  auto &w = h->tw;
  if (opts->accumulate) {
    if (w.have_par && (Rs != w.R || lth != w.lambda_th))
      return h->fail(BCHMC_ERR_STATE,
                     "%s: the accumulator holds samples of smoothing_scale = %g, lambda_th = %g; this call has %g, %g "
                     "(bchmc_tweb_reset starts another posterior)", name, w.R, w.lambda_th, Rs, lth);
    if (w.samples + 1 >= (1ull << 32)) return h->fail(BCHMC_ERR_STATE, "%s: the accumulator's sample count is full", name);
  }
  CHK(tweb_take(h, true, src != BCHMC_CORR_CHAIN_STATE, lambda != nullptr, opts->accumulate != 0));
  const size_t N = (size_t)h->g.N;
  const int nblk = tweb_blocks(h);
  if (signal) CHK(h2d(h, h->dstage, signal, N * sizeof(double)));
  w.have_t = false;
  CHK(DISPATCH(h, tweb_tensor(h, (int)src, 0.5 * Rs * Rs)));
  CHK(DISPATCH(h, tweb_eigen(h, (int)src, lth, lambda ? w.lam.get() : nullptr, nblk)));
  w.have_t = true;
  unsigned long long res[kTwebWords];
  CHK(d2h(h, res, w.part + (size_t)nblk * kTwebWords, sizeof res));
  if (lambda) CHK(d2h(h, lambda, w.lam, 3 * N * sizeof(double)));
  if (type) CHK(d2h(h, type, w.type, N));
  if (stats) {
    for (int t = 0; t < 4; t++) {
      stats->n_type[t] = res[t];
      std::memcpy(&stats->mass_type[t], &res[5 + t], sizeof(double));
    }
    stats->n_nonfinite = res[4];
  }
  if (!opts->accumulate) return BCHMC_OK;
  if (res[4])
    return h->fail(BCHMC_ERR_ARG, "%s: %llu cells of the sample have a tensor that is not finite; nothing was accumulated",
                   name, res[4]);
  {
    ProfScope ps(h, BCHMC_K_OTHER);
    k_tweb_accumulate<<<nblk_stride((long long)((N >> 2) + 4)), kTwebBlock, 0, h->stream>>>(h->g.N, w.type, w.cnt);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!w.have_par) w.R = Rs, w.lambda_th = lth, w.have_par = true;
  w.samples++;
  return BCHMC_OK;
}

int bchmc_tweb_tensor(bchmc_handle *h, int32_t component, double *out) {
  if (!h || !out) return BCHMC_ERR_ARG;
  const char *name = "tweb_tensor";
  if (component < 0 || component > 5) return h->fail(BCHMC_ERR_ARG, "%s: component = %d outside 0..5", name, (int)component);
  ENTER(h);
  if (!h->tw.have_t) return h->fail(BCHMC_ERR_STATE, "%s: no tensor in the handle: call bchmc_tweb_classify first", name);
  return DISPATCH(h, tweb_component_fetch(h, (int)component, out));
}

int bchmc_tweb_samples(bchmc_handle *h, uint64_t *n) {
  if (!h || !n) return BCHMC_ERR_ARG;
  *n = h->tw.samples;
  return BCHMC_OK;
}

int bchmc_tweb_fetch(bchmc_handle *h, int32_t type, int32_t as_probability, void *out) {
  if (!h || !out) return BCHMC_ERR_ARG;
  const char *name = "tweb_fetch";
  if (type < 0 || type > 3) return h->fail(BCHMC_ERR_ARG, "%s: type = %d outside 0..3", name, (int)type);
  ENTER(h);
  auto &w = h->tw;
  const size_t N = (size_t)h->g.N;
  if (as_probability && w.samples == 0)
    return h->fail(BCHMC_ERR_STATE, "%s: as_probability with samples = 0: the accumulator is empty", name);
  if (!w.cnt) {  // counters never taken: every count is 0
    std::memset(out, 0, N * sizeof(uint32_t));
    return BCHMC_OK;
  }
  if (!as_probability) return d2h(h, out, w.cnt + (size_t)type * N, N * sizeof(uint32_t));
  {
    ProfScope ps(h, BCHMC_K_OTHER);
    k_tweb_probability<<<nblk_stride(h->g.N), kTwebBlock, 0, h->stream>>>(h->g.N, w.cnt + (size_t)type * N, (double)w.samples,
                                                                         h->dstage.get());
    HIPCHK(hipGetLastError());
  }
  return d2h(h, out, h->dstage, N * sizeof(double));
}

int bchmc_tweb_merge(bchmc_handle *h, uint64_t n_b, const uint32_t *counts_b) {
  if (!h) return BCHMC_ERR_ARG;
  const char *name = "tweb_merge";
  if (n_b == 0) return BCHMC_OK;  // nothing to fold in: the array is not looked at
  if (!counts_b) return h->fail(BCHMC_ERR_ARG, "%s: counts_b must be given with n_b > 0", name);
  ENTER(h);
  auto &w = h->tw;
  if (n_b >= (1ull << 32) || n_b + w.samples >= (1ull << 32))
    return h->fail(BCHMC_ERR_ARG, "%s: n_b = %llu and the %llu samples held do not fit the 32-bit counters", name,
                   (unsigned long long)n_b, (unsigned long long)w.samples);
  CHK(tweb_take(h, false, false, false, true));
  const size_t N = (size_t)h->g.N;
  CHK(h2d(h, h->dstage, counts_b, 4 * N * sizeof(uint32_t)));  // 16 N bytes: exactly the staging's 2 N doubles
  {
    ProfScope ps(h, BCHMC_K_OTHER);
    k_tweb_merge<<<nblk_stride(4 * h->g.N), kTwebBlock, 0, h->stream>>>(4 * h->g.N, reinterpret_cast<const unsigned int *>(h->dstage.get()),
                                                                       w.cnt);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  w.samples += n_b;
  return BCHMC_OK;
}

int bchmc_tweb_reset(bchmc_handle *h) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  auto &w = h->tw;
  w.samples = 0;
  w.have_par = false;
  if (w.cnt) HIPCHK(hipMemsetAsync(w.cnt, 0, 4 * (size_t)h->g.N * sizeof(uint32_t), h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BCHMC_OK;
}

int bchmc_tweb_release(bchmc_handle *h) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  tweb_drop(h);
  return BCHMC_OK;
}

// ---- bchmc_bispectrum (bispec.hpp) ---------------------------------------------------------------------------------------
// doubles of the partial buffer: the rows of the contraction or of the shell statistics, whichever are more, then the
// results (3 n_shell sums of the statistics, T sums of the contraction)
static size_t bispec_part_words(const bchmc_handle *h, int n_shell) {
  const size_t T = (size_t)bispec_triplets(n_shell);
  return std::max((size_t)bispec_grid(h->g.N) * T, (size_t)kBispecStatGrid * 3 * n_shell) + 3 * (size_t)n_shell + T;
}

static void bispec_drop(bchmc_handle *h) {
  auto &w = h->bs;
  for (auto &b : w.d) (void)b.release();
  (void)w.xk.release();
  (void)w.part.release();
  (void)w.tab.release();
  w.have_tab = false;
  w.n_shell = 0;
}

// The buffers a call with n_shell shells needs, each on its first use (the tweb_take pattern): if one cannot be had
// the call gives back those it took itself.  A handle that held another n_shell has dropped its table before.
static int bispec_take(bchmc_handle *h, int n_shell, bool xk) {
  auto &w = h->bs;
  const size_t N = (size_t)h->g.N;
  bool took_d[kBispecMaxShell] = {}, took_part = false, took_tab = false, took_xk = false;
  int rc = BCHMC_OK;
  for (int s = 0; s < n_shell && !rc; s++)
    if (!w.d[s]) rc = dev_alloc(h, w.d[s], N * h->esz), took_d[s] = !rc;
  if (!rc && !w.part) rc = dev_alloc(h, w.part, bispec_part_words(h, n_shell)), took_part = !rc;
  if (!rc && !w.tab) rc = dev_alloc(h, w.tab, (size_t)bispec_triplets(n_shell)), took_tab = !rc;
  if (!rc && xk && !w.xk) rc = dev_alloc(h, w.xk, 2 * (size_t)h->g.Nhp * h->esz), took_xk = !rc;
  if (rc) {
    (void)hipStreamSynchronize(h->stream);  // the zero fills of what goes back
    for (int s = 0; s < n_shell; s++)
      if (took_d[s]) (void)w.d[s].release();
    if (took_part) (void)w.part.release();
    if (took_tab) (void)w.tab.release(), w.have_tab = false;
    if (took_xk) (void)w.xk.release();
  }
  return rc;
}

int bchmc_bispectrum(bchmc_handle *h, bchmc_corr_source src, const double *signal, const bchmc_bispec_opts *opts, double *b,
                     double *ntri, double *q, double *kmean, uint64_t *nmode, double *power) {
#pragma clang fp contract(off)
  if (!h) return BCHMC_ERR_ARG;
  const char *name = "bispectrum";
  if (!opts) return h->fail(BCHMC_ERR_ARG, "%s: opts is NULL", name);
  const double k_min = opts->k_min, dk = opts->dk;
  const int n = opts->n_shell;
  if (!(k_min >= 0.) || !(k_min <= DBL_MAX)) return h->fail(BCHMC_ERR_ARG, "%s: k_min = %g is negative or not finite", name, k_min);
  if (!(dk > 0.) || !(dk <= DBL_MAX)) return h->fail(BCHMC_ERR_ARG, "%s: dk = %g is not > 0 or not finite", name, dk);
  if (n < 1 || n > kBispecMaxShell) return h->fail(BCHMC_ERR_ARG, "%s: n_shell = %d outside 1..%d", name, n, kBispecMaxShell);
  if (!b) return h->fail(BCHMC_ERR_ARG, "%s: b is NULL", name);
  CHK(source_args(h, name, src, signal));
  ENTER(h);
  CHK(source_state(h, src));
  auto &w = h->bs;
  const Geo &g = h->g;
  const size_t N = (size_t)g.N;
  const int T = bispec_triplets(n);
  // B4: with every shell below 2/3 k_Nyquist a triplet with lo(s3) >= hi(s1) + hi(s2) has no triangle and is not computed
  const double k_nyq = g.kfac * (0.5 * (double)g.n);
  const bool rule = k_min + (double)n * dk <= (2. / 3.) * k_nyq;
  static_assert(kBispecMaxShell <= 255, "shell indices travel as bytes");
  unsigned char s3_end[kBispecMaxShell][kBispecMaxShell] = {};
  for (int s1 = 0; s1 < n; s1++)
    for (int s2 = s1; s2 < n; s2++) {
      int end = n;
      if (rule) {
        const double reach = (k_min + (double)(s1 + 1) * dk) + (k_min + (double)(s2 + 1) * dk);
        for (end = s2; end < n && !(k_min + (double)end * dk >= reach); end++) {}
      }
      s3_end[s1][s2] = (unsigned char)end;
    }
  const BispecPlan plan = bispec_plan(n, s3_end);
  if (w.n_shell != n) {  // other arrays and another partial buffer: what does not fit the new shells goes first
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int s = n; s < kBispecMaxShell; s++) (void)w.d[s].release();
    (void)w.part.release();
    (void)w.tab.release();
    w.have_tab = false;
    w.n_shell = 0;
  }
  CHK(bispec_take(h, n, src != BCHMC_CORR_CHAIN_STATE));
  w.n_shell = n;
  if (!w.have_tab || w.k_min != k_min || w.dk != dk) {
    w.have_tab = false;
    CHK(DISPATCH(h, bispec_shells(h, nullptr, k_min, dk, n)));
    CHK(DISPATCH(h, bispec_triple(h, n, plan, w.tab)));
    w.k_min = k_min, w.dk = dk, w.have_tab = true;
  }
  if (signal) CHK(h2d(h, h->dstage, signal, N * sizeof(double)));
  const void *xk = nullptr;
  CHK(DISPATCH(h, bispec_source(h, (int)src, &xk)));
  double *res = w.part + (bispec_part_words(h, n) - 3 * (size_t)n - (size_t)T);
  CHK(DISPATCH(h, bispec_stats(h, xk, k_min, dk, n, res)));
  CHK(DISPATCH(h, bispec_shells(h, xk, k_min, dk, n)));
  CHK(DISPATCH(h, bispec_triple(h, n, plan, res + 3 * n)));
  std::vector<double> hr(3 * (size_t)n + T), ht(T);
  CHK(d2h(h, hr.data(), res, hr.size() * sizeof(double)));
  CHK(d2h(h, ht.data(), w.tab, ht.size() * sizeof(double)));
  const double Nd = (double)N, L3 = g.L * g.L * g.L, NORM = L3 / Nd / Nd, BNORM = L3 * L3 / (Nd * Nd * Nd);
  std::vector<double> P(n);
  for (int s = 0; s < n; s++) {
    const double cnt = hr[s];
    P[s] = cnt > 0. ? hr[2 * n + s] / cnt * NORM : 0.;
    if (nmode) nmode[s] = (uint64_t)cnt;
    if (kmean) kmean[s] = cnt > 0. ? hr[n + s] / cnt : 0.;
    if (power) power[s] = P[s];
  }
  int t = 0;
  for (int s1 = 0; s1 < n; s1++)
    for (int s2 = s1; s2 < n; s2++)
      for (int s3 = s2; s3 < n; s3++, t++) {
        const bool computed = s3 < s3_end[s1][s2];
        const double nt = computed ? ht[t] / Nd : 0.;
        const bool filled = computed && !(nt < 0.5);
        const double bt = filled ? BNORM * (hr[3 * n + t] / (Nd * nt)) : 0.;
        b[t] = bt;
        if (ntri) ntri[t] = nt;
        if (q) {
          const double den = P[s1] * P[s2] + P[s2] * P[s3] + P[s3] * P[s1];
          q[t] = (!filled || den == 0.) ? 0. : bt / den;
        }
      }
  return BCHMC_OK;
}

int bchmc_bispec_release(bchmc_handle *h) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  bispec_drop(h);
  return BCHMC_OK;
}

// ---- bchmc_measure_*multipoles (multipoles.hpp) --------------------------------------------------------------------------
// What the three entry points check after their arrays and before anything is queued
static int mp_checks(bchmc_handle *h, const char *name, uint64_t n_bin) {
  if (n_bin == 0 || n_bin > 2048) return h->fail(BCHMC_ERR_ARG, "%s: n_bin = %llu outside 1..2048", name, (unsigned long long)n_bin);
  return BCHMC_OK;
}
// the class tables hold (n / 2 + 1)(n / 2 + 2) / 2 columns of n / 2 + 1 doubles: 0.54 GB per sum at 1024
static int mp_grid(bchmc_handle *h, const char *name) {
  if (h->g.n > 1024) return h->fail(BCHMC_ERR_UNSUPPORTED, "%s: n = %d > 1024", name, h->g.n);
  return BCHMC_OK;
}
// the geometry of a form to the caller's arrays, from the GEOM sums `hg` if this call made them
static void mp_geometry_out(bchmc_handle::Mp::Geom &c, const std::vector<double> &hg, uint64_t n_bin, double *tmode,
                            uint64_t *nmode, double *leg) {
  if (c.n_bin != n_bin) mp_geometry(c, hg, n_bin);
  std::memcpy(tmode, c.tmode.data(), n_bin * sizeof(double));
  std::memcpy(leg, c.leg.data(), 2 * n_bin * sizeof(double));
  if (nmode) std::memcpy(nmode, c.nmode.data(), n_bin * sizeof(uint64_t));
}

int bchmc_measure_multipoles(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *kmode,
                             uint64_t *nmode, double *leg, double *p) {
  if (!h || !kmode || !leg || !p) return BCHMC_ERR_ARG;
  const char *name = "measure_multipoles";
  CHK(mp_checks(h, name, n_bin));
  CHK(source_args(h, name, src, signal));
  ENTER(h);
  CHK(source_state(h, src));
  CHK(mp_grid(h, name));
  CHK(mp_take(h, 1, n_bin, false));
  if (signal) CHK(h2d(h, h->dstage, signal, h->g.N * sizeof(double)));
  const void *xk = nullptr;
  CHK(DISPATCH(h, spectrum_source(h, (int)src, &xk)));
  auto &c = h->mp.fourier;
  const size_t cells = ((size_t)n_bin + 1) * mp_segments((int)n_bin);
  std::vector<double> hg(c.n_bin == n_bin ? 0 : cells * kMpGeom), hs(cells * 3);
  CHK(DISPATCH(h, mp_auto(h, xk, n_bin, hg.empty() ? nullptr : hg.data(), hs.data())));
  mp_geometry_out(c, hg, n_bin, kmode, nmode, leg);
  const double N = (double)h->g.N, NORM = h->g.L * h->g.L * h->g.L / N / N;  // FOURIER_DEF_2, as spectrum_bins
  mp_normalise(c, mp_bins(hs, n_bin, 3), n_bin, 1, 0, NORM, p);
  return BCHMC_OK;
}

int bchmc_measure_cross_multipoles(bchmc_handle *h, bchmc_corr_source src_a, const double *signal_a, bchmc_corr_source src_b,
                                   const double *signal_b, uint64_t n_bin, double *kmode, uint64_t *nmode, double *leg,
                                   double *p_aa, double *p_bb, double *p_ab) {
  if (!h || !kmode || !leg || !p_aa || !p_bb || !p_ab) return BCHMC_ERR_ARG;
  const char *name = "measure_cross_multipoles";
  CHK(mp_checks(h, name, n_bin));
  CHK(source_args(h, name, src_a, signal_a));
  CHK(source_args(h, name, src_b, signal_b));
  ENTER(h);
  CHK(source_state(h, src_a));
  CHK(source_state(h, src_b));
  CHK(mp_grid(h, name));
  CHK(mp_take(h, 3, n_bin, src_a != BCHMC_CORR_CHAIN_STATE));
  const void *ak = nullptr, *bk = nullptr;
  CHK(DISPATCH(h, cross_source(h, (int)src_a, signal_a, h->mp.xk, &ak)));
  CHK(DISPATCH(h, cross_source(h, (int)src_b, signal_b, h->tC, &bk)));
  auto &c = h->mp.fourier;
  const size_t cells = ((size_t)n_bin + 1) * mp_segments((int)n_bin);
  std::vector<double> hg(c.n_bin == n_bin ? 0 : cells * kMpGeom), hs(cells * 9);
  CHK(DISPATCH(h, mp_cross(h, ak, bk, n_bin, hg.empty() ? nullptr : hg.data(), hs.data())));
  mp_geometry_out(c, hg, n_bin, kmode, nmode, leg);
  const double N = (double)h->g.N, NORM = h->g.L * h->g.L * h->g.L / N / N;
  const std::vector<double> sums = mp_bins(hs, n_bin, 9);
  mp_normalise(c, sums, n_bin, 3, 0, NORM, p_aa);
  mp_normalise(c, sums, n_bin, 3, 1, NORM, p_bb);
  mp_normalise(c, sums, n_bin, 3, 2, NORM, p_ab);
  return BCHMC_OK;
}

int bchmc_measure_corr_multipoles(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *rmode,
                                  uint64_t *nmode, double *leg, double *xi) {
  if (!h || !rmode || !leg || !xi) return BCHMC_ERR_ARG;
  const char *name = "measure_corr_multipoles";
  CHK(mp_checks(h, name, n_bin));
  CHK(source_args(h, name, src, signal));
  ENTER(h);
  CHK(source_state(h, src));
  CHK(mp_grid(h, name));
  CHK(mp_take(h, 1, n_bin, false));
  if (signal) CHK(h2d(h, h->dstage, signal, h->g.N * sizeof(double)));
  CHK(DISPATCH(h, corr_field(h, (int)src)));
  auto &c = h->mp.real;
  const size_t cells = ((size_t)n_bin + 1) * mp_segments((int)n_bin);
  std::vector<double> hg(c.n_bin == n_bin ? 0 : cells * kMpGeom), hs(cells * 3);
  CHK(DISPATCH(h, mp_corr(h, n_bin, hg.empty() ? nullptr : hg.data(), hs.data())));
  mp_geometry_out(c, hg, n_bin, rmode, nmode, leg);
  mp_normalise(c, mp_bins(hs, n_bin, 3), n_bin, 1, 0, 1. / (double)h->g.N, xi);
  return BCHMC_OK;
}

int bchmc_multipoles_release(bchmc_handle *h) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  mp_drop(h);
  return BCHMC_OK;
}

// max|w| and the first non-finite weight (*bad, -1: none) in one pass over the column, on the threads the staging copies
// use: it costs a read of 8 B per particle beside the 32 B the transfer reads
static double weights_pass(const double *w, uint64_t n, long long *bad) {
  const int nt = n < (1u << 20) ? 1 : (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency() / 2));
  std::vector<double> mx(nt, 0.);
  std::vector<long long> first(nt, -1);
  auto run = [&](int t) {
    const uint64_t b = n * t / nt, e = n * (t + 1) / nt;
    double m = 0.;
    for (uint64_t p = b; p < e; p++) {
      const double a = std::fabs(w[p]);
      if (!(a <= DBL_MAX)) {
        first[t] = (long long)p;
        break;
      }
      m = a > m ? a : m;
    }
    mx[t] = m;
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(run, t);
  run(0);
  for (auto &t : th) t.join();
  double m = 0.;
  *bad = -1;
  for (int t = nt - 1; t >= 0; t--) {
    m = std::max(m, mx[t]);
    if (first[t] >= 0) *bad = first[t];
  }
  return m;
}

int bchmc_density_particles(bchmc_handle *h, bchmc_part_source src, const double *x, const double *y, const double *z,
                            const double *w, uint64_t n_part, const bchmc_density_opts *opts, double *out,
                            bchmc_density_stats *stats) {
  if (!h || !opts) return BCHMC_ERR_ARG;
  const char *name = "density_particles";
  if (src != BCHMC_PART_HOST && src != BCHMC_PART_FORWARD) return h->fail(BCHMC_ERR_ARG, "%s: unknown source %d", name, (int)src);
  if (src == BCHMC_PART_HOST && n_part > 0 && (!x || !y || !z))
    return h->fail(BCHMC_ERR_ARG, "%s: x, y and z must be given for BCHMC_PART_HOST", name);
  if (src == BCHMC_PART_FORWARD && (x || y || z || w))
    return h->fail(BCHMC_ERR_ARG, "%s: x, y, z and w must be NULL for BCHMC_PART_FORWARD", name);
  if (opts->weightmass != 0 && opts->weightmass != 1)
    return h->fail(BCHMC_ERR_ARG, "%s: weightmass = %d is neither 0 nor 1", name, (int)opts->weightmass);
  const bool weighted = opts->weightmass == 1 && src == BCHMC_PART_HOST;
  if (weighted && !w && n_part > 0) return h->fail(BCHMC_ERR_ARG, "%s: weightmass = 1 without w", name);
  if (opts->mk < -1 || opts->mk > 3) return h->fail(BCHMC_ERR_ARG, "%s: mk = %d outside -1..3", name, (int)opts->mk);
  const int mk = opts->mk < 0 ? h->c.mk : opts->mk;
  if (!(opts->kernel_h >= 0.) || !std::isfinite(opts->kernel_h) || opts->kernel_h > h->g.L / 4)
    return h->fail(BCHMC_ERR_ARG, "%s: kernel_h = %g is negative, not finite or above L / 4", name, opts->kernel_h);
  const double hh = opts->kernel_h > 0. ? opts->kernel_h : h->c.particle_kernel_h;
  if (mk == 3 && !(hh > 0. && hh <= h->g.L / 4))
    return h->fail(BCHMC_ERR_ARG, "%s: the handle's particle_kernel_h = %g is not in (0, L / 4]", name, hh);
  if (opts->dest != -1 && opts->dest != BCHMC_F_NOBS)
    return h->fail(BCHMC_ERR_ARG, "%s: dest = %d is neither -1 nor BCHMC_F_NOBS", name, (int)opts->dest);
  if (!out && opts->dest == -1) return h->fail(BCHMC_ERR_ARG, "%s: no destination (out is NULL and dest is -1)", name);
  if (n_part > 2147483647ull) return h->fail(BCHMC_ERR_ARG, "%s: n_part = %llu > 2^31 - 1", name, (unsigned long long)n_part);
  if (mk == 3 && (h->c.min1 < 0. || h->c.min2 < 0. || h->c.min3 < 0.))
    return h->fail(BCHMC_ERR_UNSUPPORTED, "%s: getDensity_SPH casts x / d to an unsigned index, undefined below 0 "
                                          "(min = %g, %g, %g)", name, h->c.min1, h->c.min2, h->c.min3);
  if (src == BCHMC_PART_FORWARD && !h->have_eval)
    return h->fail(BCHMC_ERR_STATE, "%s: no forward evaluation to take the particles from", name);
  if (src == BCHMC_PART_FORWARD) n_part = (uint64_t)h->g.N;
  // the weights' own pass: a non-finite one refuses the call, the largest magnitude scales the fixed point
  double max_w = 1.;
  if (weighted) {
    long long bad = -1;
    max_w = weights_pass(w, n_part, &bad);
    if (bad >= 0) return h->fail(BCHMC_ERR_ARG, "%s: w[%lld] is not finite", name, bad);
  }
  ENTER(h);
  const CatCall cc{(int)src, mk, weighted ? 1 : 0, (int)opts->dest, hh, max_w, x, y, z, w, n_part};
  CHK(h->f32 ? Pipe<float>::density_particles(h, cc, out, stats) : Pipe<double>::density_particles(h, cc, out, stats));
  if (opts->dest == BCHMC_F_NOBS) {  // exactly what bchmc_upload(BCHMC_F_NOBS) does to the handle
    h->have[BCHMC_F_NOBS] = true;
    h->cg_valid = h->prop_g_valid = false;
  }
  return BCHMC_OK;
}

int bchmc_catalogue_release(bchmc_handle *h) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  h->cat = bchmc_handle::Cat{};
  return BCHMC_OK;
}

// A handle field, asked before anything is queued: bchmc_fetch's own refusals (fetch_ready), and one of this entry
// point's on top of them, since an input's buffer is there before its first upload.
static int interp_field_ready(bchmc_handle *h, const char *name, int f, int field) {
  CHK(fetch_ready(h, field));
  if (field <= BCHMC_F_WINDOW && !h->have[field])
    return h->fail(BCHMC_ERR_STATE, "%s: field %d: input array (bchmc_field %d) was never uploaded", name, f, field);
  return BCHMC_OK;
}

int bchmc_interp_particles(bchmc_handle *h, bchmc_part_source psrc, const double *x, const double *y, const double *z,
                           uint64_t n_part, const bchmc_interp_field *fields, int32_t n_fields,
                           const bchmc_interp_opts *opts, double *out, bchmc_interp_stats *stats) {
  if (!h) return BCHMC_ERR_ARG;
  const char *name = "interp_particles";
  if (!opts) return h->fail(BCHMC_ERR_ARG, "%s: opts is NULL", name);
  if (opts->kernel != 1 && opts->kernel != 2)
    return h->fail(BCHMC_ERR_ARG, "%s: kernel = %d is neither 1 (CIC) nor 2 (TSC)", name, (int)opts->kernel);
  if (opts->path < -1 || opts->path > 1) return h->fail(BCHMC_ERR_ARG, "%s: path = %d outside -1..1", name, (int)opts->path);
  if (n_fields < 1 || n_fields > BCHMC_INTERP_MAX_FIELDS)
    return h->fail(BCHMC_ERR_ARG, "%s: n_fields = %d outside 1..%d", name, (int)n_fields, (int)BCHMC_INTERP_MAX_FIELDS);
  if (!fields) return h->fail(BCHMC_ERR_ARG, "%s: fields is NULL", name);
  if (psrc != BCHMC_PART_HOST && psrc != BCHMC_PART_FORWARD) return h->fail(BCHMC_ERR_ARG, "%s: unknown source %d", name, (int)psrc);
  if (psrc == BCHMC_PART_HOST && n_part > 0 && (!x || !y || !z))
    return h->fail(BCHMC_ERR_ARG, "%s: x, y and z must be given for BCHMC_PART_HOST", name);
  if (psrc == BCHMC_PART_FORWARD && (x || y || z))
    return h->fail(BCHMC_ERR_ARG, "%s: x, y and z must be NULL for BCHMC_PART_FORWARD", name);
  if (psrc == BCHMC_PART_FORWARD && n_part != (uint64_t)h->g.N)
    return h->fail(BCHMC_ERR_ARG, "%s: n_part = %llu != N = %lld with BCHMC_PART_FORWARD", name, (unsigned long long)n_part, h->g.N);
  if (n_part > 2147483647ull) return h->fail(BCHMC_ERR_ARG, "%s: n_part = %llu > 2^31 - 1", name, (unsigned long long)n_part);
  if (!out && n_part > 0) return h->fail(BCHMC_ERR_ARG, "%s: out is NULL", name);
  for (int f = 0; f < n_fields; f++) {
    const bchmc_interp_field &fd = fields[f];
    if (fd.source < 0 || fd.source > BCHMC_INTERP_HANDLE_FIELD)
      return h->fail(BCHMC_ERR_ARG, "%s: field %d: unknown source %d", name, f, (int)fd.source);
    if ((fd.source == BCHMC_CORR_HOST) != (fd.host != nullptr))
      return h->fail(BCHMC_ERR_ARG, "%s: field %d: host must be given for BCHMC_CORR_HOST and NULL otherwise", name, f);
    if (fd.source == BCHMC_INTERP_HANDLE_FIELD && (fd.field < 0 || fd.field >= BCHMC_F_COUNT))
      return h->fail(BCHMC_ERR_ARG, "%s: field %d: unknown bchmc_field %d", name, f, (int)fd.field);
  }
  for (int f = 0; f < n_fields; f++) {
    const bchmc_interp_field &fd = fields[f];
    if (fd.source == BCHMC_CORR_CHAIN_STATE || fd.source == BCHMC_CORR_DELTAX) CHK(source_state(h, (bchmc_corr_source)fd.source));
    if (fd.source == BCHMC_INTERP_HANDLE_FIELD) CHK(interp_field_ready(h, name, f, fd.field));
  }
  if (psrc == BCHMC_PART_FORWARD && !h->have_eval)
    return h->fail(BCHMC_ERR_STATE, "%s: no forward evaluation to take the particles from", name);
  InterpFacts facts;
  facts.tiled = h->plan.tiled;
  facts.tx = h->plan.tp.tx, facts.ty = h->plan.tp.ty, facts.tz = h->plan.tp.tz, facts.ntiles = h->plan.tp.ntiles;
  facts.esz = (int)h->esz, facts.kernel = opts->kernel, facts.n_fields = n_fields, facts.n_part = n_part;
  facts.own_particles = psrc == BCHMC_PART_FORWARD;
  const int path = interp_path(facts, opts->path);
  if (path == kInterpNoTiles && !(facts.tiled && facts.ntiles > 0))
    return h->fail(BCHMC_ERR_UNSUPPORTED, "%s: path = 1 on a handle without a tile partition (Nx = %d)", name, h->g.n);
  if (path == kInterpNoTiles)  // no tile shape of tile_plan.hpp comes near it today: 8 x 8 x 16, four fp64 fields, 57.6 KB
    return h->fail(BCHMC_ERR_UNSUPPORTED, "%s: path = 1 with tile images of %zu bytes of LDS for %d fields, above %zu", name,
                   interp_image_bytes(facts), (int)n_fields, kInterpLdsLimit);
  if (n_part == 0) {
    if (stats) *stats = bchmc_interp_stats{0, 0, 0, path, 0};
    return BCHMC_OK;
  }
  ENTER(h);
  const ItpCall ic{(int)psrc, (int)opts->kernel, path == kInterpTile ? 1 : 0, (int)n_fields, fields, x, y, z, n_part};
  return h->f32 ? Pipe<float>::interp_particles(h, ic, out, stats) : Pipe<double>::interp_particles(h, ic, out, stats);
}

int bchmc_interp_release(bchmc_handle *h) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  h->itp = bchmc_handle::Itp{};
  return BCHMC_OK;
}

int bchmc_chain_forward(bchmc_handle *h, int use_rsd) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  if (!h->have_cq) return h->fail(BCHMC_ERR_STATE, "no chain state: call bchmc_chain_set_state first");
  clobber_proposal(h);
  CHK(DISPATCH(h, chain_forward(h, use_rsd < 0 ? h->c.rsd_model : (use_rsd ? 1 : 0))));
  return read_ctl(h, nullptr);  // synchronises; adapts the binning's record slots like bchmc_forward
}

int bchmc_hamiltonian_mass(bchmc_handle *h, const double *signal, const bchmc_mass_opts *opts, double *mass_f,
                           double *mass_r) {
  if (!h || !opts) return BCHMC_ERR_ARG;
  ENTER(h);
  const int t = h->c.mass_type;
  const bool force = (t == 2 || t == 3);
  const bool jasche = (t == 5 || t == 6 || (t == 60 && !(opts->iGibbs < opts->s_eps_total)));
  if (force && h->c.likelihood == 3)
    return h->fail(BCHMC_ERR_UNSUPPORTED, "mass_type %d needs likelihood_grad_log_like, which is an empty function for "
                                          "the GRF likelihood (gaussian_random_field.cpp:21-23)", t);
  if (force && (opts->n_bin == 0 || opts->n_bin > 2048))
    return h->fail(BCHMC_ERR_ARG, "n_bin = %llu outside 1..2048", (unsigned long long)opts->n_bin);
  if (jasche && h->g.n > 1024) return h->fail(BCHMC_ERR_UNSUPPORTED, "Jasche mass: n = %d > 1024", h->g.n);
  if (h->mass_fs) CHK(need_input(h, BCHMC_F_SIGNAL_PS, "signal_PS"));
  if (force) {
    CHK(need_input(h, BCHMC_F_NOBS, "nobs"));
    CHK(need_input(h, BCHMC_F_WINDOW, "window"));
    if (h->c.likelihood != 0) CHK(need_input(h, BCHMC_F_NOISE, "noise"));
  }
  if (jasche) {
    CHK(need_input(h, BCHMC_F_WINDOW, "window"));
    CHK(need_input(h, BCHMC_F_NOISE, "noise"));
  }
  const bool state = force || jasche;
  if (state && !signal && !h->have_cq) return h->fail(BCHMC_ERR_STATE, "no chain state: call bchmc_chain_set_state first");
  clobber_proposal(h);
  const size_t N = (size_t)h->g.N, bytes = N * sizeof(double);
  if (state && signal) CHK(h2d(h, h->dstage, signal, bytes));
  CHK(DISPATCH(h, mass_build(h, state && !signal, *opts, force, jasche)));
  if (h->mass_rs) h->cp_draw_rs = false;
  if (h->mass_fs) h->have[BCHMC_F_MASS_F] = true;
  if (h->mass_rs) h->have[BCHMC_F_MASS_R] = true;
  if (mass_f && h->mass_fs) CHK(d2h(h, mass_f, h->dstage, bytes));
  if (mass_r && h->mass_rs) CHK(d2h(h, mass_r, h->dstage + N, bytes));
  return read_ctl(h, nullptr);  // synchronises; adapts the binning's record slots to the forward model just run
}

// The front half of setup_random_test, shared by its two entry points.  mock_refusals: everything that can be refused
// is refused before anything is queued or the generator is touched; `poisson` swaps the two lines about data_model 0
// for the Poissonian mock's own.  mock_truth: the truth from 2 N Gaussians of the caller's stream, its forward model,
// the window and the count of its cells (mock_window's layout of the staging).
static int mock_refusals(bchmc_handle *h, const bchmc_mock_opts *o, const int32_t *mti, bool poisson, int *rsd) {
  if (*mti < 0 || *mti > 624) return h->fail(BCHMC_ERR_ARG, "mti = %d outside [0, 624]", (int)*mti);
  if (o->window_type != 1 && o->window_type != 10 && o->window_type != 23)
    return h->fail(BCHMC_ERR_ARG, "in barcoderunner: window_type = %d is not a valid choice!", (int)o->window_type);
  if (o->data_model != 0 && o->data_model != 1)
    return h->fail(BCHMC_ERR_ARG, "in barcoderunner: data_model = %d is not a valid choice!", (int)o->data_model);
  if (poisson) {
    if (o->data_model != 0 || h->c.likelihood != 0)
      return h->fail(BCHMC_ERR_ARG, "setup_random_test_poisson: the Poissonian mock is data_model 0 under likelihood 0 "
                                    "(data_model = %d, likelihood = %d)", (int)o->data_model, (int)h->c.likelihood);
  } else {
    if (o->data_model == 0 && h->c.likelihood == 0)
      return h->fail(BCHMC_ERR_UNSUPPORTED, "Poissonian mock data: gsl_ran_poisson consumes a data-dependent number of "
                                            "words per cell, which has no parallel form here");
    if (o->data_model == 0 && h->c.likelihood == 2)
      return h->fail(BCHMC_ERR_ARG, "in barcoderunner: linear data model was chosen (additive error), but incompatible "
                                    "likelihood!");
  }
  if (h->g.n & 1) return h->fail(BCHMC_ERR_UNSUPPORTED, "create_GARFIELD's placement needs an even Nx (%d)", h->g.n);
  *rsd = o->random_test_rsd ? 1 : 0;
  if (*rsd && !h->c.planepar) return h->fail(BCHMC_ERR_RSD_NOT_PLANEPAR, "non-plane-parallel RSD is not implemented");
  return need_input(h, BCHMC_F_SIGNAL_PS, "signal_PS");
}
static int mock_truth(bchmc_handle *h, const bchmc_mock_opts *o, int rsd, uint32_t mt[624], int32_t *mti, uint64_t *used,
                      long long *count) {
  CHK(mt_setup(h));
  CHK(DISPATCH(h, mock_alloc(h)));
  clobber_proposal(h);
  h->cg_valid = false;
  h->have[BCHMC_F_WINDOW] = h->have[BCHMC_F_NOBS] = h->have[BCHMC_F_NOISE] = false;
  const long long N = h->g.N;
  CHK(mt_draw(h, mt, mti, used, 2 * N, false, mock_place_truth));
  CHK(DISPATCH(h, mock_window(h, rsd, o->window_type)));
  unsigned long long res = 0;
  HIPCHK(hipMemcpyAsync(&res, h->mock.res, sizeof res, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *count = (long long)res;
  if (*count < 0 || *count > N) return h->fail(BCHMC_ERR_STATE, "window count %lld outside [0, N]", *count);
  return BCHMC_OK;
}

int bchmc_setup_random_test(bchmc_handle *h, const bchmc_mock_opts *o, uint32_t mt[624], int32_t *mti,
                            uint64_t *words_used, double *delta_lag, double *delta_eul) {
  if (!h || !o || !mt || !mti) return BCHMC_ERR_ARG;
  ENTER(h);
  int rsd = 0;
  CHK(mock_refusals(h, o, mti, false, &rsd));
  const long long N = h->g.N;
  uint64_t used1 = 0, used2 = 0;
  long long count = 0;
  CHK(mock_truth(h, o, rsd, mt, mti, &used1, &count));
  unsigned long long res[2] = {0, 0};
  // the noise is a second draw from the state the first one returned: its size depends on the window
  if (count > 0) CHK(mt_draw(h, mt, mti, &used2, count, true, nullptr));
  MockPar mp{o->window_type, o->data_model, h->c.likelihood, o->negative_obs, o->sigma_min, o->sigma_fac,
             h->c.rho_c,     h->c.delta_min};
  CHK(DISPATCH(h, mock_noise(h, mp)));
  HIPCHK(hipMemcpyAsync(res, h->mock.res, sizeof res, hipMemcpyDeviceToHost, h->stream));
  if (delta_lag) CHK(d2h(h, delta_lag, h->dstage, (size_t)N * sizeof(double)));
  if (delta_eul) CHK(d2h(h, delta_eul, h->dstage + N, (size_t)N * sizeof(double)));
  if (words_used) *words_used = used1 + used2;
  CHK(read_ctl(h, nullptr));  // synchronises; adapts the binning's record slots to the forward model just run
  if (res[1] != ~0ull)
    return h->fail(BCHMC_ERR_STATE, "in barcoderunner(): noise = 0 found! Index %llu", res[1]);
  h->have[BCHMC_F_WINDOW] = h->have[BCHMC_F_NOBS] = h->have[BCHMC_F_NOISE] = true;
  return BCHMC_OK;
}

// ---- bchmc_poisson_* (poisson.hpp) --------------------------------------------------------------------------------------
// The status words of a draw: taken once, kept with the sample's buffers
static int pois_stat_alloc(bchmc_handle *h) {
  auto &k = h->pois;
  if (k.stat && k.res) return BCHMC_OK;
  int rc = dev_alloc(h, k.stat, (size_t)kPoisWords);
  if (!rc) rc = dev_alloc(h, k.res, (size_t)2);
  if (rc) {
    (void)k.stat.release();
    (void)k.res.release();
  }
  return rc;
}
// The scan's buffers for `cells` cells; all or nothing, and an earlier sample is gone either way
static int pois_alloc(bchmc_handle *h, long long cells) {
  auto &k = h->pois;
  k.valid = false;
  CHK(pois_stat_alloc(h));
  if (k.cells == cells) return BCHMC_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  const long long nb = (cells + kPoisThreads - 1) / kPoisThreads, ng = (nb + kMtThreads - 1) / kMtThreads;
  auto build = [&]() -> int {
    CHK(dev_alloc(h, k.off, (size_t)cells + 1));
    CHK(dev_alloc(h, k.cnt, (size_t)nb));
    CHK(dev_alloc(h, k.boff, (size_t)nb));
    CHK(dev_alloc(h, k.gsum, (size_t)ng));
    return dev_alloc(h, k.goff, (size_t)ng);
  };
  k.cells = 0;
  if (const int rc = build()) {
    for (auto *b : {&k.off, &k.cnt, &k.boff, &k.gsum, &k.goff}) (void)b->release();
    return rc;
  }
  k.cells = cells;
  return BCHMC_OK;
}
// the status words (and the scan's total) of the draw just queued; synchronises
static int pois_read(bchmc_handle *h, bool resident, unsigned long long st[kPoisWords], unsigned long long *total) {
  HIPCHK(hipMemcpyAsync(st, h->pois.stat, kPoisWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  if (resident) HIPCHK(hipMemcpyAsync(total, h->pois.res, sizeof *total, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BCHMC_OK;
}
static int pois_opts_check(bchmc_handle *h, const char *name, const bchmc_poisson_opts *o) {
  if (o->stream >= 0x80000000u) return h->fail(BCHMC_ERR_ARG, "%s: stream = %u is not below 2^31", name, o->stream);
  if (o->rate_mode != 0 && o->rate_mode != 1) return h->fail(BCHMC_ERR_ARG, "%s: rate_mode = %d is neither 0 nor 1", name, (int)o->rate_mode);
  if (!std::isfinite(o->scale)) return h->fail(BCHMC_ERR_ARG, "%s: scale = %g is not finite", name, o->scale);
  if (o->use_window != 0 && o->use_window != 1) return h->fail(BCHMC_ERR_ARG, "%s: use_window = %d is neither 0 nor 1", name, (int)o->use_window);
  if (o->dest != -1 && o->dest != BCHMC_F_NOBS)
    return h->fail(BCHMC_ERR_ARG, "%s: dest = %d is neither -1 nor BCHMC_F_NOBS", name, (int)o->dest);
  return BCHMC_OK;
}

int bchmc_poisson_draw(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint32_t n_in,
                       const bchmc_poisson_opts *opts, double *counts, bchmc_poisson_stats *stats) {
  if (!h) return BCHMC_ERR_ARG;
  const char *name = "poisson_draw";
  if (!opts) return h->fail(BCHMC_ERR_ARG, "%s: opts is NULL", name);
  CHK(source_args(h, name, src, signal));
  CHK(pois_opts_check(h, name, opts));
  const uint32_t Nx = (uint32_t)h->g.n;
  if (src == BCHMC_CORR_HOST) {
    if (n_in < 1 || n_in > Nx) return h->fail(BCHMC_ERR_ARG, "%s: n_in = %u outside 1..Nx = %u", name, n_in, Nx);
  } else {
    if (n_in != 0 && n_in != Nx) return h->fail(BCHMC_ERR_ARG, "%s: n_in = %u with a device source (0 or Nx = %u)", name, n_in, Nx);
    n_in = Nx;
  }
  if ((opts->use_window || opts->dest == BCHMC_F_NOBS) && n_in != Nx)
    return h->fail(BCHMC_ERR_ARG, "%s: use_window = 1 and dest = BCHMC_F_NOBS need n_in == Nx (n_in = %u, Nx = %u)", name, n_in, Nx);
  ENTER(h);
  CHK(source_state(h, src));
  if (opts->use_window && !h->have[BCHMC_F_WINDOW])
    return h->fail(BCHMC_ERR_STATE, "%s: use_window = 1, but the window was never uploaded", name);
  const long long N = h->g.N, cells = (long long)n_in * n_in * n_in;
  auto &k = h->pois;
  CHK(pois_alloc(h, cells));
  if (signal) CHK(h2d(h, h->dstage, signal, (size_t)cells * sizeof(double)));
  double *cd = h->dstage + N;  // the counts as doubles: the upper half of the staging
  CHK(DISPATCH(h, pois_counts(h, (int)src, cells, signal ? h->dstage.get() : nullptr, *opts, cd, true)));
  unsigned long long st[kPoisWords], total = 0;
  CHK(pois_read(h, true, st, &total));
  if (st[kPoisBad] != ~0ull)
    return h->fail(BCHMC_ERR_ARG, "%s: lambda of cell %llu is NaN, +infinity or above 2^30; nothing was written", name, st[kPoisBad]);
  if (stats) {
    stats->n_part = total;
    stats->n_cells_drawn = st[kPoisDrawn];
    stats->max_count = st[kPoisMaxCount];
    stats->n_capped = st[kPoisCapped];
    std::memcpy(&stats->lambda_max, &st[kPoisLambdaBits], sizeof(double));
  }
  if (counts) CHK(d2h(h, counts, cd, (size_t)cells * sizeof(double)));
  if (opts->dest == BCHMC_F_NOBS) {  // exactly what bchmc_upload(BCHMC_F_NOBS) does to the handle
    CHK(DISPATCH(h, upload(h, BCHMC_F_NOBS, cd)));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have[BCHMC_F_NOBS] = true;
    h->cg_valid = h->prop_g_valid = false;
  }
  k.seed = opts->seed, k.stream = opts->stream, k.n_in = n_in, k.n_part = total, k.d_in = h->g.L / (double)n_in;
  k.valid = true;
  return BCHMC_OK;
}

int bchmc_poisson_positions(bchmc_handle *h, uint64_t first, uint64_t m, double *x, double *y, double *z) {
  if (!h) return BCHMC_ERR_ARG;
  const char *name = "poisson_positions";
  auto &k = h->pois;
  if (!k.valid) return h->fail(BCHMC_ERR_STATE, "%s: no sample: call bchmc_poisson_draw first", name);
  if (m > k.n_part || first > k.n_part - m)
    return h->fail(BCHMC_ERR_ARG, "%s: particles %llu .. %llu + %llu of a sample of %llu", name, (unsigned long long)first,
                   (unsigned long long)first, (unsigned long long)m, (unsigned long long)k.n_part);
  if (m == 0) return BCHMC_OK;
  if (!x || !y || !z) return h->fail(BCHMC_ERR_ARG, "%s: x, y and z must be given", name);
  ENTER(h);
  if (!k.cols) CHK(dev_alloc(h, k.cols, 3 * (size_t)kCatBatch));
  double *dx = k.cols, *dy = dx + kCatBatch, *dz = dy + kCatBatch;
  for (uint64_t p0 = 0; p0 < m; p0 += kCatBatch) {
    const int mb = (int)std::min<uint64_t>(kCatBatch, m - p0);
    {
      ProfScope ps(h, BCHMC_K_OTHER);
      Pipe<double>::pois_positions(h, first + p0, mb, dx, dy, dz);
      HIPCHK(hipGetLastError());
    }
    CHK(d2h(h, x + p0, dx, mb * sizeof(double)));
    CHK(d2h(h, y + p0, dy, mb * sizeof(double)));
    CHK(d2h(h, z + p0, dz, mb * sizeof(double)));
  }
  return BCHMC_OK;
}

int bchmc_poisson_density(bchmc_handle *h, const bchmc_density_opts *opts, double *out, bchmc_density_stats *stats) {
  if (!h || !opts) return BCHMC_ERR_ARG;
  const char *name = "poisson_density";
  // bchmc_density_particles' refusals, in its order, with the sample in the place of the columns
  if (opts->weightmass != 0 && opts->weightmass != 1)
    return h->fail(BCHMC_ERR_ARG, "%s: weightmass = %d is neither 0 nor 1", name, (int)opts->weightmass);
  if (opts->weightmass == 1) return h->fail(BCHMC_ERR_ARG, "%s: weightmass = 1: the sample's particles carry no weights", name);
  if (opts->mk < -1 || opts->mk > 3) return h->fail(BCHMC_ERR_ARG, "%s: mk = %d outside -1..3", name, (int)opts->mk);
  const int mk = opts->mk < 0 ? h->c.mk : opts->mk;
  if (!(opts->kernel_h >= 0.) || !std::isfinite(opts->kernel_h) || opts->kernel_h > h->g.L / 4)
    return h->fail(BCHMC_ERR_ARG, "%s: kernel_h = %g is negative, not finite or above L / 4", name, opts->kernel_h);
  const double hh = opts->kernel_h > 0. ? opts->kernel_h : h->c.particle_kernel_h;
  if (mk == 3 && !(hh > 0. && hh <= h->g.L / 4))
    return h->fail(BCHMC_ERR_ARG, "%s: the handle's particle_kernel_h = %g is not in (0, L / 4]", name, hh);
  if (opts->dest != -1 && opts->dest != BCHMC_F_NOBS)
    return h->fail(BCHMC_ERR_ARG, "%s: dest = %d is neither -1 nor BCHMC_F_NOBS", name, (int)opts->dest);
  if (!out && opts->dest == -1) return h->fail(BCHMC_ERR_ARG, "%s: no destination (out is NULL and dest is -1)", name);
  if (!h->pois.valid) return h->fail(BCHMC_ERR_STATE, "%s: no sample: call bchmc_poisson_draw first", name);
  const uint64_t n_part = h->pois.n_part;
  if (n_part > 2147483647ull) return h->fail(BCHMC_ERR_ARG, "%s: n_part = %llu > 2^31 - 1", name, (unsigned long long)n_part);
  if (mk == 3 && (h->c.min1 < 0. || h->c.min2 < 0. || h->c.min3 < 0.))
    return h->fail(BCHMC_ERR_UNSUPPORTED, "%s: getDensity_SPH casts x / d to an unsigned index, undefined below 0 "
                                          "(min = %g, %g, %g)", name, h->c.min1, h->c.min2, h->c.min3);
  ENTER(h);
  const CatCall cc{kCatSrcPoisson, mk, 0, (int)opts->dest, hh, 1., nullptr, nullptr, nullptr, nullptr, n_part};
  CHK(h->f32 ? Pipe<float>::density_particles(h, cc, out, stats) : Pipe<double>::density_particles(h, cc, out, stats));
  if (opts->dest == BCHMC_F_NOBS) {  // exactly what bchmc_upload(BCHMC_F_NOBS) does to the handle
    h->have[BCHMC_F_NOBS] = true;
    h->cg_valid = h->prop_g_valid = false;
  }
  return BCHMC_OK;
}

int bchmc_poisson_release(bchmc_handle *h) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  h->pois = bchmc_handle::Pois{};
  return BCHMC_OK;
}

int bchmc_setup_random_test_poisson(bchmc_handle *h, const bchmc_mock_opts *o, uint32_t mt[624], int32_t *mti,
                                    uint64_t *words_used, uint64_t seed, uint32_t stream, double *delta_lag,
                                    double *delta_eul) {
  if (!h || !o || !mt || !mti) return BCHMC_ERR_ARG;
  ENTER(h);
  int rsd = 0;
  CHK(mock_refusals(h, o, mti, true, &rsd));
  if (stream >= 0x80000000u) return h->fail(BCHMC_ERR_ARG, "setup_random_test_poisson: stream = %u is not below 2^31", stream);
  CHK(pois_stat_alloc(h));
  const long long N = h->g.N;
  uint64_t used = 0;
  long long count = 0;
  CHK(mock_truth(h, o, rsd, mt, mti, &used, &count));
  if (delta_lag) CHK(d2h(h, delta_lag, h->dstage, (size_t)N * sizeof(double)));
  if (delta_eul) CHK(d2h(h, delta_eul, h->dstage + N, (size_t)N * sizeof(double)));
  if (words_used) *words_used = used;
  // nobs = Poisson(rho_c (1 + delta_eul)) inside the window (barcoderunner.cc:125-131), from the staged doubles of
  // delta_eul into the lower half of the staging, then taken in like an uploaded array; noise = 0
  const bchmc_poisson_opts po{seed, stream, 0, h->c.rho_c, 1, BCHMC_F_NOBS};
  CHK(DISPATCH(h, pois_counts(h, BCHMC_CORR_HOST, N, h->dstage + N, po, h->dstage, false)));
  unsigned long long st[kPoisWords];
  CHK(pois_read(h, false, st, nullptr));
  CHK(read_ctl(h, nullptr));  // synchronises; adapts the binning's record slots to the forward model just run
  if (st[kPoisBad] != ~0ull)
    return h->fail(BCHMC_ERR_ARG, "setup_random_test_poisson: rho_c (1 + delta_eul) of cell %llu is NaN, +infinity or "
                                  "above 2^30", st[kPoisBad]);
  CHK(DISPATCH(h, upload(h, BCHMC_F_NOBS, h->dstage)));
  HIPCHK(hipMemsetAsync(h->in_arr[BCHMC_F_NOISE], 0, (size_t)N * h->esz, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->have[BCHMC_F_WINDOW] = h->have[BCHMC_F_NOBS] = h->have[BCHMC_F_NOISE] = true;
  return BCHMC_OK;
}

int bchmc_make_initial_guess(bchmc_handle *h, int32_t initial_guess, const double *file_field, int32_t smoothing_type,
                             double smoothing_scale, uint32_t mt[624], int32_t *mti, uint64_t *words_used) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  if (initial_guess < 0 || initial_guess > 4)
    return h->fail(BCHMC_ERR_ARG, "In barcoderunner: invalid choice of initial_guess (%d)!", (int)initial_guess);
  const bool draws = initial_guess >= 2;
  if (initial_guess == 1 && !file_field) return h->fail(BCHMC_ERR_ARG, "initial_guess 1 needs the field read from file");
  if (draws && (!mt || !mti)) return h->fail(BCHMC_ERR_ARG, "initial_guess %d needs the generator state", (int)initial_guess);
  if (draws && (*mti < 0 || *mti > 624)) return h->fail(BCHMC_ERR_ARG, "mti = %d outside [0, 624]", (int)*mti);
  if (initial_guess == 3 && (smoothing_type != 1 || !(smoothing_scale > 0.)))
    return h->fail(BCHMC_ERR_ARG, "initial_guess 3: only the Gaussian kernel (initial_guess_smoothing_type 1) with a "
                                  "positive scale is built (type %d, scale %g)", (int)smoothing_type, smoothing_scale);
  if (initial_guess == 2 || initial_guess == 3) {
    if (h->g.n & 1) return h->fail(BCHMC_ERR_UNSUPPORTED, "create_GARFIELD's placement needs an even Nx (%d)", h->g.n);
    CHK(need_input(h, BCHMC_F_SIGNAL_PS, "signal_PS"));
  }
  CHK(DISPATCH(h, chain_alloc(h)));
  const long long N = h->g.N;
  uint64_t used = 0;
  switch (initial_guess) {
    case 0:
      HIPCHK(hipMemsetAsync(h->cq, 0, 2 * (size_t)h->g.Nhp * h->esz, h->stream));
      break;
    case 1:
      CHK(h2d(h, h->dstage, file_field, (size_t)N * sizeof(double)));
      CHK(DISPATCH(h, r2c_state(h, h->dstage, h->ioq, h->cq)));
      break;
    case 2:
    case 3:
      CHK(mt_draw(h, mt, mti, &used, 2 * N, false, mock_place_guess));
      if (initial_guess == 3) CHK(DISPATCH(h, mock_smooth(h, smoothing_scale)));
      break;
    default:
      clobber_proposal(h);  // the R2C staging below is the trajectory's too
      CHK(mt_draw(h, mt, mti, &used, N, true, nullptr));
      CHK(DISPATCH(h, mock_guess_noise(h, 1.e-1)));
      break;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  h->have_cq = true;
  h->have_prop = false;
  h->cg_valid = h->prop_g_valid = false;
  if (words_used) *words_used = used;
  return BCHMC_OK;
}

int bchmc_philox_kat(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctr || !key || !out) return BCHMC_ERR_ARG;
  DevBuf<uint4> d;
  if (d.alloc(1) != hipSuccess) return BCHMC_ERR_NOMEM;
  k_philox_kat<<<1, 1>>>(make_uint4(ctr[0], ctr[1], ctr[2], ctr[3]), make_uint2(key[0], key[1]), d);
  uint4 r;
  const hipError_t e = hipMemcpy(&r, d, sizeof r, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return BCHMC_ERR_HIP;
  out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
  return BCHMC_OK;
}

int bchmc_tile_info(bchmc_handle *h, int32_t out[8]) {
  if (!h || !out) return BCHMC_ERR_ARG;
  out[0] = h->plan.tiled ? 1 : 0;
  out[1] = h->plan.slots.sort_direct ? 1 : 0;
  out[2] = h->plan.tp.cap;
  out[3] = (int32_t)std::min<long long>(h->plan.slots.cap_alloc, INT32_MAX);
  out[4] = h->plan.slots.slot_watch ? 1 : 0;
  out[5] = h->plan.tiled ? (h->plan.tp.tx | (h->plan.tp.ty << 8) | (h->plan.tp.tz << 16)) : 0;
  out[6] = h->plan.std81 ? 1 : 0;
  out[7] = (h->c2r2d_2 != nullptr) ? 1 : 0;
  return BCHMC_OK;
}

int bchmc_live_resources(uint64_t out[4]) {
  if (!out) return BCHMC_ERR_ARG;
  out[0] = live.dev_bufs, out[1] = live.dev_bytes, out[2] = live.pinned, out[3] = live.other;
  return BCHMC_OK;
}

int bchmc_profile(bchmc_handle *h, int enable) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  prof_collect(h);
  h->prof_on = enable != 0;
  return BCHMC_OK;
}

int bchmc_profile_read(bchmc_handle *h, double ms[BCHMC_K_COUNT], uint64_t launches[BCHMC_K_COUNT]) {
  if (!h) return BCHMC_ERR_ARG;
  ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  prof_collect(h);
  for (int i = 0; i < BCHMC_K_COUNT; i++) {
    if (ms) ms[i] = h->prof_ms[i];
    if (launches) launches[i] = h->prof_n[i];
    h->prof_ms[i] = 0.;
    h->prof_n[i] = 0;
  }
  return BCHMC_OK;
}

}  // extern "C"
