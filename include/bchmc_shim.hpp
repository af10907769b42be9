// bchmc_shim.hpp -- C++ host side above the C ABI: the reference's own function names and argument meaning for
// the leapfrog path, on a view of the reference's HAMIL_DATA / HAMIL_NUMERICAL.
//
// The reference (barlib) cannot be compiled in this image (FFTW3 / GSL headers absent), so this layer is built
// against `HamilView` -- a plain struct holding exactly the members of HAMIL_DATA / HAMIL_NUMERICAL that the path
// reads or writes (barlib/include/struct_hamil.h:51-222), under the reference's member names -- instead of against
// struct_hamil.h itself.  Inside barlib the same function bodies compile against the real structs;
// here they are compiled, linked against libbarcode_hip.so and tested (tests/test_gpu_shim.py).
//
//   reference                                              this header
//   void Hamiltonian_EoM(HAMIL_DATA*, real_prec* signali, real_prec* momentai, real_prec* signalf,
//                        real_prec* momentaf, gsl_rng*, DATA*)        HMC.cc:251-369   -> bchmc_shim::Hamiltonian_EoM
//   real_prec delta_Hamiltonian(HAMIL_DATA*, ...)                     HMC.cc:209-248   -> bchmc_shim::delta_Hamiltonian
//   void gradient_psi(HAMIL_DATA*, real_prec* signal, DATA*)          HMC.cc:146-206   -> bchmc_shim::gradient_psi
//   real_prec kinetic_term(...), real_prec psi(...)                   HMC.cc:64-143    -> bchmc_shim::kinetic_term, psi
//   void measure_spectrum(...)                      field_statistics.cpp:20-90         -> bchmc_shim::measure_spectrum
//   void measure_spec2D(N1, N2, N3, L1, L2, L3, signal, kmode, power, N_bin, planepar)
//                                                   tools/2D_powspec.cc:25-110         -> bchmc_shim::measure_spec2D
//   void getDensity_NGP / _CIC / _TSC / _SPH(N1, N2, N3, L1, L2, L3, d1, d2, d3, min1, min2, min3, xp, yp, zp, Par_mass,
//                        N_OBJ, delta[, weightmass[, kernel_h]])      massFunctions.cc:49-495 -> bchmc_shim::getDensity_NGP ..
//   void interpolate_CIC(N1, N2, N3, L1, L2, L3, d1, d2, d3, xp, yp, zp, field_grid, N_OBJ, interpolation)
//   void interpolate_TSC(N1, N2, N3, d1, d2, d3, xp, yp, zp, field_grid, N_OBJ, interpolation)
//   void interpolate_TSC_multi(N1, N2, N3, d1, d2, d3, xp, yp, zp, N_OBJ, field_grids, interpolations, N_fields)
//                                                   interpolate_grid.cpp:108-286       -> bchmc_shim::interpolate_CIC ..
//   vector<vector<real_prec>> discrete_poisson_sample(lambda, N1, N2, N3, L1, L2, L3, gsl_rng*)
//                                                   tools/poisson_upres.cc:23-65       -> bchmc_shim::discrete_poisson_sample
//   tools/poisson_upres.cc's main (:107-157)                                           -> bchmc_shim::poisson_upres
// Errors are std::runtime_error, like the reference's (single catch in main.cc:195-197).
#ifndef BCHMC_SHIM_HPP
#define BCHMC_SHIM_HPP
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "bchmc.h"

namespace bchmc_shim {

using real_prec = double;  // DOUBLE_PREC build (define_opt.h:46-50)
using ULONG = unsigned long;

// HAMIL_NUMERICAL members used by the path (struct_hamil.h:51-144), reference names.
struct HamilNumericalView {
  unsigned N1 = 0;  // = N2 = N3 (init_par.cc:116-118)
  ULONG N = 0;
  real_prec L1 = 0, min1 = 0, min2 = 0, min3 = 0, xobs = 0, yobs = 0, zobs = 0;
  bool planepar = true, periodic = true;
  int mk = 3, calc_h = 2, mass_type = 1;
  bool correct_delta = true, div_dH_by_N = false;
  real_prec particle_kernel_h = 0, kth = 4.;
  real_prec grad_psi_prior_factor = 1, grad_psi_likeli_factor = 1, deltaQ_factor = 1;
  // per-attempt state (struct_hamil.h:86-105)
  real_prec N_eps_fac = 0, eps_fac = 0, epsilon = 0;
  ULONG Neps = 0;
  real_prec dH = 0, dK = 0, dE = 0, dprior = 0, dlikeli = 0, psi_prior = 0, psi_likeli = 0;
  real_prec psi_prior_i = 0, psi_prior_f = 0, psi_likeli_i = 0, psi_likeli_f = 0, H_kin_i = 0, H_kin_f = 0;
  // sample bookkeeping read by the step-size schemes (struct_hamil.h:106-112): set by the caller per sample
  ULONG iGibbs = 1;      // sample number; scheme 3's fast initial phase runs while iGibbs == 1 (time_step.cpp:141)
  ULONG rejections = 0;  // rejected attempts of the current sample (HMC.cc:500-501)
  bool accepted = false; // outcome of the last attempt (HMC.cc:503-504)
  // read by Hamiltonian_mass (HMC_mass.cc:315-368) and HamiltonianMC's mass schedule (HMC.cc:387-400),
  // struct_hamil.h:81-119; massnum 0 means never (upstream divides by it; data/input.par:104-105 ships 0)
  ULONG N_bin = 200, massnum_init = 0, massnum_burn = 0, s_eps_total = 0;
  real_prec mass_factor = 1;
};

// HAMIL_DATA members used by the path (struct_hamil.h:146-222), reference names.
struct HamilView {
  HamilNumericalView *numerical = nullptr;
  int likelihood = 1;  // which plugin functions set_likelihood_functions bound (init_par.cc:534-559)
  int sfmodel = 1;
  bool rsd_model = false;
  real_prec rho_c = 1, delta_min = -0.999, biasP = 1, biasE = 1, ascale = 1, D1 = 1, D2 = 0, OM = 0, OL = 0;
  // inputs (caller-owned, N doubles each; mass_r / mass_f / noise may be null when the configuration never reads them)
  const real_prec *signal_PS = nullptr, *mass_f = nullptr, *mass_r = nullptr, *nobs = nullptr, *noise = nullptr,
                  *window = nullptr;
  // outputs the reference leaves in HAMIL_DATA (caller-owned, may be null)
  real_prec *gradpsi = nullptr, *deltaX = nullptr, *posx = nullptr, *posy = nullptr, *posz = nullptr;
  int device = 0;     // HIP device of this chain
  void *engine = nullptr;  // owned by the shim: created on first use, released by release()
  // step-size adaptation (DATA::numerical's tables and keys, struct_main.h:95-101,162-173): null = eps_fac stays
  // (eps_fac_update_type 0).  Caller-owned (eps_adapt_create / eps_adapt_destroy).
  struct EpsAdapt *eps = nullptr;
  // cross-chain pooling of the step-size statistics (bchmc.h): null = single chain, the reference's behaviour
  bchmc_comm *comm = nullptr;
  int comm_rank = 0;
  // generation of the input arrays as uploaded: bump with inputs_changed() where HamiltonianMC recomputes or
  // re-reads the mass (HMC.cc:400-423); engine_for() uploads only when it differs from what the engine holds
  unsigned long inputs_generation = 0, uploaded_generation = 0;
  int deterministic = 0;  // bchmc_config.deterministic: bitwise repeatable mass assignment (fixed point)
  // the same for mass_f / mass_r alone (mass_changed()): what HamiltonianMC rewrites every sample.  Unlike the other
  // inputs the mass does not enter gradient_psi or -log L, so the resident chain keeps its carried gradient.
  unsigned long mass_generation = 0, mass_uploaded_generation = 0;
  // Hamiltonian_EoM runs bchmc_leapfrog_dh, which yields the six energy terms of its four arrays with the trajectory;
  // delta_Hamiltonian may answer from them when it is the NEXT call on this view, about the same four arrays, with no
  // inputs_changed() / mass_changed() in between -- HamiltonianMC's order, HMC.cc:455-459.  The C ABI itself never
  // reuses anything.  reuse_eom_energies: 0 = delta_Hamiltonian always evaluates; 1 = reuse on array identity (the
  // caller's contract: the four arrays are not written between the two calls); 2 = identity and a 64-bit hash of the
  // full contents of all four arrays, taken in Hamiltonian_EoM and checked in delta_Hamiltonian (reads 4 N doubles
  // twice on the host: for callers that cannot make that promise).
  int reuse_eom_energies = 1;
  struct EomEnergies {
    bool valid = false;
    const real_prec *ptr[4] = {nullptr, nullptr, nullptr, nullptr};  // signali, momentai, signalf, momentaf
    std::uint64_t hash[4] = {0, 0, 0, 0};                            // mode 2 only
    double terms[6] = {0, 0, 0, 0, 0, 0};
    double dH = 0;
    unsigned long inputs_generation = 0, mass_generation = 0;
  } eom;
};

// Stand-in for gsl_rng_uniform(seed): called exactly where the reference calls it, in its order.
using uniform_fn = double (*)(void *state);

struct Attempt {
  ULONG steps_done = 0;  // < Neps iff "Leap-frogging ... stopped at %lu/%lu, momentum too high" (HMC.cc:360-364)
};

// HMC.cc:251-369.  Draws Neps then epsilon from `uniform` (260-261), clips epsilon at 2 (263-264), integrates,
// increments *count_attempts (368).  Message printing (ncurses) stays with the caller.
Attempt Hamiltonian_EoM(HamilView *hd, const real_prec *signali, const real_prec *momentai, real_prec *signalf,
                        real_prec *momentaf, uniform_fn uniform, void *rng_state, ULONG *count_attempts);
// HMC.cc:209-248: returns dH and fills the numerical->* bookkeeping (139-140, 218-245); hd->deltaX <- psi(signalf)'s.
real_prec delta_Hamiltonian(HamilView *hd, const real_prec *signali, const real_prec *momentai, const real_prec *signalf,
                            const real_prec *momentaf);
// HMC.cc:146-206: hd->gradpsi <- gradient; hd->deltaX / pos* <- this evaluation's.
void gradient_psi(HamilView *hd, const real_prec *signal);
real_prec kinetic_term(HamilView *hd, const real_prec *momenta);  // HMC.cc:64-121
real_prec psi(HamilView *hd, const real_prec *signal);            // HMC.cc:124-143 (stores psi_prior, psi_likeli)
// field_statistics.cpp:20-90
void measure_spectrum(HamilView *hd, const real_prec *signal, real_prec *kmode, real_prec *power, ULONG N_bin);
// tools/corr_fct.cc:20-80 and tools/2D_corr_fct.cc:23-124 on the device.  `signal` null: the resident chain state, or
// with of_deltaX the engine's deltaX (the density of the last forward model, e.g. of chain_forward).  rmode / corr:
// N_bin (N_bin * N_bin) values, element nbin_par + N_bin * nbin_perp.  planepar == false throws like upstream.
void measure_corr_grid(HamilView *hd, const real_prec *signal, ULONG N_bin, real_prec *rmode, ULONG *nmode,
                       real_prec *corr, bool of_deltaX = false);
void measure_corr2D(HamilView *hd, const real_prec *signal, ULONG N_bin, real_prec *rmode, ULONG *nmode, real_prec *corr,
                    bool planepar = true, bool of_deltaX = false);
// tools/interp_upres.cc:59-86 and tools/2D_corr_fct_interp.cc on the device: the field (sources as above) on an N_out^3
// grid by interpolate_CIC; its 2-D correlation function there, lifted by CIC interpolation (interp_mode 0, cells with
// rpar < L_max && rperp < L_max) or by zero padding of the power spectrum (interp_mode 1, L_max ignored).  output:
// N_out^3 values; rmode / corr as measure_corr2D's.  planepar == false throws like upstream.
void interp_field(HamilView *hd, const real_prec *signal, unsigned N_out, real_prec *output, bool of_deltaX = false);
void measure_corr2D_interp(HamilView *hd, const real_prec *signal, unsigned N_out, unsigned interp_mode, real_prec L_max,
                           ULONG N_bin, real_prec *rmode, ULONG *nmode, real_prec *corr, bool planepar = true,
                           bool of_deltaX = false);
// tools/2D_powspec.cc:25-110 on the device: the anisotropic power spectrum P(k_perp, k_par), sources as above.  kmode /
// power: N_bin * N_bin values, element nbin_par + N_bin * nbin_perp, kmode the mean 3-D |k| of the bin; the tool returns
// no mode counts (bchmc_measure_spectrum2d does).  planepar == false throws like upstream.
void measure_spec2D(HamilView *hd, const real_prec *signal, real_prec *kmode, real_prec *power, ULONG N_bin,
                    bool planepar = true, bool of_deltaX = false);
// The T-web of a sample (bchmc_tweb_classify; upstream: none): eigenvalues of the tidal tensor of the field smoothed with
// a Gaussian of smoothing_scale Mpc/h, and per cell how many exceed lambda_th (0 void, 1 sheet, 2 filament, 3 knot; 255
// where the tensor is not finite).  Sources as above.  lambda: 3 N values (lambda_1 block, lambda_2, lambda_3) or NULL;
// type: N bytes or NULL; n_type / mass_type: 4 values each or NULL.  accumulate: also one more sample of the posterior
// that tweb_probability reads; a sample with non-finite cells throws then (nothing is added, the outputs are written).
void tweb_classify(HamilView *hd, const real_prec *signal, real_prec smoothing_scale, real_prec lambda_th, bool accumulate,
                   real_prec *lambda, unsigned char *type, ULONG *n_type, real_prec *mass_type, bool of_deltaX = false);
// count / samples of one type (0..3) over the accumulated samples: N values; throws with no sample
void tweb_probability(HamilView *hd, int type, real_prec *out);
// The bispectrum of a sample (bchmc_bispectrum; upstream: none) by the FFT estimator: n_shell (1..32) shells of |k| from
// k_min in steps of dk (h/Mpc), all T = n_shell (n_shell + 1) (n_shell + 2) / 6 triplets s1 <= s2 <= s3 in lexicographic
// order.  Sources as above.  b: T values; ntri (closed mode triples), q (the reduced bispectrum): T values or NULL;
// kmean, nmode, power: n_shell values or NULL.
void measure_bispectrum(HamilView *hd, const real_prec *signal, real_prec k_min, real_prec dk, int n_shell, real_prec *b,
                        real_prec *ntri, real_prec *q, real_prec *kmean, ULONG *nmode, real_prec *power,
                        bool of_deltaX = false);
// The Legendre multipoles about the line of sight z (bchmc_measure_multipoles / bchmc_measure_corr_multipoles; upstream:
// none): P_l(k) in measure_spectrum's bins and xi_l(s) in measure_corr_grid's, l = 0, 2, 4.  Sources as above.  kmode /
// rmode: N_bin values; nmode: N_bin or NULL; leg: 2 N_bin (the means of L_2 and L_4 per bin); power / xi: 3 N_bin, l-major.
// planepar == false throws like upstream's 2-D tools.
void measure_multipoles(HamilView *hd, const real_prec *signal, ULONG N_bin, real_prec *kmode, ULONG *nmode, real_prec *leg,
                        real_prec *power, bool planepar = true, bool of_deltaX = false);
void measure_corr_multipoles(HamilView *hd, const real_prec *signal, ULONG N_bin, real_prec *rmode, ULONG *nmode,
                             real_prec *leg, real_prec *xi, bool planepar = true, bool of_deltaX = false);
// massFunctions.cc:49-495 on the device (bchmc_density_particles): a free list of N_OBJ particles onto the grid, upstream's
// argument lists behind the view.  The grid is the handle's: N1 .. min3 must be the view's own values (std::runtime_error
// otherwise -- these functions do not assign onto another grid).  NGP and TSC always read Par_mass, like upstream; CIC and
// SPH read it when weightmass is set.  delta: N values, the raw density.
void getDensity_NGP(HamilView *hd, unsigned N1, unsigned N2, unsigned N3, real_prec L1, real_prec L2, real_prec L3,
                    real_prec d1, real_prec d2, real_prec d3, real_prec min1, real_prec min2, real_prec min3,
                    const real_prec *xp, const real_prec *yp, const real_prec *zp, const real_prec *Par_mass, ULONG N_OBJ,
                    real_prec *delta);
void getDensity_CIC(HamilView *hd, ULONG N1, ULONG N2, ULONG N3, real_prec L1, real_prec L2, real_prec L3, real_prec d1,
                    real_prec d2, real_prec d3, real_prec min1, real_prec min2, real_prec min3, const real_prec *xp,
                    const real_prec *yp, const real_prec *zp, const real_prec *Par_mass, ULONG N_OBJ, real_prec *delta,
                    bool weightmass);
void getDensity_TSC(HamilView *hd, unsigned N1, unsigned N2, unsigned N3, real_prec L1, real_prec L2, real_prec L3,
                    real_prec d1, real_prec d2, real_prec d3, real_prec min1, real_prec min2, real_prec min3,
                    const real_prec *xp, const real_prec *yp, const real_prec *zp, const real_prec *Par_mass, ULONG N_OBJ,
                    real_prec *delta);
void getDensity_SPH(HamilView *hd, ULONG N1, ULONG N2, ULONG N3, real_prec L1, real_prec L2, real_prec L3, real_prec d1,
                    real_prec d2, real_prec d3, real_prec min1, real_prec min2, real_prec min3, const real_prec *xp,
                    const real_prec *yp, const real_prec *zp, const real_prec *Par_mass, ULONG N_OBJ, real_prec *delta,
                    bool weightmass, real_prec kernel_h);
// tools/poisson_upres.cc:23-65 on the device (bchmc_poisson_draw + bchmc_poisson_positions): upstream's argument list
// behind the view, with (seed, stream) of the engine's counter-based sampler in the place of the gsl_rng -- exact in
// distribution, not GSL's stream (properties P1-P5 in bchmc.h).  lambda: N1^3 rates, N1 = N2 = N3 at most the handle's
// grid size, on the handle's box (std::runtime_error otherwise).  Returns upstream's list of (x, y, z), in its order; the
// sample stays resident in the engine.
std::vector<std::vector<real_prec>> discrete_poisson_sample(HamilView *hd, const real_prec *lambda, unsigned N1, unsigned N2,
                                                            unsigned N3, real_prec L1, real_prec L2, real_prec L3,
                                                            uint64_t seed, uint32_t stream = 0);
// tools/poisson_upres.cc:107-157 end to end, without a position leaving the device: a sample of Nbar (1 + delta) of the
// N1^3 field `delta`, assigned to the handle's grid by masskernel mk (the tool's is CIC, 1).  output: N values.
void poisson_upres(HamilView *hd, const real_prec *delta, unsigned N1, real_prec Nbar, uint64_t seed, real_prec *output,
                   int mk = 1, uint32_t stream = 0);
// interpolate_grid.cpp:108-120, 194-202, 271-286 on the device (bchmc_interp_particles): host grids read at a free list of
// N_OBJ particles, upstream's argument lists behind the view.  The grid is the handle's (std::runtime_error otherwise).
// A particle outside TSC's domain, or with a non-finite coordinate, gets a quiet NaN (property I4 in bchmc.h).
// interpolate_TSC_multi takes 1 .. BCHMC_INTERP_MAX_FIELDS fields.
void interpolate_CIC(HamilView *hd, ULONG N1, ULONG N2, ULONG N3, real_prec L1, real_prec L2, real_prec L3, real_prec d1,
                     real_prec d2, real_prec d3, const real_prec *xp, const real_prec *yp, const real_prec *zp,
                     const real_prec *field_grid, ULONG N_OBJ, real_prec *interpolation);
void interpolate_TSC(HamilView *hd, ULONG N1, ULONG N2, ULONG N3, real_prec d1, real_prec d2, real_prec d3,
                     const real_prec *xp, const real_prec *yp, const real_prec *zp, const real_prec *field_grid, ULONG N_OBJ,
                     real_prec *interpolation);
void interpolate_TSC_multi(HamilView *hd, ULONG N1, ULONG N2, ULONG N3, real_prec d1, real_prec d2, real_prec d3,
                           real_prec *xp, real_prec *yp, real_prec *zp, ULONG N_OBJ, real_prec **field_grids,
                           real_prec **interpolations, int N_fields);
// Lag2Eul of the resident chain state (dump_deltas' second forward model, IOfunctionsGen.cc:158-169, with use_rsd = 0);
// hd->deltaX / pos* <- this evaluation's.  use_rsd < 0: as configured.
void chain_forward(HamilView *hd, int use_rsd);
// HMC_mass.cc:315-368 on the device at `signal` (null: the resident chain state).  The engine keeps the built mass (the
// mass generation is bumped and marked uploaded, so nothing re-uploads a host array over it, and the EoM energies are
// dropped); mass_f_out / mass_r_out (may be null) receive host copies where the mass_type has the array.
void Hamiltonian_mass(HamilView *hd, const real_prec *signal, real_prec *mass_f_out, real_prec *mass_r_out);
// HMC.cc:387-400: whether HamiltonianMC rebuilds the mass at the top of sample iGibbs (massnum 0: never).
bool massnum_due(ULONG iGibbs, ULONG massnum_init, ULONG massnum_burn);
// ---- step-size adaptation (barlib/src/hmc/leapfrog/time_step.cpp, include/hmc/leapfrog/time_step.hpp) ------------
// The keys of data/input.par:59-87 and the two tables they act on.  Host-only, O(N_a) work per call.
struct EpsAdapt;
struct EpsAdaptConfig {
  int eps_fac_update_type = 3;   // 0 none, 1 power mean every s_eps_total, 2 acceptance rate, 3 = 2 + fast initial phase
  unsigned N_a_eps_update = 100;
  real_prec acc_min = 0.6, acc_max = 0.7;
  int eps_down_smooth = 5;
  real_prec eps_up_fac = 1.;
  real_prec eps_fac_target = 0., eps_fac_power = 2.;
  ULONG s_eps_total = 10;
};
EpsAdapt *eps_adapt_create(const EpsAdaptConfig &cfg);
void eps_adapt_destroy(EpsAdapt *e);
// update_eps_fac (time_step.cpp:151-185): called before every trajectory (HMC.cc:453); may change n->eps_fac.
// Returns the message the reference prints to its ncurses window ("" when nothing was adjusted).
std::string update_eps_fac(HamilView *hd);
// update_epsilon_acc_rate_tables (time_step.cpp:187-203): one finished attempt (n->accepted, n->epsilon) into the
// tables.  The table index is (records - 1) % N_a with records = this chain's attempts plus pooled ones; for a single
// chain that is the reference's (count_attempts - 1) % N_a.
void update_epsilon_acc_rate_tables(HamilView *hd);
// Pooled records of OTHER chains (after bchmc_eps_exchange): same tables, same index rule.
void eps_adapt_append(EpsAdapt *e, bool accepted, real_prec epsilon);
ULONG eps_adapt_records(const EpsAdapt *e);
real_prec eps_adapt_acceptance_rate(const EpsAdapt *e);  // bool_mean(acc_flag_N_a), time_step.cpp:24-28

// ---- HamiltonianMC on the device-resident chain (HMC.cc:431-511) -------------------------------
// The row of performance_log.txt (HMC.cc:40-60) of one attempt.
struct AttemptLog {
  bool accepted = false;
  real_prec epsilon = 0;
  ULONG Neps = 0, steps_done = 0;
  real_prec dH = 0, dK = 0, dE = 0, dprior = 0, dlikeli = 0;
  real_prec psi_prior_i = 0, psi_prior_f = 0, psi_likeli_i = 0, psi_likeli_f = 0, H_kin_i = 0, H_kin_f = 0;
};
// Host-side momentum draw (e.g. the caller's draw_momenta on its gsl_rng, HMC_momenta.cc:42-94): fills N doubles.
using momenta_fn = void (*)(void *state, real_prec *momenta, ULONG N);
void chain_set_state(HamilView *hd, const real_prec *x);  // hd->x -> HBM, once per sample
void chain_get_state(HamilView *hd, real_prec *x);
// One sample: repeat { momenta; (Neps, epsilon) from `uniform` in the reference's order (HMC.cc:260-261); trajectory;
// dH; Metropolis test, statement for statement HMC.cc:462-486 (a uniform is consumed only when p_acceptance < 1) }
// until accepted or `itmax` attempts.  Momenta: `momenta` if given, else the engine's counter-based device draw
// (seed, attempt index).  Fills log[0 .. return value - 1]; *count_attempts advances like HMC.cc:368.
// `log` may be null; otherwise it holds `log_cap` rows and attempts beyond that are not logged (the return value still
// counts them).  Per attempt, like the reference: update_eps_fac before the trajectory (HMC.cc:453), rejections++ on a
// reject (500-501), n->accepted, update_epsilon_acc_rate_tables (506-507).  After the loop, when hd->comm is set, ONE
// bchmc_eps_exchange with this sample's records; the other chains' records are appended to the tables.
ULONG HamiltonianMC(HamilView *hd, uniform_fn uniform, void *rng_state, uint64_t seed, ULONG itmax, ULONG *count_attempts,
                    AttemptLog *log, ULONG log_cap, momenta_fn momenta, void *momenta_state);

// The same loop with the momenta drawn on the device from the caller's own gsl_rng (mt19937 only): every attempt reads
// the generator's state through `state` (store = 0: fill mt / mti from the generator), draws draw_momenta's exact
// momenta (bchmc_chain_draw_momenta_mt19937) and writes the advanced state back (store = 1) before `uniform` is called
// for Neps -- so momenta, Neps, epsilon and the Metropolis uniform come from one stream in the reference's order
// (HMC.cc:449, 260-261, 480).  INTEGRATION.md shows the barlib side (gsl_rng_state of a gsl_rng_mt19937).
using mt19937_state_fn = void (*)(void *rng_state, uint32_t mt[624], int32_t *mti, int store);
ULONG HamiltonianMC_mt19937(HamilView *hd, uniform_fn uniform, mt19937_state_fn state, void *rng_state, ULONG itmax,
                            ULONG *count_attempts, AttemptLog *log, ULONG log_cap);

// The start of a run (load_initial_fields, barcoderunner.cc:284-344, with random_test): the scalars setup_random_test
// and make_initial_guess read.  They live in upstream's NUMERICAL / OBSERVATIONAL, not in HAMIL_DATA, hence a struct of
// their own beside the views.
struct MockView {
  int window_type = 1, data_model = 0, negative_obs = 0, random_test_rsd = 0;  // init_par.cc:61-67
  real_prec sigma_min = 1., sigma_fac = 0.;                                    // init_par.cc:149-150
  int initial_guess = 0, initial_guess_smoothing_type = 1;                     // init_par.cc:99-102
  real_prec initial_guess_smoothing_scale = 0.;
  const real_prec *initial_guess_field = nullptr;  // initial_guess 1: what get_scalar read from initial_guess_file
};
// setup_random_test (barcoderunner.cc:42-205) on the device from the caller's gsl_rng (mt19937; `state` as in
// HamiltonianMC_mt19937: read before, written back after).  The engine then holds window / nobs / noise as if they had
// been uploaded; where the view has caller-owned arrays for them they receive the built values (so that a later
// inputs_changed() uploads the same numbers).  delta_lag / delta_eul may be null.  Throws like the reference.
// poisson_seed (not upstream's; null: as upstream, where the engine refuses the Poissonian mock): the mock of data_model 0
// under the Poissonian likelihood from the engine's counter-based sampler (bchmc_setup_random_test_poisson).
void setup_random_test(HamilView *hd, const MockView *m, mt19937_state_fn state, void *rng_state, real_prec *delta_lag,
                       real_prec *delta_eul, const uint64_t *poisson_seed = nullptr, uint32_t poisson_stream = 0);
// make_initial_guess (barcoderunner.cc:207-247): sets the resident chain state (read it with chain_get_state)
void make_initial_guess(HamilView *hd, const MockView *m, mt19937_state_fn state, void *rng_state);

// The four engine calls HamiltonianMC makes, as a table: the default binds the C ABI (bchmc_chain_*); the CPU tests
// bind a scripted stand-in so that the loop's bookkeeping is testable without a GPU.
struct ChainOps {
  int (*draw_momenta)(void *engine, uint64_t seed, uint64_t attempt);
  int (*set_momenta)(void *engine, const real_prec *p);
  int (*attempt)(void *engine, double eps, uint64_t neps, double *dH, double terms[6], uint64_t *steps_done);
  int (*accept)(void *engine, int accepted);
};
ULONG HamiltonianMC_ops(HamilView *hd, const ChainOps &ops, void *engine, uniform_fn uniform, void *rng_state,
                        uint64_t seed, ULONG itmax, ULONG *count_attempts, AttemptLog *log, ULONG log_cap,
                        momenta_fn momenta, void *momenta_state);

// Rank bootstrap for the RCCL transport when no launcher hands the unique id around (barcode/main.cc is a plain
// process per GPU): the 128 bytes travel through files next to `path` (<path>, <path>.want.<r>, <path>.ack.<r>).
// Every file carries the nonce of the process that wrote it and the id file echoes the nonces of the ranks it is for,
// so files left behind by an earlier run at the same path are never taken for this run's (hmc_hip_shim.cc); each rank
// removes its own files once the communicator exists.  Ranks of ONE run share `path`; two runs at the same time need
// different paths.  Sets hd->comm; throws after timeout_s seconds.
void comm_bootstrap_file(HamilView *hd, const char *path, int rank, int world, double timeout_s);
// the file protocol on its own (host only): rank 0 passes the id in, the other ranks receive it
void bootstrap_exchange_id(const char *path, int rank, int world, double timeout_s, unsigned char id[BCHMC_UNIQUE_ID_BYTES]);
void bootstrap_cleanup(const char *path, int rank);
void comm_release(HamilView *hd);

// hd's input arrays changed (HamiltonianMC recomputes the mass every sample, HMC.cc:400-423): upload them again
void inputs_changed(HamilView *hd);
// only hd->mass_f / hd->mass_r changed (HMC.cc:400-423): upload those two again
void mass_changed(HamilView *hd);
void release(HamilView *hd);

}  // namespace bchmc_shim

// C-callable hooks over the functions above (exceptions -> return code + message) so that the test-suite can
// drive the compiled C++ layer through ctypes.  0 = ok, 1 = std::runtime_error (message copied to err).
extern "C" {
int bchmc_shim_Hamiltonian_EoM(bchmc_shim::HamilView *hd, const double *signali, const double *momentai, double *signalf,
                               double *momentaf, bchmc_shim::uniform_fn uniform, void *rng_state,
                               unsigned long *count_attempts, unsigned long *steps_done, char *err, size_t errlen);
int bchmc_shim_delta_Hamiltonian(bchmc_shim::HamilView *hd, const double *signali, const double *momentai,
                                 const double *signalf, const double *momentaf, double *dH, char *err, size_t errlen);
int bchmc_shim_gradient_psi(bchmc_shim::HamilView *hd, const double *signal, char *err, size_t errlen);
int bchmc_shim_measure_spectrum(bchmc_shim::HamilView *hd, const double *signal, double *kmode, double *power,
                                unsigned long N_bin, char *err, size_t errlen);
int bchmc_shim_Hamiltonian_mass(bchmc_shim::HamilView *hd, const double *signal, double *mass_f, double *mass_r, char *err,
                                size_t errlen);
int bchmc_shim_measure_corr_grid(bchmc_shim::HamilView *hd, const double *signal, unsigned long N_bin, double *rmode,
                                 unsigned long *nmode, double *corr, int of_deltaX, char *err, size_t errlen);
int bchmc_shim_measure_corr2D(bchmc_shim::HamilView *hd, const double *signal, unsigned long N_bin, double *rmode,
                                   unsigned long *nmode, double *corr, int planepar, int of_deltaX, char *err,
                                   size_t errlen);
int bchmc_shim_interp_field(bchmc_shim::HamilView *hd, const double *signal, unsigned N_out, double *output, int of_deltaX,
                            char *err, size_t errlen);
int bchmc_shim_measure_corr2D_interp(bchmc_shim::HamilView *hd, const double *signal, unsigned N_out, unsigned interp_mode,
                                     double L_max, unsigned long N_bin, double *rmode, unsigned long *nmode, double *corr,
                                     int planepar, int of_deltaX, char *err, size_t errlen);
int bchmc_shim_measure_spec2D(bchmc_shim::HamilView *hd, const double *signal, double *kmode, double *power,
                              unsigned long N_bin, int planepar, int of_deltaX, char *err, size_t errlen);
int bchmc_shim_tweb_classify(bchmc_shim::HamilView *hd, const double *signal, double smoothing_scale, double lambda_th,
                             int accumulate, double *lambda, unsigned char *type, unsigned long *n_type, double *mass_type,
                             int of_deltaX, char *err, size_t errlen);
int bchmc_shim_tweb_probability(bchmc_shim::HamilView *hd, int type, double *out, char *err, size_t errlen);
int bchmc_shim_measure_bispectrum(bchmc_shim::HamilView *hd, const double *signal, double k_min, double dk, int n_shell,
                                  double *b, double *ntri, double *q, double *kmean, unsigned long *nmode, double *power,
                                  int of_deltaX, char *err, size_t errlen);
int bchmc_shim_measure_multipoles(bchmc_shim::HamilView *hd, const double *signal, unsigned long N_bin, double *kmode,
                                  unsigned long *nmode, double *leg, double *power, int planepar, int of_deltaX, char *err,
                                  size_t errlen);
int bchmc_shim_measure_corr_multipoles(bchmc_shim::HamilView *hd, const double *signal, unsigned long N_bin, double *rmode,
                                       unsigned long *nmode, double *leg, double *xi, int planepar, int of_deltaX,
                                       char *err, size_t errlen);
/* getDensity_NGP / _CIC / _TSC / _SPH (mk 0 .. 3) with the view's own geometry */
int bchmc_shim_getDensity(bchmc_shim::HamilView *hd, int mk, const double *xp, const double *yp, const double *zp,
                          const double *Par_mass, unsigned long N_OBJ, double *delta, int weightmass, double kernel_h,
                          char *err, size_t errlen);
/* interpolate_CIC (which = 1), interpolate_TSC (2) or interpolate_TSC_multi (3) with the view's own geometry; fields:
 * n_fields grids of N doubles one after the other, out: n_fields * N_OBJ, field-major */
int bchmc_shim_interpolate(bchmc_shim::HamilView *hd, int which, const double *xp, const double *yp, const double *zp,
                           unsigned long N_OBJ, const double *fields, int n_fields, double *out, char *err, size_t errlen);
int bchmc_shim_chain_forward(bchmc_shim::HamilView *hd, int use_rsd, char *err, size_t errlen);
int bchmc_shim_chain_set_state(bchmc_shim::HamilView *hd, const double *x, char *err, size_t errlen);
int bchmc_shim_chain_get_state(bchmc_shim::HamilView *hd, double *x, char *err, size_t errlen);
int bchmc_shim_HamiltonianMC(bchmc_shim::HamilView *hd, bchmc_shim::uniform_fn uniform, void *rng_state, uint64_t seed,
                             unsigned long itmax, unsigned long *count_attempts, bchmc_shim::AttemptLog *log,
                             unsigned long log_cap, unsigned long *n_attempts, char *err, size_t errlen);
int bchmc_shim_HamiltonianMC_mt19937(bchmc_shim::HamilView *hd, bchmc_shim::uniform_fn uniform,
                                     bchmc_shim::mt19937_state_fn state, void *rng_state, unsigned long itmax,
                                     unsigned long *count_attempts, bchmc_shim::AttemptLog *log, unsigned long log_cap,
                                     unsigned long *n_attempts, char *err, size_t errlen);
/* the same loop on a scripted engine: attempt k returns dH = script_dH[k] (CPU tests of the bookkeeping) */
int bchmc_shim_HamiltonianMC_scripted(bchmc_shim::HamilView *hd, const double *script_dH, unsigned long n_script,
                                      bchmc_shim::uniform_fn uniform, void *rng_state, unsigned long itmax,
                                      unsigned long *count_attempts, bchmc_shim::AttemptLog *log, unsigned long log_cap,
                                      unsigned long *n_attempts, char *err, size_t errlen);
int bchmc_shim_setup_random_test(bchmc_shim::HamilView *hd, const bchmc_shim::MockView *m,
                                 bchmc_shim::mt19937_state_fn state, void *rng_state, double *delta_lag,
                                 double *delta_eul, char *err, size_t errlen);
int bchmc_shim_setup_random_test_poisson(bchmc_shim::HamilView *hd, const bchmc_shim::MockView *m,
                                         bchmc_shim::mt19937_state_fn state, void *rng_state, uint64_t seed,
                                         uint32_t stream, double *delta_lag, double *delta_eul, char *err, size_t errlen);
/* discrete_poisson_sample in two steps, so that a sample is drawn once and crosses PCIe once: the draw (*n_part = the
 * sample's size; the sample stays resident), then any slice of it as three columns (bchmc_poisson_positions) */
int bchmc_shim_discrete_poisson_sample(bchmc_shim::HamilView *hd, const double *lambda, unsigned N1, uint64_t seed,
                                       uint32_t stream, uint64_t *n_part, char *err, size_t errlen);
int bchmc_shim_poisson_positions(bchmc_shim::HamilView *hd, uint64_t first, uint64_t m, double *x, double *y, double *z,
                                 char *err, size_t errlen);
int bchmc_shim_poisson_upres(bchmc_shim::HamilView *hd, const double *delta, unsigned N1, double Nbar, uint64_t seed,
                             uint32_t stream, int mk, double *output, char *err, size_t errlen);
int bchmc_shim_make_initial_guess(bchmc_shim::HamilView *hd, const bchmc_shim::MockView *m,
                                  bchmc_shim::mt19937_state_fn state, void *rng_state, char *err, size_t errlen);
size_t bchmc_shim_sizeof_mock(void);
int bchmc_shim_kinetic_term(bchmc_shim::HamilView *hd, const double *momenta, double *out, char *err, size_t errlen);
int bchmc_shim_psi(bchmc_shim::HamilView *hd, const double *signal, double *out, char *err, size_t errlen);
bchmc_shim::EpsAdapt *bchmc_shim_eps_create(int update_type, unsigned N_a, double acc_min, double acc_max, int down_smooth,
                                            double up_fac, double target, double power, unsigned long s_eps_total);
void bchmc_shim_eps_destroy(bchmc_shim::EpsAdapt *e);
void bchmc_shim_eps_append(bchmc_shim::EpsAdapt *e, int accepted, double epsilon);
unsigned long bchmc_shim_eps_records(const bchmc_shim::EpsAdapt *e);
double bchmc_shim_eps_acceptance_rate(const bchmc_shim::EpsAdapt *e);
int bchmc_shim_update_eps_fac(bchmc_shim::HamilView *hd, char *msg, size_t msglen, char *err, size_t errlen);
int bchmc_shim_update_tables(bchmc_shim::HamilView *hd, char *err, size_t errlen);
int bchmc_shim_comm_bootstrap_file(bchmc_shim::HamilView *hd, const char *path, int rank, int world, double timeout_s,
                                   char *err, size_t errlen);
int bchmc_shim_bootstrap_exchange_id(const char *path, int rank, int world, double timeout_s, unsigned char *id, char *err,
                                     size_t errlen);
void bchmc_shim_bootstrap_cleanup(const char *path, int rank);
int bchmc_shim_comm_attach(bchmc_shim::HamilView *hd, bchmc_comm *comm, int rank); /* tests: a custom-transport communicator */
void bchmc_shim_comm_release(bchmc_shim::HamilView *hd);
void bchmc_shim_inputs_changed(bchmc_shim::HamilView *hd);
void bchmc_shim_mass_changed(bchmc_shim::HamilView *hd);
size_t bchmc_shim_sizeof_attempt_log(void);
void bchmc_shim_release(bchmc_shim::HamilView *hd);
size_t bchmc_shim_sizeof_view(void);
size_t bchmc_shim_sizeof_numerical(void);
}
#endif
