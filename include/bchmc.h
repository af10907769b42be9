/*
 * bchmc.h -- C ABI of libbarcode_hip.so: MI355X-native engine for Barcode's HMC leapfrog hot path.
 *
 * This is the drop-in boundary.  Each entry point replaces a piece of the reference's C++ interface
 * (paths under /root/reference/).  The engine owns all device state (rocFFT plans, grids in HBM);
 * the caller owns every host array passed in and out.  One handle = one GPU = one Markov chain;
 * calls on one handle are not re-entrant, different handles are independent.
 *
 * Error convention: every function returns 0 on success or a BCHMC_ERR_* code; bchmc_strerror() gives
 * the text, bchmc_last_error() the detail of the last failure on a handle.  The reference throws
 * std::runtime_error in the same situations (HMC_models.cc:316-319, 296-298; struct_hamil.h:309-312);
 * the reference-side shim turns non-zero codes back into exceptions.
 */
#ifndef BCHMC_H
#define BCHMC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCHMC_ABI_VERSION 4

/* Scalars of HAMIL_NUMERICAL / HAMIL_DATA read by the path (barlib/include/struct_hamil.h:51-222);
 * filled by the shim from the HAMIL_DATA that call_hamil.cc:42 builds.  Cubic grids only, like the
 * reference (init_par.cc:116-118). */
typedef struct bchmc_config {
  uint32_t abi_version;      /* must be BCHMC_ABI_VERSION */
  uint32_t Nx;               /* N1 = N2 = N3.  Any Nx >= 4 with particle_kernel_h <= L / 4 is accepted, odd ones included:
                              * 4 runs the tile kernels on one 4^3 tile, 5, 6, 7 and every other size no tile shape divides
                              * the direct ones.  At odd Nx the reference's "Nyquist" rule i == Nx / 2 (integer division)
                              * zeroes an ordinary mode; it is kept as it is.  Entry points that need an even Nx (they
                              * return BCHMC_ERR_UNSUPPORTED naming Nx before anything is queued, the generator state and
                              * the handle untouched): bchmc_chain_draw_momenta_mt19937 with a Fourier-space mass,
                              * bchmc_setup_random_test, bchmc_make_initial_guess 2 and 3 -- all through create_GARFIELD's
                              * walk, which pairs i with Nx - i around Nx / 2 -- and bchmc_garfield_walk_index itself
                              * (BCHMC_ERR_ARG, it has no handle) */
  double L;                  /* L1 = L2 = L3 [Mpc/h] */
  double min1, min2, min3;   /* xllc, yllc, zllc */
  double xobs, yobs, zobs;
  int32_t planepar, periodic;
  int32_t mk;                /* masskernel: 0 NGP, 1 CIC, 2 TSC, 3 SPH */
  int32_t calc_h;            /* 0 (legacy), 1, 2 (SPH adjoint, default) or 3 (Fourier + TSC) */
  int32_t likelihood;        /* 0 Poisson, 1 Gaussian, 2 log-normal, 3 GRF (init_par.cc:534-559) */
  int32_t sfmodel;           /* 1 Zel'dovich; anything else: ALPT (Lag2Eul_non_zeldovich, Lag2Eul.cc:138-312, dispatcher
                              * 325-331) unless rsd_model is set, which always takes the Zel'dovich + RSD model */
  int32_t rsd_model;
  int32_t mass_type;         /* 0,1,2,3,4,5,6,60 -> mass_fs/mass_rs as struct_hamil.h:272-313 */
  int32_t correct_delta;
  int32_t div_dH_by_N;
  double particle_kernel_h;  /* SPH scale length, = particle_kernel_h_rel * cell size */
  double grad_psi_prior_factor, grad_psi_likeli_factor, deltaQ_factor;
  double rho_c, delta_min, biasP, biasE;
  double ascale, D1, D2, OM, OL;
  double kth;                /* ALPT split scale [Mpc/h] = n->kth = slength (struct_hamil.h:102,259; input.par:121) */
  int32_t precision;         /* 0: fp64 field arrays (reference DOUBLE_PREC); 1: fp32 field arrays (SINGLE_PREC-like:
                              * storage + particle-mesh arithmetic in float, k-space arithmetic and reductions in
                              * double).  The ABI's arrays are double in both modes. */
  int32_t device;            /* HIP device ordinal */
  int32_t deterministic;     /* 1: bitwise repeatable results -- the mass assignment accumulates in 64-bit fixed point
                              * (integer adds are order-independent), the density is converted and summed in a fixed
                              * order; one extra pass over the grid per force evaluation.  0: hardware float atomics,
                              * last bits vary from run to run like the reference's OpenMP build (barcode/main.cc:86-90).
                              * BCHMC_DETERMINISTIC=1 in the environment switches it on for every handle.
                              * Range: contributions are scaled to 2^46 per maximal one (W(0), or weight 1), so a cell
                              * holds 2^17 of them before the 63-bit sum wraps; a cell that passed 2^16 (or came out
                              * negative) makes the next synchronising call return BCHMC_ERR_STATE. */
  int32_t reserved0;
} bchmc_config;

enum {
  BCHMC_OK = 0,
  BCHMC_ERR_ARG = 1,
  BCHMC_ERR_MK_NOT_SPH = 2,       /* calc_h 2/3 need masskernel 3 (HMC_models.cc:316-319) */
  BCHMC_ERR_RSD_NOT_PLANEPAR = 3, /* HMC_models.cc:296-298, rsd.cc:60-62 */
  BCHMC_ERR_MASS_TYPE = 4,        /* struct_hamil.h:309-312 */
  BCHMC_ERR_UNSUPPORTED = 5,
  BCHMC_ERR_HIP = 6,
  BCHMC_ERR_ROCFFT = 7,
  BCHMC_ERR_NOMEM = 8,
  BCHMC_ERR_STATE = 9             /* e.g. an input array was never uploaded */
};

/* Arrays of HAMIL_DATA (struct_hamil.h:146-166).  Inputs are uploaded once per chain (or when
 * Hamiltonian_mass recomputes the mass, HMC.cc:400-423); outputs are fetched on demand. */
typedef enum bchmc_field {
  BCHMC_F_SIGNAL_PS = 0, /* in : prior power spectrum on the full N^3 grid (hd->signal_PS) */
  BCHMC_F_MASS_F = 1,    /* in : Fourier-space mass (hd->mass_f), full N^3 grid */
  BCHMC_F_MASS_R = 2,    /* in : real-space mass (hd->mass_r) */
  BCHMC_F_NOBS = 3,      /* in : hd->nobs */
  BCHMC_F_NOISE = 4,     /* in : hd->noise */
  BCHMC_F_WINDOW = 5,    /* in : hd->window */
  BCHMC_F_DELTAX = 6,    /* out: hd->deltaX of the last force / energy evaluation */
  BCHMC_F_POSX = 7,      /* out: hd->posx */
  BCHMC_F_POSY = 8,
  BCHMC_F_POSZ = 9,
  BCHMC_F_RHO = 10,      /* out (diagnostic): density before overdens() */
  BCHMC_F_PART_LIKE = 11,/* out (diagnostic): partial_f_delta_x_log_like */
  BCHMC_F_VX = 12,       /* out (diagnostic): likelihood_calc_V_SPH */
  BCHMC_F_VY = 13,
  BCHMC_F_VZ = 14,
  BCHMC_F_PSIX = 15,     /* out (diagnostic): theta2vel displacement */
  BCHMC_F_PSIY = 16,
  BCHMC_F_PSIZ = 17,
  BCHMC_F_GRAD_PRIOR = 18, /* out: prior term of the last bchmc_gradient (after its test factor) */
  BCHMC_F_GRAD_LIKE = 19,  /* out: likelihood term of the last bchmc_gradient (after its test factor) */
  BCHMC_F_COUNT = 20
} bchmc_field;

typedef struct bchmc_handle bchmc_handle;

/* Lifecycle.  Replaces plan_pkg construction (fftwrapper.cc:281-324, init_par.cc:418-426) and the
 * per-sample HAMIL_DATA setup (call_hamil.cc:38-42). */
int bchmc_create(const bchmc_config *cfg, bchmc_handle **out);
void bchmc_destroy(bchmc_handle *h);
const char *bchmc_strerror(int code);
const char *bchmc_last_error(const bchmc_handle *h);

/* Host -> HBM copy of one input array of N = Nx^3 doubles. */
int bchmc_upload(bchmc_handle *h, bchmc_field field, const double *host, size_t n);
/* HBM -> host copy of one output array of N doubles (state of the last force / energy evaluation). */
int bchmc_fetch(bchmc_handle *h, bchmc_field field, double *host, size_t n);

/* Hamiltonian_EoM (HMC.cc:251-369): `neps` leapfrog steps of size `eps` from (q0, p0) to (q1, p1).
 * The shim draws neps and eps from the caller's gsl_rng exactly as HMC.cc:260-264 and passes them in.
 * *steps_done < neps iff the runaway-momentum guard |p[0]| > 1e50 (HMC.cc:360-364) fired. */
int bchmc_leapfrog(bchmc_handle *h, const double *q0, const double *p0, double *q1, double *p1, double eps,
                   uint64_t neps, uint64_t *steps_done);

/* Hamiltonian_EoM (HMC.cc:251-369) and delta_Hamiltonian (HMC.cc:209-248) of the same four arrays in ONE pass --
 * what HamiltonianMC does with consecutive calls at HMC.cc:455 and 459.  Same (q1, p1, *steps_done) as bchmc_leapfrog;
 * *dH and terms as bchmc_delta_hamiltonian would return for (q0, p0, q1, p1): K and psi_prior of both ends are
 * Parseval sums of the k-space state, -log L of both ends comes from the trajectory's own first and last force
 * evaluation where log_like's forward model is the force's one (else, and for real-space masses and the GRF
 * likelihood, the energies are evaluated around the trajectory) -- four array uploads and two forward models fewer
 * than the two separate calls.  The reuse is the CALLER's statement, made by choosing this entry point: the engine
 * keeps no memory of earlier calls, and bchmc_delta_hamiltonian always evaluates what it is given.  Leaves
 * psi(q1)'s deltaX / pos* in the handle (HMC.cc:225).  (ABI version 4; replaces the pointer + sampled-content
 * cache version 3 kept inside bchmc_delta_hamiltonian.) */
int bchmc_leapfrog_dh(bchmc_handle *h, const double *q0, const double *p0, double *q1, double *p1, double eps,
                      uint64_t neps, uint64_t *steps_done, double *dH, double terms[6]);

/* kinetic_term + psi (HMC.cc:64-143): out = { H_kin, psi_prior, psi_likeli } at (q, p).  Leaves
 * deltaX / pos* of this evaluation in the handle like the reference's log_like does. */
int bchmc_energies(bchmc_handle *h, const double *q, const double *p, double out[3]);

/* kinetic_term (HMC.cc:64-121) and psi (HMC.cc:124-143) on their own: one transform and one reduction for the
 * kinetic term (needs mass_f / mass_r only); psi_out = { log_prior, log_like } with the forward model of `q` left in
 * the handle (deltaX / pos*), like the reference's log_like leaves it in HAMIL_DATA. */
int bchmc_kinetic_term(bchmc_handle *h, const double *p, double *out);
int bchmc_psi(bchmc_handle *h, const double *q, double psi_out[2]);

/* delta_Hamiltonian (HMC.cc:209-248): terms = { H_kin_i, psi_prior_i, psi_likeli_i, H_kin_f,
 * psi_prior_f, psi_likeli_f }, *dH includes div_dH_by_N.  Always a full evaluation of the arrays passed in, against
 * the inputs uploaded at the time of the call (no result of an earlier call is reused). */
int bchmc_delta_hamiltonian(bchmc_handle *h, const double *qi, const double *pi, const double *qf, const double *pf,
                            double *dH, double terms[6]);

/* gradient_psi (HMC.cc:146-206): g = prior_factor * S^-1 q + likeli_factor * d(-log L)/dq. */
int bchmc_gradient(bchmc_handle *h, const double *q, double *g);

/* Forward model only (Lag2Eul, Lag2Eul.cc:318-332 / 338-424): leaves deltaX and pos* in the handle.
 * use_rsd < 0 means "as configured". */
int bchmc_forward(bchmc_handle *h, const double *q, int use_rsd);

/* ---- device-resident variants: same semantics, all pointers are HBM addresses on the handle's device,
 * work is enqueued on the handle's stream and NOT synchronised (call bchmc_sync). ---- */
int bchmc_leapfrog_device(bchmc_handle *h, const double *d_q0, const double *d_p0, double *d_q1, double *d_p1,
                          double eps, uint64_t neps);
int bchmc_steps_done(bchmc_handle *h, uint64_t *steps_done); /* synchronises */
int bchmc_energies_device(bchmc_handle *h, const double *d_q, const double *d_p, double out[3]); /* synchronises */
/* Waits for the handle's stream.  Also the point where the engine adapts its working storage to the field it has just
 * seen: if a force evaluation overflowed the binning's per-tile record slots (that evaluation itself was still exact,
 * through the two-pass sort), they are doubled here, so a trajectory never pays for a reallocation.  bchmc_steps_done,
 * bchmc_forward and the host-array energy / gradient calls do the same. */
int bchmc_sync(bchmc_handle *h);
void *bchmc_stream(bchmc_handle *h); /* hipStream_t the engine launches on */

/* ---- device-resident chain ("next" components, built on the same path) ----
 * The current sample q and the momenta stay in HBM between attempts, so one HamiltonianMC attempt
 * (HMC.cc:445-498) costs no 4 x N-double PCIe round trip, and the -log L of both trajectory ends is taken
 * from the force evaluations the trajectory performs anyway instead of two extra forward models.
 * Host keeps the control flow: (Neps, epsilon) draws, u < exp(-dH) test, epsilon adaptation. */
int bchmc_chain_set_state(bchmc_handle *h, const double *q);   /* hd->x -> HBM */
int bchmc_chain_get_state(bchmc_handle *h, double *q);
int bchmc_chain_set_momenta(bchmc_handle *h, const double *p); /* host-drawn momenta (reference RNG order) */
/* The resident momenta live in k-space; what comes back went through a transform pair.  After a draw (either kind below)
 * for a real-space mass alone (mass_type 0, 6, 60) the cells where mass_r is not positive (<= 0 or NaN) come back exactly 0,
 * as they were drawn, for as long as mass_r is the array of the draw. */
int bchmc_chain_get_momenta(bchmc_handle *h, double *p);
/* p ~ N(0, M) on the device: counter-based Philox4x32-10.  Statistical stand-in for draw_momenta (HMC_momenta.cc:42-94),
 * whose serial GSL stream it does not reproduce.
 * The values.  Pair i = 0 .. (N + 1) / 2 - 1 of white-noise array s (s = 0: the Fourier-space part, s = 1: the real-space
 * part) takes r = philox4x32_10((i_lo, i_hi | 0x80000000, attempt, s), (seed_lo, seed_hi)), the two 53-bit uniforms
 * u1 = (((r.x << 32 | r.y) >> 11) + 0.5) 2^-53 and u2 the same from r.z, r.w, and Box-Muller in double:
 * w_s[2 i] = sqrt(-2 ln u1) cos(2 pi u2), w_s[2 i + 1] = sqrt(-2 ln u1) sin(2 pi u2) (the last one is dropped at odd N).
 * Then p = IFFT[ FFT[w_0] sqrt(mass_f N / L^3) ] (0 where mass_f <= 0) + sqrt(mass_r) w_1 (0 where mass_r <= 0), each part
 * only where mass_type has it: a pure function of (seed, attempt, cell), not of the launch shape or the handle's kind.
 * The counter map of the engine's Philox4x32-10, every consumer, key = (seed_lo, seed_hi) throughout:
 *     momentum draw, array s          (i_lo, i_hi | 0x80000000, attempt, s)      i: pair index, s in {0, 1}
 *     Poisson counts (P1 below)       (c_lo, c_hi, j, 2 stream)                  c: cell index, j: iteration < 64
 *     Poisson positions (P5 below)    (c_lo, c_hi, kk, 2 stream + 1)             kk: index of the particle in its cell
 * A pair or cell index stays below 2^63, so bit 31 of the second word is set for the momentum draw and clear for the
 * Poisson sampler: the two share no counter under any seed, attempt or stream, and one seed may serve both.
 * attempt is one counter word: attempt >= 2^32 is BCHMC_ERR_ARG, the resident momenta untouched. */
int bchmc_chain_draw_momenta(bchmc_handle *h, uint64_t seed, uint64_t attempt);
/* draw_momenta (HMC_momenta.cc:42-94) on the device from the caller's GSL mt19937 state; mt/mti in: state before the
 * draw, out: the state GSL holds after it.  words_used may be NULL.
 * Exactly the reference's momenta: create_GARFIELD's Gaussians in the walk of resolution_independent_random_grid_FS,
 * then the real-space part from the same stream (polar Box-Muller, r2 without FMA contraction; log / sqrt may differ
 * from glibc by an ulp).  The first call on a handle also precomputes the stream's jump polynomials (host, once).
 * Odd Nx with a Fourier-space mass (mass_type 1 .. 5): BCHMC_ERR_UNSUPPORTED before anything is queued, mt / mti and the
 * resident momenta untouched (the walk is defined for even Nx); the real-space types 0, 6 and 60 draw at any Nx. */
int bchmc_chain_draw_momenta_mt19937(bchmc_handle *h, uint32_t mt[624], int32_t *mti, uint64_t *words_used);
/* host only (tests, callers that skip ahead): the state `steps` outputs later */
int bchmc_mt19937_jump(const uint32_t mt_in[624], int32_t mti_in, uint64_t steps, uint32_t mt_out[624], int32_t *mti_out);
/* host only: index of cell (i, j, k) in the walk of resolution_independent_random_grid_FS (random.hpp:35-120) */
int bchmc_garfield_walk_index(uint32_t n, uint32_t i, uint32_t j, uint32_t k, uint64_t *index);
/* Hamiltonian_EoM + delta_Hamiltonian from the resident (q, p); terms as in bchmc_delta_hamiltonian.
 * The chain carries gradient_psi and -log L of its state from one attempt to the next: the last force evaluation of an
 * accepted trajectory (HMC.cc:349) is at the point where the next one starts, and a rejected attempt restarts from the
 * same point, so the evaluation of HMC.cc:279 is skipped from the second attempt on (same numbers to round-off;
 * bchmc_upload and bchmc_chain_set_state drop the carried values).  BCHMC_NO_FORCE_CARRY=1 re-evaluates every time. */
int bchmc_chain_attempt(bchmc_handle *h, double eps, uint64_t neps, double *dH, double terms[6], uint64_t *steps_done);
int bchmc_chain_get_proposal(bchmc_handle *h, double *q1, double *p1);
int bchmc_chain_accept(bchmc_handle *h, int accepted);         /* accepted: q := proposal (HMC.cc:497-498) */
/* measure_spectrum (barlib/src/field_statistics.cpp:20-90; callers barcoderunner.cc:328,532 -> dump_ps_it): binned
 * power spectrum of a field, n_bin bins of width |k|_max / n_bin.  `signal` = N host doubles, or NULL for the
 * resident chain state (no transform and no field transfer: its R2C is what the chain keeps).  kmode / power:
 * n_bin doubles each; empty bins stay 0 like upstream. */
int bchmc_measure_spectrum(bchmc_handle *h, const double *signal, uint64_t n_bin, double *kmode, double *power);
/* ---- correlation functions of a sample (upstream: tools/corr_fct.cc, tools/2D_corr_fct.cc on dumped fields) ----------
 * xi(r) and xi(r_perp, r_par) of a host field, of the resident chain state (no forward transform: its R2C is what the
 * chain keeps) or of the handle's deltaX (the Eulerian or redshift-space density of the last forward model), binned on
 * the device: A(r) = C2R[|R2C delta|^2] / N, rmax = L/2 sqrt(3), dr = rmax / n_bin, cell positions by
 * pacman_center_on_origin, bin indices (ULONG)(r / dr) with IEEE sqrt and divide and no FMA contraction, so that every
 * cell lands in the bin the host tool puts it in.  Per bin: rmode = mean 3-D distance, nmode = cells, corr = sum of A /
 * (nmode N); empty bins are 0.  n_bin: 1..2048.  Nx <= 1024 (BCHMC_ERR_UNSUPPORTED above).  rmode / nmode depend on the
 * grid and n_bin only and are kept in the handle per function, so repeated calls with one n_bin sum corr only.
 * Results are bitwise repeatable on every handle: the 2-D sums use no atomics and a fixed order, the 1-D sums are
 * exact-integer accumulations.  fp32 handles: transforms and A in float, bin sums as above.  A field that is not finite
 * gives NaN in every populated bin of corr (the host tool's sums would be NaN too); a zero field gives 0.
 * A measurement leaves the chain state, the momenta, the carried gradient and -log L, the uploaded inputs, deltaX / pos*
 * AND a pending proposal as they were (it uses the transfer staging and scratch arrays only).
 * Errors, checked before anything is queued: signal given with a source other than BCHMC_CORR_HOST, or missing with it,
 * n_bin out of range: BCHMC_ERR_ARG; no chain state, or no forward evaluation in the handle (where
 * bchmc_fetch(BCHMC_F_DELTAX) fails): BCHMC_ERR_STATE.
 * Two properties of the upstream tools:
 *  C1 (deviation) measure_corr_grid does not bound the bin index (its guard is commented out, corr_fct.cc:60-67).  The
 *     corner cell (n/2, n/2, n/2) has rtot == rmax and lands in bin n_bin exactly: upstream writes one element past
 *     rmode, corr and nmode.  The engine drops that cell, as measure_corr2D and measure_spectrum do with theirs.
 *  C2 (immaterial) absolute_squared_array(Signal, Signal) sets the real part only, so upstream's inverse transform sees
 *     |delta^|^2 + i Im delta^ and its A(r) carries the odd part (delta(r) - delta(-r)) / 2 of the field as well.  Every
 *     bin is symmetric under r -> -r, so the term cancels inside each bin; the engine transforms |delta^|^2 alone. */
typedef enum bchmc_corr_source {
  BCHMC_CORR_HOST = 0,        /* `signal`: N host doubles */
  BCHMC_CORR_CHAIN_STATE = 1, /* the resident chain state (deltaLAG); signal must be NULL */
  BCHMC_CORR_DELTAX = 2       /* the handle's deltaX (what bchmc_fetch(BCHMC_F_DELTAX) would return); signal must be NULL */
} bchmc_corr_source;
/* measure_corr_grid (tools/corr_fct.cc:20-80): rmode, corr: n_bin doubles; nmode: n_bin counts */
int bchmc_measure_corr(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *rmode,
                       uint64_t *nmode, double *corr);
/* measure_corr2D (tools/2D_corr_fct.cc:23-124), plane-parallel, line of sight = z (the axis rsd.cc:52-58 displaces):
 * arrays of n_bin * n_bin, element nbin_par + n_bin * nbin_perp */
int bchmc_measure_corr2d(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *rmode,
                         uint64_t *nmode, double *corr);
/* ---- the up-resolved 2-D correlation function (upstream: tools/2D_corr_fct_interp.cc, tools/interp_upres.cc) ------------
 * The tool lifts a field from the chain's n^3 grid to a finer n_out^3 one and runs measure_corr2D there.  Sources, their
 * errors and what a call leaves untouched are those of bchmc_measure_corr2d above (all checked before anything is queued).
 * n_out: 4..1024 (BCHMC_ERR_ARG outside: the 2-D slice kernel is laid out for <= 1024).  The fine grid -- a real n_out^3
 * array, a half-complex one, R2C / C2R plans at n_out in the handle's precision, interp_field's table and the 2-D bin
 * tables -- is built on first use, kept for the next call with the same n_out, replaced by a call with another one, and
 * freed by bchmc_upres_release and bchmc_destroy; bchmc_live_resources counts it.  If it cannot be allocated the call
 * returns the allocation's error, releases what it took and leaves the handle usable. */
/* interp_field (tools/interp_upres.cc:59-86): the source's n^3 field on an n_out^3 grid by interpolate_CIC
 * (interpolate_grid.cpp:27-103), cell pairs and weights in the reference's own double expressions, the eight terms in
 * its operand order without FMA contraction: bit for bit the tool's output on fp64 handles for a host source.  n_out < n
 * (down-sampling) is legal, as in the tool.  out: n_out^3 host doubles. */
int bchmc_interp_upres(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint32_t n_out, double *out);
/* tools/2D_corr_fct_interp.cc.  mode 0: interp_field, then its measure_corr2D (:66-174), which bins a cell only if
 * rpar < l_max && rperp < l_max (both strict); l_max must be > 0 (BCHMC_ERR_ARG otherwise, NaN included; +infinity: no
 * cut -- a small deviation: the tool writes all-zero output for l_max <= 0).  mode 1: measure_corr2D_FFTzeropad
 * (:177-312; l_max is ignored, as the tool ignores it); needs n_out >= n (BCHMC_ERR_ARG: the tool's index map folds onto
 * itself below).  Any other mode: BCHMC_ERR_ARG.  n_bin: 1..2048.  Arrays of n_bin * n_bin, element
 * nbin_par + n_bin * nbin_perp; rmode / nmode are kept with the bin tables per (n_out, n_bin, l_max-or-none).
 * Three properties of mode 1:
 *  U1 The tool sends its row i = n / 2 to frequency -n / 2 only, so for n_out > n the K = 0 plane it builds is not
 *     Hermitian; its complex-to-real transform returns the transform of the Hermitian part.  The engine writes that part,
 *     (P(I, J, 0) + P(-I, -J, 0)) / 2, and never hands the transform anything else: same numbers.
 *  U2 (immaterial) the i Im delta^ term of C2 above is dropped here too; it cancels inside every bin.
 *  U3 (kept) the tool normalises by N_out twice, so mode 1's corr is (N / N_out)^2 times the correlation function: a
 *     constant field c gives c^2 (n / n_out)^6 in every populated bin.  Kept bug for bug. */
int bchmc_measure_corr2d_interp(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint32_t n_out,
                                int32_t mode, double l_max, uint64_t n_bin, double *rmode, uint64_t *nmode, double *corr);
int bchmc_upres_release(bchmc_handle *h); /* frees the fine grid's buffers, plans and tables; later calls rebuild them */
/* measure_spectrum of any source (barcoderunner.cc:87 measures delta_eul): bchmc_measure_spectrum with the source enum,
 * its errors those of bchmc_measure_corr2d */
int bchmc_measure_spectrum_src(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin,
                               double *kmode, double *power);
/* ---- the anisotropic power spectrum P(k_perp, k_par) (upstream: tools/2D_powspec.cc on a dumped field) ------------------
 * measure_spec2D (tools/2D_powspec.cc:25-110), plane-parallel, line of sight = z (the axis rsd.cc:52-58 displaces): the
 * Fourier-space twin of bchmc_measure_corr2d.  kmax = sqrt(3) k_Nyquist, dk = kmax / (n_bin - 1); every mode of the full
 * complex grid goes to element nbin_par + n_bin * nbin_perp with nbin_perp = (ULONG)(sqrt(kx*kx + ky*ky) / dk) and
 * nbin_par = (ULONG)(sqrt(kz*kz) / dk), IEEE sqrt and divide and no FMA contraction, so that every mode lands in the bin
 * the host tool puts it in.  Per bin: kmode = mean |k|, nmode = modes, power = NORM sum |delta^|^2 / nmode with
 * NORM = L^3 / (4 pi) / N^2; empty bins are 0.  The sums run over the half-complex transform with the Hermitian weight
 * (1 for k = 0 and the Nyquist column of an even n, 2 otherwise): a mode and its conjugate partner share k_perp, k_par and
 * |k|, so this is the full-grid sum bin by bin.
 * Sources, their errors (all checked before anything is queued) and what a call leaves untouched are those of
 * bchmc_measure_corr2d above; the source's transform is obtained exactly as bchmc_measure_spectrum_src obtains it (the
 * chain state's q^ is used as it is, without a transform).  n_bin: 1..2048.  Nx <= 1024 (BCHMC_ERR_UNSUPPORTED above).
 * Arrays of n_bin * n_bin; nmode may be NULL (the tool does not return it).  kmode / nmode depend on the grid and n_bin
 * only: the bin tables and the sums of |k| are kept in the handle per n_bin (bchmc_live_resources counts the buffers,
 * bchmc_destroy frees them), so repeated calls with one n_bin sum the power only.  The sums use no atomics and a fixed
 * order: results are bitwise repeatable on every handle, which bchmc_measure_spectrum's are not.  fp32 handles: the
 * transform in float, |delta^|^2 and the sums in double.  A field that is not finite gives NaN power in every populated
 * bin (kmode and nmode are unaffected); a zero field gives 0.
 * Four properties of the upstream tool:
 *  S1 (kept) NORM carries a 1 / (4 pi) that measure_spectrum's L^3 / N^2 does not; upstream marks it "TODO: check"
 *     (2D_powspec.cc:32-35).  Kept bug for bug: the power of one field through the two entry points differs by that
 *     factor, apart from the binning.
 *  S2 (kept) dk = kmax / (n_bin - 1), not / n_bin as in measure_spectrum.  k_perp <= sqrt(2) k_Nyquist and
 *     k_par <= k_Nyquist are both below kmax, so the tool's bound test never fires: every mode is binned, sum nmode = N
 *     (unlike C1 there is no out-of-range cell), and the top perp bin and the top par bin are always empty.  With
 *     n_bin = 1, dk = +infinity and every mode lands in bin 0.
 *  S3 (immaterial) ky comes from calc_kz(j, L2, N2) (2D_powspec.cc:59); on a cubic box that is the same number.
 *  S4 kmode is the mean 3-D |k| of the bin's modes, not a (k_perp, k_par) pair. */
int bchmc_measure_spectrum2d(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *kmode,
                             uint64_t *nmode, double *power);
/* ---- the cross-spectrum of two fields (upstream: none; what a Barcode paper's reconstruction-against-truth figure is made
 * of, computed there from dumped fields) ------------------------------------------------------------------------------
 * Binning, dk, mode weights and normalisation are exactly those of bchmc_measure_spectrum_src (measure_spectrum,
 * field_statistics.cpp:20-90: (ULONG)(ktot / dk) with IEEE sqrt and divide and no FMA contraction, Hermitian weight on the
 * half-complex transforms, NORM = L^3 / N^2).  Per bin: kmode = mean |k|, nmode = modes (may be NULL), power_a / power_b =
 * what bchmc_measure_spectrum_src returns for each source, cross = NORM sum hw (re_a re_b + im_a im_b) / nmode, and
 * coeff = cross / sqrt(power_a power_b), formed on the host from those three arrays: 0 where the bin is empty or the
 * product is 0, NaN where it is NaN.  Six arrays of n_bin; empty bins are 0.  n_bin: 1..2048.
 * Each source's transform is obtained as bchmc_measure_spectrum_src obtains it (the chain state's q^ is used as it is);
 * all nine pairs of sources are legal, the same source twice and two host fields included.  One kernel reads both
 * transforms once.  The first call takes one more half-complex scratch array, which the handle keeps like the spectrum's
 * bins (bchmc_live_resources counts it, bchmc_destroy frees it).
 * Errors (all checked before anything is queued, for both sources) and what a call leaves untouched are those of
 * bchmc_measure_spectrum_src.  The sums use the float atomics of bchmc_measure_spectrum: results are NOT bitwise
 * repeatable, the last bits vary with the order in which the adds land.  fp32 handles: transforms in float, products and
 * sums in double. */
int bchmc_measure_cross_spectrum(bchmc_handle *h, bchmc_corr_source src_a, const double *signal_a,
                                 bchmc_corr_source src_b, const double *signal_b, uint64_t n_bin, double *kmode,
                                 uint64_t *nmode, double *power_a, double *power_b, double *cross, double *coeff);
/* ---- posterior mean and variance of an ensemble of samples (upstream: left to whoever reads the deltaLAG_<i> /
 * deltaEUL_<i> dumps of barcoderunner.cc:512-534) -----------------------------------------------------------------------
 * BCHMC_ENS_SLOTS independent running accumulators per handle (say deltaLAG, deltaEUL in real space, deltaEUL in redshift
 * space and a spare).  A slot is a count, kept on the host side of the handle, and two dense device arrays of N DOUBLES
 * on every handle, fp32 ones too: mean and m2, the sum of squared deviations from the mean, in the reference's cell order
 * k + n (j + n i).  The arrays are taken, zeroed on the handle's stream, by the slot's first add or merge, counted by
 * bchmc_live_resources (2 buffers, 16 N bytes per used slot) and freed by bchmc_ensemble_release and bchmc_destroy; if
 * they cannot be allocated the call returns the allocation's error, releases what it took and leaves the handle usable.
 * Eight properties:
 *  E1 add: one Welford step per cell from one sample of a source, in double, no FMA contraction, IEEE divide, in exactly
 *     this operand order with c = (double)(count + 1):  d = x - mean;  mean = mean + d / c;  m2 = m2 + d * (x - mean);
 *     so that the same lines in numpy float64 give the same bits.
 *  E2 Sources, their argument and state errors (checked before anything is queued) are those of bchmc_measure_corr2d.
 *     BCHMC_CORR_CHAIN_STATE: the real-space field bchmc_chain_get_state would return, through the same transform,
 *     without the copy to the host.  BCHMC_CORR_DELTAX: what bchmc_fetch(BCHMC_F_DELTAX) would return.  BCHMC_CORR_HOST:
 *     accumulated from the staged doubles, so an fp32 handle loses nothing of the array.  fp32 device sources are widened
 *     to double on load.
 *  E3 A call leaves the chain state, the momenta, the carried gradient and -log L, the uploaded inputs, deltaX / pos* AND a
 *     pending proposal as they were (the contract of bchmc_measure_corr).
 *  E4 A sample cell that is not finite (NaN or an infinity) makes that cell's mean and m2 NaN, for good, and touches no
 *     other cell.
 *  E5 fetch: BCHMC_ENS_MEAN needs count >= 1.  BCHMC_ENS_VARIANCE is m2 / (double)(count - 1), BCHMC_ENS_STD is
 *     sqrt(m2 / (double)(count - 1)) with IEEE sqrt and divide, computed on the device into the staging array; both need
 *     count >= 2.  BCHMC_ENS_M2 is the raw array (count >= 1); with the count and BCHMC_ENS_MEAN it is what another
 *     handle's merge takes.  BCHMC_ERR_STATE below those counts.  out: N host doubles.
 *  E6 merge folds another accumulator of the same grid -- another chain, another GPU, an earlier run read from disk -- into
 *     the slot by the pairwise update of Chan, Golub & LeVeque.  With na the slot's count and nb = count_b the host forms
 *     w = (double)nb / (double)(na + nb) and c = (double)na * (double)nb / (double)(na + nb), left to right, and the
 *     kernel does per cell, uncontracted:  d = mean_b - mean;  mean = mean + d * w;  m2 = (m2 + m2_b) + (d * d) * c.
 *     count_b == 0 is a no-op (the arrays may be NULL); a merge into an empty slot copies the two arrays bit for bit.  The
 *     arrays cross PCIe through the handle's staging, one after the other.
 *  E7 reset: count = 0, the arrays zeroed, the buffers kept.  release: every slot's buffers freed, every count 0.
 *  E8 Results are bitwise repeatable on every handle: no cell depends on another and nothing is added atomically.
 * slot outside 0 .. BCHMC_ENS_SLOTS - 1, an unknown quantity, a NULL array where one is needed: BCHMC_ERR_ARG. */
enum { BCHMC_ENS_SLOTS = 4 };
typedef enum bchmc_ens_what { BCHMC_ENS_MEAN = 0, BCHMC_ENS_VARIANCE = 1, BCHMC_ENS_STD = 2, BCHMC_ENS_M2 = 3 } bchmc_ens_what;
int bchmc_ensemble_add(bchmc_handle *h, int32_t slot, bchmc_corr_source src, const double *signal);
int bchmc_ensemble_count(bchmc_handle *h, int32_t slot, uint64_t *count);
int bchmc_ensemble_fetch(bchmc_handle *h, int32_t slot, bchmc_ens_what what, double *out);
int bchmc_ensemble_merge(bchmc_handle *h, int32_t slot, uint64_t count_b, const double *mean_b, const double *m2_b);
int bchmc_ensemble_reset(bchmc_handle *h, int32_t slot);   /* count = 0, arrays zeroed, buffers kept */
int bchmc_ensemble_release(bchmc_handle *h);               /* all slots: buffers freed, counts 0 */
/* ---- the cosmic web of a sample: the T-web (upstream: none; what the users of a density-posterior sampler of this family
 * make of its samples -- Hahn et al. 2007 for the classification, Forero-Romero et al. 2009 for the threshold, Leclercq,
 * Jasche & Wandelt 2015 for the posterior over an ensemble) ----------------------------------------------------------
 * Let x be the source field and x^ its half-complex transform, obtained as bchmc_measure_spectrum_src obtains it (the
 * chain state's q^ is used as it is).  Indices (i, j, k) belong to the axes (x, y, z); k_a = kval(index_a, n, kfac), the
 * wave numbers of every k-space kernel of the engine.  Ten properties:
 *  T1 Potential and tensor.  laplace(phi) = x and T_ab = d_a d_b phi:  T^_ab = (k_a k_b / k^2) W(k) x^, 0 at k = 0.
 *  T2 Smoothing.  W = exp(-k^2 R^2 / 2), upstream's Gaussian kernel (convolution.cpp:286); R = smoothing_scale >= 0 in
 *     Mpc/h, R = 0: none.
 *  T3 Nyquist rule, even n only.  An off-diagonal component (a != b) is zero wherever the index of axis a or of axis b is
 *     n / 2: there k_a k_b has opposite signs at a mode and at its conjugate partner, which is the same element.  The
 *     diagonal components keep those modes (k_a^2 is even).  So all six arrays are transforms of real fields and no C2R
 *     is handed a non-Hermitian plane (the concern of nyq_keep and of U1 above).  At odd n no mode is special.
 *  T4 Trace.  T_xx + T_yy + T_zz = x_s - mean(x_s) in every cell, x_s the smoothed field; the three eigenvalues sum to
 *     the same number.
 *  T5 Eigenvalues.  Per cell lambda_1 >= lambda_2 >= lambda_3, computed in double on every handle by cyclic Jacobi
 *     rotations (backward stable on degenerate tensors such as (lambda, 0, 0); a diagonal tensor returns its diagonal
 *     exactly).  The tensor arrays are of the handle's storage type and widened on load.
 *  T6 Type = the number of eigenvalues with lambda > lambda_th, strictly: 0 void, 1 sheet, 2 filament, 3 knot.  A cell
 *     whose tensor is not finite gets type 255 and NaN eigenvalues, and counts in n_nonfinite only.
 *  T7 Statistics.  n_type: cells per type, exact.  mass_type: the sum of 1 + x over the type's cells, x the UNSMOOTHED
 *     source in real space (BCHMC_CORR_HOST: the staged doubles; BCHMC_CORR_CHAIN_STATE: the field
 *     bchmc_chain_get_state would return; BCHMC_CORR_DELTAX: what bchmc_fetch(BCHMC_F_DELTAX) would return), summed in
 *     double in a fixed order: per-workgroup partials, then one ordered reduction, no float atomics.  All outputs of a
 *     call are bitwise repeatable on every handle.
 *  T8 Posterior accumulator.  Four uint32 counters per cell, type-major (16 N bytes), taken zeroed by the first
 *     accumulating call or merge.  accumulate = 1 adds 1 to the counter of each cell's type and 1 to the sample count, in
 *     a pass of its own over the device-resident type map after the statistics have been read back; if
 *     n_nonfinite > 0 that pass is not launched and the call returns BCHMC_ERR_ARG naming the count, with lambda, type
 *     and stats written all the same.  The accumulator remembers the (smoothing_scale, lambda_th) of the first sample a
 *     classify put in; an accumulating call with another pair is BCHMC_ERR_STATE until bchmc_tweb_reset (a merge brings
 *     counters, not their parameters: keeping those equal across chains is the caller's).  bchmc_tweb_fetch returns the
 *     counters of one type (N uint32) or, as_probability != 0, (double)count / (double)samples with IEEE divide (N
 *     doubles).  bchmc_tweb_merge adds another chain's 4 N counters; integer addition is exact and associative, so any
 *     merge order gives the same bits.  n_b + samples >= 2^32: BCHMC_ERR_ARG; n_b == 0: a no-op (counts_b may be NULL).
 *  T9 Sources, their argument and state errors, and what a call leaves untouched -- the chain state, the momenta, the
 *     carried gradient and -log L, the uploaded inputs, deltaX / pos* and a pending proposal -- are those of
 *     bchmc_measure_corr2d.  Everything is checked before anything is queued.  Also BCHMC_ERR_ARG: opts NULL,
 *     smoothing_scale negative or not finite, lambda_th not finite, accumulate other than 0 / 1, component outside
 *     0..5, type outside 0..3.  BCHMC_ERR_STATE: bchmc_tweb_tensor before any classify, bchmc_tweb_fetch with
 *     as_probability and samples == 0.  Any Nx bchmc_create accepts works, odd ones included.
 *  T10 Buffers.  The feature owns the six real arrays of T (storage type; bchmc_tweb_tensor returns one of the last
 *     classify as doubles), the N-byte type map, a few hundred words of partial sums, at most one half-complex array
 *     (none for the chain state), 3 N doubles of eigenvalue staging once a caller has asked for lambda, and the
 *     accumulator; otherwise it uses the handle's transfer staging and scratch.  Each is built on first use and kept;
 *     bchmc_live_resources counts them, bchmc_tweb_release and bchmc_destroy free them (release also empties the
 *     accumulator).  If one cannot be allocated the call returns the allocation's error, releases what it took and
 *     leaves the handle usable.
 * lambda: 3 N doubles, the lambda_1 block, then lambda_2, then lambda_3, or NULL.  type: N bytes or NULL.  stats or NULL.
 * (Added within ABI version 4: no struct or existing entry point changed.) */
typedef struct bchmc_tweb_opts  { double smoothing_scale, lambda_th; int32_t accumulate, reserved0; } bchmc_tweb_opts;
typedef struct bchmc_tweb_stats { uint64_t n_type[4], n_nonfinite; double mass_type[4]; } bchmc_tweb_stats;
int bchmc_tweb_classify(bchmc_handle *h, bchmc_corr_source src, const double *signal, const bchmc_tweb_opts *opts,
                        double *lambda /* 3 N or NULL */, uint8_t *type /* N or NULL */, bchmc_tweb_stats *stats /* or NULL */);
int bchmc_tweb_tensor(bchmc_handle *h, int32_t component /* 0..5 = xx, xy, xz, yy, yz, zz */, double *out /* N */);
int bchmc_tweb_samples(bchmc_handle *h, uint64_t *n);
int bchmc_tweb_fetch(bchmc_handle *h, int32_t type /* 0..3 */, int32_t as_probability, void *out /* N uint32, or N double */);
int bchmc_tweb_merge(bchmc_handle *h, uint64_t n_b, const uint32_t *counts_b /* 4 N, type-major */);
int bchmc_tweb_reset(bchmc_handle *h);     /* samples = 0, counters zeroed, buffers kept */
int bchmc_tweb_release(bchmc_handle *h);   /* every buffer of the feature freed, samples = 0 */
/* ---- the bispectrum of a sample (upstream: none; the FFT estimator of Scoccimarro 2015 and Sefusatti et al. 2016: the
 * third test of a reconstruction after P(k) and r(k) -- deltaLAG under the Gaussian prior should have none, deltaX should
 * carry the tree-level bispectrum of the data) -------------------------------------------------------------------------
 * Let x be the source field and x^ its half-complex transform, obtained as bchmc_measure_spectrum_src obtains it (the
 * chain state's q^ is used as it is).  Wave numbers are kval(index, n, kfac); |k| = sqrt(kx kx + ky ky + kz kz) with IEEE
 * sqrt and divide and no FMA contraction, as bchmc_measure_spectrum forms it.  N = n^3, L the box side.  Ten properties:
 *  B1 Shells.  k_min >= 0 and dk > 0 in h/Mpc, n_shell in 1..32.  A mode with |k| >= k_min belongs to shell
 *     s = (ULONG)((|k| - k_min) / dk) if s < n_shell, else to none; the mode k = 0 belongs to none whatever k_min is.  The
 *     shell depends on |k| only, so every filtered array is the transform of a real field, Nyquist planes of an even n
 *     included, and no C2R is handed a non-Hermitian plane.  lo(s) = k_min + s dk, hi(s) = k_min + (s + 1) dk.
 *  B2 Shell fields.  D_s = C2R[x^ 1_s] and I_s = C2R[1_s], unnormalised inverse transforms, arrays of the storage type.
 *  B3 Triplets.  All (s1, s2, s3) with s1 <= s2 <= s3 in lexicographic order, T = n_shell (n_shell + 1) (n_shell + 2) / 6
 *     <= 5984.  S_t = sum over cells of D_s1 D_s2 D_s3; ntri_t = sum over cells of I_s1 I_s2 I_s3 / N, the number of
 *     ordered mode triples (k1, k2, k3) of the three shells that close; B_t = (L^3)^2 / N^3 * S_t / (N ntri_t).  (sum over
 *     cells of D1 D2 D3 = N times the sum of x^1 x^2 x^3 over closed triangles, and B is V^2 / N^3 times its mean:
 *     consistent with the L^3 / N^2 of bchmc_measure_spectrum.)  Triangles close modulo the grid, k1 + k2 + k3 = 0 mod n
 *     per axis, as in every FFT estimator: a caller who wants true triangles only keeps k_min + n_shell dk <= 2/3 k_Nyquist,
 *     k_Nyquist = pi n / L.  The call does not refuse other shells.
 *  B4 Empty triplets.  If k_min + n_shell dk <= 2/3 k_Nyquist, a triplet with lo(s3) >= hi(s1) + hi(s2) (evaluated in
 *     double as written) cannot hold a triangle and is not computed: ntri = 0, B = 0.  Every other triplet is computed; if
 *     its ntri < 0.5 then B = 0 and Q = 0.  ntri is returned as a double.  On an fp64 handle rint(ntri) is the exact count
 *     wherever (N + 18 log2(n)) 2^-53 M^2 < 1/2, M the largest nmode of the three shells: |I_s| <= M and
 *     ||I_s||_2 = sqrt(N M_s), each I_s carries the error of one C2R and the sum that of N terms (tests/bispec_bound.py);
 *     that covers every shell of grids up to 32^3 and shells of up to 7 10^4 modes at 96^3.
 *  B5 Per shell.  nmode: the exact count of full-grid modes (a stored mode counts for itself and its conjugate partner);
 *     kmean: their mean |k|; power: L^3 / N^2 * sum hw |x^|^2 / nmode.  One k-space pass, per-workgroup partials and one
 *     ordered reduction, no float atomics.  Empty shells give 0.
 *  B6 Reduced bispectrum.  Q_t = B_t / (P1 P2 + P2 P3 + P3 P1) from the returned B and power; 0 where the denominator is 0
 *     or the triplet is empty (not computed, or ntri < 0.5), NaN where it is NaN.
 *  B7 Determinism.  Everything is summed in double on every handle and in a fixed order: a lane's cells in order, one
 *     lane per triplet and workgroup, then one ordered reduction over the workgroups.  All outputs are bitwise
 *     repeatable.  On an fp32 handle the transforms, D_s and I_s are float; products and sums are double.
 *  B8 Non-finite fields.  A field that is not finite gives NaN in B of every computed triplet with ntri >= 0.5 and in
 *     power of every populated shell; nmode, kmean and ntri do not depend on the field.  A zero field gives 0.  (Narrower
 *     than "every computed triplet": a computed triplet with ntri < 0.5 holds no triangle and B4 sets its B to 0 whatever
 *     the field is; B4 takes precedence.)
 *  B9 Sources, their argument and state errors, and what a call leaves untouched -- the chain state, the momenta, the
 *     carried gradient and -log L, the uploaded inputs, deltaX / pos* and a pending proposal -- are those of
 *     bchmc_measure_corr2d.  Everything is checked before anything is queued.  Also BCHMC_ERR_ARG: opts NULL, k_min
 *     negative or not finite, dk <= 0 or not finite, n_shell outside 1..32, b NULL.  Any Nx bchmc_create accepts works,
 *     odd ones included.
 *  B10 Buffers.  The feature owns n_shell real arrays of the storage type, the partial sums (workgroups x T doubles, at
 *     most 512 workgroups), the table of the T triangle sums and at most one half-complex array (none for the chain
 *     state); otherwise it uses the handle's transfer staging and scratch.  I_s and ntri depend on (grid, k_min, dk,
 *     n_shell) only: the table is built by the first call and kept, a call with other shells replaces it, so a later
 *     sample costs n_shell filter + C2R passes and one contraction.  bchmc_live_resources counts every buffer,
 *     bchmc_bispec_release and bchmc_destroy free them.  If one cannot be allocated the call returns the allocation's
 *     error, releases what it took and leaves the handle usable.
 * b: T doubles.  ntri, q: T doubles or NULL.  kmean, power: n_shell doubles or NULL.  nmode: n_shell or NULL.
 * (Added within ABI version 4: no struct or existing entry point changed.) */
typedef struct bchmc_bispec_opts { double k_min, dk; int32_t n_shell, reserved0; } bchmc_bispec_opts;
int bchmc_bispectrum(bchmc_handle *h, bchmc_corr_source src, const double *signal, const bchmc_bispec_opts *opts,
                     double *b /* T */, double *ntri /* T or NULL */, double *q /* T or NULL */,
                     double *kmean /* n_shell or NULL */, uint64_t *nmode /* n_shell or NULL */, double *power /* n_shell or NULL */);
int bchmc_bispec_release(bchmc_handle *h);   /* every buffer of the feature freed */
/* ---- RSD multipoles of a sample: P_l(k) and xi_l(s), l = 0, 2, 4 (upstream: none; computed there from dumped fields; the
 * compressed form of the maps bchmc_measure_spectrum2d and bchmc_measure_corr2d return) -----------------------------------
 * Line of sight = z, the axis rsd.cc:52-58 displaces; plane-parallel only.  With mu^2 = z^2 / (x^2 + y^2 + z^2) of a mode's
 * wave vector or a cell's separation:  L_0 = 1,  L_2 = 1.5 mu^2 - 0.5,  L_4 = (35 mu^4 - 30 mu^2 + 3) / 8, evaluated in
 * double in exactly this operand order without FMA contraction.  Nine properties:
 *  M1 Fourier space.  Bins, dk, mode weights and normalisation are exactly those of bchmc_measure_spectrum_src: bin
 *     (ULONG)(ktot / dk), ktot = sqrt(kx kx + ky ky + kz kz) with IEEE sqrt and divide and no FMA contraction, dk =
 *     |k|_max / n_bin, Hermitian weight hw on the half-complex transform, NORM = L^3 / N^2 (not the 1 / (4 pi) of S1).
 *     kmode = mean |k| of the bin's modes, nmode = full-grid modes (may be NULL),
 *     p[l / 2][b] = (2 l + 1) NORM sum hw |x^|^2 L_l(mu) / nmode[b], laid out [3][n_bin], l-major.
 *  M2 leg[0][b], leg[1][b] = the mean of L_2 and of L_4 over the bin's modes, laid out [2][n_bin]: the leakage of the
 *     discrete mu into l = 2, 4, which a caller subtracts to correct low-k bins.  kmode, nmode and leg depend on the grid
 *     and n_bin only and are kept in the handle per form for the last n_bin.
 *  M3 The mode k = 0 (the cell r = 0) has no mu: it counts in l = 0, kmode and nmode exactly as measure_spectrum
 *     (measure_corr) counts it and contributes 0 to l = 2, 4 and to leg.
 *  M4 Cross form.  p_aa, p_bb: what bchmc_measure_multipoles returns for each source, bit for bit; p_ab: the same with the
 *     summand re_a re_b + im_a im_b (the imaginary parts of a mode and its partner cancel, as in
 *     bchmc_measure_cross_spectrum).  All nine pairs of sources are legal; with the same source twice the three are equal
 *     bit for bit.  One pass reads both transforms once.
 *  M5 Configuration space.  A(r) is exactly the grid bchmc_measure_corr builds; cell coordinates by
 *     pacman_center_on_origin, rmax = L/2 sqrt(3), dr = rmax / n_bin, bin (ULONG)(rtot / dr), the corner cell with
 *     rtot == rmax dropped (C1).  xi[l / 2][b] = (2 l + 1) sum A L_l / (nmode[b] N); rmode, nmode, leg as above.  Auto only.
 *  M6 Empty bins are 0.  A source that is not finite gives NaN in every populated bin of every l (of p_ab too if either
 *     source is not finite); kmode, rmode, nmode and leg do not depend on the field.  A zero field gives 0.
 *  M7 Determinism.  No atomics and a fixed order: rows that share the whole column of (ktot, mu) against kz -- the up to
 *     eight (i, j) with the same unordered pair of |frequencies| -- are summed first, in ascending row order; then each bin
 *     over those classes and ascending kz by a fixed partition and tree; everything in double.  All outputs are bitwise
 *     repeatable on every handle, run to run and call to call, which bchmc_measure_spectrum's are not.  fp32 handles:
 *     transforms in float, products and sums in double.
 *  M8 Sources, their argument and state errors, and what a call leaves untouched -- the chain state, the momenta, the
 *     carried gradient and -log L, the uploaded inputs, deltaX / pos* and a pending proposal -- are those of
 *     bchmc_measure_corr2d, checked before anything is queued, for both sources of the cross form.  Also BCHMC_ERR_ARG: a
 *     NULL array other than nmode, n_bin outside 1..2048.  Nx <= 1024 (BCHMC_ERR_UNSUPPORTED above).  Odd grids and the
 *     smallest ones are accepted.
 *  M9 Buffers.  The feature owns the class tables of the grid (48 bytes per class, (n/2 + 1)(n/2 + 2) / 2 classes), the
 *     class sums (classes x (n/2 + 1) doubles per sum: 8.7 MB at 256, 0.54 GB at 1024; three sums once the cross form
 *     has run -- accepted inside the Nx limit, not chunked), the partial sums of the bins and at most one half-complex
 *     array (only when the cross form's first source needs a transform); otherwise it uses the handle's transfer staging
 *     and scratch.  Each is taken on first use and kept; bchmc_live_resources counts them, bchmc_multipoles_release and
 *     bchmc_destroy free them.  If one cannot be allocated the call returns the allocation's error, releases every buffer
 *     of the feature and leaves the handle usable.
 * (Added within ABI version 4: no struct or existing entry point changed.) */
int bchmc_measure_multipoles(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *kmode,
                             uint64_t *nmode /* or NULL */, double *leg /* [2][n_bin] */, double *p /* [3][n_bin] */);
int bchmc_measure_cross_multipoles(bchmc_handle *h, bchmc_corr_source src_a, const double *signal_a,
                                   bchmc_corr_source src_b, const double *signal_b, uint64_t n_bin, double *kmode,
                                   uint64_t *nmode /* or NULL */, double *leg, double *p_aa, double *p_bb, double *p_ab);
int bchmc_measure_corr_multipoles(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint64_t n_bin, double *rmode,
                                  uint64_t *nmode /* or NULL */, double *leg /* [2][n_bin] */, double *xi /* [3][n_bin] */);
int bchmc_multipoles_release(bchmc_handle *h);   /* every buffer of the feature freed */
/* ---- a particle catalogue onto the grid (upstream: getDensity_NGP / _CIC / _TSC / _SPH, massFunctions.cc:49-495, as
 * tools/density.cc, tools/poisson_upres.cc and Lag2Eul.cc:117-126 call them) ---------------------------------------------
 * The raw density of a free list of n_part particles -- no overdens, no normalisation -- on the handle's grid, L and
 * min1..3, by the masskernel opts->mk, assigned on the device.  n_part has nothing to do with N: the catalogue crosses
 * PCIe in batches of 2^20 particles, so the device memory of a call does not grow with it; n_part = 0 gives a zero field.
 * Seven properties:
 *  D1 Domain test.  NGP, CIC and SPH keep a particle with min <= x < min + L on every axis; TSC's test is closed above
 *     (massFunctions.cc:195: x == min + L is kept and lands in cell 0).  A non-finite coordinate fails both.  stats->n_in /
 *     n_lost count the particles that passed / failed the test of the kernel in force.
 *  D2 Cell index.  NGP and TSC: floor((x - min) / d) mod n.  CIC: getCICcells / getCICweights, the coordinate shifted by
 *     d / 2 and folded, min not subtracted.  SPH: (ULONG)(x / d) without min, cell centres at (ix + 0.5) d
 *     (massFunctions.cc:434-440) -- each exactly as the handle's own scatter of the same mk treats it.  SPH with a
 *     negative min is refused (BCHMC_ERR_UNSUPPORTED): upstream's cast of a negative double is undefined.
 *  D3 Weights.  weightmass = 0: every particle counts 1 (tools/density.cc, poisson_upres.cc; for NGP and TSC, which always
 *     read Par_mass upstream, a mass array of ones).  weightmass = 1: w[p] is upstream's `mass` (Lag2Eul.cc), any sign.
 *  D4 Precision.  fp64 handles: double throughout.  fp32 handles: the positions are converted to float first (the domain
 *     test, the cell and the weights see the float's value), the arithmetic is that of the handle's own direct kernels of
 *     the mk (double, the CIC / TSC products rounded to float once); every handle accumulates in double, in LDS and on
 *     the grid, and `out` is not rounded to float (the nobs of dest = BCHMC_F_NOBS is, like an uploaded array).
 *  D5 Deterministic handles accumulate in 64-bit fixed point, scale 2^46 / (max|w| x the largest kernel value: W(0) for
 *     SPH, 1 otherwise), and convert each cell once: `out` is bitwise equal across calls, across
 *     bchmc_catalogue_release, across handles and under any permutation of the catalogue.  A cell whose RUNNING sum
 *     passes 2^16 maximal contributions in magnitude makes THIS call return BCHMC_ERR_STATE, with nothing written to out
 *     or nobs: every add to the grid is looked at as it lands, so that no count of particles can wrap the 64-bit sum
 *     unseen.  With weights of one sign the running sum never exceeds the final one and the answer depends on the data
 *     alone; with both signs a cell whose partial sums can pass the limit while its final sum does not (|S_c| below,
 *     A_c = sum |w W| above 2^16 max|w| times the kernel's largest value) may be refused in one order of arrival and
 *     accepted in another -- the field, when one is returned, is the same bits either way.
 *     Other handles use hardware float atomics: last bits vary with the order, like the reference's OpenMP build.
 *  D6 What a call leaves alone: the chain state, the momenta, a pending proposal, deltaX, rho, Psi, pos* and the record
 *     slots of the trajectory (it uses the transfer staging and buffers of its own).  dest = BCHMC_F_NOBS invalidates
 *     exactly what bchmc_upload(BCHMC_F_NOBS) invalidates -- the carried gradient and -log L -- and nothing more.
 *  D7 Where the handle has a tile partition and min is 0, the particles are sorted by the tile of their home cell and a
 *     tile's records are cut into work items of bounded length, so a cell holding any number of particles is spread over
 *     many workgroups; stats->max_per_tile is the largest tile population of a batch (of the catalogue up to 2^20
 *     particles; beyond that it depends on how the catalogue's order spreads a tile over the batches).  Otherwise (odd
 *     Nx, min != 0, an SPH scale length whose halo does not fit) one thread per particle adds to the grid directly, in
 *     the same arithmetic, and max_per_tile is 0.  SPH at h = d (any h whose stencil hull is the standard 81-cell one)
 *     visits the 81 cells of the hull with the folded spline of the handle's own tile kernels, on either path; other scale lengths
 *     walk upstream's (2 reach + 1)^3 cube.
 * BCHMC_PART_FORWARD with mk = 1 on an SPH handle is tools/LAG2EULer.cc's output for the handle's cosmology (its ascale
 * argument is the handle's ascale and D1).
 * The buffers (bchmc_live_resources counts them) are built by the first call, kept for the next, and freed by
 * bchmc_catalogue_release and bchmc_destroy.
 * Refused before anything is queued, the handle untouched: x, y or z NULL with BCHMC_PART_HOST, or any of x, y, z, w given
 * with BCHMC_PART_FORWARD; weightmass = 1 with w == NULL; weightmass other than 0 / 1; mk outside -1..3; kernel_h
 * negative, not finite or above L / 4; dest other than -1 or BCHMC_F_NOBS; out == NULL with dest == -1; n_part > 2^31 - 1;
 * a non-finite weight (found by a threaded pass over w on the host, which also yields max|w|, before the device sees
 * the call) -- all BCHMC_ERR_ARG;
 * BCHMC_PART_FORWARD when no forward model has run: BCHMC_ERR_STATE. */
typedef enum { BCHMC_PART_HOST = 0,     /* x, y, z (and w) are host arrays of n_part doubles */
               BCHMC_PART_FORWARD = 1   /* the handle's own particles after the last forward model: the positions
                                           bchmc_fetch(BCHMC_F_POSX..Z) would return; x, y, z, w must be NULL */
} bchmc_part_source;

typedef struct bchmc_density_opts {
  int32_t mk;            /* 0 NGP, 1 CIC, 2 TSC, 3 SPH; -1: the handle's mk */
  int32_t weightmass;    /* 0: every particle counts 1 (w ignored, may be NULL); 1: w[p] */
  double  kernel_h;      /* SPH scale length; 0: the handle's particle_kernel_h.  Refused above L / 4 */
  int32_t dest;          /* -1: host array `out` only; BCHMC_F_NOBS: also becomes the handle's nobs, as if uploaded */
  int32_t reserved0;
} bchmc_density_opts;

typedef struct bchmc_density_stats {
  uint64_t n_in, n_lost;     /* passed / failed the kernel's own domain test (non-finite positions are lost) */
  uint64_t max_per_tile;     /* largest tile population met in one batch of 2^20 particles (0 on the direct path) */
} bchmc_density_stats;

int bchmc_density_particles(bchmc_handle *h, bchmc_part_source src, const double *x, const double *y, const double *z,
                            const double *w, uint64_t n_part, const bchmc_density_opts *opts, double *out /* N or NULL */,
                            bchmc_density_stats *stats /* or NULL */);
int bchmc_catalogue_release(bchmc_handle *h);   /* frees the catalogue buffers; a later call rebuilds them */

/* ---- interpolate_CIC / interpolate_TSC / interpolate_TSC_multi of a free particle catalogue (interpolate_grid.cpp:82-120,
 * 134-202, 207-286; HMC_models_unused.cpp:22-25 reads deltaX, nobs, noise and window this way) --------------------------
 * One to four grid fields read at the positions of n_part particles, on the device: the reverse direction of
 * bchmc_density_particles.  out[f * n_part + p] is field f at particle p.  Seven properties:
 *  I1 Positions.  BCHMC_PART_HOST: host columns, which cross PCIe in the catalogue's batches of 2^20 particles; the results
 *     return batch by batch, so the device memory of a call does not grow with n_part.  BCHMC_PART_FORWARD: the handle's
 *     own particles after the last forward model (x, y, z NULL, n_part = N; out[f * N + p] belongs to lattice particle p).
 *     Neither interpolator takes min1..3 upstream: coordinates are box coordinates whatever the handle's min is.
 *     On fp32 handles a position is converted to float first; the domain test, the cells and the weights see the float's
 *     value (D4 of bchmc_density_particles).
 *  I2 Fields.  BCHMC_CORR_HOST: `host`, N doubles, held as the handle's storage type like an uploaded array.
 *     BCHMC_CORR_CHAIN_STATE: the real-space field bchmc_chain_get_state returns.  BCHMC_CORR_DELTAX and
 *     BCHMC_INTERP_HANDLE_FIELD: what bchmc_fetch of BCHMC_F_DELTAX / of `field` would return at that moment (PSIX..Z,
 *     VX..Z, RHO, PART_LIKE, the uploaded NOBS / NOISE / WINDOW and the rest), with bchmc_fetch's own errors.  The
 *     sources are staged once per call into n_fields grid arrays the feature owns.  Several fields in one call are
 *     interpolate_TSC_multi, or several interpolate_CICs: one set of cells and weights per particle serves all of them.
 *  I3 Arithmetic.  Double, the reference's expressions in its operand order, no FMA contraction.  CIC: getCICcells /
 *     getCICweights with both folds of pacman_coordinate, the eight terms of :92-99 each as F * a * b * c left to right,
 *     summed in source order.  TSC: :142-188, the 27 terms in i, j, k order as wx[i] * wy[j] * wz[k] * field, with
 *     wx[2] and wy[2] computed from dz as upstream computes them (:166-167).  A field value is read in the storage type
 *     and widened; `out` is never rounded to float.
 *  I4 Domain.  CIC folds: every finite coordinate is in.  TSC upstream casts xp / d to unsigned without a test (undefined
 *     below 0, past the array from cell n on): a particle is kept if 0 <= x and (unsigned)(x / d) < n on every axis --
 *     x < L is not enough (n = 9, L = 1: the double below 1.0 lands in cell 9).  A non-finite coordinate is lost under
 *     either kernel.  A lost particle gets a quiet NaN in every field of `out` and counts in stats->n_lost, the others
 *     in n_in.
 *  I5 No result depends on another particle, on the path, on the batch or on the order inside a tile, and nothing is
 *     added atomically to a result: every handle, deterministic or not, returns the same bits.
 *  I6 What a call leaves alone: the chain state, the momenta, a pending proposal, deltaX, rho, Psi, pos*, the carried
 *     gradient and -log L, and the record slots (it uses the transfer staging and buffers of its own, none of the
 *     catalogue's: bchmc_catalogue_release and bchmc_interp_release are independent, in either order).
 *  I7 Paths.  opts->path = 1: the particles of a batch are binned by the tile of their home cell (cell_index1 for CIC,
 *     the particle's cell for TSC), a tile's records are cut into work items of bounded length, and a work item reads the
 *     fields from an LDS image of tile plus halo; stats->max_per_tile is the largest tile population of a batch.
 *     path = 0: one thread per particle reads the grid, in the same arithmetic; max_per_tile is 0.  path = -1: the engine
 *     decides (interp_plan.hpp; DESIGN 9.8 has the figures behind the rule).  stats->path_used says which one ran.
 * The buffers (bchmc_live_resources counts them) are built by the first call, kept for the next, and freed by
 * bchmc_interp_release and bchmc_destroy.  n_part = 0 succeeds and writes nothing.
 * Refused before anything is queued, the handle usable: opts NULL; kernel other than 1 / 2; path outside -1..1; n_fields
 * outside 1..BCHMC_INTERP_MAX_FIELDS; fields NULL; a BCHMC_CORR_HOST field without its array, or an array given with
 * another source; an unknown source or bchmc_field; out NULL with n_part > 0; a NULL column with BCHMC_PART_HOST; a column
 * given, or n_part != N, with BCHMC_PART_FORWARD; n_part > 2^31 - 1 -- all BCHMC_ERR_ARG.  No chain state, no forward
 * evaluation for a field or for BCHMC_PART_FORWARD, a never-uploaded input: BCHMC_ERR_STATE.  path = 1 on a handle
 * without a tile partition (odd Nx; bchmc_tile_info): BCHMC_ERR_UNSUPPORTED. */
enum { BCHMC_INTERP_MAX_FIELDS = 4 };
enum { BCHMC_INTERP_HANDLE_FIELD = 3 };  /* a source beside the three of bchmc_corr_source: `field` names a bchmc_field */
typedef struct bchmc_interp_field {
  int32_t source;      /* bchmc_corr_source (HOST, CHAIN_STATE, DELTAX), or BCHMC_INTERP_HANDLE_FIELD = 3 */
  int32_t field;       /* a bchmc_field when source is BCHMC_INTERP_HANDLE_FIELD, else ignored */
  const double *host;  /* N doubles for HOST, NULL otherwise */
} bchmc_interp_field;
typedef struct bchmc_interp_opts {
  int32_t kernel;      /* 1 CIC, 2 TSC (the mk numbering) */
  int32_t path;        /* -1 the engine decides; 0 direct kernel; 1 tile kernel (BCHMC_ERR_UNSUPPORTED where the handle has no tiles) */
  int32_t reserved[2];
} bchmc_interp_opts;
typedef struct bchmc_interp_stats { uint64_t n_in, n_lost, max_per_tile; int32_t path_used, reserved; } bchmc_interp_stats;

int bchmc_interp_particles(bchmc_handle *h, bchmc_part_source psrc, const double *x, const double *y, const double *z,
                           uint64_t n_part, const bchmc_interp_field *fields, int32_t n_fields,
                           const bchmc_interp_opts *opts, double *out /* n_fields * n_part, field-major */,
                           bchmc_interp_stats *stats /* or NULL */);
int bchmc_interp_release(bchmc_handle *h);   /* frees the interpolation buffers; a later call rebuilds them */
/* Lag2Eul of the resident chain state: bchmc_forward without the host array (it starts from the chain's q^, so no field
 * crosses PCIe and no transform pair is spent).  use_rsd as there.  Leaves deltaX / pos* in the handle, synchronises and
 * adapts the binning's record slots like bchmc_forward; drops a pending proposal like it.  The chain state, the momenta
 * and the carried gradient / -log L are untouched.  With bchmc_fetch this gives dump_deltas' arrays
 * (IOfunctionsGen.cc:136-171): deltaRSS from use_rsd = 1, deltaEUL from use_rsd = 0. */
int bchmc_chain_forward(bchmc_handle *h, int use_rsd);
/* Hamiltonian_mass (HMC_mass.cc:315-368; HamiltonianMC calls it at HMC.cc:387-423) for the handle's mass_type. */
typedef struct bchmc_mass_opts {
  uint64_t n_bin;               /* HAMIL_NUMERICAL::N_bin (types 2, 3); 1..2048 like bchmc_measure_spectrum */
  double mass_factor;           /* HAMIL_NUMERICAL::mass_factor */
  uint64_t iGibbs, s_eps_total; /* type 60's switch */
} bchmc_mass_opts;
/* Hamiltonian_mass at `signal` (N host doubles, or NULL = resident chain state).  The handle then uses the new mass
 * exactly as if it had been uploaded; mass_f / mass_r (may be NULL) receive host copies of what was built (an array the
 * type has none of is left untouched).  Does not touch the chain's q, momenta, carried gradient or -log L; drops a
 * pending proposal like bchmc_forward.  deltaX / pos* afterwards: the likelihood force's forward model (types 2, 3),
 * Lag2Eul(signal) (5, 6, 60 after its switch), unchanged otherwise.  Types 2 and 3 with the GRF likelihood:
 * BCHMC_ERR_UNSUPPORTED (upstream's likelihood_grad_log_like is an empty function there). */
int bchmc_hamiltonian_mass(bchmc_handle *h, const double *signal, const bchmc_mass_opts *opts, double *mass_f,
                           double *mass_r);
/* ---- the start of a run: load_initial_fields (barcoderunner.cc:284-344) with random_test = true --------------------
 * setup_random_test (:42-205) and make_initial_guess (:207-247) on the device, from the SAME GSL mt19937 state the chain
 * later draws its momenta from: mt / mti in: the state before the call, out: what GSL holds after it (the convention of
 * bchmc_chain_draw_momenta_mt19937, so the three calls chain).  words_used may be NULL. */
typedef struct bchmc_mock_opts {
  int32_t window_type;      /* 1 ones, 10 zeros in the first N/2 cells, 23 one where delta_eul > 3 (:91-113, upstream's
                             * code, not its comment); anything else BCHMC_ERR_ARG */
  int32_t data_model;       /* 0 linear, 1 log-normal (:117-188); anything else BCHMC_ERR_ARG */
  int32_t negative_obs;     /* 0: nobs of the Gaussian likelihood is clamped at 0 (:140-142) */
  int32_t random_test_rsd;  /* 1: Lag2Eul_rsd_zeldovich whatever sfmodel says, 0: Lag2Eul(sfmodel), never RSD (:67-82) */
  double sigma_min, sigma_fac;
} bchmc_mock_opts;
/* Needs signal_PS uploaded (it is upstream's o->Power).  Stream order: 2 N Gaussians for create_GARFIELD in the walk of
 * resolution_independent_random_grid_FS, then ONE gsl_ran_gaussian(sigma_i) per cell with window > 0 in cell order and
 * none for the others (with window_type 23 that count depends on the forward model, so the noise is a second stream
 * draw sized after an 8-byte read-back).  Per cell, Lambda as upstream: Gaussian likelihood sigma = sigma_min +
 * sigma_fac Lambda, nobs = Lambda + g, clamped at 0 unless negative_obs; GRF likelihood sigma = sigma_min + sigma_fac
 * delta_lag^2, nobs = delta_lag + g; data_model 1: Lambda = lognormal_likelihood_f_delta_x_i_calc, sigma = sigma_fac,
 * nobs of an unwindowed cell = log((rho_c (1 + delta_min))^2).  g = sigma * y * sqrt(-2 log r2 / r2), products in GSL's
 * order, no FMA contraction.  noise of an unwindowed cell is 0 (upstream leaves it unwritten).
 * Afterwards window, nobs and noise are in the handle exactly as if they had been uploaded (bchmc_fetch reads them);
 * the carried gradient / -log L and a pending proposal are dropped; deltaX / pos* are those of the truth; delta_lag /
 * delta_eul (may be NULL) receive the truth and its forward model (dump_deltas' arrays).  The chain state is untouched.
 * Refused before anything is queued or the generator is touched: data_model 0 with the log-normal likelihood
 * (BCHMC_ERR_ARG, upstream's text, :156), and data_model 0 with the Poissonian likelihood (BCHMC_ERR_UNSUPPORTED):
 * gsl_ran_poisson consumes a data-dependent number of words per cell through the rejection loops of gsl_ran_gamma_int /
 * gsl_ran_binomial, so where cell i starts in the stream depends on every earlier cell's draw -- not a scan with
 * bounded state.  After the draw: a windowed cell with noise == 0 under likelihood 1 or 3 -> BCHMC_ERR_STATE naming the
 * first such index (:190-198); the generator has then advanced like upstream's, the three arrays count as not uploaded.
 * Odd Nx: BCHMC_ERR_UNSUPPORTED, refused like the two cases above (create_GARFIELD's walk is defined for even Nx). */
int bchmc_setup_random_test(bchmc_handle *h, const bchmc_mock_opts *o, uint32_t mt[624], int32_t *mti,
                            uint64_t *words_used, double *delta_lag, double *delta_eul);
/* make_initial_guess: sets the resident chain state like bchmc_chain_set_state.  initial_guess 0: zero; 1: file_field (N
 * host doubles); 2: create_GARFIELD(signal_PS) from the stream, placed in k-space directly; 3: the same, then
 * kernelcomp(smoothing_scale, smoothing_type) o convcomp as one k-space multiply (type 1, the Gaussian kernel, only;
 * others BCHMC_ERR_ARG); 4: N draws gsl_ran_gaussian(r, 0.1) in cell order.  Cases 0 and 1 leave the generator as it is
 * (mt / mti may be NULL) and report 0 words.  Odd Nx: 2 and 3 return BCHMC_ERR_UNSUPPORTED before anything is queued
 * (create_GARFIELD's walk), generator and chain state untouched; 0, 1 and 4 work at any Nx. */
int bchmc_make_initial_guess(bchmc_handle *h, int32_t initial_guess, const double *file_field, int32_t smoothing_type,
                             double smoothing_scale, uint32_t mt[624], int32_t *mti, uint64_t *words_used);
/* ---- Poisson samples of a density field (upstream: discrete_poisson_sample, tools/poisson_upres.cc:23-65, and the
 * Poissonian mock of setup_random_test, barcoderunner.cc:117-131) -------------------------------------------------------
 * gsl_ran_poisson consumes a data-dependent number of words of a serial stream, which no parallel form reproduces.  Like
 * bchmc_chain_draw_momenta, these entry points draw from a counter-based Philox4x32-10 stand-in instead -- here exact in
 * distribution: the count of cell c = k + n (j + n i) of an n_in^3 rate grid is a pure function of (seed, stream, c,
 * lambda_c), whatever the launch shape, the handle's kind or its precision.  Eight properties:
 *  P1 Uniforms, k_white_noise's convention.  r = philox4x32_10((c_lo, c_hi, j, 2 stream), (seed_lo, seed_hi)),
 *     u = (((r.x << 32 | r.y) >> 11) + 0.5) 2^-53, v the same from r.z, r.w; j is the iteration.  stream < 2^31.
 *  P2 Rate.  rate_mode 0: lambda = scale (1 + x) (poisson_upres.cc:127's Nbar (1 + delta), barcoderunner.cc:125's
 *     rho_c (1 + delta_eul)); 1: lambda = scale x.  x is read in the storage type and widened, the product is formed in
 *     double, uncontracted.  use_window = 1: a cell whose handle window is not > 0 gets count 0 and draws nothing
 *     (barcoderunner.cc:126, 160).  lambda <= 0 (and -infinity): 0, as GSL.  A NaN, a +infinity or a lambda above 2^30
 *     refuses the call with BCHMC_ERR_ARG naming the first such cell index: nothing is written to counts or made nobs,
 *     and the handle holds no sample afterwards (an earlier one is gone: the draw had taken its buffers).
 *  P3 0 < lambda < 10: inversion by sequential search with j = 0 and u only:
 *       p = exp(-lambda); s = p; k = 0;  while (u > s && k < 256) { k++; p = p * lambda / (double)k; s = s + p; }
 *     (the cap is there because u can round to 1.0).
 *  P4 lambda >= 10: Hoermann's PTRS (1993).  b = 0.931 + 2.53 sqrt(lambda), a = -0.059 + 0.02483 b,
 *     1/alpha = 1.1239 + 1.1328 / (b - 3.4), v_r = 0.9277 - 3.6224 / (b - 2).  Per iteration j = 0, 1, ...: U = u - 0.5,
 *     us = 0.5 - |U|, k = floor((2 a / us + b) U + lambda + 0.43); accept if us >= 0.07 && v <= v_r; retry if k < 0 ||
 *     (us < 0.013 && v > us); otherwise accept iff log v + log(1/alpha) - log(a / us^2 + b) <= -lambda + k log lambda -
 *     lgamma(k + 1).  At most 64 iterations.  All of it in double, uncontracted, in this operand order: the same lines in
 *     numpy float64 give the same counts except where a decision is closer than the last bits of exp / log / lgamma.
 *     stats->n_capped counts the cells that ran into either cap (they return the last candidate); expected 0.
 *  P5 The resident sample.  The handle keeps the exclusive 64-bit scan off[0 .. n_in^3] of the counts, (seed, stream,
 *     n_in, n_part) and d_in = L / n_in -- 8 bytes per cell, nothing per particle.  Particle p lies in the cell c with
 *     off[c] <= p < off[c + 1], found by an upper-bound search that steps over runs of empty cells, at index
 *     kk = p - off[c]; its position is upstream's (:52-58) with gsl_rng_uniform's 32-bit resolution:
 *     x = d_in (double)i + ((double)w.x 2^-32) d_in, y from w.y and j, z from w.z and k,
 *     w = philox4x32_10((c_lo, c_hi, kk, 2 stream + 1), seed), uncontracted, in box coordinates (min is not added, as in
 *     the tool).  Particle order is upstream's: cells in order, kk within a cell.
 *  P6 bchmc_poisson_draw.  Sources, their argument and state errors: bchmc_measure_corr2d's.  BCHMC_CORR_HOST: n_in in
 *     1..Nx, `signal` = n_in^3 doubles (staged in the lower half of the transfer staging and read as doubles on every
 *     handle); device sources: n_in = 0 or Nx.  use_window = 1 and dest = BCHMC_F_NOBS need n_in == Nx (BCHMC_ERR_ARG),
 *     use_window = 1 an uploaded window (BCHMC_ERR_STATE).  counts (may be NULL): n_in^3 doubles.  dest = BCHMC_F_NOBS
 *     does to the handle exactly what bchmc_upload(BCHMC_F_NOBS) of the counts would.  A draw replaces the resident
 *     sample and leaves alone what D6 of bchmc_density_particles lists.  The buffers are counted by
 *     bchmc_live_resources and freed by bchmc_poisson_release and bchmc_destroy; after an allocation failure the handle
 *     holds no sample and stays usable.  Also BCHMC_ERR_ARG: opts NULL, stream >= 2^31, rate_mode or use_window other
 *     than 0 / 1, a scale that is not finite, dest other than -1 / BCHMC_F_NOBS.
 *  P7 bchmc_poisson_positions: particles [first, first + m) of the resident sample as doubles on every handle --
 *     discrete_poisson_sample's list in batches of the caller's own size.  first + m > n_part, or a NULL column with
 *     m > 0: BCHMC_ERR_ARG; no sample: BCHMC_ERR_STATE; m = 0 succeeds.
 *  P8 bchmc_poisson_density: the resident sample onto the handle's grid through the catalogue's pipeline, batch by batch,
 *     the columns filled on the device: no position crosses PCIe.  With mk = 1 this is poisson_upres.cc end to end.
 *     Options, refusals, properties D1-D7 and stats are those of bchmc_density_particles with weightmass = 0;
 *     weightmass = 1: BCHMC_ERR_ARG; n_part > 2^31 - 1: BCHMC_ERR_ARG; no sample: BCHMC_ERR_STATE.
 * Not built: GSL's own Poisson stream, per-particle weights, a device pointer to the positions, n_in > Nx.
 * (Added within ABI version 4: no struct or existing entry point changed.) */
typedef struct bchmc_poisson_opts {
  uint64_t seed;
  uint32_t stream;       /* < 2^31 */
  int32_t rate_mode;     /* 0: lambda = scale (1 + x); 1: lambda = scale x */
  double scale;
  int32_t use_window;    /* 1: cells whose window is not > 0 draw nothing */
  int32_t dest;          /* -1, or BCHMC_F_NOBS: the counts also become the handle's nobs, as if uploaded */
} bchmc_poisson_opts;
typedef struct bchmc_poisson_stats {
  uint64_t n_part, n_cells_drawn, max_count, n_capped;  /* particles, cells with lambda > 0 inside the window, ... */
  double lambda_max;                                    /* over the cells that drew (0: none did) */
} bchmc_poisson_stats;
int bchmc_poisson_draw(bchmc_handle *h, bchmc_corr_source src, const double *signal, uint32_t n_in,
                       const bchmc_poisson_opts *opts, double *counts /* n_in^3 or NULL */,
                       bchmc_poisson_stats *stats /* or NULL */);
int bchmc_poisson_positions(bchmc_handle *h, uint64_t first, uint64_t m, double *x, double *y, double *z);
int bchmc_poisson_density(bchmc_handle *h, const bchmc_density_opts *opts, double *out /* N or NULL */,
                          bchmc_density_stats *stats /* or NULL */);
int bchmc_poisson_release(bchmc_handle *h);   /* frees the sample and its scratch; a later draw rebuilds them */
/* bchmc_setup_random_test with data_model = 0 on a likelihood = 0 handle, the case it refuses: the 2 N Gaussians of the
 * truth come from the caller's mt19937 state, so the truth, its forward model and the window are bit for bit those of
 * bchmc_setup_random_test and the generator advances by those words only; then nobs = the sampler above at
 * scale = rho_c, rate_mode 0, use_window = 1 of the truth's deltaX under (seed, stream), 0 outside the window, and noise
 * is 0 everywhere (upstream leaves it unwritten).  The three arrays count as uploaded; the resident sample of
 * bchmc_poisson_draw is left alone.  Any other likelihood or data_model: BCHMC_ERR_ARG; stream >= 2^31: BCHMC_ERR_ARG;
 * all other refusals, and their order, are those of bchmc_setup_random_test.
 * One refusal comes after the draw, like bchmc_setup_random_test's noise == 0: a cell inside the window whose
 * rho_c (1 + delta_eul) is NaN, +infinity or above 2^30 -> BCHMC_ERR_ARG naming the first such index.  The generator has
 * then advanced by the truth's words, delta_lag / delta_eul and words_used are written, deltaX / pos* are the truth's and
 * the window is built, but window, nobs and noise count as not uploaded and nobs and noise are as they were.
 * (Added within ABI version 4: no struct or existing entry point changed.) */
int bchmc_setup_random_test_poisson(bchmc_handle *h, const bchmc_mock_opts *o, uint32_t mt[624], int32_t *mti,
                                    uint64_t *words_used, uint64_t seed, uint32_t stream, double *delta_lag,
                                    double *delta_eul);
int bchmc_philox_kat(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]); /* known-answer hook for tests */

/* Diagnostic (tests, logs): how the particle-mesh path is currently set up.  out = { tile-sorted path in use, one-pass
 * binning in use, record slots per tile in use, record slots per tile allocated, long trajectories poll the slot words,
 * tile shape in cells tx | ty << 8 | tz << 16 (0 without tiles), unrolled 81-cell kernels in use, ALPT planes pipeline
 * available }. */
int bchmc_tile_info(bchmc_handle *h, int32_t out[8]);

/* Diagnostic (tests): what all handles and communicators of this process hold on the device right now.  out = { device
 * buffers, their bytes, pinned host buffers, other objects (events, streams, rocFFT plans and execution infos) }; every
 * count returns to its earlier value when what was created in between has been destroyed. */
int bchmc_live_resources(uint64_t out[4]);

/* Diagnostic (tests, diagnostics): the particle stage of the forward model from a displacement given in real space
 * instead of from a field.  psi: 3 N host doubles, the x, y and z components one after the other; particle i starts at
 * the centre of lattice cell i and is displaced by (psi[i], psi[N + i], psi[2 N + i]) (particle_pos, Lag2Eul.cc), so a
 * test can put every particle at a place of its choice.  psi is converted to the handle's field type and then takes
 * exactly the path a forward model takes after the C2R of its displacement, with the handle's state as it is: tile
 * binning into the record slots, the two-pass sort and the sub-cell ordering after an overflow, mass assignment (every
 * masskernel, tiles or not, deterministic or not), sum of rho.  use_rsd as in bchmc_forward.
 * with_force != 0: then the likelihood force of that density from the uploaded nobs / noise / window (all inputs must
 * have been uploaded as for bchmc_gradient: BCHMC_ERR_STATE otherwise; GRF likelihood: BCHMC_ERR_UNSUPPORTED) up to,
 * and excluding, the transform to k-space that ends it: partial_f_delta_x_log_like and, for calc_h 0 / 2 / 3, V.
 * Ends like bchmc_forward: synchronises and adapts the binning's record slots; a pending proposal and the chain's
 * carried gradient / -log L are dropped; the chain state and the momenta are untouched.  Afterwards bchmc_fetch gives
 * POS*, PSI*, RHO, DELTAX and, after with_force, PART_LIKE and V* of this evaluation.
 * Not reachable through it: the fused z pass + binning of the trajectory steps at 128^3 and above (k_zbin_direct),
 * which takes Psi^ from k-space.  Its binning half is an implementation of its own (a hash table of 4 Nx slots that can
 * run full, keyed on pairs of counters whose two counts share one 64-bit word, one 64-bit global reservation per pair);
 * bchmc_probe_displacement_z below reaches it, tests/test_gpu_zbin_positions.py holds it to the same bounds.
 * (Added within ABI version 4: no struct or existing entry point changed.) */
int bchmc_probe_displacement(bchmc_handle *h, const double *psi, int use_rsd, int with_force);

/* Diagnostic (tests): the same through the fused z pass + binning (k_zbin_direct), the binning of every force evaluation
 * at 256^3 and 512^3 (at 128^3 under BCHMC_ZBIN_128=1).  psi, use_rsd and with_force as above.  psi is converted to the
 * handle's field type, scaled by 1 / Nx (exact: Nx is a power of two here) and transformed along z by k_zr2c into the
 * layout the engine's y pass leaves behind; then the particle stage runs as in a trajectory, with the engine's own
 * k_zbin_direct launches.  store_psi != 0: the variant that stores Psi on the way, as the evaluations at the ends of a
 * trajectory do (PSI* and POS* can be fetched; Psi is what the kernel used: psi after the z round trip, bitwise psi where
 * psi is constant along each z row).  store_psi == 0: the interior-step variant, followed by the launch that returns at
 * once unless a segment overflowed and then writes Psi for the two-pass sort (PSI* / POS* are meaningful after an
 * overflow only).  Ends like bchmc_probe_displacement.
 * BCHMC_ERR_UNSUPPORTED, naming the reason, wherever the engine itself would not take this path (Nx other than 256 / 512
 * / 128 with BCHMC_ZBIN_128=1, masskernel != 3 or calc_h != 2, no tile binning, BCHMC_NO_ZBIN=1); then nothing is
 * queued and the handle's state is as before, a pending proposal included.
 * (Added within ABI version 4: no struct or existing entry point changed.) */
int bchmc_probe_displacement_z(bchmc_handle *h, const double *psi, int use_rsd, int with_force, int store_psi);

/* ---- measurement hooks (bench.py): per-kernel-class HIP-event timing on the engine's stream ---- */
enum {
  BCHMC_K_FFT_C2R = 0, BCHMC_K_FFT_R2C, BCHMC_K_KSPACE_DRIFT_ZA, BCHMC_K_SCATTER, BCHMC_K_MEAN_PARTIAL,
  BCHMC_K_GATHER, BCHMC_K_KSPACE_FORCE_KICK, BCHMC_K_SORT, BCHMC_K_OTHER, BCHMC_K_COUNT
};
int bchmc_profile(bchmc_handle *h, int enable);                 /* 1: record events around every launch */
int bchmc_profile_read(bchmc_handle *h, double ms[BCHMC_K_COUNT], uint64_t launches[BCHMC_K_COUNT]); /* and reset */
const char *bchmc_kernel_name(int kernel_class);

/* ---- cross-chain step-size statistics -------------------------------------------------------
 * Chains are independent (one per GPU); the only exchange on the path is this record, one per finished attempt,
 * so that every chain's acceptance / epsilon tables (acc_flag_N_a, epsilon_N_a: struct_main.h:172-173, written by
 * update_epsilon_acc_rate_tables, time_step.cpp:187-203, read by update_eps_fac, :151-185) fill world_size times
 * faster.  A chain that never calls bchmc_eps_exchange behaves exactly like the single-chain reference. */
typedef struct bchmc_eps_record {
  double epsilon;
  int32_t accepted;
  int32_t neps;
} bchmc_eps_record;

/* Records one rank contributes per exchange.  The exchange happens ONCE PER SAMPLE (a fixed point every rank
 * reaches the same number of times), never per attempt: the attempt loop ends at a data-dependent iteration, so a
 * per-attempt collective would pair up records of different samples and deadlock the rank with more rejections.
 * A sample with more attempts than this sends the rest with the next exchange(s). */
#define BCHMC_EPS_BATCH 32
#define BCHMC_UNIQUE_ID_BYTES 128 /* sizeof(ncclUniqueId) */

typedef struct bchmc_comm bchmc_comm;
/* Transport used by a custom communicator: all-gather `bytes_per_rank` bytes of host memory from every rank into
 * `recv` (world * bytes_per_rank, rank order).  Returns 0 on success.  (MPI_Allgather in an MPI-launched barcode;
 * an in-process stub in the CPU tests.) */
typedef int (*bchmc_allgather_fn)(void *ctx, const void *send, void *recv, size_t bytes_per_rank);

/* RCCL transport: rank 0 calls bchmc_comm_unique_id and hands the 128 bytes to the other ranks (a file, an
 * environment variable, MPI_Bcast: the shim's bootstrap helper uses a file), then every rank
 * calls bchmc_comm_create: ncclCommInitRank on `device`, a side stream and a 2 x world x 520-byte staging buffer.
 * librccl is loaded on first use (dlopen), so single-chain runs do not depend on it.  On failure *out still holds an
 * object (bchmc_comm_last_error tells why); release it with bchmc_comm_destroy like a working one. */
int bchmc_comm_unique_id(unsigned char id[BCHMC_UNIQUE_ID_BYTES]);
int bchmc_comm_create(const unsigned char id[BCHMC_UNIQUE_ID_BYTES], int rank, int world, int device, bchmc_comm **out);
int bchmc_comm_create_custom(bchmc_allgather_fn fn, void *ctx, int rank, int world, bchmc_comm **out);
void bchmc_comm_destroy(bchmc_comm *c);
const char *bchmc_comm_last_error(const bchmc_comm *c);
/* One exchange (ncclAllGather of 520 bytes per rank on the side stream): queue `n_mine` (>= 0) records of this rank,
 * send the oldest <= BCHMC_EPS_BATCH queued ones, and return every rank's contribution in rank order, the own one
 * included: all[0 .. *n_all - 1], rank_of[i] = contributing rank of all[i] (rank_of may be NULL).  `cap` = capacity of
 * `all`, at least world * BCHMC_EPS_BATCH (checked before anything is sent).  Every rank of the communicator must call
 * it the same number of times.  Failure semantics: a call that returns non-zero has queued nothing of `mine` on this
 * rank -- retry with the same records, or drop them; after a TRANSPORT failure (the collective itself broke) the
 * communicator is no longer usable: the peers may or may not have completed the all-gather. */
int bchmc_eps_exchange(bchmc_comm *c, const bchmc_eps_record *mine, int n_mine, bchmc_eps_record *all, int *rank_of,
                       int cap, int *n_all);
int bchmc_comm_pending(const bchmc_comm *c); /* own records still queued for a later exchange */
int bchmc_comm_world(const bchmc_comm *c);   /* ranks of the communicator (sizes the caller's `all` / `rank_of`) */
int bchmc_comm_rank(const bchmc_comm *c);
const char *bchmc_comm_transport(const bchmc_comm *c); /* "rccl", "custom" or "none" (one rank, nothing to move) */

#ifdef __cplusplus
}
#endif
#endif /* BCHMC_H */
