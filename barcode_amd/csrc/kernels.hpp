// kernels.hpp -- HIP kernels of the bchmc engine (gfx950 / CDNA4, wave64).
//
// State lives in Fourier space: qk = R2C[q], pk = R2C[p] (unnormalised forward transforms, half-complex
// n x n x (n/2+1), z fastest).  Everything that is diagonal in k (prior force S^-1 q, drift M^-1 p, the
// Zel'dovich displacement kernel, the inverse-Laplacian-divergence of V, kicks) is done pointwise on those
// arrays; only the particle-mesh part (displace, SPH scatter, likelihood partials, SPH-gradient gather)
// runs in real space.  Reference lines restated by each kernel are cited at the kernel.
//
// Every kernel is a template on T, the STORAGE type of the field arrays (double = reference DOUBLE_PREC,
// float = BASELINE config 5).  k-space arithmetic, k-vectors, reductions and the per-cell likelihood are always
// done in double; the particle-mesh kernels (positions, spline evaluations, LDS accumulation) compute in T.
#pragma once
#include "common.hpp"

#include "kspace_step.hpp"  // Conversions, spectrum multipliers, first-step kick + drift + Zel'dovich kernel
#include "forward_model.hpp"  // Particle positions, SPH mass assignment (direct kernels), mean density, likelihood partials, direct SPH-gradient gather
#include "kspace_force.hpp"  // Force assembly, fused step boundary, rollback, Parseval energies, element-wise helpers, GRF likelihood
#include "variants.hpp"  // NGP / CIC / TSC mass assignment and the calc_h 0 / 3 likelihood-force variants
#include "rng.hpp"  // Philox4x32-10 momentum draw
#include "mt_draw.hpp"  // draw_momenta from the caller's GSL mt19937 stream: jump-ahead segments, polar pairs, walk placement
#include "tiles.hpp"  // Tile-sorted particle-mesh path: binning, scan, LDS scatter / gather kernels
#include "tiles_low.hpp"  // NGP / CIC / TSC mass assignment and calc_h = 3's TSC interpolation on the same records
#include "catalogue.hpp"  // bchmc_density_particles: a free, weighted particle catalogue onto the grid (count, scan, fill, LDS scatter, direct)
#include "interp_particles.hpp"  // bchmc_interp_particles: grid fields read at a free particle catalogue (count, fill, LDS gather, direct)
#include "alpt.hpp"  // ALPT displacement (Lag2Eul_non_zeldovich)
#include "spectrum.hpp"  // measure_spectrum
#include "corr.hpp"  // measure_corr_grid / measure_corr2D: |x^|^2, integer LDS histogram (1-D), sorted-row slices (2-D)
#include "spec2d.hpp"  // measure_spec2D: sorted-row slices over chunks of k, Hermitian-weighted reduce
#include "cross_spectrum.hpp"  // bchmc_measure_cross_spectrum: k_spectrum over two transforms at once
#include "ensemble.hpp"  // bchmc_ensemble_*: Welford and Chan updates of a running mean and m2, variance / standard deviation
#include "tweb.hpp"  // bchmc_tweb_*: tidal-tensor components in k-space, Jacobi eigenvalues and web type per cell, posterior counters
#include "bispec.hpp"  // bchmc_bispectrum: per-shell statistics of x^, the shell filter, the triple contraction over cells and its ordered reduce
#include "multipoles.hpp"  // bchmc_measure_*multipoles: sums over classes of rows that share a column of |k| and mu, ordered shell sums weighted by L_0, L_2, L_4
#include "upres.hpp"  // interp_field (CIC gather onto another grid) and the zero-padded power spectrum of 2D_corr_fct_interp.cc
#include "mock.hpp"  // setup_random_test / make_initial_guess: window, rank of windowed cells on the stream, noise, guesses
#include "poisson.hpp"  // bchmc_poisson_*: Poisson counts of a rate grid (inversion / PTRS on Philox uniforms), their scan, particle positions
#include "mass.hpp"  // Hamiltonian_mass: element-wise masses and the Jasche+13 first-order diagonal
#include "step_boundary_x.hpp"  // Planes mode: step boundary with the x passes of both transforms fused in
#include "alpt_x.hpp"  // Planes mode of the ALPT displacement: mix + cell-boundary average with the x passes fused in
#include "zpass.hpp"  // Planes mode: the y and z passes of the inverse transform by the engine, the z pass ending in the binning
