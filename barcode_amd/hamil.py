"""Host-side mirror of the reference's interface for the leapfrog path, on top of the C ABI.

Same names, argument meaning and bookkeeping as ``barlib/src/HMC.cc`` so that callers (and tests) read
like the reference: ``Hamiltonian_EoM``, ``delta_Hamiltonian``, ``gradient_psi``, ``kinetic_term``, ``psi``
operate on a ``HamilData`` (the reference's ``HAMIL_DATA`` + ``HAMIL_NUMERICAL``).  The arithmetic all
happens in ``libbarcode_hip.so``; this layer only draws (Neps, epsilon), forwards arrays and stores the
scalars the reference keeps for its performance log (``HMC.cc:40-60``).
"""
from dataclasses import dataclass

import numpy as np

from .engine import Engine


@dataclass
class HamilNumerical:
    """The per-attempt scalars of HAMIL_NUMERICAL (struct_hamil.h:86-92, 101-105)."""
    N_eps_fac: float = 8.0
    eps_fac: float = 0.0
    Neps: int = 0
    epsilon: float = 0.0
    accepted: bool = False
    dH: float = 0.0
    dK: float = 0.0
    dE: float = 0.0
    dprior: float = 0.0
    dlikeli: float = 0.0
    psi_prior: float = 0.0
    psi_likeli: float = 0.0
    psi_prior_i: float = 0.0
    psi_prior_f: float = 0.0
    psi_likeli_i: float = 0.0
    psi_likeli_f: float = 0.0
    H_kin_i: float = 0.0
    H_kin_f: float = 0.0
    steps_done: int = 0
    count_attempts: int = 0
    iGibbs: int = 1        # sample number (struct_hamil.h:106): scheme 3's fast initial phase runs while it is 1
    rejections: int = 0    # rejected attempts of the current sample (HMC.cc:500-501)
    # read by Hamiltonian_mass (struct_hamil.h:81-119; defaults data/input.par:129,150)
    N_bin: int = 200
    mass_factor: float = 1.0
    s_eps_total: int = 0   # mass_type 60: ones while iGibbs < s_eps_total, the Jasche mass afterwards


class HamilData:
    """HAMIL_DATA: parameters + input arrays bound to one engine handle (one chain, one GPU)."""

    def __init__(self, params, device=0, N_eps_fac=8.0, eps_fac=None, **arrays):
        self.params = params
        self.engine = Engine(params, device=device)
        self.numerical = HamilNumerical(N_eps_fac=N_eps_fac,
                                        eps_fac=params.eps_heuristic() if eps_fac is None else eps_fac)
        self.gradpsi = None
        if arrays:
            self.engine.upload(**arrays)

    # hd->deltaX / hd->pos*: state of the last force or energy evaluation
    @property
    def deltaX(self):
        return self.engine.fetch("deltaX")

    def pos(self):
        return tuple(self.engine.fetch(k) for k in ("posx", "posy", "posz"))


def Hamiltonian_EoM(hd, signali, momentai, uniform):
    """HMC.cc:251-369.  ``uniform`` stands for ``gsl_rng_uniform(seed)``; it is called exactly twice, in the
    reference's order (Neps first, then epsilon; HMC.cc:260-261)."""
    n = hd.numerical
    n.Neps = int(n.N_eps_fac * uniform()) + 1
    n.epsilon = float(n.eps_fac * uniform())
    if n.epsilon > 2.0:
        n.epsilon = 2.0
    # one pass: the trajectory and the six energy terms of its four arrays (bchmc_leapfrog_dh), kept for the
    # delta_Hamiltonian that HamiltonianMC calls next about the same arrays (HMC.cc:455-459; the C++ shim does the same)
    signalf, momentaf, done, dH, t = hd.engine.leapfrog_dh(signali, momentai, n.epsilon, n.Neps)
    hd._eom = ((signali, momentai, signalf, momentaf), dH, t)
    n.steps_done = done
    n.count_attempts += 1  # data->numerical->count_attempts++ (HMC.cc:368)
    return signalf, momentaf


def gradient_psi(hd, signal):
    """HMC.cc:146-206: fills hd.gradpsi."""
    hd.gradpsi = hd.engine.gradient(signal)
    return hd.gradpsi


def kinetic_term(hd, momenta, signal=None):
    """HMC.cc:64-121.  The engine evaluates all three energy terms in one call; ``signal`` defaults to zeros."""
    q = np.zeros(hd.engine.N) if signal is None else signal
    return float(hd.engine.energies(q, momenta)[0])


def psi(hd, signal, momenta=None):
    """HMC.cc:124-143: returns psi_prior + psi_likelihood and stores both in hd.numerical."""
    p = np.zeros(hd.engine.N) if momenta is None else momenta
    e = hd.engine.energies(signal, p)
    hd.numerical.psi_prior, hd.numerical.psi_likeli = float(e[1]), float(e[2])
    return float(e[1] + e[2])


def delta_Hamiltonian(hd, signali, momentai, signalf, momentaf):
    """HMC.cc:209-248, including the performance-log bookkeeping."""
    n = hd.numerical
    kept, hd._eom = getattr(hd, "_eom", None), None  # one use, only as the next call about the very same arrays
    if kept is not None and all(a is b for a, b in zip(kept[0], (signali, momentai, signalf, momentaf))):
        dH, t = kept[1], kept[2]
    else:
        dH, t = hd.engine.delta_hamiltonian(signali, momentai, signalf, momentaf)
    n.H_kin_i, n.psi_prior_i, n.psi_likeli_i = (float(x) for x in t[:3])
    n.H_kin_f, n.psi_prior_f, n.psi_likeli_f = (float(x) for x in t[3:])
    n.psi_prior, n.psi_likeli = n.psi_prior_f, n.psi_likeli_f
    n.dprior = n.psi_prior_f - n.psi_prior_i
    n.dlikeli = n.psi_likeli_f - n.psi_likeli_i
    n.dK = n.H_kin_f - n.H_kin_i
    n.dE = (n.psi_prior_f + n.psi_likeli_f) - (n.psi_prior_i + n.psi_likeli_i)
    n.dH = float(dH)
    return n.dH


def measure_spectrum(hd, signal=None, N_bin=200):
    """field_statistics.cpp:20-90 -> (kmode, power).  ``signal`` None = the resident chain state (what
    barcoderunner.cc:530-533 measures after every sample, without moving the field off the device)."""
    return hd.engine.measure_spectrum(signal, N_bin)


def measure_corr_grid(hd, signal=None, N_bin=0, source=None):
    """tools/corr_fct.cc:20-80 -> (rmode, nmode, corr).  ``signal`` None = the resident chain state, or with
    ``source="deltaX"`` the density of the last forward model; ``N_bin`` 0 = the tools' automatic bin count."""
    return hd.engine.measure_corr(signal, N_bin, source)


def interp_field(hd, N_out, signal=None, source=None):
    """tools/interp_upres.cc:59-86 -> the field on an N_out^3 grid (CIC interpolation)."""
    return hd.engine.interp_upres(N_out, signal, source)


def measure_corr2D_interp(hd, N_out, signal=None, N_bin=0, interp_mode=0, L_max=float("inf"), source=None, planepar=True):
    """tools/2D_corr_fct_interp.cc -> (rmode, nmode, corr) shaped (N_bin, N_bin) of the field lifted to N_out^3:
    ``interp_mode`` 0 CIC interpolation with the ``L_max`` cut, 1 zero padding of the power spectrum."""
    if not planepar:
        raise RuntimeError("non-plane-parallel option not yet implemented")  # 2D_corr_fct_interp.cc:120
    return hd.engine.measure_corr2d_interp(N_out, signal, N_bin, interp_mode, L_max, source)


def measure_corr2D(hd, signal=None, N_bin=0, source=None, planepar=True):
    """tools/2D_corr_fct.cc:23-124 -> (rmode, nmode, corr) shaped (N_bin, N_bin), r_perp first."""
    if not planepar:
        raise RuntimeError("non-plane-parallel option not yet implemented")  # 2D_corr_fct.cc:75
    return hd.engine.measure_corr2d(signal, N_bin, source)


def measure_spec2D(hd, signal=None, N_bin=200, source=None, planepar=True):
    """tools/2D_powspec.cc:25-110 -> (kmode, nmode, power) shaped (N_bin, N_bin), k_perp first.  ``signal`` None = the
    resident chain state, or with ``source="deltaX"`` the density of the last forward model."""
    if not planepar:
        raise RuntimeError("non-plane-parallel option not yet implemented")  # 2D_powspec.cc:71
    return hd.engine.measure_spectrum2d(signal, N_bin, source)


def measure_cross_spectrum(hd, signal_a=None, signal_b=None, N_bin=200, source_a=None, source_b=None):
    """The cross-spectrum of two fields in measure_spectrum's bins -> (kmode, nmode, power_a, power_b, cross, coeff).  A
    side without a signal is the resident chain state, or with ``source_*="deltaX"`` the density of the last forward
    model: reconstruction against truth without a field leaving the device but the truth."""
    return hd.engine.measure_cross_spectrum(signal_a, signal_b, N_bin, source_a, source_b)


def ensemble_add(hd, slot, signal=None, source=None):
    """One more sample into running accumulator ``slot`` of the posterior mean and variance: ``signal`` None = the
    resident chain state, or with ``source="deltaX"`` the density of the last forward model."""
    hd.engine.ensemble_add(slot, signal, source)


def ensemble_fetch(hd, slot, what="mean"):
    """``"mean"``, ``"variance"``, ``"std"`` or ``"m2"`` of accumulator ``slot`` -> N values."""
    return hd.engine.ensemble_fetch(slot, what)


def tweb_classify(hd, signal=None, source=None, smoothing_scale=0., lambda_th=0., accumulate=False):
    """The T-web of a sample: eigenvalues of the tidal tensor of the field smoothed with a Gaussian of
    ``smoothing_scale`` Mpc/h and, per cell, how many exceed ``lambda_th`` (0 void, 1 sheet, 2 filament, 3 knot).
    ``signal`` None = the resident chain state, or with ``source="deltaX"`` the density of the last forward model.
    ``accumulate``: also one more sample of the posterior that ``tweb_probability`` reads.  Returns ``Engine.tweb_classify``'s
    dict (lambda, type, n_type, n_nonfinite, mass_type)."""
    return hd.engine.tweb_classify(signal, source, smoothing_scale, lambda_th, accumulate)


def tweb_probability(hd, type):
    """The posterior probability of ``type`` ("void", "sheet", "filament", "knot" or 0..3) per cell over the samples
    ``tweb_classify(..., accumulate=True)`` has seen -> N values."""
    return hd.engine.tweb_fetch(type, as_probability=True)


def measure_bispectrum(hd, signal=None, source=None, k_min=0., dk=None, n_shell=8, units="h/Mpc"):
    """The bispectrum of a sample by the FFT estimator (Scoccimarro 2015): ``n_shell`` shells of |k| from ``k_min`` in
    steps of ``dk`` (h/Mpc, or fundamentals with ``units="kf"``), all triplets s1 <= s2 <= s3.  ``signal`` None = the
    resident chain state, or with ``source="deltaX"`` the density of the last forward model.  Returns
    ``Engine.bispectrum``'s dict (triplets, b, ntri, q, kmean, nmode, power)."""
    return hd.engine.bispectrum(signal, source, k_min, dk, n_shell, units)


def measure_multipoles(hd, signal=None, N_bin=200, source=None, planepar=True):
    """The Legendre multipoles P_l(k), l = 0, 2, 4, about the line of sight z in measure_spectrum's bins.  ``signal``
    None = the resident chain state, or with ``source="deltaX"`` the density of the last forward model.  Returns
    ``Engine.measure_multipoles``'s dict (k, nmode, leg2, leg4, p0, p2, p4)."""
    if not planepar:
        raise RuntimeError("non-plane-parallel option not yet implemented")  # as 2D_powspec.cc:71
    return hd.engine.measure_multipoles(signal, source, N_bin)


def measure_corr_multipoles(hd, signal=None, N_bin=None, source=None, planepar=True):
    """The multipoles xi_l(s), l = 0, 2, 4, of the correlation function in measure_corr_grid's bins.  Returns
    ``Engine.measure_corr_multipoles``'s dict (r, nmode, leg2, leg4, xi0, xi2, xi4)."""
    if not planepar:
        raise RuntimeError("non-plane-parallel option not yet implemented")  # as 2D_corr_fct.cc:75
    return hd.engine.measure_corr_multipoles(signal, source, N_bin)


def getDensity(hd, mk, xp, yp, zp, Par_mass=None, weightmass=False, kernel_h=0.0, to_nobs=False):
    """getDensity_NGP / _CIC / _TSC / _SPH (massFunctions.cc:49-495; ``mk`` 0 .. 3 picks the one, None the handle's) of a
    free particle list on ``hd``'s grid, upstream's argument order from ``xp`` on -> (delta, stats).  ``weightmass``
    False: every particle counts 1 whatever ``Par_mass`` holds (CIC and SPH upstream; NGP and TSC always read Par_mass
    there, so pass True with it for those).  ``kernel_h`` 0: the handle's scale length."""
    w = Par_mass if weightmass else None
    if weightmass and Par_mass is None:
        raise ValueError("weightmass without Par_mass")
    return hd.engine.density_particles(xp, yp, zp, w, mk=mk, kernel_h=kernel_h, to_nobs=to_nobs)


def discrete_poisson_sample(hd, field, Nbar, seed, stream=0):
    """discrete_poisson_sample (tools/poisson_upres.cc:23-65) of ``Nbar (1 + field)`` (:127) on the device: ``field`` is an
    n_in^3 grid with n_in <= the handle's Nx on the handle's box.  The counts come from the engine's counter-based
    sampler under ``(seed, stream)`` -- exact in distribution, not GSL's stream -- the particles in upstream's order.
    Returns (x, y, z, stats); the sample stays resident in the engine."""
    _, st = hd.engine.poisson_draw(field, seed=seed, stream=stream, scale=Nbar, counts=False)
    x, y, z = hd.engine.poisson_positions(0, st["n_part"])
    return x, y, z, st


def poisson_upres(hd, field, Nbar, seed, mk=1, stream=0):
    """tools/poisson_upres.cc end to end: a Poisson sample of ``Nbar (1 + field)`` (``field``: n_in^3, n_in <= Nx) assigned
    to the handle's Nx^3 grid by masskernel ``mk`` (the tool's is CIC, 1), without a position leaving the device.
    Returns (density, stats) with the draw's and the assignment's stats merged."""
    _, st = hd.engine.poisson_draw(field, seed=seed, stream=stream, scale=Nbar, counts=False)
    rho, ds = hd.engine.poisson_density(mk=mk)
    st.update(ds)
    return rho, st


def interpolate_CIC(hd, xp, yp, zp, field_grid, path=None):
    """interpolate_CIC (interpolate_grid.cpp:108-120) of a field at a free particle list on ``hd``'s grid, upstream's
    argument order from ``xp`` on -> N_OBJ values.  ``field_grid``: an array of N values, ``"chain"``, ``"deltax"`` or a
    bchmc_field name (``"psix"``, ``"window"`` ...), read on the device."""
    return hd.engine.interp_particles(xp, yp, zp, [field_grid], kernel="cic", path=path)[0][0]


def interpolate_TSC(hd, xp, yp, zp, field_grid, path=None):
    """interpolate_TSC (interpolate_grid.cpp:194-202) -> N_OBJ values, NaN for a particle outside the kernel's domain."""
    return hd.engine.interp_particles(xp, yp, zp, [field_grid], kernel="tsc", path=path)[0][0]


def interpolate_TSC_multi(hd, xp, yp, zp, field_grids, path=None):
    """interpolate_TSC_multi (interpolate_grid.cpp:271-286) of 1 .. 4 fields -> (N_fields, N_OBJ): one set of cells and
    weights per particle serves all of them."""
    return hd.engine.interp_particles(xp, yp, zp, list(field_grids), kernel="tsc", path=path)[0]


def Hamiltonian_mass(hd, signal=None):
    """HMC_mass.cc:315-368 on the device at ``signal`` (None: the resident chain state); the engine takes the new mass
    as if it had been uploaded.  Returns (mass_f, mass_r), None where the mass_type has none."""
    n = hd.numerical
    return hd.engine.hamiltonian_mass(signal, n_bin=n.N_bin, mass_factor=n.mass_factor, iGibbs=n.iGibbs,
                                      s_eps_total=n.s_eps_total)


def massnum_due(iGibbs, massnum_init, massnum_burn):
    """HMC.cc:387-400: whether HamiltonianMC recomputes the mass at the top of sample ``iGibbs``.  massnum == 0 means
    never (upstream divides by it; data/input.par:104-105 ships 0)."""
    massnum = massnum_burn if iGibbs > massnum_burn else massnum_init
    if massnum == 0:
        return False
    return iGibbs % massnum == 0 or iGibbs == 1


def HamiltonianMC(hd, uniform, seed=1, itmax=2000, ring=None, group=None, momenta=None, eps_cfg=None,
                  massnum_init=0, massnum_burn=0):
    """One sample of the reference's HamiltonianMC loop (HMC.cc:431-511) on the device-resident chain:
    repeat { draw momenta; draw (Neps, epsilon); trajectory; dH; Metropolis test } until accepted.

    ``uniform`` stands for ``gsl_rng_uniform`` and is consumed in the reference's order per attempt: Neps, epsilon
    (HMC.cc:260-261), then the acceptance draw only if p_acc < 1 (HMC.cc:478-480).  Momenta come from the engine's
    counter-based device generator (``seed``, attempt index) unless ``momenta`` (a callable returning a host
    array, e.g. a port of the GSL draw) is given.  ``momenta="mt19937"`` draws them on the device from ``uniform``
    itself, which must then be a ``gsl_mt19937.GslMT19937``: momenta, Neps, epsilon and the Metropolis uniform share
    one stream in the reference's order (HMC.cc:449, 260-261, 480), as in an upstream run seeded alike.  The chain
    state must have been set with ``hd.engine.chain_set_state``.  Returns the list of per-attempt records (the performance-log row, HMC.cc:40-60).

    Step-size bookkeeping as upstream: ``update_eps_fac`` before every trajectory (HMC.cc:453; needs ``ring`` and
    ``eps_cfg``, a ``time_step.EpsConfig``), ``rejections`` += 1 on a reject (500-501), the attempt into the ring
    (``update_epsilon_acc_rate_tables``, 506-507).  With a ``group``, ONE exchange after the loop -- the fixed point
    every chain reaches once per sample -- pools the other chains' records into the ring.

    Mass: at the top of the sample, when ``massnum_due(iGibbs, massnum_init, massnum_burn)`` (HMC.cc:387-400), the
    mass is rebuilt on the device from the resident state (``Hamiltonian_mass``); a mass_r holding a NaN raises like
    HMC.cc:404-406.  The defaults (0) never rebuild it.
    """
    from . import time_step
    n = hd.numerical
    e = hd.engine
    if massnum_due(n.iGibbs, massnum_init, massnum_burn):
        _, mass_r = Hamiltonian_mass(hd)
        if mass_r is not None and np.isnan(mass_r).any():
            raise RuntimeError("auxmass_r contains a NaN! aborting.")
    exact = isinstance(momenta, str)
    if exact:
        from .gsl_mt19937 import GslMT19937
        if momenta != "mt19937":
            raise ValueError("momenta: None, a callable or \"mt19937\", not %r" % (momenta,))
        if not isinstance(uniform, GslMT19937):
            raise TypeError('momenta="mt19937" draws from `uniform`, which must be a GslMT19937')
    log = []
    for _ in range(itmax):
        attempt = n.count_attempts
        if exact:
            e.chain_draw_momenta_mt19937(uniform)
        elif momenta is None:
            e.chain_draw_momenta(seed, attempt)
        else:
            e.chain_set_momenta(momenta())
        if ring is not None and eps_cfg is not None:
            n.eps_fac = time_step.update_eps_fac(n.eps_fac, ring, eps_cfg, iGibbs=n.iGibbs, rejections=n.rejections)
        n.Neps = int(n.N_eps_fac * uniform()) + 1
        n.epsilon = float(n.eps_fac * uniform())
        if n.epsilon > 2.0:
            n.epsilon = 2.0
        dH, t, done = e.chain_attempt(n.epsilon, n.Neps)
        n.count_attempts += 1
        n.steps_done = done
        n.H_kin_i, n.psi_prior_i, n.psi_likeli_i, n.H_kin_f, n.psi_prior_f, n.psi_likeli_f = (float(x) for x in t)
        n.dprior, n.dlikeli = n.psi_prior_f - n.psi_prior_i, n.psi_likeli_f - n.psi_likeli_i
        n.dK = n.H_kin_f - n.H_kin_i
        n.dE = n.dprior + n.dlikeli
        n.dH = float(dH)
        # HMC.cc:462-486, statement for statement: a uniform is consumed only when p_acceptance < 1.  (A NaN dH
        # leaves p_acceptance at 1 there; the reference build traps FE_INVALID before that, main.cc:66-78.)
        p_acceptance = 1.0
        if dH < 0.0:
            p_acceptance = 1.0
        elif np.exp(-dH) < 1.0:
            p_acceptance = float(np.exp(-dH))
        if p_acceptance >= 1.0:
            accepted = True
        else:
            accepted = uniform() < p_acceptance
        n.accepted = bool(accepted)
        e.chain_accept(accepted)
        if not accepted:
            n.rejections += 1
        if ring is not None:
            ring.record(accepted, n.epsilon)
        log.append(dict(accepted=n.accepted, epsilon=n.epsilon, Neps=n.Neps, dH=n.dH, dK=n.dK, dE=n.dE,
                        dprior=n.dprior, dlikeli=n.dlikeli, psi_prior_i=n.psi_prior_i, psi_prior_f=n.psi_prior_f,
                        psi_likeli_i=n.psi_likeli_i, psi_likeli_f=n.psi_likeli_f, H_kin_i=n.H_kin_i,
                        H_kin_f=n.H_kin_f, steps_done=done, eps_fac=n.eps_fac))
        if accepted:
            break
    if group is not None and ring is not None:
        group.pool_into(ring, [(r["epsilon"], r["accepted"], r["Neps"]) for r in log])
    return log
