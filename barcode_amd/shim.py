"""ctypes view of the compiled C++ host layer (``barcode_amd/shim/hmc_hip_shim.cc``, ``include/bchmc_shim.hpp``).

The C++ layer is the product's host side in the reference's language: ``Hamiltonian_EoM``, ``delta_Hamiltonian``,
``gradient_psi``, ``measure_spectrum`` on a view of ``HAMIL_DATA`` / ``HAMIL_NUMERICAL``, throwing
``std::runtime_error`` like the reference.  This module only exists so that the test-suite can drive that compiled
code (through its ``extern "C"`` hooks) with the same seeded cases it uses everywhere else.
"""
import ctypes as C
import os

import numpy as np

from . import engine as _engine

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

SHIM_EXPORTS = ("bchmc_shim_Hamiltonian_EoM", "bchmc_shim_delta_Hamiltonian", "bchmc_shim_gradient_psi",
                "bchmc_shim_measure_spectrum", "bchmc_shim_chain_set_state", "bchmc_shim_chain_get_state",
                "bchmc_shim_HamiltonianMC", "bchmc_shim_HamiltonianMC_mt19937", "bchmc_shim_release", "bchmc_shim_sizeof_view",
                "bchmc_shim_sizeof_numerical", "bchmc_shim_sizeof_attempt_log",
                "bchmc_shim_HamiltonianMC_scripted", "bchmc_shim_kinetic_term", "bchmc_shim_psi",
                "bchmc_shim_eps_create", "bchmc_shim_eps_destroy", "bchmc_shim_eps_append", "bchmc_shim_eps_records",
                "bchmc_shim_eps_acceptance_rate", "bchmc_shim_update_eps_fac", "bchmc_shim_update_tables",
                "bchmc_shim_comm_bootstrap_file", "bchmc_shim_comm_attach", "bchmc_shim_comm_release",
                "bchmc_shim_inputs_changed", "bchmc_shim_mass_changed", "bchmc_shim_bootstrap_exchange_id",
                "bchmc_shim_bootstrap_cleanup", "bchmc_shim_Hamiltonian_mass",
                "bchmc_shim_setup_random_test", "bchmc_shim_make_initial_guess", "bchmc_shim_sizeof_mock",
                "bchmc_shim_measure_corr_grid", "bchmc_shim_measure_corr2D", "bchmc_shim_chain_forward",
                "bchmc_shim_interp_field", "bchmc_shim_measure_corr2D_interp", "bchmc_shim_measure_spec2D",
                "bchmc_shim_getDensity", "bchmc_shim_interpolate", "bchmc_shim_setup_random_test_poisson",
                "bchmc_shim_discrete_poisson_sample", "bchmc_shim_poisson_positions", "bchmc_shim_poisson_upres",
                "bchmc_shim_tweb_classify", "bchmc_shim_tweb_probability", "bchmc_shim_measure_bispectrum",
                "bchmc_shim_measure_multipoles", "bchmc_shim_measure_corr_multipoles")

_dp = C.POINTER(C.c_double)


class HamilNumericalView(C.Structure):
    """bchmc_shim::HamilNumericalView (members of HAMIL_NUMERICAL, struct_hamil.h:51-144)."""
    _fields_ = [
        ("N1", C.c_uint), ("N", C.c_ulong),
        ("L1", C.c_double), ("min1", C.c_double), ("min2", C.c_double), ("min3", C.c_double),
        ("xobs", C.c_double), ("yobs", C.c_double), ("zobs", C.c_double),
        ("planepar", C.c_bool), ("periodic", C.c_bool),
        ("mk", C.c_int), ("calc_h", C.c_int), ("mass_type", C.c_int),
        ("correct_delta", C.c_bool), ("div_dH_by_N", C.c_bool),
        ("particle_kernel_h", C.c_double), ("kth", C.c_double),
        ("grad_psi_prior_factor", C.c_double), ("grad_psi_likeli_factor", C.c_double), ("deltaQ_factor", C.c_double),
        ("N_eps_fac", C.c_double), ("eps_fac", C.c_double), ("epsilon", C.c_double), ("Neps", C.c_ulong),
        ("dH", C.c_double), ("dK", C.c_double), ("dE", C.c_double), ("dprior", C.c_double), ("dlikeli", C.c_double),
        ("psi_prior", C.c_double), ("psi_likeli", C.c_double),
        ("psi_prior_i", C.c_double), ("psi_prior_f", C.c_double), ("psi_likeli_i", C.c_double),
        ("psi_likeli_f", C.c_double), ("H_kin_i", C.c_double), ("H_kin_f", C.c_double),
        ("iGibbs", C.c_ulong), ("rejections", C.c_ulong), ("accepted", C.c_bool),
        ("N_bin", C.c_ulong), ("massnum_init", C.c_ulong), ("massnum_burn", C.c_ulong), ("s_eps_total", C.c_ulong),
        ("mass_factor", C.c_double),
    ]


class EomEnergies(C.Structure):
    """bchmc_shim::HamilView::EomEnergies: the six terms Hamiltonian_EoM keeps for the delta_Hamiltonian that follows."""
    _fields_ = [("valid", C.c_bool), ("ptr", _dp * 4), ("hash", C.c_uint64 * 4), ("terms", C.c_double * 6),
                ("dH", C.c_double), ("inputs_generation", C.c_ulong), ("mass_generation", C.c_ulong)]


class HamilView(C.Structure):
    """bchmc_shim::HamilView (members of HAMIL_DATA, struct_hamil.h:146-222)."""
    _fields_ = [
        ("numerical", C.POINTER(HamilNumericalView)),
        ("likelihood", C.c_int), ("sfmodel", C.c_int), ("rsd_model", C.c_bool),
        ("rho_c", C.c_double), ("delta_min", C.c_double), ("biasP", C.c_double), ("biasE", C.c_double),
        ("ascale", C.c_double), ("D1", C.c_double), ("D2", C.c_double), ("OM", C.c_double), ("OL", C.c_double),
        ("signal_PS", _dp), ("mass_f", _dp), ("mass_r", _dp), ("nobs", _dp), ("noise", _dp), ("window", _dp),
        ("gradpsi", _dp), ("deltaX", _dp), ("posx", _dp), ("posy", _dp), ("posz", _dp),
        ("device", C.c_int), ("engine", C.c_void_p),
        ("eps", C.c_void_p), ("comm", C.c_void_p), ("comm_rank", C.c_int),
        ("inputs_generation", C.c_ulong), ("uploaded_generation", C.c_ulong), ("deterministic", C.c_int),
        ("mass_generation", C.c_ulong), ("mass_uploaded_generation", C.c_ulong),
        ("reuse_eom_energies", C.c_int), ("eom", EomEnergies),
    ]


class AttemptLog(C.Structure):
    """bchmc_shim::AttemptLog: one row of performance_log.txt (HMC.cc:40-60)."""
    _fields_ = [("accepted", C.c_bool), ("epsilon", C.c_double), ("Neps", C.c_ulong), ("steps_done", C.c_ulong),
                ("dH", C.c_double), ("dK", C.c_double), ("dE", C.c_double), ("dprior", C.c_double),
                ("dlikeli", C.c_double), ("psi_prior_i", C.c_double), ("psi_prior_f", C.c_double),
                ("psi_likeli_i", C.c_double), ("psi_likeli_f", C.c_double), ("H_kin_i", C.c_double),
                ("H_kin_f", C.c_double)]


UNIFORM_FN = C.CFUNCTYPE(C.c_double, C.c_void_p)
class MockView(C.Structure):
    """bchmc_shim::MockView (include/bchmc_shim.hpp): the scalars of setup_random_test / make_initial_guess."""
    _fields_ = [("window_type", C.c_int), ("data_model", C.c_int), ("negative_obs", C.c_int),
                ("random_test_rsd", C.c_int), ("sigma_min", C.c_double), ("sigma_fac", C.c_double),
                ("initial_guess", C.c_int), ("initial_guess_smoothing_type", C.c_int),
                ("initial_guess_smoothing_scale", C.c_double), ("initial_guess_field", C.POINTER(C.c_double))]


# bchmc_shim::mt19937_state_fn: void (*)(void *rng_state, uint32_t mt[624], int32_t *mti, int store)
MT_STATE_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_int)


def load():
    """Load libbarcode_shim.so (after libbarcode_hip.so, which it links).  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    _engine.load()
    path = os.path.join(_HERE, "libbarcode_shim.so")
    if not os.path.exists(path):
        raise ImportError("%s is missing: run `make -C barcode_amd/shim` (after barcode_amd/csrc)" % path)
    lib = C.CDLL(path)
    for s in SHIM_EXPORTS:
        getattr(lib, s)
    hv, sz, ul = C.POINTER(HamilView), C.c_size_t, C.c_ulong
    lib.bchmc_shim_sizeof_view.restype = sz
    lib.bchmc_shim_sizeof_numerical.restype = sz
    lib.bchmc_shim_Hamiltonian_EoM.argtypes = [hv, _dp, _dp, _dp, _dp, UNIFORM_FN, C.c_void_p, C.POINTER(ul),
                                               C.POINTER(ul), C.c_char_p, sz]
    lib.bchmc_shim_delta_Hamiltonian.argtypes = [hv, _dp, _dp, _dp, _dp, _dp, C.c_char_p, sz]
    lib.bchmc_shim_gradient_psi.argtypes = [hv, _dp, C.c_char_p, sz]
    lib.bchmc_shim_measure_spectrum.argtypes = [hv, _dp, _dp, _dp, ul, C.c_char_p, sz]
    lib.bchmc_shim_Hamiltonian_mass.argtypes = [hv, _dp, _dp, _dp, C.c_char_p, sz]
    lib.bchmc_shim_measure_corr_grid.argtypes = [hv, _dp, ul, _dp, C.POINTER(ul), _dp, C.c_int, C.c_char_p, sz]
    lib.bchmc_shim_measure_corr2D.argtypes = [hv, _dp, ul, _dp, C.POINTER(ul), _dp, C.c_int, C.c_int, C.c_char_p, sz]
    lib.bchmc_shim_interp_field.argtypes = [hv, _dp, C.c_uint, _dp, C.c_int, C.c_char_p, sz]
    lib.bchmc_shim_measure_corr2D_interp.argtypes = [hv, _dp, C.c_uint, C.c_uint, C.c_double, ul, _dp, C.POINTER(ul), _dp,
                                                     C.c_int, C.c_int, C.c_char_p, sz]
    lib.bchmc_shim_measure_spec2D.argtypes = [hv, _dp, _dp, _dp, ul, C.c_int, C.c_int, C.c_char_p, sz]
    lib.bchmc_shim_tweb_classify.argtypes = [hv, _dp, C.c_double, C.c_double, C.c_int, _dp, C.POINTER(C.c_ubyte),
                                             C.POINTER(ul), _dp, C.c_int, C.c_char_p, sz]
    lib.bchmc_shim_tweb_probability.argtypes = [hv, C.c_int, _dp, C.c_char_p, sz]
    lib.bchmc_shim_measure_bispectrum.argtypes = [hv, _dp, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(ul),
                                                  _dp, C.c_int, C.c_char_p, sz]
    lib.bchmc_shim_measure_multipoles.argtypes = [hv, _dp, ul, _dp, C.POINTER(ul), _dp, _dp, C.c_int, C.c_int, C.c_char_p, sz]
    lib.bchmc_shim_measure_corr_multipoles.argtypes = [hv, _dp, ul, _dp, C.POINTER(ul), _dp, _dp, C.c_int, C.c_int,
                                                       C.c_char_p, sz]
    lib.bchmc_shim_getDensity.argtypes = [hv, C.c_int, _dp, _dp, _dp, _dp, ul, _dp, C.c_int, C.c_double, C.c_char_p, sz]
    lib.bchmc_shim_interpolate.argtypes = [hv, C.c_int, _dp, _dp, _dp, ul, _dp, C.c_int, _dp, C.c_char_p, sz]
    lib.bchmc_shim_chain_forward.argtypes = [hv, C.c_int, C.c_char_p, sz]
    lib.bchmc_shim_chain_set_state.argtypes = [hv, _dp, C.c_char_p, sz]
    lib.bchmc_shim_chain_get_state.argtypes = [hv, _dp, C.c_char_p, sz]
    lib.bchmc_shim_HamiltonianMC.argtypes = [hv, UNIFORM_FN, C.c_void_p, C.c_uint64, ul, C.POINTER(ul),
                                             C.POINTER(AttemptLog), ul, C.POINTER(ul), C.c_char_p, sz]
    lib.bchmc_shim_HamiltonianMC_mt19937.argtypes = [hv, UNIFORM_FN, MT_STATE_FN, C.c_void_p, ul, C.POINTER(ul),
                                                     C.POINTER(AttemptLog), ul, C.POINTER(ul), C.c_char_p, sz]
    lib.bchmc_shim_sizeof_mock.restype = sz
    lib.bchmc_shim_setup_random_test.argtypes = [hv, C.POINTER(MockView), MT_STATE_FN, C.c_void_p, _dp, _dp,
                                                 C.c_char_p, sz]
    lib.bchmc_shim_setup_random_test_poisson.argtypes = [hv, C.POINTER(MockView), MT_STATE_FN, C.c_void_p, C.c_uint64,
                                                         C.c_uint32, _dp, _dp, C.c_char_p, sz]
    lib.bchmc_shim_discrete_poisson_sample.argtypes = [hv, _dp, C.c_uint, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64),
                                                       C.c_char_p, sz]
    lib.bchmc_shim_poisson_positions.argtypes = [hv, C.c_uint64, C.c_uint64, _dp, _dp, _dp, C.c_char_p, sz]
    lib.bchmc_shim_poisson_upres.argtypes = [hv, _dp, C.c_uint, C.c_double, C.c_uint64, C.c_uint32, C.c_int, _dp,
                                             C.c_char_p, sz]
    lib.bchmc_shim_make_initial_guess.argtypes = [hv, C.POINTER(MockView), MT_STATE_FN, C.c_void_p, C.c_char_p, sz]
    lib.bchmc_shim_HamiltonianMC_scripted.argtypes = [hv, _dp, ul, UNIFORM_FN, C.c_void_p, ul, C.POINTER(ul),
                                                      C.POINTER(AttemptLog), ul, C.POINTER(ul), C.c_char_p, sz]
    lib.bchmc_shim_kinetic_term.argtypes = [hv, _dp, _dp, C.c_char_p, sz]
    lib.bchmc_shim_psi.argtypes = [hv, _dp, _dp, C.c_char_p, sz]
    lib.bchmc_shim_eps_create.argtypes = [C.c_int, C.c_uint, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                          C.c_double, ul]
    lib.bchmc_shim_eps_create.restype = C.c_void_p
    lib.bchmc_shim_eps_destroy.argtypes = [C.c_void_p]
    lib.bchmc_shim_eps_destroy.restype = None
    lib.bchmc_shim_eps_append.argtypes = [C.c_void_p, C.c_int, C.c_double]
    lib.bchmc_shim_eps_append.restype = None
    lib.bchmc_shim_eps_records.argtypes = [C.c_void_p]
    lib.bchmc_shim_eps_records.restype = ul
    lib.bchmc_shim_eps_acceptance_rate.argtypes = [C.c_void_p]
    lib.bchmc_shim_eps_acceptance_rate.restype = C.c_double
    lib.bchmc_shim_update_eps_fac.argtypes = [hv, C.c_char_p, sz, C.c_char_p, sz]
    lib.bchmc_shim_update_tables.argtypes = [hv, C.c_char_p, sz]
    lib.bchmc_shim_comm_bootstrap_file.argtypes = [hv, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_char_p, sz]
    lib.bchmc_shim_bootstrap_exchange_id.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_ubyte),
                                                     C.c_char_p, sz]
    lib.bchmc_shim_bootstrap_cleanup.argtypes = [C.c_char_p, C.c_int]
    lib.bchmc_shim_bootstrap_cleanup.restype = None
    lib.bchmc_shim_comm_attach.argtypes = [hv, C.c_void_p, C.c_int]
    lib.bchmc_shim_comm_release.argtypes = [hv]
    lib.bchmc_shim_comm_release.restype = None
    lib.bchmc_shim_inputs_changed.argtypes = [hv]
    lib.bchmc_shim_inputs_changed.restype = None
    lib.bchmc_shim_mass_changed.argtypes = [hv]
    lib.bchmc_shim_mass_changed.restype = None
    lib.bchmc_shim_sizeof_attempt_log.restype = sz
    lib.bchmc_shim_release.argtypes = [hv]
    lib.bchmc_shim_release.restype = None
    if lib.bchmc_shim_sizeof_view() != C.sizeof(HamilView) or \
            lib.bchmc_shim_sizeof_numerical() != C.sizeof(HamilNumericalView) or \
            lib.bchmc_shim_sizeof_attempt_log() != C.sizeof(AttemptLog) or \
            lib.bchmc_shim_sizeof_mock() != C.sizeof(MockView):
        raise ImportError("bchmc_shim.hpp and barcode_amd/shim.py disagree on the struct layouts")
    _lib = lib
    return lib


class ShimError(RuntimeError):
    """The C++ layer threw std::runtime_error."""


def bootstrap_exchange_id(path, rank, world, unique_id=None, timeout_s=30.0):
    """bchmc_shim::bootstrap_exchange_id: the file protocol that carries rank 0's 128-byte id to the other ranks
    (host only).  Rank 0 passes ``unique_id``; every rank gets the id back."""
    lib = load()
    buf = (C.c_ubyte * _engine.UNIQUE_ID_BYTES)()
    if rank == 0:
        buf[:] = bytes(unique_id)
    err = C.create_string_buffer(512)
    if lib.bchmc_shim_bootstrap_exchange_id(str(path).encode(), int(rank), int(world), float(timeout_s), buf, err, len(err)):
        raise ShimError(err.value.decode())
    return bytes(buf)


def bootstrap_cleanup(path, rank):
    load().bchmc_shim_bootstrap_cleanup(str(path).encode(), int(rank))


def _p(a):
    return a.ctypes.data_as(_dp)


class ShimHamil:
    """A HAMIL_DATA view filled from HamilParams + arrays, driving the compiled C++ functions."""

    def __init__(self, params, N_eps_fac=8.0, eps_fac=None, device=0, **arrays):
        self.lib = load()
        p = params
        self.N = p.N
        n = HamilNumericalView()
        n.N1, n.N, n.L1 = p.Nx, p.N, p.L
        for k in ("min1", "min2", "min3", "xobs", "yobs", "zobs", "mk", "calc_h", "mass_type", "particle_kernel_h",
                  "kth", "grad_psi_prior_factor", "grad_psi_likeli_factor", "deltaQ_factor"):
            setattr(n, k, getattr(p, k))
        n.planepar, n.periodic = bool(p.planepar), bool(p.periodic)
        n.correct_delta, n.div_dH_by_N = bool(p.correct_delta), bool(p.div_dH_by_N)
        n.N_eps_fac = N_eps_fac
        n.N_bin, n.mass_factor = 200, 1.0  # data/input.par:129,150; massnum_* = 0: the mass is never rebuilt
        n.eps_fac = p.eps_heuristic() if eps_fac is None else eps_fac
        self.numerical = n
        hd = HamilView()
        hd.numerical = C.pointer(n)
        hd.likelihood, hd.sfmodel, hd.rsd_model = p.likelihood, p.sfmodel, bool(p.rsd_model)
        for k in ("rho_c", "delta_min", "biasP", "biasE", "ascale", "D1", "D2", "OM", "OL"):
            setattr(hd, k, getattr(p, k))
        self._keep = {}
        for k in ("signal_PS", "mass_f", "mass_r", "nobs", "noise", "window"):
            if arrays.get(k) is not None:
                a = np.ascontiguousarray(arrays[k], dtype=np.float64).reshape(-1)
                self._keep[k] = a
                setattr(hd, k, _p(a))
        for k in ("gradpsi", "deltaX", "posx", "posy", "posz"):
            a = np.zeros(p.N)
            self._keep[k] = a
            setattr(hd, k, _p(a))
        hd.device = device
        hd.reuse_eom_energies = 1
        self.hd = hd
        self.count_attempts = C.c_ulong(0)
        self._err = C.create_string_buffer(512)

    def _chk(self, rc):
        if rc:
            raise ShimError(self._err.value.decode())

    def _in(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        assert a.size == self.N
        return a

    def Hamiltonian_EoM(self, signali, momentai, uniform, out=None):
        qf, pf = out if out is not None else (np.empty(self.N), np.empty(self.N))
        done = C.c_ulong(0)
        cb = UNIFORM_FN(lambda _state: float(uniform()))
        self._chk(self.lib.bchmc_shim_Hamiltonian_EoM(C.byref(self.hd), _p(self._in(signali)), _p(self._in(momentai)),
                                                      _p(qf), _p(pf), cb, None, C.byref(self.count_attempts),
                                                      C.byref(done), self._err, len(self._err)))
        return qf, pf, int(done.value)

    def delta_Hamiltonian(self, signali, momentai, signalf, momentaf):
        dH = C.c_double(0)
        self._chk(self.lib.bchmc_shim_delta_Hamiltonian(C.byref(self.hd), _p(self._in(signali)), _p(self._in(momentai)),
                                                        _p(self._in(signalf)), _p(self._in(momentaf)), C.byref(dH),
                                                        self._err, len(self._err)))
        return dH.value

    def gradient_psi(self, signal):
        self._chk(self.lib.bchmc_shim_gradient_psi(C.byref(self.hd), _p(self._in(signal)), self._err, len(self._err)))
        return self._keep["gradpsi"]

    def measure_spectrum(self, signal, N_bin=200):
        km, pw = np.empty(N_bin), np.empty(N_bin)
        self._chk(self.lib.bchmc_shim_measure_spectrum(C.byref(self.hd), _p(self._in(signal)), _p(km), _p(pw), N_bin,
                                                       self._err, len(self._err)))
        return km, pw

    def Hamiltonian_mass(self, signal=None):
        """bchmc_shim::Hamiltonian_mass at ``signal`` (None: the resident state) -> (mass_f, mass_r), None where the
        mass_type has none."""
        t = self.numerical.mass_type
        mf = np.empty(self.N) if t in (1, 2, 3, 4, 5) else None
        mr = np.empty(self.N) if t in (0, 5, 6, 60) else None
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_shim_Hamiltonian_mass(C.byref(self.hd), sig, None if mf is None else _p(mf),
                                                       None if mr is None else _p(mr), self._err, len(self._err)))
        return mf, mr

    def _corr(self, cells, signal, N_bin, of_deltaX, planepar=None):
        size = int(N_bin) ** cells if 1 <= int(N_bin) <= 2048 else 1  # out of range: refused before anything is written
        rm, co, nm = np.empty(size), np.empty(size), np.empty(size, dtype=np.uint64)
        sig = None if signal is None else _p(self._in(signal))
        nmp = nm.ctypes.data_as(C.POINTER(C.c_ulong))
        tail = (int(bool(of_deltaX)), self._err, len(self._err))
        if cells == 1:
            rc = self.lib.bchmc_shim_measure_corr_grid(C.byref(self.hd), sig, int(N_bin), _p(rm), nmp, _p(co), *tail)
        else:
            rc = self.lib.bchmc_shim_measure_corr2D(C.byref(self.hd), sig, int(N_bin), _p(rm), nmp, _p(co),
                                                    int(bool(planepar)), *tail)
        self._chk(rc)
        shape = (int(N_bin),) * cells
        return rm.reshape(shape), nm.reshape(shape), co.reshape(shape)

    def measure_corr_grid(self, signal, N_bin, of_deltaX=False):
        """bchmc_shim::measure_corr_grid at ``signal`` (None: the resident state, or deltaX) -> (rmode, nmode, corr)."""
        return self._corr(1, signal, N_bin, of_deltaX)

    def measure_corr2D(self, signal, N_bin, planepar=True, of_deltaX=False):
        return self._corr(2, signal, N_bin, of_deltaX, planepar)

    def interp_field(self, signal, N_out, of_deltaX=False):
        """bchmc_shim::interp_field at ``signal`` (None: the resident state, or deltaX) -> N_out^3 values."""
        out = np.empty(int(N_out) ** 3 if 4 <= int(N_out) <= 1024 else 1)
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_shim_interp_field(C.byref(self.hd), sig, int(N_out), _p(out), int(bool(of_deltaX)),
                                                   self._err, len(self._err)))
        return out

    def measure_corr2D_interp(self, signal, N_out, N_bin, interp_mode=0, L_max=np.inf, planepar=True, of_deltaX=False):
        """bchmc_shim::measure_corr2D_interp -> (rmode, nmode, corr) shaped (N_bin, N_bin)."""
        size = int(N_bin) ** 2 if 1 <= int(N_bin) <= 2048 else 1
        rm, co, nm = np.empty(size), np.empty(size), np.empty(size, dtype=np.uint64)
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_shim_measure_corr2D_interp(
            C.byref(self.hd), sig, int(N_out), int(interp_mode), float(L_max), int(N_bin), _p(rm),
            nm.ctypes.data_as(C.POINTER(C.c_ulong)), _p(co), int(bool(planepar)), int(bool(of_deltaX)), self._err,
            len(self._err)))
        shape = (int(N_bin),) * 2
        return rm.reshape(shape), nm.reshape(shape), co.reshape(shape)

    def tweb_classify(self, signal, smoothing_scale=0.0, lambda_th=0.0, accumulate=False, of_deltaX=False):
        """bchmc_shim::tweb_classify at ``signal`` (None: the resident state, or deltaX) -> (lambda (3, N), type (N,)
        uint8, n_type (4,), mass_type (4,))."""
        lam, typ = np.empty((3, self.N)), np.empty(self.N, dtype=np.uint8)
        nt, mt = np.zeros(4, dtype=np.uint64), np.zeros(4)
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_shim_tweb_classify(
            C.byref(self.hd), sig, float(smoothing_scale), float(lambda_th), int(bool(accumulate)), _p(lam.reshape(-1)),
            typ.ctypes.data_as(C.POINTER(C.c_ubyte)), nt.ctypes.data_as(C.POINTER(C.c_ulong)), _p(mt),
            int(bool(of_deltaX)), self._err, len(self._err)))
        return lam, typ, nt, mt

    def tweb_probability(self, type):
        """bchmc_shim::tweb_probability -> N values."""
        out = np.empty(self.N)
        self._chk(self.lib.bchmc_shim_tweb_probability(C.byref(self.hd), int(type), _p(out), self._err, len(self._err)))
        return out

    def measure_bispectrum(self, signal, k_min, dk, n_shell, of_deltaX=False):
        """bchmc_shim::measure_bispectrum at ``signal`` (None: the resident state, or deltaX) -> (b, ntri, q) of T values
        and (kmean, nmode, power) of n_shell values."""
        n = min(max(int(n_shell), 0), 32)  # out of range: refused before anything is written
        T = n * (n + 1) * (n + 2) // 6
        b, ntri, q = np.zeros(T), np.zeros(T), np.zeros(T)
        km, nm, pw = np.zeros(n), np.zeros(n, dtype=np.uint64), np.zeros(n)
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_shim_measure_bispectrum(
            C.byref(self.hd), sig, float(k_min), float(dk), int(n_shell), _p(b), _p(ntri), _p(q), _p(km),
            nm.ctypes.data_as(C.POINTER(C.c_ulong)), _p(pw), int(bool(of_deltaX)), self._err, len(self._err)))
        return b, ntri, q, km, nm, pw

    def _multipoles(self, fn, signal, N_bin, planepar, of_deltaX):
        size = int(N_bin) if 1 <= int(N_bin) <= 2048 else 1  # out of range: refused before anything is written
        tm, nm, leg, out = np.empty(size), np.empty(size, dtype=np.uint64), np.empty((2, size)), np.empty((3, size))
        sig = None if signal is None else _p(self._in(signal))
        self._chk(fn(C.byref(self.hd), sig, int(N_bin), _p(tm), nm.ctypes.data_as(C.POINTER(C.c_ulong)),
                     _p(leg.reshape(-1)), _p(out.reshape(-1)), int(bool(planepar)), int(bool(of_deltaX)), self._err,
                     len(self._err)))
        return tm, nm, leg, out

    def measure_multipoles(self, signal, N_bin=200, planepar=True, of_deltaX=False):
        """bchmc_shim::measure_multipoles at ``signal`` (None: the resident state, or deltaX) -> (kmode, nmode, leg (2,
        N_bin), power (3, N_bin)), l = 0, 2, 4 along the first axis of power."""
        return self._multipoles(self.lib.bchmc_shim_measure_multipoles, signal, N_bin, planepar, of_deltaX)

    def measure_corr_multipoles(self, signal, N_bin=200, planepar=True, of_deltaX=False):
        """bchmc_shim::measure_corr_multipoles -> (rmode, nmode, leg (2, N_bin), xi (3, N_bin))."""
        return self._multipoles(self.lib.bchmc_shim_measure_corr_multipoles, signal, N_bin, planepar, of_deltaX)

    def measure_spec2D(self, signal, N_bin=200, planepar=True, of_deltaX=False):
        """bchmc_shim::measure_spec2D at ``signal`` (None: the resident state, or deltaX) -> (kmode, power) shaped
        (N_bin, N_bin); the tool returns no mode counts."""
        size = int(N_bin) ** 2 if 1 <= int(N_bin) <= 2048 else 1  # out of range: refused before anything is written
        km, pw = np.empty(size), np.empty(size)
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_shim_measure_spec2D(C.byref(self.hd), sig, _p(km), _p(pw), int(N_bin),
                                                     int(bool(planepar)), int(bool(of_deltaX)), self._err, len(self._err)))
        shape = (int(N_bin),) * 2
        return km.reshape(shape), pw.reshape(shape)

    def getDensity(self, mk, xp, yp, zp, Par_mass=None, weightmass=False, kernel_h=0.0):
        """bchmc_shim::getDensity_NGP / _CIC / _TSC / _SPH (``mk`` 0 .. 3) of a free particle list on the view's grid ->
        delta (N values, the raw density).  NGP and TSC always read ``Par_mass`` like upstream (ones when None)."""
        cols = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (xp, yp, zp)]
        n_obj = cols[0].size
        if Par_mass is None:
            Par_mass = np.ones(n_obj)
        mass = np.ascontiguousarray(Par_mass, dtype=np.float64).reshape(-1)
        if any(a.size != n_obj for a in cols[1:] + [mass]):
            raise ValueError("catalogue columns differ in length")
        delta = np.empty(self.N)
        self._chk(self.lib.bchmc_shim_getDensity(C.byref(self.hd), int(mk), _p(cols[0]), _p(cols[1]), _p(cols[2]), _p(mass),
                                                 n_obj, _p(delta), int(bool(weightmass)), float(kernel_h), self._err,
                                                 len(self._err)))
        return delta

    def _interpolate(self, which, xp, yp, zp, fields):
        cols = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (xp, yp, zp)]
        n_obj = cols[0].size
        if any(a.size != n_obj for a in cols[1:]):
            raise ValueError("catalogue columns differ in length")
        grids = np.ascontiguousarray([self._in(f) for f in fields])
        out = np.empty((len(fields), n_obj))
        self._chk(self.lib.bchmc_shim_interpolate(C.byref(self.hd), which, _p(cols[0]), _p(cols[1]), _p(cols[2]), n_obj,
                                                  _p(grids.reshape(-1)), len(fields), _p(out.reshape(-1)), self._err,
                                                  len(self._err)))
        return out

    def interpolate_CIC(self, xp, yp, zp, field_grid):
        """bchmc_shim::interpolate_CIC of a host grid at a free particle list -> N_OBJ values."""
        return self._interpolate(1, xp, yp, zp, [field_grid])[0]

    def interpolate_TSC(self, xp, yp, zp, field_grid):
        """bchmc_shim::interpolate_TSC -> N_OBJ values (NaN outside TSC's domain)."""
        return self._interpolate(2, xp, yp, zp, [field_grid])[0]

    def interpolate_TSC_multi(self, xp, yp, zp, field_grids):
        """bchmc_shim::interpolate_TSC_multi of 1 .. 4 host grids -> (N_fields, N_OBJ)."""
        return self._interpolate(3, xp, yp, zp, list(field_grids))

    def chain_forward(self, use_rsd=-1):
        """bchmc_shim::chain_forward: Lag2Eul of the resident state; returns the view's deltaX array."""
        self._chk(self.lib.bchmc_shim_chain_forward(C.byref(self.hd), int(use_rsd), self._err, len(self._err)))
        return self._keep["deltaX"]

    def chain_set_state(self, x):
        self._chk(self.lib.bchmc_shim_chain_set_state(C.byref(self.hd), _p(self._in(x)), self._err, len(self._err)))

    def chain_get_state(self):
        x = np.empty(self.N)
        self._chk(self.lib.bchmc_shim_chain_get_state(C.byref(self.hd), _p(x), self._err, len(self._err)))
        return x

    def HamiltonianMC(self, uniform, seed=1, itmax=2000):
        """One sample of the C++ HamiltonianMC loop (device momentum draw).  Returns the list of attempt records."""
        log = (AttemptLog * itmax)()
        n = C.c_ulong(0)
        cb = UNIFORM_FN(lambda _state: float(uniform()))
        self._chk(self.lib.bchmc_shim_HamiltonianMC(C.byref(self.hd), cb, None, int(seed), int(itmax),
                                                    C.byref(self.count_attempts), log, int(itmax), C.byref(n),
                                                    self._err, len(self._err)))
        return [{k: getattr(log[i], k) for k, _ in AttemptLog._fields_} for i in range(n.value)]

    @staticmethod
    def _state_fn(rng):
        def state(_rng, mt, mti, store):
            if store:
                rng.set_state(np.ctypeslib.as_array(mt, shape=(624,)).copy(), mti[0])
            else:
                key, pos = rng.get_state()
                np.ctypeslib.as_array(mt, shape=(624,))[:] = key
                mti[0] = pos

        return MT_STATE_FN(state)

    def setup_random_test(self, rng, window_type=1, data_model=0, negative_obs=False, random_test_rsd=False,
                          sigma_min=1.0, sigma_fac=0.0, poisson_seed=None, poisson_stream=0):
        """bchmc_shim::setup_random_test from ``rng`` (a ``GslMT19937``, advanced in place): (delta_lag, delta_eul).
        ``poisson_seed``: the Poissonian mock from the engine's counter-based sampler (None: refused, as upstream's
        stream has no parallel form)."""
        m = MockView(int(window_type), int(data_model), int(bool(negative_obs)), int(bool(random_test_rsd)),
                     float(sigma_min), float(sigma_fac), 0, 1, 0.0, None)
        dl, de = np.empty(self.N), np.empty(self.N)
        if poisson_seed is None:
            self._chk(self.lib.bchmc_shim_setup_random_test(C.byref(self.hd), C.byref(m), self._state_fn(rng), None, _p(dl),
                                                            _p(de), self._err, len(self._err)))
        else:
            self._chk(self.lib.bchmc_shim_setup_random_test_poisson(C.byref(self.hd), C.byref(m), self._state_fn(rng), None,
                                                                    int(poisson_seed), int(poisson_stream), _p(dl), _p(de),
                                                                    self._err, len(self._err)))
        return dl, de

    def discrete_poisson_sample(self, lam, seed, stream=0):
        """bchmc_shim::discrete_poisson_sample of an N1^3 grid of rates (N1 <= the view's) -> (n_part, 3) positions."""
        lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(-1)
        n1 = int(round(lam.size ** (1.0 / 3.0)))
        if n1 ** 3 != lam.size:
            raise ValueError("%d rates are no cube" % lam.size)
        n = C.c_uint64(0)
        self._chk(self.lib.bchmc_shim_discrete_poisson_sample(C.byref(self.hd), _p(lam), n1, int(seed), int(stream),
                                                              C.byref(n), self._err, len(self._err)))
        x, y, z = np.empty(n.value), np.empty(n.value), np.empty(n.value)
        if n.value:  # the sample is resident: one fetch
            self._chk(self.lib.bchmc_shim_poisson_positions(C.byref(self.hd), 0, n.value, _p(x), _p(y), _p(z), self._err,
                                                            len(self._err)))
        return np.stack([x, y, z], axis=1)

    def poisson_upres(self, delta, Nbar, seed, mk=1, stream=0):
        """bchmc_shim::poisson_upres: a sample of Nbar (1 + delta) (``delta``: N1^3 values) on the view's grid -> N values."""
        delta = np.ascontiguousarray(delta, dtype=np.float64).reshape(-1)
        n1 = int(round(delta.size ** (1.0 / 3.0)))
        if n1 ** 3 != delta.size:
            raise ValueError("%d values are no cube" % delta.size)
        out = np.empty(self.N)
        self._chk(self.lib.bchmc_shim_poisson_upres(C.byref(self.hd), _p(delta), n1, float(Nbar), int(seed), int(stream),
                                                    int(mk), _p(out), self._err, len(self._err)))
        return out

    def make_initial_guess(self, rng, initial_guess=0, file_field=None, smoothing_type=1, smoothing_scale=0.0):
        """bchmc_shim::make_initial_guess from ``rng``: sets the resident chain state."""
        ff = None if file_field is None else np.ascontiguousarray(file_field, dtype=np.float64).reshape(-1)
        m = MockView(1, 0, 0, 0, 1.0, 0.0, int(initial_guess), int(smoothing_type), float(smoothing_scale),
                     None if ff is None else _p(ff))
        self._chk(self.lib.bchmc_shim_make_initial_guess(C.byref(self.hd), C.byref(m), self._state_fn(rng), None,
                                                         self._err, len(self._err)))

    def HamiltonianMC_mt19937(self, rng, itmax=2000):
        """One sample of the C++ loop with the exact device draw from ``rng`` (a ``gsl_mt19937.GslMT19937``), which
        supplies the uniforms too and is advanced in place.  Returns the list of attempt records."""
        log = (AttemptLog * itmax)()
        n = C.c_ulong(0)
        cb = UNIFORM_FN(lambda _state: float(rng.uniform()))
        sf = self._state_fn(rng)
        self._chk(self.lib.bchmc_shim_HamiltonianMC_mt19937(C.byref(self.hd), cb, sf, None, int(itmax),
                                                            C.byref(self.count_attempts), log, int(itmax), C.byref(n),
                                                            self._err, len(self._err)))
        return [{k: getattr(log[i], k) for k, _ in AttemptLog._fields_} for i in range(n.value)]

    def HamiltonianMC_scripted(self, script_dH, uniform, itmax=2000, log_cap=None):
        """The same C++ loop on a scripted engine (attempt k returns dH = script_dH[k]): bookkeeping tests, no GPU."""
        cap = itmax if log_cap is None else int(log_cap)
        log = (AttemptLog * max(cap, 1))()
        n = C.c_ulong(0)
        cb = UNIFORM_FN(lambda _state: float(uniform()))
        sc = np.ascontiguousarray(script_dH, dtype=np.float64)
        self._chk(self.lib.bchmc_shim_HamiltonianMC_scripted(C.byref(self.hd), _p(sc), sc.size, cb, None, int(itmax),
                                                             C.byref(self.count_attempts),
                                                             log if cap > 0 else None, cap, C.byref(n), self._err,
                                                             len(self._err)))
        return n.value, [{k: getattr(log[i], k) for k, _ in AttemptLog._fields_} for i in range(min(n.value, cap))]

    def kinetic_term(self, momenta):
        out = C.c_double(0)
        self._chk(self.lib.bchmc_shim_kinetic_term(C.byref(self.hd), _p(self._in(momenta)), C.byref(out), self._err,
                                                   len(self._err)))
        return out.value

    def psi(self, signal):
        out = C.c_double(0)
        self._chk(self.lib.bchmc_shim_psi(C.byref(self.hd), _p(self._in(signal)), C.byref(out), self._err,
                                          len(self._err)))
        return out.value

    # ---- step-size adaptation (time_step.cpp) -------------------------------------------------------------
    def eps_attach(self, cfg):
        """Create the C++ EpsAdapt from a barcode_amd.time_step.EpsConfig and hang it on hd->eps."""
        e = self.lib.bchmc_shim_eps_create(cfg.eps_fac_update_type, cfg.N_a_eps_update, cfg.acc_min, cfg.acc_max,
                                           cfg.eps_down_smooth, cfg.eps_up_fac, cfg.eps_fac_target, cfg.eps_fac_power,
                                           cfg.s_eps_total)
        if not e:
            raise ShimError("eps_adapt_create failed")
        self.hd.eps = e
        return e

    def eps_append(self, accepted, epsilon):
        self.lib.bchmc_shim_eps_append(self.hd.eps, int(bool(accepted)), float(epsilon))

    def eps_records(self):
        return int(self.lib.bchmc_shim_eps_records(self.hd.eps))

    def eps_acceptance_rate(self):
        return float(self.lib.bchmc_shim_eps_acceptance_rate(self.hd.eps))

    def update_eps_fac(self):
        msg = C.create_string_buffer(256)
        self._chk(self.lib.bchmc_shim_update_eps_fac(C.byref(self.hd), msg, len(msg), self._err, len(self._err)))
        return msg.value.decode()

    def update_epsilon_acc_rate_tables(self):
        self._chk(self.lib.bchmc_shim_update_tables(C.byref(self.hd), self._err, len(self._err)))

    def comm_attach(self, comm, rank):
        self.lib.bchmc_shim_comm_attach(C.byref(self.hd), comm, int(rank))

    def comm_bootstrap_file(self, path, rank, world, timeout_s=60.0):
        self._chk(self.lib.bchmc_shim_comm_bootstrap_file(C.byref(self.hd), path.encode(), int(rank), int(world),
                                                          float(timeout_s), self._err, len(self._err)))

    def comm_release(self):
        self.lib.bchmc_shim_comm_release(C.byref(self.hd))

    def inputs_changed(self):
        self.lib.bchmc_shim_inputs_changed(C.byref(self.hd))

    def mass_changed(self):
        """Only mass_f / mass_r were rewritten (HMC.cc:400-423): the resident chain keeps its carried gradient."""
        self.lib.bchmc_shim_mass_changed(C.byref(self.hd))

    def out(self, name):
        """hd->gradpsi / deltaX / posx / posy / posz as the C++ layer left them."""
        return self._keep[name]

    def close(self):
        self.lib.bchmc_shim_release(C.byref(self.hd))
        if self.hd.eps:
            self.lib.bchmc_shim_eps_destroy(self.hd.eps)
            self.hd.eps = None
