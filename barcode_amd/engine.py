"""ctypes binding of ``libbarcode_hip.so`` (C ABI: ``include/bchmc.h``).

There is no CPU fallback: if the HIP library is missing or fails to load this module raises.
``torch`` is imported first on purpose: it brings the process-wide HIP runtime (``libamdhip64.so.7``) and
rocFFT that our library then binds to, so device pointers of torch tensors and the engine's stream live
in the same runtime.
"""
import ctypes as C
import os

import numpy as np
import torch  # noqa: F401  (must precede loading libbarcode_hip.so, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# BCHMC_LIB: an alternative build of the same library (A/B runs of kernel variants on one box)
LIB_PATH = os.environ.get("BCHMC_LIB") or os.path.join(_HERE, "libbarcode_hip.so")
ABI_VERSION = 4

FIELDS = dict(signal_PS=0, mass_f=1, mass_r=2, nobs=3, noise=4, window=5, deltaX=6, posx=7, posy=8, posz=9,
              rho=10, part_like=11, Vx=12, Vy=13, Vz=14, psix=15, psiy=16, psiz=17, grad_prior=18, grad_like=19)
INPUT_FIELDS = ("signal_PS", "mass_f", "mass_r", "nobs", "noise", "window")
K_COUNT = 9


class BchmcConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("Nx", C.c_uint32), ("L", C.c_double),
        ("min1", C.c_double), ("min2", C.c_double), ("min3", C.c_double),
        ("xobs", C.c_double), ("yobs", C.c_double), ("zobs", C.c_double),
        ("planepar", C.c_int32), ("periodic", C.c_int32),
        ("mk", C.c_int32), ("calc_h", C.c_int32), ("likelihood", C.c_int32), ("sfmodel", C.c_int32),
        ("rsd_model", C.c_int32), ("mass_type", C.c_int32), ("correct_delta", C.c_int32),
        ("div_dH_by_N", C.c_int32),
        ("particle_kernel_h", C.c_double),
        ("grad_psi_prior_factor", C.c_double), ("grad_psi_likeli_factor", C.c_double),
        ("deltaQ_factor", C.c_double),
        ("rho_c", C.c_double), ("delta_min", C.c_double), ("biasP", C.c_double), ("biasE", C.c_double),
        ("ascale", C.c_double), ("D1", C.c_double), ("D2", C.c_double), ("OM", C.c_double), ("OL", C.c_double),
        ("kth", C.c_double),
        ("precision", C.c_int32), ("device", C.c_int32), ("deterministic", C.c_int32), ("reserved0", C.c_int32),
    ]


class EpsRecord(C.Structure):
    _fields_ = [("epsilon", C.c_double), ("accepted", C.c_int32), ("neps", C.c_int32)]


class MassOpts(C.Structure):
    """bchmc_mass_opts: the HAMIL_NUMERICAL scalars Hamiltonian_mass reads."""
    _fields_ = [("n_bin", C.c_uint64), ("mass_factor", C.c_double), ("iGibbs", C.c_uint64), ("s_eps_total", C.c_uint64)]


class MockOpts(C.Structure):
    """bchmc_mock_opts: the NUMERICAL / OBSERVATIONAL scalars setup_random_test reads (barcoderunner.cc:42-205)."""
    _fields_ = [("window_type", C.c_int32), ("data_model", C.c_int32), ("negative_obs", C.c_int32),
                ("random_test_rsd", C.c_int32), ("sigma_min", C.c_double), ("sigma_fac", C.c_double)]


class DensityOpts(C.Structure):
    """bchmc_density_opts: kernel, weights, SPH scale length and destination of bchmc_density_particles."""
    _fields_ = [("mk", C.c_int32), ("weightmass", C.c_int32), ("kernel_h", C.c_double), ("dest", C.c_int32),
                ("reserved0", C.c_int32)]


class PoissonOpts(C.Structure):
    """bchmc_poisson_opts: seed and stream of the counter-based draw, the rate's form and scale, window and destination."""
    _fields_ = [("seed", C.c_uint64), ("stream", C.c_uint32), ("rate_mode", C.c_int32), ("scale", C.c_double),
                ("use_window", C.c_int32), ("dest", C.c_int32)]


class PoissonStats(C.Structure):
    """bchmc_poisson_stats."""
    _fields_ = [("n_part", C.c_uint64), ("n_cells_drawn", C.c_uint64), ("max_count", C.c_uint64),
                ("n_capped", C.c_uint64), ("lambda_max", C.c_double)]


class DensityStats(C.Structure):
    """bchmc_density_stats."""
    _fields_ = [("n_in", C.c_uint64), ("n_lost", C.c_uint64), ("max_per_tile", C.c_uint64)]


class TwebOpts(C.Structure):
    """bchmc_tweb_opts."""
    _fields_ = [("smoothing_scale", C.c_double), ("lambda_th", C.c_double), ("accumulate", C.c_int32),
                ("reserved0", C.c_int32)]


class TwebStats(C.Structure):
    """bchmc_tweb_stats."""
    _fields_ = [("n_type", C.c_uint64 * 4), ("n_nonfinite", C.c_uint64), ("mass_type", C.c_double * 4)]


class BispecOpts(C.Structure):
    """bchmc_bispec_opts."""
    _fields_ = [("k_min", C.c_double), ("dk", C.c_double), ("n_shell", C.c_int32), ("reserved0", C.c_int32)]


class InterpField(C.Structure):
    """bchmc_interp_field: one source of bchmc_interp_particles."""
    _fields_ = [("source", C.c_int32), ("field", C.c_int32), ("host", C.POINTER(C.c_double))]


class InterpOpts(C.Structure):
    """bchmc_interp_opts."""
    _fields_ = [("kernel", C.c_int32), ("path", C.c_int32), ("reserved", C.c_int32 * 2)]


class InterpStats(C.Structure):
    """bchmc_interp_stats."""
    _fields_ = [("n_in", C.c_uint64), ("n_lost", C.c_uint64), ("max_per_tile", C.c_uint64), ("path_used", C.c_int32),
                ("reserved", C.c_int32)]


INTERP_MAX_FIELDS = 4       # BCHMC_INTERP_MAX_FIELDS
INTERP_HANDLE_FIELD = 3     # BCHMC_INTERP_HANDLE_FIELD
INTERP_KERNELS = dict(cic=1, tsc=2)
INTERP_PATHS = {None: -1, "direct": 0, "tile": 1, -1: -1, 0: 0, 1: 1}

# bchmc_part_source
PART_SOURCES = dict(host=0, forward=1)
F_NOBS = 3  # BCHMC_F_NOBS


# which mass arrays a mass_type has (struct_hamil.h:272-313)
MASS_F_TYPES = (1, 2, 3, 4, 5)
MASS_R_TYPES = (0, 5, 6, 60)


EPS_BATCH = 32            # BCHMC_EPS_BATCH
UNIQUE_ID_BYTES = 128     # BCHMC_UNIQUE_ID_BYTES
PACKET_BYTES = 8 + 16 * EPS_BATCH
# bchmc_allgather_fn: int (*)(void *ctx, const void *send, void *recv, size_t bytes_per_rank)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)


class BchmcError(RuntimeError):
    """Raised for any non-zero return code; mirrors the reference's std::runtime_error."""

    def __init__(self, code, text, detail=""):
        super().__init__("bchmc error %d (%s)%s" % (code, text, (": " + detail) if detail else ""))
        self.code = code


_lib = None

# every symbol include/bchmc.h declares; tests check that the library exports all of them
EXPORTS = ("bchmc_create", "bchmc_destroy", "bchmc_strerror", "bchmc_last_error", "bchmc_upload", "bchmc_fetch",
           "bchmc_leapfrog", "bchmc_leapfrog_dh", "bchmc_energies", "bchmc_delta_hamiltonian", "bchmc_gradient", "bchmc_forward",
           "bchmc_leapfrog_device", "bchmc_steps_done", "bchmc_energies_device", "bchmc_sync", "bchmc_stream",
           "bchmc_profile", "bchmc_profile_read", "bchmc_kernel_name", "bchmc_tile_info", "bchmc_live_resources",
           "bchmc_chain_set_state", "bchmc_chain_get_state", "bchmc_chain_set_momenta", "bchmc_chain_get_momenta",
           "bchmc_chain_draw_momenta", "bchmc_chain_attempt", "bchmc_chain_get_proposal", "bchmc_chain_accept",
           "bchmc_measure_spectrum", "bchmc_philox_kat", "bchmc_kinetic_term", "bchmc_psi",
           "bchmc_comm_unique_id", "bchmc_comm_create", "bchmc_comm_create_custom", "bchmc_comm_destroy",
           "bchmc_comm_last_error", "bchmc_eps_exchange", "bchmc_comm_pending", "bchmc_comm_world", "bchmc_comm_rank",
           "bchmc_comm_transport", "bchmc_garfield_walk_index", "bchmc_hamiltonian_mass",
           "bchmc_setup_random_test", "bchmc_make_initial_guess", "bchmc_measure_corr", "bchmc_chain_forward",
           "bchmc_probe_displacement", "bchmc_probe_displacement_z", "bchmc_interp_upres", "bchmc_upres_release", "bchmc_measure_spectrum_src",
           "bchmc_density_particles", "bchmc_catalogue_release", "bchmc_interp_particles", "bchmc_interp_release",
           "bchmc_measure_cross_spectrum", "bchmc_ensemble_add", "bchmc_ensemble_count", "bchmc_ensemble_fetch",
           "bchmc_ensemble_merge", "bchmc_ensemble_reset", "bchmc_ensemble_release",
           "bchmc_poisson_draw", "bchmc_poisson_positions", "bchmc_poisson_density", "bchmc_poisson_release",
           "bchmc_setup_random_test_poisson",
           "bchmc_tweb_classify", "bchmc_tweb_tensor", "bchmc_tweb_samples", "bchmc_tweb_fetch", "bchmc_tweb_merge",
           "bchmc_tweb_reset", "bchmc_tweb_release",
           "bchmc_bispectrum", "bchmc_bispec_release",
           "bchmc_measure_multipoles", "bchmc_measure_cross_multipoles", "bchmc_measure_corr_multipoles",
           "bchmc_multipoles_release")
# declared as well, listed apart: the header scan of the ABI test matches names of letters and underscores only
EXPORTS_MT19937 = ("bchmc_chain_draw_momenta_mt19937", "bchmc_mt19937_jump")
EXPORTS_CORR2D = ("bchmc_measure_corr2d", "bchmc_measure_corr2d_interp")  # a digit in the name, like the two above
EXPORTS_SPEC2D = ("bchmc_measure_spectrum2d",)  # likewise

# bchmc_corr_source
CORR_SOURCES = dict(host=0, chain=1, deltaX=2)
ENS_SLOTS = 4                                         # BCHMC_ENS_SLOTS
ENS_WHAT = dict(mean=0, variance=1, std=2, m2=3)      # bchmc_ens_what
TWEB_TYPES = dict(void=0, sheet=1, filament=2, knot=3)  # the number of eigenvalues above lambda_th
TWEB_COMPONENTS = dict(xx=0, xy=1, xz=2, yy=3, yz=4, zz=5)
BISPEC_MAX_SHELL = 32                                 # kBispecMaxShell
TWEB_NONFINITE = 255                                  # the type of a cell whose tensor is not finite


def load():
    """Load the HIP library (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, dp, u64 = C.c_void_p, C.POINTER(C.c_double), C.c_uint64
    lib.bchmc_create.argtypes = [C.POINTER(BchmcConfig), C.POINTER(vp)]
    lib.bchmc_destroy.argtypes = [vp]
    lib.bchmc_destroy.restype = None
    lib.bchmc_strerror.argtypes = [C.c_int]
    lib.bchmc_strerror.restype = C.c_char_p
    lib.bchmc_last_error.argtypes = [vp]
    lib.bchmc_last_error.restype = C.c_char_p
    lib.bchmc_upload.argtypes = [vp, C.c_int, dp, C.c_size_t]
    lib.bchmc_fetch.argtypes = [vp, C.c_int, dp, C.c_size_t]
    lib.bchmc_leapfrog.argtypes = [vp, dp, dp, dp, dp, C.c_double, u64, C.POINTER(u64)]
    lib.bchmc_leapfrog_dh.argtypes = [vp, dp, dp, dp, dp, C.c_double, u64, C.POINTER(u64), dp, dp]
    lib.bchmc_energies.argtypes = [vp, dp, dp, dp]
    lib.bchmc_delta_hamiltonian.argtypes = [vp, dp, dp, dp, dp, dp, dp]
    lib.bchmc_gradient.argtypes = [vp, dp, dp]
    lib.bchmc_forward.argtypes = [vp, dp, C.c_int]
    lib.bchmc_leapfrog_device.argtypes = [vp, vp, vp, vp, vp, C.c_double, u64]
    lib.bchmc_steps_done.argtypes = [vp, C.POINTER(u64)]
    lib.bchmc_energies_device.argtypes = [vp, vp, vp, dp]
    lib.bchmc_sync.argtypes = [vp]
    lib.bchmc_stream.argtypes = [vp]
    lib.bchmc_stream.restype = vp
    lib.bchmc_tile_info.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.bchmc_live_resources.argtypes = [C.POINTER(u64)]
    lib.bchmc_profile.argtypes = [vp, C.c_int]
    lib.bchmc_profile_read.argtypes = [vp, dp, C.POINTER(u64)]
    lib.bchmc_kernel_name.argtypes = [C.c_int]
    lib.bchmc_kernel_name.restype = C.c_char_p
    lib.bchmc_chain_set_state.argtypes = [vp, dp]
    lib.bchmc_chain_get_state.argtypes = [vp, dp]
    lib.bchmc_chain_set_momenta.argtypes = [vp, dp]
    lib.bchmc_chain_get_momenta.argtypes = [vp, dp]
    lib.bchmc_chain_draw_momenta.argtypes = [vp, u64, u64]
    lib.bchmc_chain_attempt.argtypes = [vp, C.c_double, u64, dp, dp, C.POINTER(u64)]
    lib.bchmc_chain_get_proposal.argtypes = [vp, dp, dp]
    lib.bchmc_chain_accept.argtypes = [vp, C.c_int]
    lib.bchmc_measure_spectrum.argtypes = [vp, dp, C.c_uint64, dp, dp]
    lib.bchmc_hamiltonian_mass.argtypes = [vp, dp, C.POINTER(MassOpts), dp, dp]
    lib.bchmc_measure_corr.argtypes = [vp, C.c_int, dp, C.c_uint64, dp, C.POINTER(u64), dp]
    lib.bchmc_measure_corr2d.argtypes = [vp, C.c_int, dp, C.c_uint64, dp, C.POINTER(u64), dp]
    lib.bchmc_interp_upres.argtypes = [vp, C.c_int, dp, C.c_uint32, dp]
    lib.bchmc_measure_corr2d_interp.argtypes = [vp, C.c_int, dp, C.c_uint32, C.c_int32, C.c_double, C.c_uint64, dp,
                                                C.POINTER(u64), dp]
    lib.bchmc_upres_release.argtypes = [vp]
    lib.bchmc_measure_spectrum_src.argtypes = [vp, C.c_int, dp, C.c_uint64, dp, dp]
    lib.bchmc_measure_spectrum2d.argtypes = [vp, C.c_int, dp, C.c_uint64, dp, C.POINTER(u64), dp]
    lib.bchmc_measure_cross_spectrum.argtypes = [vp, C.c_int, dp, C.c_int, dp, C.c_uint64, dp, C.POINTER(u64), dp, dp, dp, dp]
    lib.bchmc_ensemble_add.argtypes = [vp, C.c_int32, C.c_int, dp]
    lib.bchmc_ensemble_count.argtypes = [vp, C.c_int32, C.POINTER(u64)]
    lib.bchmc_ensemble_fetch.argtypes = [vp, C.c_int32, C.c_int, dp]
    lib.bchmc_ensemble_merge.argtypes = [vp, C.c_int32, u64, dp, dp]
    lib.bchmc_ensemble_reset.argtypes = [vp, C.c_int32]
    lib.bchmc_ensemble_release.argtypes = [vp]
    lib.bchmc_tweb_classify.argtypes = [vp, C.c_int, dp, C.POINTER(TwebOpts), dp, C.POINTER(C.c_uint8), C.POINTER(TwebStats)]
    lib.bchmc_tweb_tensor.argtypes = [vp, C.c_int32, dp]
    lib.bchmc_tweb_samples.argtypes = [vp, C.POINTER(u64)]
    lib.bchmc_tweb_fetch.argtypes = [vp, C.c_int32, C.c_int32, vp]
    lib.bchmc_tweb_merge.argtypes = [vp, u64, C.POINTER(C.c_uint32)]
    lib.bchmc_tweb_reset.argtypes = [vp]
    lib.bchmc_tweb_release.argtypes = [vp]
    lib.bchmc_bispectrum.argtypes = [vp, C.c_int, dp, C.POINTER(BispecOpts), dp, dp, dp, dp, C.POINTER(u64), dp]
    lib.bchmc_bispec_release.argtypes = [vp]
    lib.bchmc_measure_multipoles.argtypes = [vp, C.c_int, dp, C.c_uint64, dp, C.POINTER(u64), dp, dp]
    lib.bchmc_measure_cross_multipoles.argtypes = [vp, C.c_int, dp, C.c_int, dp, C.c_uint64, dp, C.POINTER(u64), dp, dp, dp, dp]
    lib.bchmc_measure_corr_multipoles.argtypes = [vp, C.c_int, dp, C.c_uint64, dp, C.POINTER(u64), dp, dp]
    lib.bchmc_multipoles_release.argtypes = [vp]
    lib.bchmc_chain_forward.argtypes = [vp, C.c_int]
    lib.bchmc_density_particles.argtypes = [vp, C.c_int, dp, dp, dp, dp, u64, C.POINTER(DensityOpts), dp,
                                            C.POINTER(DensityStats)]
    lib.bchmc_catalogue_release.argtypes = [vp]
    lib.bchmc_interp_particles.argtypes = [vp, C.c_int, dp, dp, dp, u64, C.POINTER(InterpField), C.c_int32,
                                           C.POINTER(InterpOpts), dp, C.POINTER(InterpStats)]
    lib.bchmc_interp_release.argtypes = [vp]
    lib.bchmc_probe_displacement.argtypes = [vp, dp, C.c_int, C.c_int]
    lib.bchmc_probe_displacement_z.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int]
    lib.bchmc_philox_kat.argtypes = [C.POINTER(C.c_uint32)] * 3
    lib.bchmc_kinetic_term.argtypes = [vp, dp, dp]
    lib.bchmc_psi.argtypes = [vp, dp, dp]
    lib.bchmc_comm_unique_id.argtypes = [C.POINTER(C.c_ubyte)]
    lib.bchmc_comm_create.argtypes = [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    lib.bchmc_comm_create_custom.argtypes = [ALLGATHER_FN, vp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.bchmc_comm_destroy.argtypes = [vp]
    lib.bchmc_comm_destroy.restype = None
    lib.bchmc_comm_last_error.argtypes = [vp]
    lib.bchmc_comm_last_error.restype = C.c_char_p
    lib.bchmc_eps_exchange.argtypes = [vp, C.POINTER(EpsRecord), C.c_int, C.POINTER(EpsRecord), C.POINTER(C.c_int),
                                       C.c_int, C.POINTER(C.c_int)]
    lib.bchmc_comm_pending.argtypes = [vp]
    lib.bchmc_comm_world.argtypes = [vp]
    lib.bchmc_comm_rank.argtypes = [vp]
    lib.bchmc_comm_transport.argtypes = [vp]
    lib.bchmc_comm_transport.restype = C.c_char_p
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    lib.bchmc_chain_draw_momenta_mt19937.argtypes = [vp, u32p, i32p, C.POINTER(u64)]
    lib.bchmc_mt19937_jump.argtypes = [u32p, C.c_int32, u64, u32p, i32p]
    lib.bchmc_garfield_walk_index.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(u64)]
    lib.bchmc_setup_random_test.argtypes = [vp, C.POINTER(MockOpts), u32p, i32p, C.POINTER(u64), dp, dp]
    lib.bchmc_poisson_draw.argtypes = [vp, C.c_int, dp, C.c_uint32, C.POINTER(PoissonOpts), dp, C.POINTER(PoissonStats)]
    lib.bchmc_poisson_positions.argtypes = [vp, u64, u64, dp, dp, dp]
    lib.bchmc_poisson_density.argtypes = [vp, C.POINTER(DensityOpts), dp, C.POINTER(DensityStats)]
    lib.bchmc_poisson_release.argtypes = [vp]
    lib.bchmc_setup_random_test_poisson.argtypes = [vp, C.POINTER(MockOpts), u32p, i32p, C.POINTER(u64), u64, C.c_uint32,
                                                    dp, dp]
    lib.bchmc_make_initial_guess.argtypes = [vp, C.c_int32, dp, C.c_int32, C.c_double, u32p, i32p, C.POINTER(u64)]
    _lib = lib
    return lib


def philox_kat(ctr, key):
    """Philox4x32-10 block on the device (known-answer hook)."""
    lib = load()
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    o = (C.c_uint32 * 4)()
    rc = lib.bchmc_philox_kat(c, k, o)
    if rc:
        raise BchmcError(rc, lib.bchmc_strerror(rc).decode())
    return [int(x) for x in o]


def bispec_triplets(n_shell):
    """All (s1, s2, s3) with s1 <= s2 <= s3 < n_shell in lexicographic order, the order of bchmc_bispectrum: (T, 3) int32."""
    n = int(n_shell)
    return np.array([(a, b, c) for a in range(n) for b in range(a, n) for c in range(b, n)], dtype=np.int32).reshape(-1, 3)


def live_resources():
    """(device buffers, their bytes, pinned host buffers, other objects) the library holds in this process right now."""
    lib = load()
    out = (C.c_uint64 * 4)()
    rc = lib.bchmc_live_resources(out)
    if rc:
        raise BchmcError(rc, lib.bchmc_strerror(rc).decode())
    return tuple(int(x) for x in out)


def _u32p(a):
    assert a.dtype == np.uint32 and a.flags.c_contiguous and a.size == 624
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def mt19937_jump(mt, mti, steps):
    """GSL mt19937 state (``mt[624]``, ``mti``) -> the state ``steps`` outputs later (host, jump-ahead)."""
    lib = load()
    src = np.ascontiguousarray(mt, dtype=np.uint32)
    out = np.zeros(624, dtype=np.uint32)
    mo = C.c_int32()
    rc = lib.bchmc_mt19937_jump(_u32p(src), int(mti), int(steps), _u32p(out), C.byref(mo))
    if rc:
        raise BchmcError(rc, lib.bchmc_strerror(rc).decode())
    return out, mo.value


def garfield_walk_index(n, i, j, k):
    """Position of cell (i, j, k) in the walk of resolution_independent_random_grid_FS (random.hpp:35-120)."""
    lib = load()
    idx = C.c_uint64()
    rc = lib.bchmc_garfield_walk_index(int(n), int(i), int(j), int(k), C.byref(idx))
    if rc:
        raise BchmcError(rc, lib.bchmc_strerror(rc).decode())
    return idx.value


def corr_auto_nbin(n, L):
    """The correlation tools' "N_bin = 0" rule (2D_corr_fct.cc:277-286): ceil(rmax / d), rmax = L/2 sqrt(3), d = L/n."""
    rmax = float(L) / 2 * np.sqrt(3)
    return int(np.ceil(rmax / (float(L) / float(n))))


def make_config(params, device=0, precision=0, deterministic=0):
    cfg = BchmcConfig()
    cfg.abi_version = ABI_VERSION
    cfg.Nx = int(params.Nx)
    cfg.L = float(params.L)
    for name, _ in BchmcConfig._fields_:
        if name in ("abi_version", "Nx", "L", "precision", "device", "deterministic", "reserved0"):
            continue
        setattr(cfg, name, getattr(params, name))
    cfg.precision = int(precision)
    cfg.device = int(device)
    cfg.deterministic = int(deterministic)
    return cfg


def _p(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Engine:
    """One chain on one GPU: owns a ``bchmc_handle``."""

    def __init__(self, params, device=0, precision=0, deterministic=0):
        """precision 0: fp64 field arrays (reference DOUBLE_PREC); 1: fp32 field arrays (BASELINE config 5).
        Host arrays are float64 either way.  deterministic 1: bitwise repeatable mass assignment (fixed point)."""
        self.lib = load()
        self.precision = int(precision)
        self.params = params
        self.Nx = int(params.Nx)
        self.N = self.Nx ** 3
        self._tweb_par = None  # (smoothing_scale, lambda_th) of the samples tweb_classify has accumulated
        self.h = C.c_void_p()
        cfg = make_config(params, device, precision, deterministic)
        rc = self.lib.bchmc_create(C.byref(cfg), C.byref(self.h))
        if rc:
            detail = self.lib.bchmc_last_error(self.h).decode() if self.h else ""
            text = self.lib.bchmc_strerror(rc).decode()
            self.close()
            raise BchmcError(rc, text, detail)

    def close(self):
        if getattr(self, "h", None):
            self.lib.bchmc_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise BchmcError(rc, self.lib.bchmc_strerror(rc).decode(), self.lib.bchmc_last_error(self.h).decode())

    def _in(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if a.size != self.N:
            raise ValueError("expected %d elements, got %d" % (self.N, a.size))
        return a

    # ---- arrays --------------------------------------------------------------------------------
    def upload(self, **arrays):
        for k, v in arrays.items():
            self._chk(self.lib.bchmc_upload(self.h, FIELDS[k], _p(self._in(v)), self.N))

    def fetch(self, name):
        out = np.empty(self.N)
        self._chk(self.lib.bchmc_fetch(self.h, FIELDS[name], _p(out), self.N))
        return out

    # ---- host-array entry points (what the reference shim binds) ---------------------------------
    def leapfrog(self, q0, p0, eps, neps, out=None):
        """``out=(q1, p1)``: caller-owned result arrays (the reference allocates signalf / momentaf once per sample,
        HMC.cc:375); fresh arrays otherwise."""
        q1, p1 = out if out is not None else (np.empty(self.N), np.empty(self.N))
        done = C.c_uint64()
        self._chk(self.lib.bchmc_leapfrog(self.h, _p(self._in(q0)), _p(self._in(p0)), _p(q1), _p(p1), float(eps),
                                          int(neps), C.byref(done)))
        return q1, p1, done.value

    def leapfrog_dh(self, q0, p0, eps, neps, out=None):
        """Hamiltonian_EoM + delta_Hamiltonian of the same four arrays in one pass (bchmc_leapfrog_dh).
        Returns (q1, p1, steps_done, dH, terms[6])."""
        q1, p1 = out if out is not None else (np.empty(self.N), np.empty(self.N))
        done, dH = C.c_uint64(), C.c_double()
        terms = np.zeros(6)
        self._chk(self.lib.bchmc_leapfrog_dh(self.h, _p(self._in(q0)), _p(self._in(p0)), _p(q1), _p(p1), float(eps),
                                             int(neps), C.byref(done), C.byref(dH), _p(terms)))
        return q1, p1, done.value, dH.value, terms

    def kinetic_term(self, p):
        out = C.c_double()
        self._chk(self.lib.bchmc_kinetic_term(self.h, _p(self._in(p)), C.byref(out)))
        return out.value

    def psi(self, q):
        out = np.zeros(2)
        self._chk(self.lib.bchmc_psi(self.h, _p(self._in(q)), _p(out)))
        return out

    def energies(self, q, p):
        out = np.zeros(3)
        self._chk(self.lib.bchmc_energies(self.h, _p(self._in(q)), _p(self._in(p)), _p(out)))
        return out

    def delta_hamiltonian(self, qi, pi, qf, pf):
        dH = C.c_double()
        terms = np.zeros(6)
        self._chk(self.lib.bchmc_delta_hamiltonian(self.h, _p(self._in(qi)), _p(self._in(pi)), _p(self._in(qf)),
                                                   _p(self._in(pf)), C.byref(dH), _p(terms)))
        return dH.value, terms

    def gradient(self, q):
        g = np.empty(self.N)
        self._chk(self.lib.bchmc_gradient(self.h, _p(self._in(q)), _p(g)))
        return g

    def forward(self, q, rsd=-1):
        self._chk(self.lib.bchmc_forward(self.h, _p(self._in(q)), int(rsd)))

    def probe_displacement(self, psi, rsd, with_force=False):
        """Tests, diagnostics: the particle stage of the forward model (binning, mass assignment, sum of rho) from a
        displacement given in real space, ``psi[3, N]`` = (x, y, z), instead of from a field; with ``with_force`` also
        the likelihood force up to V (needs the inputs uploaded).  ``fetch("posx" / "rho" / "deltaX" / "part_like" /
        "Vx" ...)`` afterwards, like after ``forward``."""
        psi = np.ascontiguousarray(psi, dtype=np.float64).reshape(-1)
        if psi.size != 3 * self.N:
            raise ValueError("psi must hold 3 N = %d values, got %d" % (3 * self.N, psi.size))
        self._chk(self.lib.bchmc_probe_displacement(self.h, _p(psi), int(rsd), int(bool(with_force))))

    def probe_displacement_z(self, psi, rsd, with_force=False, store_psi=True):
        """Tests: ``probe_displacement`` through the fused z pass + binning (k_zbin_direct; 256^3, 512^3, 128^3 under
        BCHMC_ZBIN_128=1; BchmcError UNSUPPORTED elsewhere).  ``store_psi``: Psi is stored on the way (``fetch("psix")``
        is what the kernel used: psi after the z round trip); without it the interior-step variant runs."""
        psi = np.ascontiguousarray(psi, dtype=np.float64).reshape(-1)
        if psi.size != 3 * self.N:
            raise ValueError("psi must hold 3 N = %d values, got %d" % (3 * self.N, psi.size))
        self._chk(self.lib.bchmc_probe_displacement_z(self.h, _p(psi), int(rsd), int(bool(with_force)),
                                                      int(bool(store_psi))))

    # ---- device-resident entry points (torch tensors on the engine's device, float64, contiguous) ----
    @staticmethod
    def _dptr(t):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
        return C.c_void_p(t.data_ptr())

    def leapfrog_device(self, q0, p0, q1, p1, eps, neps):
        self._chk(self.lib.bchmc_leapfrog_device(self.h, self._dptr(q0), self._dptr(p0), self._dptr(q1),
                                                 self._dptr(p1), float(eps), int(neps)))

    def steps_done(self):
        v = C.c_uint64()
        self._chk(self.lib.bchmc_steps_done(self.h, C.byref(v)))
        return v.value

    def energies_device(self, q, p):
        out = np.zeros(3)
        self._chk(self.lib.bchmc_energies_device(self.h, self._dptr(q), self._dptr(p), _p(out)))
        return out

    def sync(self):
        self._chk(self.lib.bchmc_sync(self.h))

    @property
    def stream(self):
        return self.lib.bchmc_stream(self.h)

    # ---- device-resident chain ------------------------------------------------
    def chain_set_state(self, q):
        self._chk(self.lib.bchmc_chain_set_state(self.h, _p(self._in(q))))

    def chain_get_state(self):
        q = np.empty(self.N)
        self._chk(self.lib.bchmc_chain_get_state(self.h, _p(q)))
        return q

    def chain_set_momenta(self, p):
        self._chk(self.lib.bchmc_chain_set_momenta(self.h, _p(self._in(p))))

    def chain_get_momenta(self):
        p = np.empty(self.N)
        self._chk(self.lib.bchmc_chain_get_momenta(self.h, _p(p)))
        return p

    def chain_draw_momenta(self, seed, attempt):
        self._chk(self.lib.bchmc_chain_draw_momenta(self.h, int(seed), int(attempt)))

    def chain_draw_momenta_mt19937(self, rng):
        """draw_momenta (HMC_momenta.cc:42-94) on the device from ``rng`` (a ``GslMT19937``), which is advanced in
        place to the state GSL holds after the draw.  Returns the number of words consumed."""
        mt, mti = rng.get_state()
        mt = np.ascontiguousarray(mt, dtype=np.uint32).copy()
        m = C.c_int32(int(mti))
        used = C.c_uint64()
        self._chk(self.lib.bchmc_chain_draw_momenta_mt19937(self.h, _u32p(mt), C.byref(m), C.byref(used)))
        rng.set_state(mt, m.value)
        return used.value

    def _with_rng(self, rng, call):
        """Run ``call(mt, mti, used)`` on the state of ``rng`` (a ``GslMT19937``); the generator is advanced in place
        when the call succeeds, and left as it was when it raises.  Returns the words consumed."""
        mt, mti = rng.get_state()
        mt = np.ascontiguousarray(mt, dtype=np.uint32).copy()
        m = C.c_int32(int(mti))
        used = C.c_uint64()
        self._chk(call(_u32p(mt), C.byref(m), C.byref(used)))
        rng.set_state(mt, m.value)
        return used.value

    def setup_random_test(self, rng, window_type=1, data_model=0, negative_obs=False, random_test_rsd=False,
                          sigma_min=None, sigma_fac=0.0, deltas=True):
        """setup_random_test (barcoderunner.cc:42-205) on the device from ``rng``: the truth field from ``signal_PS``,
        its forward model, the window, nobs and noise, which the engine then holds as if they had been uploaded
        (``fetch("window")`` ...).  Defaults: data/input.par.  Returns (words used, delta_lag, delta_eul); the two
        arrays are None with ``deltas=False``."""
        o = MockOpts(int(window_type), int(data_model), int(bool(negative_obs)), int(bool(random_test_rsd)),
                     float(self.params.sigma_min if sigma_min is None else sigma_min), float(sigma_fac))
        dl, de = (np.empty(self.N), np.empty(self.N)) if deltas else (None, None)
        used = self._with_rng(rng, lambda mt, m, u: self.lib.bchmc_setup_random_test(
            self.h, C.byref(o), mt, m, u, None if dl is None else _p(dl), None if de is None else _p(de)))
        return used, dl, de

    def setup_random_test_poisson(self, rng, seed, stream=0, window_type=1, random_test_rsd=False, deltas=True):
        """The Poissonian mock of setup_random_test (data_model 0 under likelihood 0, which ``setup_random_test``
        refuses): truth, forward model and window from ``rng`` exactly as there, then nobs ~ Poisson(rho_c (1 + deltaX))
        inside the window from the counter-based sampler of ``poisson_draw`` under (seed, stream), noise = 0.  Returns
        (words used, delta_lag, delta_eul)."""
        o = MockOpts(int(window_type), 0, 0, int(bool(random_test_rsd)), float(self.params.sigma_min), 0.0)
        dl, de = (np.empty(self.N), np.empty(self.N)) if deltas else (None, None)
        used = self._with_rng(rng, lambda mt, m, u: self.lib.bchmc_setup_random_test_poisson(
            self.h, C.byref(o), mt, m, u, int(seed), int(stream), None if dl is None else _p(dl),
            None if de is None else _p(de)))
        return used, dl, de

    def make_initial_guess(self, rng, initial_guess=0, file_field=None, smoothing_type=1, smoothing_scale=0.0):
        """make_initial_guess (barcoderunner.cc:207-247): sets the resident chain state; 2, 3 and 4 draw from ``rng``
        (0 and 1 leave it alone, and ``rng`` may be None).  Returns the words used."""
        ff = None if file_field is None else _p(self._in(file_field))
        if rng is None:
            used = C.c_uint64()
            self._chk(self.lib.bchmc_make_initial_guess(self.h, int(initial_guess), ff, int(smoothing_type),
                                                        float(smoothing_scale), None, None, C.byref(used)))
            return used.value
        return self._with_rng(rng, lambda mt, m, u: self.lib.bchmc_make_initial_guess(
            self.h, int(initial_guess), ff, int(smoothing_type), float(smoothing_scale), mt, m, u))

    def chain_attempt(self, eps, neps):
        dH, done = C.c_double(), C.c_uint64()
        terms = np.zeros(6)
        self._chk(self.lib.bchmc_chain_attempt(self.h, float(eps), int(neps), C.byref(dH), _p(terms), C.byref(done)))
        return dH.value, terms, done.value

    def chain_get_proposal(self):
        q1, p1 = np.empty(self.N), np.empty(self.N)
        self._chk(self.lib.bchmc_chain_get_proposal(self.h, _p(q1), _p(p1)))
        return q1, p1

    def chain_accept(self, accepted):
        self._chk(self.lib.bchmc_chain_accept(self.h, int(bool(accepted))))

    def measure_spectrum(self, signal=None, n_bin=200, source=None):
        """measure_spectrum (field_statistics.cpp:20-90) of a host field, or of the resident chain state when
        ``signal`` is None (nothing but 2 x n_bin doubles crosses PCIe).  ``source``: "host", "chain" or "deltaX" (the
        handle's deltaX, what barcoderunner.cc:87 measures) as in ``measure_corr``.  Returns (kmode, power)."""
        kmode, power = np.empty(n_bin), np.empty(n_bin)
        sig = None if signal is None else _p(self._in(signal))
        if source is None:
            self._chk(self.lib.bchmc_measure_spectrum(self.h, sig, int(n_bin), _p(kmode), _p(power)))
        else:
            self._chk(self.lib.bchmc_measure_spectrum_src(self.h, CORR_SOURCES[source], sig, int(n_bin), _p(kmode),
                                                          _p(power)))
        return kmode, power

    def measure_spectrum2d(self, signal=None, n_bin=200, source=None):
        """measure_spec2D (tools/2D_powspec.cc:25-110), plane-parallel along z: the anisotropic power spectrum of a host
        field, of the resident chain state (the default without a signal) or of the handle's deltaX, sources as in
        ``measure_corr``.  Returns (kmode, nmode, power) shaped (n_bin, n_bin) with k_perp as the first axis (the tool's
        element ``par + n_bin * perp``); kmode is the mean 3-D |k| of a bin."""
        if source is None:
            source = "chain" if signal is None else "host"
        n_bin = int(n_bin)
        size = n_bin ** 2 if 1 <= n_bin <= 2048 else 1  # out of range: the library refuses before it writes
        kmode, power, nmode = np.empty(size), np.empty(size), np.empty(size, dtype=np.uint64)
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_measure_spectrum2d(self.h, CORR_SOURCES[source], sig, n_bin, _p(kmode),
                                                    nmode.ctypes.data_as(C.POINTER(C.c_uint64)), _p(power)))
        shape = (n_bin, n_bin)
        return kmode.reshape(shape), nmode.reshape(shape), power.reshape(shape)

    def measure_cross_spectrum(self, signal_a=None, signal_b=None, n_bin=200, source_a=None, source_b=None):
        """The cross-spectrum of two fields in measure_spectrum's bins (bchmc_measure_cross_spectrum).  Each side is a
        host field, the resident chain state (the default without a signal) or the handle's deltaX, sources as in
        ``measure_corr``.  Returns (kmode, nmode, power_a, power_b, cross, coeff), n_bin each;
        coeff = cross / sqrt(power_a power_b), 0 in an empty bin."""
        src = [s if s is not None else ("chain" if sig is None else "host")
               for s, sig in ((source_a, signal_a), (source_b, signal_b))]
        n_bin = int(n_bin)
        size = n_bin if 1 <= n_bin <= 2048 else 1  # out of range: the library refuses before it writes
        kmode, pa, pb, cross, coeff = (np.empty(size) for _ in range(5))
        nmode = np.empty(size, dtype=np.uint64)
        sa = None if signal_a is None else _p(self._in(signal_a))
        sb = None if signal_b is None else _p(self._in(signal_b))
        self._chk(self.lib.bchmc_measure_cross_spectrum(self.h, CORR_SOURCES[src[0]], sa, CORR_SOURCES[src[1]], sb, n_bin,
                                                        _p(kmode), nmode.ctypes.data_as(C.POINTER(C.c_uint64)), _p(pa),
                                                        _p(pb), _p(cross), _p(coeff)))
        return kmode, nmode, pa, pb, cross, coeff

    # ---- ensemble accumulators (bchmc_ensemble_*) --------------------------------------------------
    def ensemble_add(self, slot, signal=None, source=None):
        """One more sample into running accumulator ``slot`` (0 .. ENS_SLOTS - 1): a host field, the resident chain
        state (the default without a signal) or the handle's deltaX, sources as in ``measure_corr``.  One Welford step
        per cell on the device; the sample does not cross PCIe unless it is a host field."""
        if source is None:
            source = "chain" if signal is None else "host"
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_ensemble_add(self.h, int(slot), CORR_SOURCES[source], sig))

    def ensemble_count(self, slot):
        n = C.c_uint64()
        self._chk(self.lib.bchmc_ensemble_count(self.h, int(slot), C.byref(n)))
        return n.value

    def ensemble_fetch(self, slot, what="mean"):
        """``what``: "mean" (needs one sample), "variance" = m2 / (count - 1) or "std" (two), "m2" (the raw sum of
        squared deviations).  Returns N doubles."""
        out = np.empty(self.N)
        self._chk(self.lib.bchmc_ensemble_fetch(self.h, int(slot), ENS_WHAT[what] if isinstance(what, str) else int(what),
                                                _p(out)))
        return out

    def ensemble_export(self, slot):
        """(count, mean, m2) of a slot: what ``ensemble_merge`` of another handle takes.  An empty slot gives zeros."""
        count = self.ensemble_count(slot)
        if count == 0:
            return 0, np.zeros(self.N), np.zeros(self.N)
        return count, self.ensemble_fetch(slot, "mean"), self.ensemble_fetch(slot, "m2")

    def ensemble_merge(self, slot, count, mean, m2):
        """Folds another accumulator of the same grid (another chain, another GPU, an earlier run) into ``slot`` by the
        pairwise update of Chan, Golub & LeVeque.  ``count == 0`` is a no-op; a merge into an empty slot copies."""
        count = int(count)
        if count == 0:
            self._chk(self.lib.bchmc_ensemble_merge(self.h, int(slot), 0, None, None))
            return
        self._chk(self.lib.bchmc_ensemble_merge(self.h, int(slot), count, _p(self._in(mean)), _p(self._in(m2))))

    def ensemble_reset(self, slot):
        """count = 0 and zeroed arrays; the buffers are kept."""
        self._chk(self.lib.bchmc_ensemble_reset(self.h, int(slot)))

    def ensemble_release(self):
        """Frees the buffers of every slot; a later ``ensemble_add`` takes them again."""
        self._chk(self.lib.bchmc_ensemble_release(self.h))

    # ---- the T-web of a sample (bchmc_tweb_*) ---------------------------------------------------------
    def tweb_classify(self, signal=None, source=None, smoothing_scale=0.0, lambda_th=0.0, accumulate=False,
                      want_lambda=True, want_type=True):
        """The cosmic-web type of every cell of a host field, of the resident chain state (the default without a
        signal) or of the handle's deltaX, sources as in ``measure_corr``: eigenvalues of the tidal tensor of the field
        smoothed with a Gaussian of ``smoothing_scale`` Mpc/h, type = how many exceed ``lambda_th`` (0 void, 1 sheet,
        2 filament, 3 knot; 255 where the tensor is not finite).  ``accumulate``: also one more sample into the
        posterior counters.  Returns a dict: ``lambda`` (3, N) descending or None, ``type`` (N,) uint8 or None,
        ``n_type`` (4,) uint64, ``n_nonfinite``, ``mass_type`` (4,) sums of 1 + x over each type's cells.  A sample with
        non-finite cells raises under ``accumulate`` (nothing is added); the dict is then the exception's ``result``."""
        if source is None:
            source = "chain" if signal is None else "host"
        sig = None if signal is None else _p(self._in(signal))
        opts = TwebOpts(float(smoothing_scale), float(lambda_th), int(accumulate), 0)
        lam = np.empty((3, self.N)) if want_lambda else None
        typ = np.empty(self.N, dtype=np.uint8) if want_type else None
        st = TwebStats()
        rc = self.lib.bchmc_tweb_classify(self.h, CORR_SOURCES[source], sig, C.byref(opts),
                                          None if lam is None else _p(lam.reshape(-1)),
                                          None if typ is None else typ.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st))
        res = {"lambda": lam, "type": typ, "n_type": np.array(list(st.n_type), dtype=np.uint64),
               "n_nonfinite": int(st.n_nonfinite), "mass_type": np.array(list(st.mass_type))}
        if rc:
            err = BchmcError(rc, self.lib.bchmc_strerror(rc).decode(), self.lib.bchmc_last_error(self.h).decode())
            err.result = res if (accumulate and st.n_nonfinite) else None
            raise err
        if accumulate:
            self._tweb_par = (float(smoothing_scale), float(lambda_th))
        return res

    def tweb_tensor(self, component):
        """One component ("xx", "xy", "xz", "yy", "yz", "zz" or 0..5) of the tensor of the last ``tweb_classify``."""
        out = np.empty(self.N)
        c = TWEB_COMPONENTS[component] if isinstance(component, str) else int(component)
        self._chk(self.lib.bchmc_tweb_tensor(self.h, c, _p(out)))
        return out

    def tweb_samples(self):
        n = C.c_uint64()
        self._chk(self.lib.bchmc_tweb_samples(self.h, C.byref(n)))
        return n.value

    def tweb_fetch(self, type, as_probability=False):
        """The posterior counters of one type ("void", "sheet", "filament", "knot" or 0..3): N uint32, or with
        ``as_probability`` count / samples as N doubles (needs one sample)."""
        t = TWEB_TYPES[type] if isinstance(type, str) else int(type)
        out = np.empty(self.N, dtype=np.float64 if as_probability else np.uint32)
        self._chk(self.lib.bchmc_tweb_fetch(self.h, t, int(bool(as_probability)), out.ctypes.data_as(C.c_void_p)))
        return out

    def tweb_export(self):
        """(samples, counters (4, N) uint32): what ``tweb_merge`` of another handle takes."""
        return self.tweb_samples(), np.stack([self.tweb_fetch(t) for t in range(4)])

    def tweb_merge(self, samples, counts):
        """Adds another chain's counters (4, N), type-major, of ``samples`` samples.  ``samples == 0`` is a no-op."""
        samples = int(samples)
        if samples == 0:
            self._chk(self.lib.bchmc_tweb_merge(self.h, 0, None))
            return
        c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if c.size != 4 * self.N:
            raise ValueError("expected %d counters, got %d" % (4 * self.N, c.size))
        self._chk(self.lib.bchmc_tweb_merge(self.h, samples, c.ctypes.data_as(C.POINTER(C.c_uint32))))

    def tweb_reset(self):
        """samples = 0 and zeroed counters; the buffers are kept."""
        self._chk(self.lib.bchmc_tweb_reset(self.h))
        self._tweb_par = None

    def tweb_release(self):
        """Frees every buffer of the feature, the counters included; a later ``tweb_classify`` takes them again."""
        self._chk(self.lib.bchmc_tweb_release(self.h))
        self._tweb_par = None

    # ---- the bispectrum of a sample (bchmc_bispectrum) ---------------------------------------------------
    def bispectrum(self, signal=None, source=None, k_min=0.0, dk=None, n_shell=8, units="h/Mpc"):
        """The bispectrum of a host field, of the resident chain state (the default without a signal) or of the
        handle's deltaX, sources as in ``measure_corr``, by the FFT estimator: ``n_shell`` (1..32) shells of |k| from
        ``k_min`` in steps of ``dk``, in h/Mpc or with ``units="kf"`` in units of the fundamental 2 pi / L (``dk``
        None: one fundamental), all triplets s1 <= s2 <= s3.  Returns a dict: ``triplets`` (T, 3) int32, ``b`` (T,),
        ``ntri`` (T,) the number of closed mode triples, ``q`` (T,) the reduced bispectrum, and per shell ``kmean``,
        ``nmode`` (uint64) and ``power``."""
        if source is None:
            source = "chain" if signal is None else "host"
        if units not in ("h/Mpc", "kf"):
            raise ValueError("units must be 'h/Mpc' or 'kf', got %r" % (units,))
        kf = 2.0 * np.pi / float(self.params.L)
        scale = kf if units == "kf" else 1.0
        dk = kf if dk is None else float(dk) * scale
        n = int(n_shell)
        sig = None if signal is None else _p(self._in(signal))
        opts = BispecOpts(float(k_min) * scale, dk, n, 0)
        ns = min(max(n, 0), BISPEC_MAX_SHELL)  # a refused n_shell reaches the library with arrays that are never written
        trip = bispec_triplets(ns)
        T = len(trip)
        b, ntri, q = np.zeros(T), np.zeros(T), np.zeros(T)
        kmean, nmode, power = np.zeros(ns), np.zeros(ns, dtype=np.uint64), np.zeros(ns)
        self._chk(self.lib.bchmc_bispectrum(self.h, CORR_SOURCES[source], sig, C.byref(opts), _p(b), _p(ntri), _p(q),
                                            _p(kmean), nmode.ctypes.data_as(C.POINTER(C.c_uint64)), _p(power)))
        return dict(triplets=trip, b=b, ntri=ntri, q=q, kmean=kmean, nmode=nmode, power=power)

    def bispec_release(self):
        """Frees every buffer of the bispectrum; a later ``bispectrum`` takes them again and rebuilds its table."""
        self._chk(self.lib.bchmc_bispec_release(self.h))

    # ---- RSD multipoles of a sample (bchmc_measure_*multipoles) --------------------------------------------
    def measure_multipoles(self, signal=None, source=None, n_bin=200):
        """The Legendre multipoles P_l(k), l = 0, 2, 4, about the line of sight z of a host field, of the resident chain
        state (the default without a signal) or of the handle's deltaX, sources as in ``measure_corr``, in
        ``measure_spectrum``'s bins and normalisation.  Returns a dict of n_bin values each: ``k`` (mean |k|), ``nmode``
        (uint64), ``leg2`` / ``leg4`` (the mean of L_2 / L_4 over the bin's modes: the discrete-mu leakage) and ``p0``,
        ``p2``, ``p4``.  Bitwise repeatable."""
        if source is None:
            source = "chain" if signal is None else "host"
        n_bin = int(n_bin)
        size = n_bin if 1 <= n_bin <= 2048 else 1  # out of range: the library refuses before it writes
        k, leg, p, nmode = np.empty(size), np.empty((2, size)), np.empty((3, size)), np.empty(size, dtype=np.uint64)
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_measure_multipoles(self.h, CORR_SOURCES[source], sig, n_bin, _p(k),
                                                    nmode.ctypes.data_as(C.POINTER(C.c_uint64)), _p(leg.reshape(-1)),
                                                    _p(p.reshape(-1))))
        return dict(k=k, nmode=nmode, leg2=leg[0], leg4=leg[1], p0=p[0], p2=p[1], p4=p[2])

    def measure_cross_multipoles(self, signal_a=None, signal_b=None, source_a=None, source_b=None, n_bin=200):
        """The multipoles of two fields and of their cross-spectrum in one pass, each side as in ``measure_multipoles``.
        Returns a dict: ``k, nmode, leg2, leg4`` and ``paa0, paa2, paa4``, ``pbb0 ..``, ``pab0 ..``; ``paa*`` and
        ``pbb*`` are what ``measure_multipoles`` gives for each side, bit for bit."""
        src = [s if s is not None else ("chain" if sig is None else "host")
               for s, sig in ((source_a, signal_a), (source_b, signal_b))]
        n_bin = int(n_bin)
        size = n_bin if 1 <= n_bin <= 2048 else 1
        k, leg, nmode = np.empty(size), np.empty((2, size)), np.empty(size, dtype=np.uint64)
        p = {t: np.empty((3, size)) for t in ("aa", "bb", "ab")}
        sa = None if signal_a is None else _p(self._in(signal_a))
        sb = None if signal_b is None else _p(self._in(signal_b))
        self._chk(self.lib.bchmc_measure_cross_multipoles(
            self.h, CORR_SOURCES[src[0]], sa, CORR_SOURCES[src[1]], sb, n_bin, _p(k),
            nmode.ctypes.data_as(C.POINTER(C.c_uint64)), _p(leg.reshape(-1)), _p(p["aa"].reshape(-1)),
            _p(p["bb"].reshape(-1)), _p(p["ab"].reshape(-1))))
        out = dict(k=k, nmode=nmode, leg2=leg[0], leg4=leg[1])
        for t, arr in p.items():
            for i, l in enumerate((0, 2, 4)):
                out["p%s%d" % (t, l)] = arr[i]
        return out

    def measure_corr_multipoles(self, signal=None, source=None, n_bin=None):
        """The multipoles xi_l(s), l = 0, 2, 4, of the correlation function in ``measure_corr``'s bins (``n_bin`` None:
        its automatic bin count), sources as there.  Returns a dict: ``r`` (mean separation), ``nmode``, ``leg2``,
        ``leg4``, ``xi0``, ``xi2``, ``xi4``."""
        if source is None:
            source = "chain" if signal is None else "host"
        n_bin = int(n_bin) if n_bin else corr_auto_nbin(self.Nx, self.params.L)
        size = n_bin if 1 <= n_bin <= 2048 else 1
        r, leg, xi, nmode = np.empty(size), np.empty((2, size)), np.empty((3, size)), np.empty(size, dtype=np.uint64)
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_measure_corr_multipoles(self.h, CORR_SOURCES[source], sig, n_bin, _p(r),
                                                         nmode.ctypes.data_as(C.POINTER(C.c_uint64)), _p(leg.reshape(-1)),
                                                         _p(xi.reshape(-1))))
        return dict(r=r, nmode=nmode, leg2=leg[0], leg4=leg[1], xi0=xi[0], xi2=xi[1], xi4=xi[2])

    def multipoles_release(self):
        """Frees every buffer of the multipoles; a later call takes them again and gives the same bits."""
        self._chk(self.lib.bchmc_multipoles_release(self.h))

    def _measure_corr(self, fn, cells, signal, n_bin, source):
        if source is None:
            source = "chain" if signal is None else "host"
        n_bin = int(n_bin) if n_bin else corr_auto_nbin(self.Nx, self.params.L)
        size = n_bin ** cells if 1 <= n_bin <= 2048 else 1  # out of range: the library refuses before it writes
        rmode, corr, nmode = np.empty(size), np.empty(size), np.empty(size, dtype=np.uint64)
        sig = None if signal is None else _p(self._in(signal))
        self._chk(fn(self.h, CORR_SOURCES[source], sig, n_bin, _p(rmode), nmode.ctypes.data_as(C.POINTER(C.c_uint64)),
                     _p(corr)))
        shape = (n_bin,) * cells
        return rmode.reshape(shape), nmode.reshape(shape), corr.reshape(shape)

    def measure_corr(self, signal=None, n_bin=0, source=None):
        """measure_corr_grid (tools/corr_fct.cc:20-80) of a host field (``source="host"``), of the resident chain state
        (``"chain"``, the default without a signal) or of the handle's deltaX (``"deltaX"``).  ``n_bin=0``: the tools'
        automatic bin count.  Returns (rmode, nmode, corr), n_bin each."""
        return self._measure_corr(self.lib.bchmc_measure_corr, 1, signal, n_bin, source)

    def measure_corr2d(self, signal=None, n_bin=0, source=None):
        """measure_corr2D (tools/2D_corr_fct.cc:23-124), plane-parallel along z.  Returns (rmode, nmode, corr) shaped
        (n_bin, n_bin) with r_perp as the first axis (the tool's element ``par + n_bin * perp``)."""
        return self._measure_corr(self.lib.bchmc_measure_corr2d, 2, signal, n_bin, source)

    def interp_upres(self, n_out, signal=None, source=None):
        """interp_field (tools/interp_upres.cc:59-86): the source's field on an n_out^3 grid by CIC interpolation.
        Sources as in ``measure_corr``.  Returns n_out^3 doubles."""
        if source is None:
            source = "chain" if signal is None else "host"
        n_out = int(n_out)
        out = np.empty(n_out ** 3 if 4 <= n_out <= 1024 else 1)  # out of range: the library refuses before it writes
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_interp_upres(self.h, CORR_SOURCES[source], sig, n_out, _p(out)))
        return out

    def measure_corr2d_interp(self, n_out, signal=None, n_bin=0, mode=0, l_max=np.inf, source=None):
        """tools/2D_corr_fct_interp.cc: the source lifted to an n_out^3 grid by CIC interpolation (``mode=0``, binning
        the cells with r_par < l_max and r_perp < l_max) or by zero padding of its power spectrum (``mode=1``, which
        ignores l_max), then measure_corr2D there.  ``n_bin=0``: the tool's automatic count ceil(rmax / d_out).
        Returns (rmode, nmode, corr) shaped (n_bin, n_bin) like ``measure_corr2d``."""
        if source is None:
            source = "chain" if signal is None else "host"
        n_out = int(n_out)
        n_bin = int(n_bin) if n_bin else corr_auto_nbin(max(n_out, 1), self.params.L)
        size = n_bin ** 2 if 1 <= n_bin <= 2048 else 1
        rmode, corr, nmode = np.empty(size), np.empty(size), np.empty(size, dtype=np.uint64)
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_measure_corr2d_interp(self.h, CORR_SOURCES[source], sig, n_out, int(mode), float(l_max),
                                                       n_bin, _p(rmode), nmode.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       _p(corr)))
        shape = (n_bin, n_bin)
        return rmode.reshape(shape), nmode.reshape(shape), corr.reshape(shape)

    def upres_release(self):
        """Frees the fine grid's buffers, plans and tables; a later call rebuilds them."""
        self._chk(self.lib.bchmc_upres_release(self.h))

    def density_particles(self, x=None, y=None, z=None, w=None, mk=None, kernel_h=0.0, to_nobs=False, source="host",
                          download=True):
        """getDensity_NGP / _CIC / _TSC / _SPH (massFunctions.cc:49-495) of a free particle catalogue on the device: the raw
        density of the particles (x, y, z), each counting ``w[p]`` (1 without ``w``), on the handle's grid.  ``mk``: 0 NGP,
        1 CIC, 2 TSC, 3 SPH, None: the handle's.  ``kernel_h``: SPH scale length, 0: the handle's.  ``to_nobs``: the field
        also becomes the handle's nobs, as if uploaded.  ``source="forward"``: the handle's own particles after the last
        forward model (no columns).  ``download=False`` (with ``to_nobs``): the field stays on the device, nothing grid-sized
        crosses PCIe, and rho is None.  Returns (rho, stats), stats = dict(n_in, n_lost, max_per_tile)."""
        cols = [None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (x, y, z, w)]
        n_part = 0 if cols[0] is None else cols[0].size
        for a in cols[1:]:
            if a is not None and a.size != n_part:
                raise ValueError("catalogue columns differ in length")
        opts = DensityOpts(-1 if mk is None else int(mk), 0 if w is None else 1, float(kernel_h),
                           F_NOBS if to_nobs else -1, 0)
        st = DensityStats()
        if not download and not to_nobs:
            raise ValueError("download=False leaves the field nowhere unless to_nobs is set")
        out = np.empty(self.N) if download else None
        ptr = [None if a is None else _p(a) for a in cols]
        self._chk(self.lib.bchmc_density_particles(self.h, PART_SOURCES[source], ptr[0], ptr[1], ptr[2], ptr[3], n_part,
                                                   C.byref(opts), None if out is None else _p(out), C.byref(st)))
        return out, dict(n_in=int(st.n_in), n_lost=int(st.n_lost), max_per_tile=int(st.max_per_tile))

    def catalogue_release(self):
        """Frees the catalogue buffers of ``density_particles``; a later call rebuilds them."""
        self._chk(self.lib.bchmc_catalogue_release(self.h))

    def poisson_draw(self, signal=None, seed=0, stream=0, scale=1.0, rate_mode=0, n_in=None, use_window=False,
                     to_nobs=False, source=None, counts=True):
        """Poisson counts of a rate grid on the device (discrete_poisson_sample's draw, tools/poisson_upres.cc:23-65):
        cell c gets Poisson(scale (1 + x_c)) (``rate_mode=0``) or Poisson(scale x_c) (1), a pure function of (seed,
        stream, c, lambda_c).  ``signal``: n_in^3 values with n_in <= Nx (``n_in=None``: the cube root of its size);
        without it the resident chain state (``source="chain"``) or the handle's deltaX (``"deltaX"``).  ``use_window``:
        cells outside the uploaded window draw nothing; ``to_nobs``: the counts also become the handle's nobs.  The sample
        stays resident for ``poisson_positions`` / ``poisson_density``.  Returns (counts or None, stats), stats =
        dict(n_part, n_cells_drawn, max_count, n_capped, lambda_max)."""
        if source is None:
            source = "chain" if signal is None else "host"
        sig = None
        if signal is not None:
            sig = np.ascontiguousarray(signal, dtype=np.float64).reshape(-1)
            if n_in is None:
                n_in = int(round(sig.size ** (1.0 / 3.0)))
            if int(n_in) ** 3 != sig.size:
                raise ValueError("signal of %d values is no n_in^3 grid (n_in = %s)" % (sig.size, n_in))
        n_in = 0 if n_in is None else int(n_in)
        cells = (n_in or self.Nx) ** 3 if 0 <= n_in <= self.Nx else 1  # out of range: the library refuses before it writes
        out = np.empty(cells) if counts else None
        o = PoissonOpts(int(seed), int(stream), int(rate_mode), float(scale), int(bool(use_window)),
                        F_NOBS if to_nobs else -1)
        st = PoissonStats()
        self._chk(self.lib.bchmc_poisson_draw(self.h, CORR_SOURCES[source], None if sig is None else _p(sig), n_in,
                                              C.byref(o), None if out is None else _p(out), C.byref(st)))
        return out, dict(n_part=int(st.n_part), n_cells_drawn=int(st.n_cells_drawn), max_count=int(st.max_count),
                         n_capped=int(st.n_capped), lambda_max=float(st.lambda_max))

    def poisson_positions(self, first=0, m=None, n_part=None):
        """Particles [first, first + m) of the resident sample, upstream's order (cells in order, then within a cell), in
        box coordinates.  ``m=None``: up to ``n_part`` (the draw's stats).  Returns (x, y, z)."""
        if m is None:
            if n_part is None:
                raise ValueError("give m, or n_part of the draw")
            m = int(n_part) - int(first)
        m = max(int(m), 0)
        x, y, z = np.empty(m), np.empty(m), np.empty(m)
        self._chk(self.lib.bchmc_poisson_positions(self.h, int(first), m, _p(x), _p(y), _p(z)))
        return x, y, z

    def poisson_density(self, mk=None, kernel_h=0.0, to_nobs=False, download=True):
        """The resident sample onto the handle's grid through ``density_particles``' pipeline, the positions made on the
        device batch by batch (with ``mk=1``: tools/poisson_upres.cc end to end).  Arguments and result as there."""
        if not download and not to_nobs:
            raise ValueError("download=False leaves the field nowhere unless to_nobs is set")
        opts = DensityOpts(-1 if mk is None else int(mk), 0, float(kernel_h), F_NOBS if to_nobs else -1, 0)
        st = DensityStats()
        out = np.empty(self.N) if download else None
        self._chk(self.lib.bchmc_poisson_density(self.h, C.byref(opts), None if out is None else _p(out), C.byref(st)))
        return out, dict(n_in=int(st.n_in), n_lost=int(st.n_lost), max_per_tile=int(st.max_per_tile))

    def poisson_release(self):
        """Frees the resident sample and its scratch; a later ``poisson_draw`` rebuilds them."""
        self._chk(self.lib.bchmc_poisson_release(self.h))

    def interp_particles(self, x=None, y=None, z=None, fields=(), kernel="cic", path=None, source="host"):
        """interpolate_CIC / interpolate_TSC / interpolate_TSC_multi (interpolate_grid.cpp:108-286) on the device: one to
        four grid fields read at the particles (x, y, z).  A field is an array of N values, ``"chain"`` (the resident chain
        state), ``"deltax"`` or a bchmc_field name (``FIELDS``: ``"psix"``, ``"Vx"``, ``"window"`` ...).  ``kernel``:
        ``"cic"`` or ``"tsc"``.  ``path``: None the engine decides, ``"direct"`` / 0, ``"tile"`` / 1.
        ``source="forward"``: the handle's own particles after the last forward model (no columns).  A lost particle (TSC
        outside its domain, a non-finite coordinate) is NaN in every field.
        Returns (values[n_fields, n_part], stats), stats = dict(n_in, n_lost, max_per_tile, path_used)."""
        cols = [None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (x, y, z)]
        n_part = self.N if source == "forward" else (0 if cols[0] is None else cols[0].size)
        for a in cols[1:]:
            if a is not None and cols[0] is not None and a.size != cols[0].size:
                raise ValueError("catalogue columns differ in length")
        fields = list(fields)
        keep, fd = [], (InterpField * max(len(fields), 1))()
        lower = {k.lower(): v for k, v in FIELDS.items()}
        for k, f in enumerate(fields):
            if isinstance(f, str):
                name = f.lower()
                if name == "chain":
                    fd[k] = InterpField(CORR_SOURCES["chain"], 0, None)
                elif name == "deltax":
                    fd[k] = InterpField(CORR_SOURCES["deltaX"], 0, None)
                elif name in lower:
                    fd[k] = InterpField(INTERP_HANDLE_FIELD, lower[name], None)
                else:
                    raise ValueError("unknown field %r" % f)
            else:
                keep.append(self._in(f))
                fd[k] = InterpField(CORR_SOURCES["host"], 0, _p(keep[-1]))
        out = np.empty((len(fields), n_part))
        opts = InterpOpts(INTERP_KERNELS[kernel] if isinstance(kernel, str) else int(kernel), INTERP_PATHS[path])
        st = InterpStats()
        ptr = [None if a is None else _p(a) for a in cols]
        self._chk(self.lib.bchmc_interp_particles(self.h, PART_SOURCES[source], ptr[0], ptr[1], ptr[2], n_part, fd,
                                                  len(fields), C.byref(opts), _p(out.reshape(-1)) if out.size else None,
                                                  C.byref(st)))
        return out, dict(n_in=int(st.n_in), n_lost=int(st.n_lost), max_per_tile=int(st.max_per_tile),
                         path_used=int(st.path_used))

    def interp_release(self):
        """Frees the buffers of ``interp_particles``; a later call rebuilds them."""
        self._chk(self.lib.bchmc_interp_release(self.h))

    def chain_forward(self, rsd=-1):
        """Lag2Eul of the resident chain state: ``forward(chain_get_state(), rsd)`` without the field leaving the
        device.  ``fetch("deltaX")`` etc. afterwards."""
        self._chk(self.lib.bchmc_chain_forward(self.h, int(rsd)))

    def hamiltonian_mass(self, signal=None, n_bin=200, mass_factor=1.0, iGibbs=1, s_eps_total=0):
        """Hamiltonian_mass (HMC_mass.cc:315-368) on the device at a host field, or at the resident chain state when
        ``signal`` is None; the engine then uses the new mass as if it had been uploaded.  Defaults: N_bin and
        mass_factor of data/input.par:129,150.  Returns (mass_f, mass_r), None where the mass_type has none."""
        t = int(self.params.mass_type)
        mf = np.empty(self.N) if t in MASS_F_TYPES else None
        mr = np.empty(self.N) if t in MASS_R_TYPES else None
        o = MassOpts(int(n_bin), float(mass_factor), int(iGibbs), int(s_eps_total))
        sig = None if signal is None else _p(self._in(signal))
        self._chk(self.lib.bchmc_hamiltonian_mass(self.h, sig, C.byref(o), None if mf is None else _p(mf),
                                                  None if mr is None else _p(mr)))
        return mf, mr

    def tile_info(self):
        out = (C.c_int32 * 8)()
        self._chk(self.lib.bchmc_tile_info(self.h, out))
        keys = ("tiled", "one_pass", "cap", "cap_alloc", "watch", "tile_shape", "unrolled81", "alpt_planes")
        info = dict(zip(keys, [int(v) for v in out]))
        w = info["tile_shape"]
        info["tile_shape"] = (w & 255, (w >> 8) & 255, (w >> 16) & 255)  # (tx, ty, tz) in cells; zeros without tiles
        return info

    # ---- measurement ---------------------------------------------------------------------------
    def profile(self, enable):
        self._chk(self.lib.bchmc_profile(self.h, int(bool(enable))))

    def profile_read(self):
        ms = np.zeros(K_COUNT)
        n = (C.c_uint64 * K_COUNT)()
        self._chk(self.lib.bchmc_profile_read(self.h, _p(ms), n))
        return {self.lib.bchmc_kernel_name(i).decode(): (float(ms[i]), int(n[i])) for i in range(K_COUNT)}


class Comm:
    """The cross-chain record exchange of include/bchmc.h (``bchmc_comm``): RCCL transport (``unique_id`` from rank 0)
    or a custom host all-gather (``allgather(send_bytes) -> bytes of all ranks``; tests, MPI, torch.distributed)."""

    def __init__(self, rank, world, device=0, unique_id=None, allgather=None):
        self.lib = load()
        self.rank, self.world = int(rank), int(world)
        self.h = C.c_void_p()
        self._cb = None
        if allgather is not None or world == 1 and unique_id is None:
            def _fn(_ctx, send, recv, nbytes):
                try:
                    out = allgather(C.string_at(send, nbytes))
                    if len(out) != nbytes * self.world:
                        return 2
                    C.memmove(recv, out, len(out))
                    return 0
                except Exception:  # a Python exception must not unwind through the C caller
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cb = ALLGATHER_FN(_fn) if allgather is not None else C.cast(None, ALLGATHER_FN)
            rc = self.lib.bchmc_comm_create_custom(self._cb, None, self.rank, self.world, C.byref(self.h))
        else:
            buf = (C.c_ubyte * UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
            rc = self.lib.bchmc_comm_create(buf, self.rank, self.world, int(device), C.byref(self.h))
        if rc:
            detail = self.lib.bchmc_comm_last_error(self.h).decode() if self.h else ""
            self.close()
            raise BchmcError(rc, self.lib.bchmc_strerror(rc).decode(), detail)

    @staticmethod
    def unique_id():
        lib = load()
        buf = (C.c_ubyte * UNIQUE_ID_BYTES)()
        rc = lib.bchmc_comm_unique_id(buf)
        if rc:
            raise BchmcError(rc, lib.bchmc_strerror(rc).decode(), "bchmc_comm_unique_id (is librccl loadable?)")
        return bytes(buf)

    def exchange(self, records):
        """records: list of (epsilon, accepted, neps) of this rank's finished attempts (may be empty).
        Returns [(rank, epsilon, accepted, neps), ...] of every rank's contribution to this exchange."""
        n = len(records)
        mine = (EpsRecord * max(n, 1))()
        for i, (eps, acc, neps) in enumerate(records):
            mine[i].epsilon, mine[i].accepted, mine[i].neps = float(eps), int(bool(acc)), int(neps)
        cap = self.world * EPS_BATCH
        out, who, got = (EpsRecord * cap)(), (C.c_int * cap)(), C.c_int(0)
        rc = self.lib.bchmc_eps_exchange(self.h, mine, n, out, who, cap, C.byref(got))
        if rc:
            raise BchmcError(rc, self.lib.bchmc_strerror(rc).decode(), self.lib.bchmc_comm_last_error(self.h).decode())
        return [(int(who[i]), float(out[i].epsilon), bool(out[i].accepted), int(out[i].neps)) for i in range(got.value)]

    def pending(self):
        return int(self.lib.bchmc_comm_pending(self.h))

    def info(self):
        """What the communicator itself reports (not what the caller asked for): world, rank, transport."""
        return dict(world=int(self.lib.bchmc_comm_world(self.h)), rank=int(self.lib.bchmc_comm_rank(self.h)),
                    transport=self.lib.bchmc_comm_transport(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.bchmc_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
