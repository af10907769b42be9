"""CPU checks around the 2-D power spectrum P(k_perp, k_par): the numpy restatement of the reference's tool
(tests/spec2d_restatement.py) against itself, against closed forms and against the structure the engine's tables rely
on (S2: every mode is binned; counts = rows of the perp bin x Hermitian weights of the par bin's run), the declarations
of the new entry point through every layer, and the file writer."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from barcode_amd import inputs, io
from barcode_amd.params import HamilParams
from tests import spec2d_restatement as sr
from tests.test_corr_restatement import CTYPE, header_args, rel_bins, rel_max
from tests.util import TOL_FIELD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (4, 5, 8, 9, 16)


def n_bins_of(n):
    return (1, 2, n, 7, 50)


def field(n, L, which="truth"):
    return inputs.make_fields(HamilParams(Nx=n, L=L))[which]


def box_of(n):
    return 200. * n / 64.


@pytest.mark.parametrize("n", SIZES)
def test_half_grid_restatement_equals_the_literal_full_grid_loop(n):
    """nmode equal, kmode to 1e-14 relative per populated bin, power to 1e-13 of its maximum."""
    L = box_of(n)
    sig = field(n, L)
    for n_bin in n_bins_of(n):
        k1, n1, p1 = sr.spec2d_loops(sig, n, L, n_bin)
        k2, n2, p2 = sr.spec2d(sig, n, L, n_bin)
        assert n1.dtype == n2.dtype == np.uint64 and np.array_equal(n1, n2), (n, n_bin)
        assert rel_bins(k2, k1, n1) <= 1e-14, (n, n_bin)
        assert rel_max(p2, p1) <= 1e-13, (n, n_bin)
        assert np.all(k2[n2 == 0] == 0) and np.all(p2[n2 == 0] == 0)


@pytest.mark.parametrize("n", SIZES + (128,))
def test_structure_of_the_bins(n):
    """S2: sum nmode = n^3 (no out-of-range mode), the last perp bin and the last par bin are empty for n_bin >= 2, and
    nmode[perp][par] = rows of the perp bin x sum of the Hermitian weights over the par bin's run of k.  The par bin
    does not decrease along k <= n / 2, so every par bin is one run."""
    L = box_of(n)
    for n_bin in n_bins_of(n) + (200,):
        nperp, npar = sr.bin_indices(n, L, n_bin)
        assert np.all(np.diff(npar.astype(np.int64)) >= 0)
        rows, weight = sr.rows_per_perp_bin(n, L, n_bin), sr.weight_per_par_bin(n, L, n_bin)
        assert int(rows.sum()) == n * n and int(weight.sum()) == n
        S = np.zeros((n, n, n // 2 + 1), dtype=np.complex128)
        nmode = sr.spec2d_of_transform(S, n, L, n_bin)[1].reshape(n_bin, n_bin)
        assert int(nmode.sum()) == n ** 3
        assert np.array_equal(nmode, rows[:, None] * weight[None, :])
        if n_bin >= 2:
            assert not nmode[n_bin - 1, :].any() and not nmode[:, n_bin - 1].any()
        else:
            assert int(nmode[0, 0]) == n ** 3
    assert math.isinf(sr.kmax_dk(n, L, 1)[1])


# ---- closed forms, shared with tests/test_gpu_spec2d.py -------------------------------------------------------
KNOWN_N, KNOWN_NBIN, KNOWN_M = 16, 16, 3


def known_constant(n, c):
    return np.full(n ** 3, c)


def known_cosine(n, a, m, axis):
    """a cos(2 pi m x_axis / L) on the grid [i, j, k]; axis 2 is z, the line of sight."""
    shape = [1, 1, 1]
    shape[axis] = n
    wave = a * np.cos(2 * np.pi * m * np.arange(n) / n).reshape(shape)
    return np.broadcast_to(wave, (n, n, n)).reshape(-1).copy()


def _only_bin(res, n_bin, perp, par, want):
    """power is `want` at [perp, par] and (to TOL_FIELD of it) nothing anywhere else; empty bins exactly 0."""
    kmode, nmode, power = (np.asarray(a).reshape(n_bin, n_bin) for a in res)
    assert nmode[perp, par] > 0
    assert abs(power[perp, par] - want) <= TOL_FIELD * want
    rest = power.copy()
    rest[perp, par] = 0.
    assert np.max(np.abs(rest)) <= TOL_FIELD * want
    assert np.all(power[nmode == 0] == 0)
    return nmode


def check_constant(res, n, L, n_bin, c):
    """delta = c: the transform is c N at k = 0 and 0 elsewhere, so element 0 holds NORM (c N)^2 / nmode[0]."""
    nmode = np.asarray(res[1]).ravel()
    _only_bin(res, n_bin, 0, 0, sr.norm_of(n, L) * (c * float(n ** 3)) ** 2 / float(nmode[0]))


def check_cosine(res, n, L, n_bin, a, m, axis):
    """delta = a cos(2 pi m x / L) along one axis: the transform is a N / 2 at the two modes +-m of that axis.  Along z
    they sit at (perp 0, par bin of m 2 pi / L), along x at (perp bin of the same |k|, par 0): the element order
    par + n_bin * perp and the line of sight."""
    _, dk = sr.kmax_dk(n, L, n_bin)
    b = sr.bin_of(sr.calc_ki(m, L, n), dk)
    assert 0 < b < n_bin
    perp, par = (0, b) if axis == 2 else (b, 0)
    nmode = np.asarray(res[1]).reshape(n_bin, n_bin)
    want = sr.norm_of(n, L) * 2. * (a * float(n ** 3) / 2.) ** 2 / float(nmode[perp, par])
    _only_bin(res, n_bin, perp, par, want)
    return perp, par


def check_known_answers(measure, n, L, n_bin, m):
    """`measure(signal)` -> (kmode, nmode, power) of n_bin^2 each."""
    check_constant(measure(known_constant(n, 1.7)), n, L, n_bin, 1.7)
    bz = check_cosine(measure(known_cosine(n, 1.3, m, 2)), n, L, n_bin, 1.3, m, 2)
    bx = check_cosine(measure(known_cosine(n, 1.3, m, 0)), n, L, n_bin, 1.3, m, 0)
    assert len({bz, bx, (0, 0)}) == 3  # the three answers sit in three different bins


def test_known_answers_of_the_restatement():
    n, L = KNOWN_N, box_of(KNOWN_N)
    for fn in (sr.spec2d, sr.spec2d_loops):
        check_known_answers(lambda sig: fn(sig, n, L, KNOWN_NBIN), n, L, KNOWN_NBIN, KNOWN_M)


def test_s1_one_bin_holds_the_mean_power_over_four_pi():
    """S1 and S2 together: with n_bin = 1 the single bin is L^3 / (4 pi) / N^2 x the mean of |delta^|^2 over ALL modes
    of the full grid (measure_spectrum's normalisation is L^3 / N^2, without the 4 pi)."""
    n, L = 8, box_of(8)
    sig = field(n, L)
    S = np.fft.fftn(sig.reshape(n, n, n))
    P = S.real ** 2 + S.imag ** 2
    N = float(n ** 3)
    power = sr.spec2d(sig, n, L, 1)[2]
    assert abs(power[0] - L ** 3 / (4 * math.pi) / N ** 2 * P.sum() / N) <= 1e-13 * power[0]


# ---- declarations ---------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_documents_s1_to_s4():
    text = open(os.path.join(ROOT, "include", "bchmc.h")).read()
    assert header_args("bchmc_measure_spectrum2d") == ["bchmc_handle *", "bchmc_corr_source", "const double *", "uint64_t",
                                                       "double *", "uint64_t *", "double *"]
    assert re.search(r"^#define BCHMC_ABI_VERSION 4\s*$", text, flags=re.M)
    doc = text[:text.index("int bchmc_measure_spectrum2d(")].rsplit("/* ----", 1)[1]
    for tag in ("S1", "S2", "S3", "S4", "4 pi", "n_bin - 1", "2D_powspec.cc", "nmode may be NULL"):
        assert tag in doc, tag


def test_engine_binds_the_entry_point_like_the_header():
    from barcode_amd import engine
    lib = engine.load()
    name = "bchmc_measure_spectrum2d"
    assert list(getattr(lib, name).argtypes) == [CTYPE[t] for t in header_args(name)]
    assert name in engine.EXPORTS_CORR2D + engine.EXPORTS_SPEC2D and name not in engine.EXPORTS
    assert callable(engine.Engine.measure_spectrum2d)
    lib.bchmc_measure_spectrum2d.restype = C.c_int
    x = np.zeros(1)
    dp = x.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.bchmc_measure_spectrum2d(None, 0, dp, 1, dp, None, dp) == 1  # a null handle: BCHMC_ERR_ARG, no device


def test_shim_hamil_and_io_bind_the_new_names():
    from barcode_amd import hamil, shim
    lib = shim.load()
    name = "bchmc_shim_measure_spec2D"
    assert name in shim.SHIM_EXPORTS and getattr(lib, name).argtypes
    text = open(os.path.join(ROOT, "include", "bchmc_shim.hpp")).read()
    assert re.search(r"\bvoid measure_spec2D\(HamilView \*hd", text) and name in text
    assert "-> bchmc_shim::measure_spec2D" in text[:text.index("#ifndef BCHMC_SHIM_HPP")]  # the opening name map
    assert callable(shim.ShimHamil.measure_spec2D)
    with pytest.raises(RuntimeError, match="non-plane-parallel option not yet implemented"):
        hamil.measure_spec2D(None, planepar=False)
    assert callable(io.dump_pow2D) and callable(io.pow2d_filenames)


def test_pow2d_writer(tmp_path, monkeypatch):
    """2D_powspec.cc:130,162-163: <out>_k and <out>_P, <out> = <in>_pow2D by default, n_bin^2 raw doubles each, under
    write_array's extension rule."""
    monkeypatch.chdir(tmp_path)
    os.mkdir("v1.2")
    rng = np.random.default_rng(7)
    nb = 12
    k, P = rng.random((nb, nb)), rng.random((nb, nb))
    assert io.pow2d_filenames("deltaRSS") == ("deltaRSS_pow2D_k", "deltaRSS_pow2D_P")
    assert io.pow2d_filenames("deltaRSS", "spec") == ("spec_k", "spec_P")
    for fin, fout, base, ext in (("deltaRSS", None, "deltaRSS_pow2D", ".dat"), ("deltaRSS", "spec", "spec", ".dat"),
                                 (os.path.join("v1.2", "d"), None, os.path.join("v1.2", "d_pow2D"), "")):
        paths = io.dump_pow2D(fin, k, P, fout)
        assert paths == (base + "_k" + ext, base + "_P" + ext)
        assert os.path.getsize(paths[0]) == os.path.getsize(paths[1]) == 8 * nb * nb
        assert io.read_array(base + "_k", nb * nb).tobytes() == k.tobytes()
        assert io.read_array(base + "_P", nb * nb).tobytes() == P.tobytes()
