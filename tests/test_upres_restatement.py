"""The numpy restatement of tools/interp_upres.cc and tools/2D_corr_fct_interp.cc (tests/upres_restatement.py) against
itself -- literal loops against the vectorised forms, the three properties U1-U3 of the zero-padding mode, the exact
cases of interp_field and of the L_max cut -- and the host layers' bindings and file names.  No GPU.

Bounds.  Two float64 evaluations of one sum of at most 16^3 = 4096 terms differ by at most 4096 * 2^-53 = 4.5e-13 of the
sum of the magnitudes; TOL_SUM = 1e-12 of max |corr| covers that worst case (measured: a few 1e-16).  Two float64
transforms of one array differ by a few ulp times log2 N of the largest element; TOL_FFT = 1e-14 of the maximum."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import corr_restatement as cr
from tests import upres_restatement as ur
from tests.test_corr_restatement import CTYPE, ROOT, header_args

TOL_SUM = 1e-12
TOL_FFT = 1e-14
TOL_RMODE = 1e-14

# (n, n_out): the pairs of DESIGN 9.5's table -- integer and non-integer ratios, odd fine and odd coarse grids, identity
PAIRS = ((4, 8), (6, 8), (5, 8), (8, 16), (8, 12), (6, 9), (4, 10), (8, 8))


def field(n, seed=3, mean=0.2):
    return np.random.default_rng(seed).standard_normal(n ** 3) + mean


def same_bins(a, b, tol):
    rm, nm, co = a
    rm0, nm0, co0 = b
    assert np.array_equal(nm, nm0)
    pop = nm0 > 0
    assert np.all(rm[~pop] == 0) and np.all(co[~pop] == 0)
    assert np.max(np.abs(rm[pop] - rm0[pop]) / np.where(rm0[pop] > 0, rm0[pop], 1.)) <= TOL_RMODE
    lvl = float(np.max(np.abs(co - co0)) / np.max(np.abs(co0)))
    assert lvl <= tol, lvl
    return lvl


@pytest.mark.parametrize("n,n_out", PAIRS + ((8, 4), (6, 4), (12, 8)))
def test_interp_field_loops_equal_the_vectorised_form(n, n_out):
    L = 75.
    sig = field(n)
    assert np.array_equal(ur.interp_field_loops(sig, n, L, n_out), ur.interp_field(sig, n, L, n_out))
    i0, i1, dx = ur.cic_table(n, n_out, L)
    assert np.all((i0 >= 0) & (i0 < n) & (i1 == (i0 + 1) % n)) and np.all((dx >= 0) & (dx < 1 + 1e-12))


def test_interp_field_identity_is_bitwise():
    """n = n_out = 16, L = 100: d = 6.25 is exact, every xpos / d is the integer m, dx = 0 and tx = 1."""
    n, L = 16, 100.
    i0, i1, dx = ur.cic_table(n, n, L)
    assert np.array_equal(i0, np.arange(n)) and not dx.any()
    sig = field(n)
    assert np.array_equal(ur.interp_field(sig, n, L, n), sig)


@pytest.mark.parametrize("n,n_out", PAIRS + ((16, 8), (12, 8)))
def test_constant_field_interpolates_to_itself(n, n_out):
    """The eight weights sum to 1 up to their roundings: each product of three carries <= 2 roundings, the product with
    the field one more and the seven additions one each -- within 4 ulp of the constant."""
    c = 1.7
    out = ur.interp_field(np.full(n ** 3, c), n, 100., n_out)
    assert np.max(np.abs(out - c)) <= 4 * np.spacing(c)


@pytest.mark.parametrize("n,n_out", ((4, 8), (6, 8), (5, 8), (8, 12), (6, 9), (8, 8)))
def test_mode0_loops_equal_the_vectorised_form(n, n_out):
    L = 100.
    sig = field(n)
    for n_bin, l_max in ((n_out, math.inf), (cr.auto_nbin(n_out, L), L / 4), (5, 3 * L / n_out)):
        same_bins(ur.corr2d_interp_cic_loops(sig, n, L, n_out, n_bin, l_max),
                  ur.corr2d_interp_cic(sig, n, L, n_out, n_bin, l_max), TOL_SUM)


@pytest.mark.parametrize("n,n_out", ((4, 8), (6, 8), (5, 8), (8, 12), (6, 9), (4, 10), (8, 8)))
def test_mode1_loops_equal_the_vectorised_form(n, n_out):
    L = 100.
    sig = field(n)
    for odd in (False, True):
        assert np.array_equal(ur.zeropad_power_loops(sig, n, n_out, odd), ur.zeropad_power(sig, n, n_out, odd))
    for n_bin in (n_out, cr.auto_nbin(n_out, L)):
        for u1 in ("literal", "hermitian"):
            same_bins(ur.corr2d_zeropad_loops(sig, n, L, n_out, n_bin, u1), ur.corr2d_zeropad(sig, n, L, n_out, n_bin, u1),
                      TOL_SUM)


@pytest.mark.parametrize("n,n_out", PAIRS)
def test_u1_the_literal_array_transforms_like_its_hermitian_part(n, n_out):
    sig = field(n)
    P = ur.zeropad_power(sig, n, n_out)
    m = ur._neg(n_out)
    plane = P[:, :, 0]
    asym = float(np.max(np.abs(plane - np.conj(plane[np.ix_(m, m)]))) / np.max(np.abs(plane)))
    # the tool's row n / 2 has no partner once the grids differ (at odd n it is an ordinary mode whose partner moved)
    assert asym > 1e-6 if n_out > n else asym <= TOL_FFT
    lit, her = ur.zeropad_corr_field(P, n_out, "literal"), ur.zeropad_corr_field(P, n_out, "hermitian")
    lvl = float(np.max(np.abs(lit - her)) / np.max(np.abs(her)))
    print("U1 %d -> %d: literal irfftn against the explicit Hermitian part: %.2e of max" % (n, n_out, lvl))
    assert lvl <= TOL_FFT


@pytest.mark.parametrize("n,n_out", PAIRS)
def test_u2_the_odd_term_cancels_in_every_bin(n, n_out):
    L = 100.
    sig = field(n)
    A0 = ur.zeropad_corr_field(ur.zeropad_power(sig, n, n_out, False), n_out, "literal")
    A1 = ur.zeropad_corr_field(ur.zeropad_power(sig, n, n_out, True), n_out, "literal")
    moved = float(np.max(np.abs(A1 - A0)) / np.max(np.abs(A0)))
    for n_bin in (n_out, cr.auto_nbin(n_out, L)):
        lvl = same_bins(ur.bins2d(A1, n_out, L, n_bin), ur.bins2d(A0, n_out, L, n_bin), TOL_FFT)
        print("U2 %d -> %d n_bin %d: field moved by %.2e of max, bins by %.2e" % (n, n_out, n_bin, moved, lvl))
    assert moved > 1e-6  # the term is there


@pytest.mark.parametrize("n,n_out", PAIRS)
def test_u3_mode1_is_normalised_twice(n, n_out):
    c, L = 1.7, 100.
    rm, nm, co = ur.corr2d_zeropad(np.full(n ** 3, c), n, L, n_out, n_out)
    want = c * c * (float(n) / n_out) ** 6
    assert nm.sum() > 0 and np.max(np.abs(co[nm > 0] - want)) <= 1e-13 * want
    if (n, n_out) == (8, 16):
        assert abs(want - 0.0451562) < 1e-7


def test_mode1_at_equal_grids_is_corr2d():
    n, L = 8, 100.
    sig = field(n)
    for n_bin in (n, cr.auto_nbin(n, L)):
        same_bins(ur.corr2d_zeropad(sig, n, L, n, n_bin), cr.corr2d(sig, n, L, n_bin), TOL_FFT)


def test_the_cut_is_strict():
    """n_out = 16, L = 100: d_out = 6.25 and l_max = 18.75 = 3 d_out are exact.  The cell at 3 d_out fails `<`: 5 values
    per axis remain, 25 rows (2^2 + 2^2 = 8 < 9) times 5 = 125 cells; the next double admits it: the 29 lattice points
    with a^2 + b^2 <= 9 times 7 = 203."""
    n, n_out, L = 8, 16, 100.
    sig = field(n)
    l_max = 3 * (L / n_out)
    assert l_max == 18.75
    for fn in (ur.corr2d_interp_cic, ur.corr2d_interp_cic_loops):
        assert int(fn(sig, n, L, n_out, n_out, l_max)[1].sum()) == 125
        assert int(fn(sig, n, L, n_out, n_out, math.nextafter(l_max, math.inf))[1].sum()) == 203
    assert int(ur.corr2d_interp_cic(sig, n, L, n_out, n_out, 0.5 * L / n_out)[1].sum()) == 1  # the origin alone
    full = ur.corr2d_interp_cic(sig, n, L, n_out, n_out, math.inf)
    same_bins(full, ur.bins2d(cr.corr_field(ur.interp_field(sig, n, L, n_out), n_out), n_out, L, n_out), 0.)


# ---- the host layers ---------------------------------------------------------------------------------------------------
CTYPE_UP = dict(CTYPE, **{"uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double})


def test_engine_binds_the_upres_entry_points_like_the_header():
    from barcode_amd import engine
    lib = engine.load()
    for name in ("bchmc_interp_upres", "bchmc_measure_corr2d_interp", "bchmc_upres_release", "bchmc_measure_spectrum_src"):
        want = [CTYPE_UP[t] for t in header_args(name)]
        assert list(getattr(lib, name).argtypes) == want, name
        assert name in engine.EXPORTS + engine.EXPORTS_CORR2D
    for meth in ("interp_upres", "measure_corr2d_interp", "upres_release"):
        assert callable(getattr(engine.Engine, meth))
    import inspect
    assert "source" in inspect.signature(engine.Engine.measure_spectrum).parameters
    text = open(os.path.join(ROOT, "include", "bchmc.h")).read()
    assert "#define BCHMC_ABI_VERSION 4" in text  # new functions only


def test_shim_and_hamil_bind_the_upres_hooks():
    from barcode_amd import hamil, shim
    lib = shim.load()
    for name in ("bchmc_shim_interp_field", "bchmc_shim_measure_corr2D_interp"):
        assert name in shim.SHIM_EXPORTS and getattr(lib, name).argtypes
    text = open(os.path.join(ROOT, "include", "bchmc_shim.hpp")).read()
    for name in ("interp_field", "measure_corr2D_interp"):
        assert re.search(r"\bvoid %s\(HamilView \*hd" % name, text) and "bchmc_shim_" + name in text
    assert callable(hamil.interp_field) and callable(shim.ShimHamil.interp_field)
    with pytest.raises(RuntimeError, match="non-plane-parallel option not yet implemented"):
        hamil.measure_corr2D_interp(None, 16, planepar=False)


def test_upres_writers(tmp_path, monkeypatch):
    """The tools' default names (interp_upres.cc:45, 2D_corr_fct_interp.cc:338,397,427-428, powspec.cc:40), relative to
    the working directory, with write_array's extension rule for the raw arrays."""
    from barcode_amd import io
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(5)
    assert io.interp_filename("deltaEUL_3", 32) == "deltaEUL_3_interpCIC32"
    assert io.corr_interp_filenames("d", 32, 28) == ("d_interpCIC32_corr2D_r", "d_interpCIC32_corr2D_eta")
    assert io.corr_interp_filenames("d", 32, 28, True) == ("d_interpCIC32_corr2D_Nbin28_r", "d_interpCIC32_corr2D_Nbin28_eta")
    f = rng.standard_normal(8 ** 3)
    path = io.dump_interp("deltaEUL_3", 8, f)
    assert path == "deltaEUL_3_interpCIC8.dat" and np.array_equal(io.read_array(path, f.size), f)
    r, c = rng.random((28, 28)), rng.standard_normal((28, 28))
    paths = io.dump_corr_interp("deltaEUL_3", 32, r, c, auto_nbin=True)
    assert paths == ("deltaEUL_3_interpCIC32_corr2D_Nbin28_r.dat", "deltaEUL_3_interpCIC32_corr2D_Nbin28_eta.dat")
    assert np.array_equal(io.read_array(paths[0], r.size), r.ravel()) and np.array_equal(io.read_array(paths[1], c.size), c.ravel())
    k, p = np.array([0., 0.1, 0.2]), np.array([1., 2., 0.])
    assert io.dump_pow("deltaEUL_3", k, p) == "deltaEUL_3_pow"
    assert open("deltaEUL_3_pow").read() == "0.1   2\n"
