"""The two statements of the RSD multipoles in tests/multipole_reference.py against each other, without a GPU.

The criterion everywhere (``agree``): nmode equal as integers; the mean |k| or r and leg to TOL_RMODE = 1e-14 (relative
for the means of |k| and r; for leg relative to 1, the bound of |L_l|, because a mean of L_l can be arbitrarily close to
0); |M_l - M_l^def| <= (2 l + 1) TOL_FIELD max |M_0^def|, since |L_l| <= 1 lets l carry at most (2 l + 1) times the
monopole's error.  Four wrong restatements each miss it."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import multipole_reference as mr
from tests.util import TOL_FIELD

TOL_RMODE = 1e-14
GRIDS = (4, 5, 8, 9, 12, 16)
NBINS = (1, 7, 32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def box_of(n):
    return 200. * n / 64.


@functools.lru_cache(maxsize=None)
def white(n):
    f = np.random.RandomState(1000 + n).standard_normal(n ** 3)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def definition(kind, n, n_bin):
    fn = mr.power_def if kind == "power" else mr.corr_def
    return fn(white(n), n, box_of(n), n_bin)


def misses(got, want, tol=TOL_FIELD, key="m", ref=None):
    """The list of what ``got`` misses of the criterion against ``want`` (empty: it agrees).  ``ref``: the array whose
    l = 0 row scales the bound (default: want[key])."""
    bad = []
    if not np.array_equal(got["nmode"], want["nmode"]):
        bad.append("nmode")
    pop = want["nmode"] > 0
    if np.any(np.abs(got["t"] - want["t"]) > TOL_RMODE * np.abs(want["t"])):
        bad.append("t")
    if np.any(np.abs(got["leg"] - want["leg"]) > TOL_RMODE):
        bad.append("leg")
    scale = np.max(np.abs((want[key] if ref is None else ref)[0]))
    for a, ell in enumerate(mr.ELLS):
        if np.any(np.abs(got[key][a] - want[key][a]) > (2 * ell + 1) * tol * scale):
            bad.append("l=%d" % ell)
        if np.any(got[key][a][~pop] != 0):
            bad.append("empty l=%d" % ell)
    return bad


@pytest.mark.parametrize("n_bin", NBINS)
@pytest.mark.parametrize("n", GRIDS)
def test_restatement_agrees_with_definition(n, n_bin):
    L = box_of(n)
    for kind, fn in (("power", mr.power), ("corr", mr.corr)):
        want = definition(kind, n, n_bin)
        got = fn(white(n), n, L, n_bin)
        assert misses(got, want) == [], (kind, n, n_bin)
        assert got["nmode"].dtype == np.uint64
    # every mode is counted but those with |k| == |k|_max, which fall past the last bin as in measure_spectrum: the one
    # corner of an even n, the eight corners (+-n/2, +-n/2, +-n/2) of an odd one
    assert int(definition("power", n, n_bin)["nmode"].sum()) == n ** 3 - (8 if n % 2 else 1)


@pytest.mark.parametrize("mutant", mr.MUTANTS)
def test_wrong_restatements_miss_the_criterion(mutant):
    """line of sight x; 35 mu^2 for 30 mu^2 in L_4; no Hermitian weight; no (2 l + 1)"""
    missed = []
    for n in GRIDS:
        for n_bin in NBINS:
            bad = misses(mr.power(white(n), n, box_of(n), n_bin, mutant=mutant), definition("power", n, n_bin))
            if mutant != "no_hw":
                bad += misses(mr.corr(white(n), n, box_of(n), n_bin, mutant=mutant), definition("corr", n, n_bin))
            if bad:
                missed.append((n, n_bin, bad))
    print(mutant, "missed on", len(missed), "of", len(GRIDS) * len(NBINS), "cases")
    assert missed, mutant


KNOWN = (((0, 0, 1), 5., 9.), ((1, 0, 0), -2.5, 3.375), ((1, 0, 1), 1.25, -117. / 32.))
KNOWN_N, KNOWN_M, KNOWN_NBIN = (8, 9), 2, 7


def check_known_answers(measure, n, L, n_bin, m):
    """``measure(field)`` -> (3, n_bin) multipoles.  A wave along z: P_2 = 5 P_0, P_4 = 9 P_0 in its bin; along x:
    -2.5 and 3.375; along (m, 0, m), mu^2 = 1/2: 1.25 and -117/32; 0 in every other bin; each to 1e-12 relative."""
    for direction, r2, r4 in KNOWN:
        mvec = tuple(m * c for c in direction)
        p = measure(mr.plane_wave(n, L, mvec))
        kabs = mr.kfac_of(L) * m * np.sqrt(float(sum(direction)))
        b = int(kabs / mr.spectrum_dk(n, L, n_bin))
        p0 = p[0, b]
        assert p0 > 0, (n, direction)
        assert abs(p[1, b] - r2 * p0) <= 1e-12 * abs(r2 * p0), (n, direction, p[1, b] / p0)
        assert abs(p[2, b] - r4 * p0) <= 1e-12 * abs(r4 * p0), (n, direction, p[2, b] / p0)
        other = np.delete(p, b, axis=1)
        assert np.max(np.abs(other)) <= 1e-12 * p0, (n, direction)


@pytest.mark.parametrize("n", KNOWN_N)
def test_known_answers(n):
    L = box_of(n)
    for fn in (mr.power_def, mr.power):
        check_known_answers(lambda f: fn(f, n, L, KNOWN_NBIN)["m"], n, L, KNOWN_NBIN, KNOWN_M)


KAISER_BETA = 0.5


@pytest.mark.parametrize("n", (8, 9, 16))
def test_kaiser_field(n):
    """x^ = (1 + beta mu^2) e^{i phi}: P_l = (2 l + 1) NORM mean[(1 + beta mu^2)^2 L_l] per bin from the geometry alone"""
    L = box_of(n)
    field, _ = mr.kaiser_field(n, L, KAISER_BETA, 77 + n)
    for n_bin in (7, 32):
        nmode, want = mr.kaiser_expected(n, L, n_bin, KAISER_BETA)
        for fn in (mr.power_def, mr.power):
            got = fn(field, n, L, n_bin)
            assert np.array_equal(got["nmode"], nmode)
            for a, ell in enumerate(mr.ELLS):
                assert np.max(np.abs(got["m"][a] - want[a])) <= (2 * ell + 1) * TOL_FIELD * np.max(np.abs(want[0])), (n, ell)
        assert np.max(np.abs(want[1])) > 0.1 * np.max(want[0])  # the quadrupole is there


def test_cross_of_a_field_with_itself_and_with_its_negative():
    n, nb = 8, 7
    L = box_of(n)
    f = white(n)
    same = mr.power(f, n, L, nb, other=f)
    assert np.array_equal(same["m"], same["mbb"]) and np.array_equal(same["m"], same["mab"])
    neg = mr.power(f, n, L, nb, other=-f)
    assert np.array_equal(neg["mab"], -neg["m"])
    assert misses(mr.power(f, n, L, nb), definition("power", n, nb)) == []


def test_abi_and_bindings_name_the_entry_points():
    """The header declares the four entry points, the library exports them, and engine.py, shim.py, hamil.py and io.py
    carry their layers (no device is touched)."""
    from barcode_amd import engine, hamil, io, shim
    names = ("bchmc_measure_multipoles", "bchmc_measure_cross_multipoles", "bchmc_measure_corr_multipoles",
             "bchmc_multipoles_release")
    text = open(os.path.join(ROOT, "include", "bchmc.h")).read()
    raw = C.CDLL(engine.LIB_PATH)
    for name in names:
        assert re.search(r"int %s\(" % name, text), name
        assert name in engine.EXPORTS and hasattr(raw, name)
    lib = engine.load()
    assert len(lib.bchmc_measure_multipoles.argtypes) == 8 and len(lib.bchmc_measure_cross_multipoles.argtypes) == 12
    assert lib.bchmc_measure_multipoles(None, 0, None, 4, None, None, None, None) == 1  # BCHMC_ERR_ARG, no device touched
    assert lib.bchmc_multipoles_release(None) == 1
    for name in ("measure_multipoles", "measure_cross_multipoles", "measure_corr_multipoles", "multipoles_release"):
        assert callable(getattr(engine.Engine, name))
    slib = shim.load()
    for name in ("bchmc_shim_measure_multipoles", "bchmc_shim_measure_corr_multipoles"):
        assert name in shim.SHIM_EXPORTS and getattr(slib, name).argtypes
    assert callable(hamil.measure_multipoles) and callable(hamil.measure_corr_multipoles)
    assert callable(io.dump_multipoles) and callable(io.read_multipoles)


def test_table_round_trip(tmp_path):
    """io.dump_multipoles / read_multipoles return every column bit for bit, for both forms"""
    from barcode_amd import io
    n, nb = 8, 7
    for kind, keys in (("power", ("k", "p0", "p2", "p4")), ("corr", ("r", "xi0", "xi2", "xi4"))):
        d = definition(kind, n, nb)
        res = {keys[0]: d["t"], "nmode": d["nmode"], "leg2": d["leg"][0], "leg4": d["leg"][1]}
        res.update({k: d["m"][a] for a, k in enumerate(keys[1:])})
        path = io.dump_multipoles(res, str(tmp_path), kind)
        back = io.read_multipoles(path)
        assert sorted(back) == sorted(res)
        for k in res:
            assert back[k].dtype == res[k].dtype and np.array_equal(back[k], res[k]), (kind, k)
