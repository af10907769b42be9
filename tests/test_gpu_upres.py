"""bchmc_interp_upres / bchmc_measure_corr2d_interp / bchmc_upres_release / bchmc_measure_spectrum_src on the device
against the numpy restatement of tools/interp_upres.cc and tools/2D_corr_fct_interp.cc (tests/upres_restatement.py).
Every bin is compared, the empty ones included:

* nmode: equal.
* rmode: max relative difference <= 1e-14 over populated bins, empty bins exactly 0.
* corr: max |engine - restatement| <= TOL_FIELD max |restatement| on fp64 handles, TOL_F32_FIELD on fp32 handles: the
  project's bounds for the same transform-and-sum pipeline (tests/test_gpu_corr.py).
* interp_upres: <= 1e-14 max |input| on fp64 handles -- with identical weights only the order and fusion of about ten
  roundings can differ, 1.1e-15, so the bound has a margin of 9 -- and TOL_F32_FIELD max |input| on fp32 handles; bit for
  bit where the grids are equal.

The fields carry a mean of 0.3: with n_bin = 1 the one bin of the uncut function is (mean delta)^2, which is rounding
noise for a zero-mean field (tests/test_gpu_corr.py's first test).  The measured levels are printed (run with -s)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from barcode_amd import hamil, inputs
from barcode_amd.engine import BchmcError, Engine, live_resources
from barcode_amd.params import HamilParams
from tests import corr_restatement as cr
from tests import upres_restatement as ur
from tests.test_gpu_corr import chain_run, compare, tol_of
from tests.util import TOL_FIELD, Case, rel_l2

pytestmark = pytest.mark.gpu

TOL_INTERP = 1e-14

# n -> n_out: integer and non-integer ratios, an odd fine and an odd coarse grid, identity, and two down-samplings
# (legal for interp_field and mode 0; mode 1 is refused there)
SHAPES = ((8, 16), (8, 12), (6, 9), (5, 8), (16, 16), (16, 8), (12, 8))
L_SMALL = 100.  # d and d_out exact at 16 -> 16 and 8 -> 16


@functools.lru_cache(maxsize=None)
def field(n, seed=7):
    p = HamilParams(Nx=n, L=L_SMALL)
    f = inputs.make_fields(p)["truth"].reshape(-1) + 0.3
    f.setflags(write=False)
    return f


def l_max_values(L, n_out):
    d_out = L / n_out
    return (math.inf, L / 4, 3 * d_out, 0.5 * d_out)


def n_bin_values(L, n_out):
    return (n_out, cr.auto_nbin(n_out, L), 1, 200, 2048)


@functools.lru_cache(maxsize=None)
def corr_field_of(n, n_out, mode):
    """The restatement's correlation field on the fine grid, once per shape and mode (shared by every binning of it)."""
    sig = field(n)
    if mode == 0:
        A = cr.corr_field(ur.interp_field(sig, n, L_SMALL, n_out), n_out)
    else:
        A = ur.zeropad_corr_field(ur.zeropad_power(sig, n, n_out), n_out, "hermitian")
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def want_bins(n, n_out, mode, n_bin, l_max):
    return ur.bins2d(corr_field_of(n, n_out, mode), n_out, L_SMALL, n_bin, l_max if mode == 0 else None)


def check_interp(tag, got, want, scale, precision, bitwise=False):
    lvl = float(np.max(np.abs(got - want)) / scale)
    print("%s: interp_upres differs by %.2e of max |input|" % (tag, lvl))
    if bitwise and not precision:
        assert np.array_equal(got, want), tag
    assert lvl <= (tol_of(precision) if precision else TOL_INTERP), (tag, lvl)


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("n,n_out", SHAPES)
def test_interp_upres_of_a_host_field(n, n_out, precision):
    sig = field(n)
    e = Engine(HamilParams(Nx=n, L=L_SMALL), precision=precision)
    got = e.interp_upres(n_out, sig)
    assert got.shape == (n_out ** 3,)
    check_interp("%d -> %d" % (n, n_out), got, ur.interp_field(sig, n, L_SMALL, n_out), np.max(np.abs(sig)), precision,
                 bitwise=(n == n_out))
    if n == n_out and not precision:
        assert np.array_equal(got, sig)  # identity: d exact, dx = 0
    e.close()


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("n,n_out", SHAPES)
def test_both_modes_every_n_bin_and_cut(n, n_out, precision):
    sig = field(n)
    e = Engine(HamilParams(Nx=n, L=L_SMALL), precision=precision)
    tol = tol_of(precision)
    for n_bin in n_bin_values(L_SMALL, n_out):
        for l_max in l_max_values(L_SMALL, n_out):
            tag = "%d -> %d %s mode 0 n_bin %d l_max %g" % (n, n_out, "fp32" if precision else "fp64", n_bin, l_max)
            got = e.measure_corr2d_interp(n_out, sig, n_bin, 0, l_max)
            assert got[0].shape == (n_bin, n_bin)
            compare(tag, got, want_bins(n, n_out, 0, n_bin, l_max), tol)
        tag = "%d -> %d %s mode 1 n_bin %d" % (n, n_out, "fp32" if precision else "fp64", n_bin)
        if n_out >= n:
            compare(tag, e.measure_corr2d_interp(n_out, sig, n_bin, 1), want_bins(n, n_out, 1, n_bin, math.inf), tol)
        else:
            with pytest.raises(BchmcError) as err:
                e.measure_corr2d_interp(n_out, sig, n_bin, 1)
            assert err.value.code == 1
    # the automatic bin count is the tool's, ceil(rmax / d_out)
    assert e.measure_corr2d_interp(n_out, sig)[0].shape == (cr.auto_nbin(n_out, L_SMALL),) * 2
    if n == n_out:  # zero padding onto the same grid is measure_corr2d
        nb = cr.auto_nbin(n, L_SMALL)
        compare("mode 1 at equal grids against measure_corr2d", e.measure_corr2d_interp(n, sig, nb, 1),
                e.measure_corr2d(sig, nb), tol)
        compare("mode 1 at equal grids against corr2d", e.measure_corr2d_interp(n, sig, nb, 1),
                cr.corr2d(sig, n, L_SMALL, nb), tol)
    # the strict cut: 125 cells at l_max = 3 d_out exactly, 203 at the next double (16^3 fine grids with d_out = 6.25)
    if n_out == 16:
        l3 = 3 * (L_SMALL / n_out)
        assert int(e.measure_corr2d_interp(n_out, sig, n_out, 0, l3)[1].sum()) == 125
        assert int(e.measure_corr2d_interp(n_out, sig, n_out, 0, math.nextafter(l3, math.inf))[1].sum()) == 203
    e.close()


@pytest.mark.parametrize("pad", ("0", "1"))
def test_padded_and_unpadded_rows(pad, monkeypatch):
    """16 -> 32 with the row padding of both half-complex layouts forced off and on (k_zeropad_embed reads one and writes
    the other)."""
    monkeypatch.setenv("BCHMC_FFT_PAD", pad)
    n, n_out = 16, 32
    sig = field(n)
    e = Engine(HamilParams(Nx=n, L=L_SMALL))
    e.chain_set_state(sig)
    check_interp("pad %s" % pad, e.interp_upres(n_out, sig), ur.interp_field(sig, n, L_SMALL, n_out), np.max(np.abs(sig)), 0)
    for n_bin in (n_out, cr.auto_nbin(n_out, L_SMALL)):
        for signal, source in ((sig, None), (None, "chain")):
            tag = "pad %s %s n_bin %d" % (pad, source or "host", n_bin)
            compare(tag + " mode 0", e.measure_corr2d_interp(n_out, signal, n_bin, 0, L_SMALL / 4, source),
                    want_bins(n, n_out, 0, n_bin, L_SMALL / 4), TOL_FIELD)
            compare(tag + " mode 1", e.measure_corr2d_interp(n_out, signal, n_bin, 1, source=source),
                    want_bins(n, n_out, 1, n_bin, math.inf), TOL_FIELD)
    e.close()


@pytest.mark.parametrize("n,n_out", ((64, 128), (128, 256)))
def test_natural_layouts_once(n, n_out):
    """The padded half-complex rows these sizes get by default, on the coarse and on the fine side, whole workgroups of
    128 and 256 threads in the slice kernel and perp bins cut into many slices; mode 0 with the cut at L / 4, mode 1
    whole."""
    L = 200. * n / 64.
    rng = np.random.default_rng(11)
    x = np.arange(n) * (2 * np.pi / n)
    sig = (rng.standard_normal((n, n, n)) + 2. * np.cos(3 * x)[:, None, None] * np.cos(2 * x)[None, :, None] +
           1.5 * np.cos(5 * x)[None, None, :]).reshape(-1) + 0.3
    nb = cr.auto_nbin(n_out, L)
    e = Engine(HamilParams(Nx=n, L=L))
    fine = ur.interp_field(sig, n, L, n_out)
    check_interp("%d -> %d" % (n, n_out), e.interp_upres(n_out, sig), fine, np.max(np.abs(sig)), 0)
    compare("%d -> %d mode 0" % (n, n_out), e.measure_corr2d_interp(n_out, sig, nb, 0, L / 4),
            ur.bins2d(cr.corr_field(fine, n_out), n_out, L, nb, L / 4), TOL_FIELD)
    del fine
    compare("%d -> %d mode 1" % (n, n_out), e.measure_corr2d_interp(n_out, sig, nb, 1),
            ur.corr2d_zeropad(sig, n, L, n_out, nb, "literal"), TOL_FIELD)
    e.close()


def check_source(tag, e, sig, n, L, n_out, source, precision):
    """interp_upres and both modes of the field `sig` the engine holds as `source`."""
    tol = tol_of(precision)
    check_interp(tag, e.interp_upres(n_out, None, source), ur.interp_field(sig, n, L, n_out), np.max(np.abs(sig)), precision)
    out = []
    for nb in (n_out, cr.auto_nbin(n_out, L)):
        got0 = e.measure_corr2d_interp(n_out, None, nb, 0, L / 4, source)
        compare("%s mode 0 n_bin %d" % (tag, nb), got0, ur.corr2d_interp_cic(sig, n, L, n_out, nb, L / 4), tol)
        got1 = e.measure_corr2d_interp(n_out, None, nb, 1, source=source)
        compare("%s mode 1 n_bin %d" % (tag, nb), got1, ur.corr2d_zeropad(sig, n, L, n_out, nb), tol)
        out.append(got1[2])
    return out


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_all_sources_on_an_rsd_chain(precision):
    n, n_out = 16, 24
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    L = c.p.L
    e = c.engine(precision=precision)
    e.chain_set_state(c.q0)
    check_source("set_state", e, e.chain_get_state(), n, L, n_out, "chain", precision)
    e.chain_set_momenta(c.p0)
    e.chain_attempt(c.eps, 3)
    e.chain_accept(True)
    q = e.chain_get_state()
    assert rel_l2(q, c.q0) > 1e-6
    check_source("accepted", e, q, n, L, n_out, "chain", precision)
    two = {}
    for rsd in (1, 0):
        e.chain_forward(rsd)
        dX = e.fetch("deltaX")
        two[rsd] = check_source("deltaX rsd %d" % rsd, e, dX, n, L, n_out, "deltaX", precision)
        assert np.array_equal(e.fetch("deltaX"), dX)
    diff = np.max(np.abs(two[1][0] - two[0][0])) / np.max(np.abs(two[0][0]))
    assert diff > 1e-3  # redshift space against real space: two different fields were measured
    got = e.measure_corr2d_interp(n_out, c.truth, n_out, 1)
    compare("host on the chain's handle", got, ur.corr2d_zeropad(c.truth, n, L, n_out, n_out), tol_of(precision))
    e.close()


def upres_all(e, c, n_out):
    """Every call of this file's entry points on all three sources."""
    out = []
    for sig, src in ((None, "chain"), (None, "deltaX"), (c.truth, "host")):
        out.append((e.interp_upres(n_out, sig, src),))
        out.append(e.measure_corr2d_interp(n_out, sig, n_out, 0, c.p.L / 4, src))
        out.append(e.measure_corr2d_interp(n_out, sig, 9, 1, source=src))
        e.measure_spectrum(sig, 20, src)  # called for what it must leave alone; its float atomics are not repeatable
    return out


def test_measurements_change_nothing_else():
    """The state, the momenta, deltaX, and dH, the six terms and the proposal of a following attempt (which starts from
    the carried gradient and -log L) are bit for bit those of a run that only called chain_forward between its attempts."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)

    def forward_only(e):
        e.chain_forward(-1)
        return e.fetch("deltaX")

    def measure(e):
        e.chain_forward(-1)
        out = upres_all(e, c, 24) + upres_all(e, c, 16)
        e.upres_release()
        return e.fetch("deltaX"), out

    plain = chain_run(c, forward_only)
    meas = chain_run(c, measure)
    for k in ("state", "mom", "terms", "prop"):
        assert np.array_equal(plain[k], meas[k]), k
    assert plain["dH"] == meas["dH"] and np.array_equal(plain["extra"], meas["extra"][0])
    again = chain_run(c, measure)  # a fresh handle gives the same measurements, bit for bit
    for a, b in zip(meas["extra"][1], again["extra"][1]):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_pending_proposal_survives():
    c = Case(Nx=16, likelihood=1, rsd_model=1)
    e = c.engine()
    e.chain_set_state(c.q0)
    e.chain_set_momenta(c.p0)
    e.chain_attempt(c.eps, 3)
    q1, p1 = e.chain_get_proposal()
    upres_all(e, c, 24)
    q1b, p1b = e.chain_get_proposal()
    assert np.array_equal(q1b, q1) and np.array_equal(p1b, p1)
    e.chain_accept(True)
    assert np.array_equal(e.chain_get_state(), q1)
    e.close()


def test_repeatable():
    """Two calls on one handle (the second with the cached tables) and two fresh handles: array_equal."""
    n, n_out = 16, 24
    sig = field(n)
    runs = []
    for _ in range(2):
        e = Engine(HamilParams(Nx=n, L=L_SMALL))
        e.chain_set_state(sig)
        for _ in range(2):
            r = []
            for nb in (n_out, 5, 2048):
                for signal, src in ((sig, None), (None, "chain")):
                    r.append(e.measure_corr2d_interp(n_out, signal, nb, 0, L_SMALL / 4, src))
                    r.append(e.measure_corr2d_interp(n_out, signal, nb, 1, source=src))
            r.append((e.interp_upres(n_out, sig),))
            runs.append(r)
        e.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_error_paths_then_a_good_call():
    n, n_out = 16, 24
    sig = np.array(field(n))
    e = Engine(HamilParams(Nx=n, L=L_SMALL))
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    rm, co, nm = np.zeros(4), np.zeros(4), np.zeros(4, dtype=np.uint64)
    args = (rm.ctypes.data_as(dp), nm.ctypes.data_as(up), co.ctypes.data_as(dp))
    s = sig.ctypes.data_as(dp)
    out = np.zeros(1)
    o = out.ctypes.data_as(dp)
    m2d, itp, spc = e.lib.bchmc_measure_corr2d_interp, e.lib.bchmc_interp_upres, e.lib.bchmc_measure_spectrum_src
    inf = math.inf
    assert m2d(e.h, 0, s, n_out, 0, inf, 0, *args) == 1 and m2d(e.h, 0, s, n_out, 0, inf, 2049, *args) == 1  # n_bin
    assert m2d(e.h, 0, s, 3, 0, inf, 2, *args) == 1 and m2d(e.h, 0, s, 1025, 0, inf, 2, *args) == 1          # n_out
    assert m2d(e.h, 0, s, n_out, 2, inf, 2, *args) == 1 and m2d(e.h, 0, s, n_out, -1, inf, 2, *args) == 1    # mode
    assert m2d(e.h, 0, s, 8, 1, inf, 2, *args) == 1                                    # mode 1 with n_out < n
    for bad in (0., -1., math.nan, -inf):
        assert m2d(e.h, 0, s, n_out, 0, bad, 2, *args) == 1                            # mode 0 with l_max not > 0
    assert m2d(e.h, 0, None, n_out, 0, inf, 2, *args) == 1                             # host source without a signal
    assert m2d(e.h, 1, s, n_out, 0, inf, 2, *args) == 1 and m2d(e.h, 2, s, n_out, 1, inf, 2, *args) == 1
    assert m2d(e.h, 3, None, n_out, 0, inf, 2, *args) == 1                             # unknown source
    assert m2d(e.h, 1, None, n_out, 0, inf, 2, *args) == 9 and m2d(e.h, 2, None, n_out, 1, inf, 2, *args) == 9
    assert m2d(e.h, 0, s, n_out, 0, inf, 2, None, args[1], args[2]) == 1 and m2d(None, 0, s, n_out, 0, inf, 2, *args) == 1
    assert itp(e.h, 0, s, 3, o) == 1 and itp(e.h, 0, s, 1025, o) == 1 and itp(e.h, 0, None, n_out, o) == 1
    assert itp(e.h, 1, s, n_out, o) == 1 and itp(e.h, 0, s, n_out, None) == 1
    assert itp(e.h, 1, None, n_out, o) == 9 and itp(e.h, 2, None, n_out, o) == 9
    km, pw = np.zeros(4), np.zeros(4)
    kp = (km.ctypes.data_as(dp), pw.ctypes.data_as(dp))
    assert spc(e.h, 0, s, 0, *kp) == 1 and spc(e.h, 0, s, 2049, *kp) == 1 and spc(e.h, 0, None, 4, *kp) == 1
    assert spc(e.h, 2, s, 4, *kp) == 1 and spc(e.h, 1, None, 4, *kp) == 9 and spc(e.h, 2, None, 4, *kp) == 9
    assert e.lib.bchmc_upres_release(None) == 1
    assert not rm.any() and not co.any() and not nm.any() and not out.any() and not km.any() and not pw.any()
    base = live_resources()
    with pytest.raises(BchmcError) as err:
        e.measure_corr2d_interp(n_out, sig, 4, 0, 0.)
    assert err.value.code == 1
    with pytest.raises(BchmcError) as err:
        e.interp_upres(2048, sig)
    assert err.value.code == 1
    assert live_resources() == base  # nothing was built for a refused call
    e.upres_release()                # with nothing held: fine
    compare("after the errors", e.measure_corr2d_interp(n_out, sig, n_out, 1), want_bins(n, n_out, 1, n_out, math.inf), TOL_FIELD)
    e.close()


def test_live_resources_return_to_their_start():
    n = 16
    sig = field(n)
    start = live_resources()
    e = Engine(HamilParams(Nx=n, L=L_SMALL))
    e.measure_corr2d(sig, n)  # the coarse tables and the staging are not the fine grid's
    base = live_resources()
    e.interp_upres(24, sig)
    held = live_resources()
    assert held[0] > base[0] and held[1] > base[1] and held[3] == base[3] + 3  # two plans and an execution info
    e.measure_corr2d_interp(24, sig, 24, 0, 30.)
    more = live_resources()
    assert more[0] > held[0] and more[3] == held[3]  # the bin tables joined; the same n_out kept the grid
    e.measure_corr2d_interp(12, sig, 24, 0, 30.)     # another n_out replaces it
    assert live_resources()[1] < more[1] and live_resources()[3] == held[3]
    e.upres_release()
    assert live_resources() == base
    e.measure_corr2d_interp(24, sig, 24, 1)          # and a later call rebuilds
    assert live_resources()[3] == held[3]
    e.close()
    assert live_resources() == start


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_spectrum_of_every_source(precision):
    """measure_spectrum(source="deltaX") against the oracle's measure_spectrum of fetch("deltaX"); the other two sources
    against the entry point they restate."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)
    e = c.engine(precision=precision)
    e.chain_set_state(c.q0)
    e.chain_forward(1)
    dX = e.fetch("deltaX")
    tol = 1e-12 if precision == 0 else 2e-5
    for nb in (20, 200):
        kmo, pwo = c.oracle.measure_spectrum(dX, nb)
        km, pw = e.measure_spectrum(None, nb, "deltaX")
        lvl = float(np.max(np.abs(pw - pwo)) / pwo.max())
        print("spectrum of deltaX, %d bins: %.2e of max" % (nb, lvl))
        assert np.allclose(km, kmo, rtol=1e-13, atol=0) and np.allclose(pw, pwo, rtol=tol, atol=tol * pwo.max())
        # the same transform into the same sums; the sums are float atomics, so equal to rounding, not bit for bit
        for a, b in ((e.measure_spectrum(None, nb, "chain"), e.measure_spectrum(None, nb)),
                     (e.measure_spectrum(c.truth, nb, "host"), e.measure_spectrum(c.truth, nb))):
            assert np.allclose(a[0], b[0], rtol=1e-13, atol=0) and np.allclose(a[1], b[1], rtol=tol, atol=tol * b[1].max())
    assert np.array_equal(e.fetch("deltaX"), dX)
    e.close()


def test_shim_and_hamil_layers():
    """bchmc_shim::interp_field / measure_corr2D_interp and the hamil.py names equal the engine calls; planepar = false
    raises upstream's text."""
    from barcode_amd.shim import ShimError, ShimHamil
    n, n_out = 16, 24
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    e = c.engine()
    e.chain_set_state(c.q0)
    hd = ShimHamil(c.p, **c.arrays())
    hd.chain_set_state(c.q0)
    nb = cr.auto_nbin(n_out, c.p.L)
    for sig, src in ((c.truth, None), (None, "chain")):
        assert np.array_equal(hd.interp_field(sig, n_out), e.interp_upres(n_out, sig, src))
        for mode, l_max in ((0, c.p.L / 4), (1, math.inf)):
            got = hd.measure_corr2D_interp(sig, n_out, nb, mode, l_max)
            want = e.measure_corr2d_interp(n_out, sig, nb, mode, l_max, src)
            assert all(np.array_equal(x, y) for x, y in zip(got, want))
    hd.chain_forward(1)
    e.chain_forward(1)
    got, want = hd.measure_corr2D_interp(None, n_out, nb, 1, of_deltaX=True), e.measure_corr2d_interp(n_out, None, nb, 1, source="deltaX")
    assert np.array_equal(got[1], want[1]) and np.max(np.abs(got[2] - want[2])) <= TOL_FIELD * np.max(np.abs(want[2]))
    assert rel_l2(hd.interp_field(None, n_out, of_deltaX=True), e.interp_upres(n_out, None, "deltaX")) < TOL_FIELD
    with pytest.raises(ShimError, match="non-plane-parallel option not yet implemented"):
        hd.measure_corr2D_interp(c.truth, n_out, nb, planepar=False)
    hd.close()

    class View:  # what hamil.py's functions read of a HamilData
        engine = e
    assert np.array_equal(hamil.interp_field(View, n_out, c.truth), e.interp_upres(n_out, c.truth))
    for got, want in ((hamil.measure_corr2D_interp(View, n_out, c.truth, 0, 0, 30.), e.measure_corr2d_interp(n_out, c.truth, nb, 0, 30.)),
                      (hamil.measure_corr2D_interp(View, n_out, None, nb, 1), e.measure_corr2d_interp(n_out, None, nb, 1))):
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    e.close()
