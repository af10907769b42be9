"""bchmc_measure_multipoles, bchmc_measure_cross_multipoles and bchmc_measure_corr_multipoles on the device against the
vectorised restatement of tests/multipole_reference.py (its transform is numpy.fft.rfftn in float64).  Every bin is
compared, the empty ones included:

* nmode: equal.  A mode in another bin is a failure, not a tolerance.
* kmode / rmode: relative difference <= 1e-14 (TOL_RMODE); leg: difference <= 1e-14 of 1, the bound of |L_l| (a mean of
  L_l can be arbitrarily close to 0, so "relative" is relative to that bound).
* P_l and xi_l: |engine - restatement| <= (2 l + 1) TOL_FIELD max |l = 0 restatement| on fp64 handles, TOL_F32_FIELD on
  fp32 handles; empty bins exactly 0.

With n_bin = 1 the single bin of xi_0 is (sum_r A(r) - A(corner)) / (nmode N) ~ (mean delta)^2: rounding noise for a
zero-mean field, so that "of max |restatement|" bounds nothing (tests/test_gpu_corr.py meets the same).  The n_bin = 1
case of xi_l therefore measures the same field with a mean of 0.3 added.

The measured levels are printed by every test (run with -s)."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

from barcode_amd import engine as engine_mod
from barcode_amd import hamil, inputs, io
from barcode_amd.engine import BchmcError, Engine
from barcode_amd.params import HamilParams
from tests import multipole_reference as mr
from tests.test_gpu_parity import TOL_F32_FIELD
from tests.test_multipoles_cpu import KAISER_BETA, KNOWN_M, KNOWN_N, KNOWN_NBIN, check_known_answers
from tests.util import TOL_FIELD, Case

pytestmark = pytest.mark.gpu

TOL_RMODE = 1e-14
PKEYS, XKEYS = ("p0", "p2", "p4"), ("xi0", "xi2", "xi4")


def tol_of(precision):
    return TOL_F32_FIELD if precision else TOL_FIELD


def box_of(n):
    return 200. * n / 64.


@functools.lru_cache(maxsize=None)
def fields_of(n):
    f = inputs.make_fields(HamilParams(Nx=n, L=box_of(n)))
    out = {k: f[k] for k in ("truth", "q0")}
    out["truth_mean"] = f["truth"] + 0.3
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _restated(kind, n, which, n_bin, other):
    f = fields_of(n)
    if kind == "corr":
        return mr.corr(f[which], n, box_of(n), n_bin)
    return mr.power(f[which], n, box_of(n), n_bin, other=None if other is None else f[other])


def restated(kind, n, which, n_bin, other=None):
    """The restatement of one of the fields, computed once and shared (n_bin = 2048 only runs on the small grids)."""
    return _restated(kind, n, which, n_bin, other)


def stack(res, keys):
    return np.stack([res[k] for k in keys])


def compare(tag, res, want, tol, tkey="k", keys=PKEYS, wkey="m", scale_from="m"):
    """An engine dict against the restatement's, all bins."""
    nm, nm0 = res["nmode"], want["nmode"]
    assert nm.dtype == np.uint64 and np.array_equal(nm, nm0), "%s: %d bins differ in nmode" % (tag, int((nm != nm0).sum()))
    pop = nm0 > 0
    t, t0 = res[tkey], want["t"]
    leg = np.stack([res["leg2"], res["leg4"]])
    got = stack(res, keys)
    assert np.all(t[~pop] == 0) and np.all(leg[:, ~pop] == 0) and np.all(got[:, ~pop] == 0), tag
    lvl_t = float(np.max(np.abs(t[pop] - t0[pop]) / np.where(t0[pop] > 0, t0[pop], 1.)))
    lvl_l = float(np.max(np.abs(leg - want["leg"])))
    scale = float(np.max(np.abs(want[scale_from][0])))
    lvl = [float(np.max(np.abs(got[a] - want[wkey][a]))) / scale / (2 * ell + 1) for a, ell in enumerate(mr.ELLS)]
    print("%s: %d bins (%d populated, %d elements), t rel %.2e, leg %.2e, l = 0, 2, 4: %.2e %.2e %.2e of (2l+1) max" %
          ((tag, nm.size, int(pop.sum()), int(nm.sum()), lvl_t, lvl_l) + tuple(lvl)))
    assert lvl_t <= TOL_RMODE, (tag, lvl_t)
    assert lvl_l <= TOL_RMODE, (tag, lvl_l)
    assert max(lvl) <= tol, (tag, lvl)


def compare_cross(tag, res, want, tol):
    for t, wkey in (("aa", "m"), ("bb", "mbb"), ("ab", "mab")):
        # the bound of the cross term is that of the larger auto term: |re_a re_b + im_a im_b| <= (|a|^2 + |b|^2) / 2
        scale_from = wkey if t != "ab" else ("m" if np.max(np.abs(want["m"][0])) >= np.max(np.abs(want["mbb"][0])) else "mbb")
        compare("%s p%s" % (tag, t), res, want, tol, keys=tuple("p%s%d" % (t, l) for l in mr.ELLS), wkey=wkey,
                scale_from=scale_from)


def same(a, b):
    assert sorted(a) == sorted(b)
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def nbins_of(n):
    return (1, 7, 64) + ((2048,) if n <= 16 else ())


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("n", (4, 5, 9, 16, 128))
def test_grids_all_entry_points(n, precision):
    """n = 4: the smallest grid; 5 and 9: odd, no Nyquist column, every k > 0 weighs 2; 16: unpadded rows; 128: padded
    rows (nhp != nh) and two chunks of columns, the second a one-column tail.  A host field, the resident chain state and
    the pair of them."""
    f = fields_of(n)
    tol = tol_of(precision)
    e = Engine(HamilParams(Nx=n, L=box_of(n)), precision=precision)
    e.chain_set_state(f["q0"])
    for n_bin in nbins_of(n):
        tag = "%d^3 %s n_bin %d" % (n, "fp32" if precision else "fp64", n_bin)
        want = restated("power", n, "q0", n_bin, "truth")  # m: q0, mbb: truth, mab: their cross term
        got = e.measure_multipoles(f["truth"], n_bin=n_bin)
        assert all(got[k].shape == (n_bin,) for k in got)
        compare(tag + " host", got, want, tol, wkey="mbb", scale_from="mbb")
        assert int(got["nmode"].sum()) == n ** 3 - (8 if n % 2 else 1)  # |k| == |k|_max falls past the last bin
        auto = e.measure_multipoles(n_bin=n_bin)
        compare(tag + " chain", auto, want, tol)
        cross = e.measure_cross_multipoles(None, f["truth"], n_bin=n_bin)
        compare_cross(tag + " chain x host", cross, want, tol)
        for l in mr.ELLS:  # the cross call's auto terms are the auto calls', bit for bit
            assert np.array_equal(cross["paa%d" % l], auto["p%d" % l]) and np.array_equal(cross["pbb%d" % l], got["p%d" % l])
        which = "truth_mean" if n_bin == 1 else "truth"
        xi = e.measure_corr_multipoles(f[which], n_bin=n_bin)
        compare(tag + " xi host", xi, restated("corr", n, which, n_bin), tol, "r", XKEYS)
        if n_bin != 1:
            compare(tag + " xi chain", e.measure_corr_multipoles(n_bin=n_bin), restated("corr", n, "q0", n_bin), tol, "r", XKEYS)
    e.close()


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_deltax_and_the_pairs_of_sources(precision):
    """deltaX after chain_forward in redshift and in real space; the cross form on (chain state, deltaX), (host, host) and
    the same source twice, where the three sets are equal bit for bit."""
    n = 16
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    L, tol = c.p.L, tol_of(precision)
    e = c.engine(precision=precision)
    e.chain_set_state(c.q0)
    quad = {}
    for rsd in (1, 0):
        e.chain_forward(rsd)
        dX = e.fetch("deltaX")
        for nb in (16, 7):
            got = e.measure_multipoles(source="deltaX", n_bin=nb)
            compare("deltaX rsd %d n_bin %d" % (rsd, nb), got, mr.power(dX, n, L, nb), tol)
            compare("deltaX rsd %d n_bin %d xi" % (rsd, nb), e.measure_corr_multipoles(source="deltaX", n_bin=nb),
                    mr.corr(dX, n, L, nb), tol, "r", XKEYS)
            cross = e.measure_cross_multipoles(source_a="chain", source_b="deltaX", n_bin=nb)
            compare_cross("chain x deltaX rsd %d n_bin %d" % (rsd, nb), cross, mr.power(c.q0, n, L, nb, other=dX), tol)
            assert all(np.array_equal(cross["pbb%d" % l], got["p%d" % l]) for l in mr.ELLS)
            quad[rsd, nb] = got["p2"] - 5. * got["leg2"] * got["p0"]
        assert np.array_equal(e.fetch("deltaX"), dX)  # the measurements left it alone
    for nb in (16, 7):
        diff = np.max(np.abs(quad[1, nb] - quad[0, nb])) / np.max(np.abs(e.measure_multipoles(source="deltaX", n_bin=nb)["p0"]))
        print("leakage-corrected quadrupole, redshift against real space, n_bin %d: %.2e of max P_0" % (nb, diff))
        assert diff > 1e-3  # far above either tolerance: two different fields were measured
    nb = 7
    hh = e.measure_cross_multipoles(c.truth, c.q0, n_bin=nb)
    compare_cross("host x host", hh, mr.power(c.truth, n, L, nb, other=c.q0), tol)
    for kw in (dict(signal_a=c.truth, signal_b=c.truth), dict(), dict(source_a="deltaX", source_b="deltaX")):
        tw = e.measure_cross_multipoles(n_bin=nb, **kw)
        for l in mr.ELLS:
            assert np.array_equal(tw["paa%d" % l], tw["pbb%d" % l]) and np.array_equal(tw["paa%d" % l], tw["pab%d" % l])
    e.close()


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_consistent_with_the_existing_measurements(precision):
    """p0 against bchmc_measure_cross_spectrum's power_a (measure_spectrum_src's numbers with the mode counts beside
    them) and xi0 against bchmc_measure_corr: the same nmode, the values within the tolerance of the maximum."""
    n = 16
    f = fields_of(n)
    tol = tol_of(precision)
    e = Engine(HamilParams(Nx=n, L=box_of(n)), precision=precision)
    e.chain_set_state(f["q0"])
    for nb in (7, 64):
        for sig in (None, f["truth"]):
            got = e.measure_multipoles(sig, n_bin=nb)
            km, nm, pa = e.measure_cross_spectrum(sig, sig, nb)[:3]
            km1, p1 = e.measure_spectrum(sig, nb, "chain" if sig is None else "host")
            assert np.array_equal(got["nmode"], nm)
            pop = nm > 0
            # their kmode is a float-atomic sum of up to N positive terms in any order: N 2^-52 bounds its relative error
            assert np.max(np.abs(got["k"][pop] - km[pop])) <= n ** 3 * 2. ** -52 * np.max(km)
            for p in (pa, p1):
                assert np.max(np.abs(got["p0"] - p)) <= tol * np.max(np.abs(p))
            xi = e.measure_corr_multipoles(sig, n_bin=nb)
            rm, nmr, co = e.measure_corr(sig, nb)
            assert np.array_equal(xi["nmode"], nmr)
            assert np.max(np.abs(xi["r"] - rm)) <= TOL_RMODE * np.max(rm)
            assert np.max(np.abs(xi["xi0"] - co)) <= tol * np.max(np.abs(co))
    e.close()


def test_known_answers_and_kaiser_through_the_c_abi():
    """The closed forms of tests/test_multipoles_cpu.py with the arrays handed to the library directly (nmode NULL too),
    then the Kaiser field through the engine."""
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    for n in KNOWN_N:
        L, nb = box_of(n), KNOWN_NBIN
        e = Engine(HamilParams(Nx=n, L=L))

        def measure(sig):
            sig = np.ascontiguousarray(sig, dtype=np.float64)
            outs = []
            for with_nm in (True, False):
                km, leg, p = np.full(nb, -1.), np.full(2 * nb, -1.), np.full(3 * nb, -1.)
                nm = np.full(nb, 7, dtype=np.uint64)
                assert e.lib.bchmc_measure_multipoles(e.h, 0, sig.ctypes.data_as(dp), nb, km.ctypes.data_as(dp),
                                                      nm.ctypes.data_as(up) if with_nm else None, leg.ctypes.data_as(dp),
                                                      p.ctypes.data_as(dp)) == 0
                outs.append((km, leg, p))
                if with_nm:
                    assert np.array_equal(nm, mr.power(sig, n, L, nb)["nmode"])
                else:
                    assert np.all(nm == 7)  # not written through another pointer
            assert all(np.array_equal(a, b) for a, b in zip(*outs))  # nmode may be NULL
            return outs[0][2].reshape(3, nb)

        check_known_answers(measure, n, L, nb, KNOWN_M)
        e.close()
    n = 16
    L = box_of(n)
    field, _ = mr.kaiser_field(n, L, KAISER_BETA, 77 + n)
    e = Engine(HamilParams(Nx=n, L=L))
    for nb in (7, 32):
        nmode, want = mr.kaiser_expected(n, L, nb, KAISER_BETA)
        got = e.measure_multipoles(field, n_bin=nb)
        assert np.array_equal(got["nmode"], nmode)
        for a, ell in enumerate(mr.ELLS):
            lvl = np.max(np.abs(got["p%d" % ell] - want[a])) / np.max(np.abs(want[0])) / (2 * ell + 1)
            print("Kaiser field n_bin %d l = %d: %.2e of (2l+1) max P_0" % (nb, ell, lvl))
            assert lvl <= TOL_FIELD
    e.close()


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("n", (16, 128))
def test_bitwise_repeatable(n, precision):
    """No atomics and a fixed order: two calls, a call after another n_bin, a call after multipoles_release and a second
    handle all give the same bits in every array of all three entry points."""
    f = fields_of(n)
    p = HamilParams(Nx=n, L=box_of(n))

    def measure(e, nb):
        return (e.measure_multipoles(n_bin=nb), e.measure_multipoles(f["truth"], n_bin=nb),
                e.measure_cross_multipoles(None, f["truth"], n_bin=nb), e.measure_corr_multipoles(n_bin=nb))

    runs = []
    for _ in range(2):
        e = Engine(p, precision=precision)
        e.chain_set_state(f["q0"])
        runs.append([measure(e, nb) for nb in (64, 7, 64)])
        e.multipoles_release()
        runs.append([measure(e, nb) for nb in (64, 7, 64)])
        e.close()
    for other in runs:
        assert all(same(a, b) for a, b in zip(other[0], other[2]))  # n_bin = 64 before and after n_bin = 7
        for x, y in zip(runs[0], other):
            assert all(same(a, b) for a, b in zip(x, y))
    compare("%d^3 repeat" % n, runs[-1][2][0], restated("power", n, "q0", 64), tol_of(precision))


def test_a_measurement_leaves_the_state_alone():
    """With a pending proposal: the chain state, the momenta, the proposal and deltaX are bit for bit what they were,
    chain_accept succeeds, and the next attempt (from the carried gradient) returns the dH of a twin that did not
    measure."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)

    def run(measure):
        e = Engine(c.p, deterministic=1)
        e.upload(**c.arrays())
        e.chain_set_state(c.q0)
        e.chain_set_momenta(c.p0)
        e.chain_attempt(c.eps, 3)
        before = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + (e.fetch("deltaX"),)
        if measure:
            want = mr.power(c.q0, 16, c.p.L, 16)
            for sig, src in ((None, "chain"), (c.truth, "host"), (None, "deltaX")):
                assert np.array_equal(e.measure_multipoles(sig, src, 16)["nmode"], want["nmode"])
                e.measure_corr_multipoles(sig, src, 16)
                e.measure_cross_multipoles(sig, None, src, "deltaX", 16)
            compare("chain, proposal pending", e.measure_multipoles(n_bin=16), want, TOL_FIELD)
        after = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + (e.fetch("deltaX"),)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        e.chain_accept(1)
        assert np.array_equal(e.chain_get_state(), before[2])
        e.chain_set_momenta(0.9 * c.p0)
        dH, terms, done = e.chain_attempt(c.eps, 3)
        e.close()
        return dH, terms, done

    plain, meas = run(False), run(True)
    assert plain[0] == meas[0] and np.array_equal(plain[1], meas[1]) and plain[2] == meas[2] == 3


def test_refusals():
    """Every BCHMC_ERR_ARG and BCHMC_ERR_STATE case of the header, for all three entry points and for either source of
    the cross form: nothing is written, and the next call is right."""
    n, nb = 16, 16
    f = fields_of(n)
    sig = np.array(f["truth"])
    want = restated("power", n, "truth", nb)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    bufs = [np.zeros(12) for _ in range(6)]
    nm = np.zeros(4, dtype=np.uint64)
    t, leg, p, p2, p3 = (b.ctypes.data_as(dp) for b in bufs[:5])
    nmp = nm.ctypes.data_as(up)
    s = sig.ctypes.data_as(dp)
    e = Engine(HamilParams(Nx=n, L=box_of(n)))
    ARG, STATE = 1, 9
    bad_sources = ((ARG, 1, s), (ARG, 2, s),      # a signal with a source that is not the host
                   (ARG, 0, None),                # the host source without a signal
                   (ARG, 3, None),                # an unknown source
                   (STATE, 1, None),              # no chain state
                   (STATE, 2, None))              # deltaX before any forward model
    calls = []
    for fn in (e.lib.bchmc_measure_multipoles, e.lib.bchmc_measure_corr_multipoles):
        for code, src, sg in bad_sources:
            calls.append((code, fn, (e.h, src, sg, 2, t, nmp, leg, p)))
        for bad_nb in (0, 2049):
            calls.append((ARG, fn, (e.h, 0, s, bad_nb, t, nmp, leg, p)))
        calls.append((ARG, fn, (None, 0, s, 2, t, nmp, leg, p)))
        calls.append((ARG, fn, (e.h, 0, s, 2, None, nmp, leg, p)))
        calls.append((ARG, fn, (e.h, 0, s, 2, t, nmp, None, p)))
        calls.append((ARG, fn, (e.h, 0, s, 2, t, nmp, leg, None)))
    fx = e.lib.bchmc_measure_cross_multipoles
    for code, src, sg in bad_sources:
        calls.append((code, fx, (e.h, src, sg, 0, s, 2, t, nmp, leg, p, p2, p3)))
        calls.append((code, fx, (e.h, 0, s, src, sg, 2, t, nmp, leg, p, p2, p3)))
    for bad_nb in (0, 2049):
        calls.append((ARG, fx, (e.h, 0, s, 0, s, bad_nb, t, nmp, leg, p, p2, p3)))
    calls.append((ARG, fx, (None, 0, s, 0, s, 2, t, nmp, leg, p, p2, p3)))
    for hole in (6, 8, 9, 10, 11):
        args = [e.h, 0, s, 0, s, 2, t, nmp, leg, p, p2, p3]
        args[hole] = None
        calls.append((ARG, fx, tuple(args)))
    for code, fn, args in calls:
        assert fn(*args) == code, (fn.__name__, args[1:4])
        assert not any(b.any() for b in bufs) and not nm.any()
    compare("after %d refusals" % len(calls), e.measure_multipoles(sig, n_bin=nb), want, TOL_FIELD)
    assert engine_mod.live_resources()  # and the handle is alive
    for call, code in ((lambda: e.measure_multipoles(sig, n_bin=2049), ARG),
                       (lambda: e.measure_corr_multipoles(None, "deltaX", 4), STATE),
                       (lambda: e.measure_cross_multipoles(sig, None, n_bin=4), STATE)):
        with pytest.raises(BchmcError) as err:
            call()
        assert err.value.code == code
    e.close()


def test_non_finite_and_zero_fields():
    n, nb = 16, 16
    f = fields_of(n)
    want = restated("power", n, "truth", nb)
    wantx = restated("corr", n, "truth", nb)
    e = Engine(HamilParams(Nx=n, L=box_of(n)))
    for bad in (np.nan, np.inf):
        sig = np.array(f["truth"]).reshape(-1)
        sig[1234] = bad
        for res, w, keys, tk in ((e.measure_multipoles(sig, n_bin=nb), want, PKEYS, "k"),
                                 (e.measure_corr_multipoles(sig, n_bin=nb), wantx, XKEYS, "r")):
            pop = w["nmode"] > 0
            assert np.array_equal(res["nmode"], w["nmode"])
            for k in keys:
                assert np.all(np.isnan(res[k][pop])) and np.all(res[k][~pop] == 0)
            assert np.max(np.abs(res[tk] - w["t"])) <= TOL_RMODE * np.max(w["t"])
            assert np.max(np.abs(np.stack([res["leg2"], res["leg4"]]) - w["leg"])) <= TOL_RMODE
        cr = e.measure_cross_multipoles(sig, f["truth"], n_bin=nb)
        pop = want["nmode"] > 0
        assert np.all(np.isnan(cr["paa0"][pop])) and np.all(np.isnan(cr["pab4"][pop]))
        compare("finite side of a cross call", cr, want, TOL_FIELD, keys=("pbb0", "pbb2", "pbb4"))
    for res, keys in ((e.measure_multipoles(np.zeros(n ** 3), n_bin=nb), PKEYS),
                      (e.measure_corr_multipoles(np.zeros(n ** 3), n_bin=nb), XKEYS)):
        assert all(np.all(res[k] == 0) for k in keys)
    compare("after NaN, inf and zero", e.measure_multipoles(f["truth"], n_bin=nb), want, TOL_FIELD)
    e.close()


def test_layers_agree():
    """hamil.measure_multipoles / measure_corr_multipoles, the shim's functions and io.dump_multipoles / read_multipoles
    return the engine's arrays bit for bit (the sums are repeatable across handles); planepar = false raises upstream's
    text."""
    import tempfile
    from barcode_amd.shim import ShimError, ShimHamil
    n, nb = 16, 16
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    e = c.engine()
    e.chain_set_state(c.q0)
    hd = ShimHamil(c.p, **c.arrays())
    hd.chain_set_state(c.q0)
    for sig in (c.truth, None):
        res, xi = e.measure_multipoles(sig, n_bin=nb), e.measure_corr_multipoles(sig, n_bin=nb)
        for got, r, tk, keys in ((hd.measure_multipoles(sig, nb), res, "k", PKEYS),
                                 (hd.measure_corr_multipoles(sig, nb), xi, "r", XKEYS)):
            assert np.array_equal(got[0], r[tk]) and np.array_equal(got[1], r["nmode"])
            assert np.array_equal(got[2], np.stack([r["leg2"], r["leg4"]])) and np.array_equal(got[3], stack(r, keys))
    for name in ("measure_multipoles", "measure_corr_multipoles"):
        with pytest.raises(ShimError, match="non-plane-parallel option not yet implemented"):
            getattr(hd, name)(c.truth, nb, planepar=False)
    hd.close()

    class View:  # what hamil.py's functions read of a HamilData
        engine = e
    e.chain_forward(1)
    assert same(hamil.measure_multipoles(View, c.truth, nb), e.measure_multipoles(c.truth, n_bin=nb))
    assert same(hamil.measure_multipoles(View, None, nb, "deltaX"), e.measure_multipoles(source="deltaX", n_bin=nb))
    assert same(hamil.measure_corr_multipoles(View, None, nb), e.measure_corr_multipoles(n_bin=nb))
    assert hamil.measure_multipoles(View)["p0"].shape == (200,)
    for fn in (hamil.measure_multipoles, hamil.measure_corr_multipoles):
        with pytest.raises(RuntimeError, match="non-plane-parallel option not yet implemented"):
            fn(View, c.truth, nb, planepar=False)
    with tempfile.TemporaryDirectory() as d:
        for tag, res in (("pk", e.measure_multipoles(n_bin=nb)), ("xi", e.measure_corr_multipoles(n_bin=nb))):
            back = io.read_multipoles(io.dump_multipoles(res, d, tag))
            assert same(back, res) and back["nmode"].dtype == np.uint64
    e.close()


def test_buffers_are_counted_released_and_returned():
    """bchmc_live_resources counts the feature's buffers (the two class tables, the class sums, the bin partials; one
    half-complex array more once the cross form's first source needed a transform), sees them reused by other bin
    counts and forms, is back at the handle's own count after multipoles_release and at its start after close()."""
    gc.collect()
    start = engine_mod.live_resources()
    n = 16
    f = fields_of(n)
    e = Engine(HamilParams(Nx=n, L=box_of(n)))
    e.chain_set_state(f["q0"])
    created = engine_mod.live_resources()
    first_res = e.measure_multipoles(n_bin=16)
    first = engine_mod.live_resources()
    print("live resources: start %s, created %s, measured %s" % (start, created, first))
    assert first[0] == created[0] + 4 and first[1] > created[1]
    e.measure_multipoles(n_bin=50)
    e.measure_corr_multipoles(n_bin=16)
    e.measure_cross_multipoles(n_bin=16)  # the chain state twice: no transform, no array for one
    assert engine_mod.live_resources()[0] == first[0]
    e.measure_cross_multipoles(f["truth"], None, n_bin=16)
    assert engine_mod.live_resources()[0] == first[0] + 1
    e.multipoles_release()
    assert engine_mod.live_resources() == created
    e.multipoles_release()  # nothing held: a no-op
    assert same(e.measure_multipoles(n_bin=16), first_res)
    assert engine_mod.live_resources()[0] == created[0] + 4
    e.close()
    assert engine_mod.live_resources() == start
