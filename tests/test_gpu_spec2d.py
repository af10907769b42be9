"""bchmc_measure_spectrum2d on the device against the vectorised numpy restatement of the reference's measure_spec2D
(tests/spec2d_restatement.py; its own transform is numpy.fft.rfftn in float64).  Every bin is compared, the empty ones
included:

* nmode: equal.  A mode that changed its bin is a failure, not a tolerance.
* kmode: max relative difference <= 1e-14 over populated bins (the TOL_RMODE of the correlation tests), empty bins
  exactly 0.
* power: max |engine - restatement| <= TOL_FIELD max |restatement| on fp64 handles, TOL_F32_FIELD on fp32 handles (the
  project's single-evaluation bounds); empty bins exactly 0.

The measured levels are printed by every test (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

from barcode_amd import engine as engine_mod
from barcode_amd import hamil, inputs
from barcode_amd.engine import BchmcError, Engine
from barcode_amd.params import HamilParams
from tests import spec2d_restatement as sr
from tests.test_gpu_parity import TOL_F32_FIELD
from tests.test_spec2d_restatement import KNOWN_M, KNOWN_N, KNOWN_NBIN, check_known_answers
from tests.util import TOL_FIELD, Case

pytestmark = pytest.mark.gpu

TOL_RMODE = 1e-14


def tol_of(precision):
    return TOL_F32_FIELD if precision else TOL_FIELD


def box_of(n):
    return 200. * n / 64.


@functools.lru_cache(maxsize=None)
def fields_of(n):
    f = inputs.make_fields(HamilParams(Nx=n, L=box_of(n)))
    for a in f.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _restated(n, which, n_bin):
    res = sr.spec2d(fields_of(n)[which], n, box_of(n), n_bin)
    for a in res:
        a.setflags(write=False)
    return res


def restated(n, which, n_bin):
    """The restatement of one of make_fields' fields, computed once and shared read-only (n_bin = 2048 is only used on
    the small grids, where it costs milliseconds, and its 3 x 32 MB are not kept)."""
    return _restated(n, which, n_bin) if n_bin <= 256 else sr.spec2d(fields_of(n)[which], n, box_of(n), n_bin)


def compare(tag, got, want, tol):
    """(kmode, nmode, power) of the engine against the restatement's, all bins."""
    km, nm, pw = (np.asarray(a).ravel() for a in got)
    km0, nm0, pw0 = (np.asarray(a).ravel() for a in want)
    assert nm.dtype == np.uint64 and np.array_equal(nm, nm0), "%s: %d bins differ in nmode" % (tag, int((nm != nm0).sum()))
    pop = nm0 > 0
    assert np.all(km[~pop] == 0) and np.all(pw[~pop] == 0), tag
    lvl_k = float(np.max(np.abs(km[pop] - km0[pop]) / np.where(km0[pop] > 0, km0[pop], 1.)))
    lvl_p = float(np.max(np.abs(pw - pw0)) / np.max(np.abs(pw0)))
    print("%s: %d bins (%d populated, %d modes), kmode rel %.2e, power %.2e of max" %
          (tag, nm.size, int(pop.sum()), int(nm.sum()), lvl_k, lvl_p))
    assert lvl_k <= TOL_RMODE, (tag, lvl_k)
    assert lvl_p <= tol, (tag, lvl_p)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("n", (4, 5, 9, 16, 128))
def test_host_field_and_chain_state(n, precision):
    """n = 4: the smallest grid; 5 and 9: odd, no Nyquist column, every k > 0 weighs 2; 16: unpadded rows; 128: padded
    rows (nhp != nh) and two chunks of columns, the second a one-column tail."""
    L = box_of(n)
    f = fields_of(n)
    e = Engine(HamilParams(Nx=n, L=L), precision=precision)
    e.chain_set_state(f["q0"])
    for n_bin in ((n, 200) if n == 128 else (1, 2, n, 200, 2048)):
        tag = "%d^3 %s n_bin %d" % (n, "fp32" if precision else "fp64", n_bin)
        got = e.measure_spectrum2d(f["truth"], n_bin)
        assert got[0].shape == got[1].shape == got[2].shape == (n_bin, n_bin)
        compare(tag + " host", got, restated(n, "truth", n_bin), tol_of(precision))
        compare(tag + " chain", e.measure_spectrum2d(None, n_bin), restated(n, "q0", n_bin), tol_of(precision))
        assert int(got[1].sum()) == n ** 3
    e.close()


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_deltax_in_redshift_and_real_space(precision):
    n = 16
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    e = c.engine(precision=precision)
    e.chain_set_state(c.q0)
    power = {}
    for rsd in (1, 0):
        e.chain_forward(rsd)
        dX = e.fetch("deltaX")
        for nb in (n, 7):
            got = e.measure_spectrum2d(None, nb, "deltaX")
            compare("deltaX rsd %d n_bin %d" % (rsd, nb), got, sr.spec2d(dX, n, c.p.L, nb), tol_of(precision))
            power[rsd, nb] = got[2]
        assert np.array_equal(e.fetch("deltaX"), dX)  # the measurement left it alone
    for nb in (n, 7):
        diff = np.max(np.abs(power[1, nb] - power[0, nb])) / np.max(np.abs(power[0, nb]))
        print("2-D power, redshift space against real space, n_bin %d: %.2e of max" % (nb, diff))
        assert diff > 1e-3  # far above either tolerance: two different fields were measured
    e.close()


def test_known_answers_through_the_c_abi():
    """The three closed forms of tests/test_spec2d_restatement.py, with the arrays handed to the library directly."""
    n, nb = KNOWN_N, KNOWN_NBIN
    L = box_of(n)
    e = Engine(HamilParams(Nx=n, L=L))
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)

    def measure(sig):
        sig = np.ascontiguousarray(sig, dtype=np.float64)
        km, pw, nm = np.full(nb * nb, -1.), np.full(nb * nb, -1.), np.full(nb * nb, 7, dtype=np.uint64)
        rc = e.lib.bchmc_measure_spectrum2d(e.h, 0, sig.ctypes.data_as(dp), nb, km.ctypes.data_as(dp),
                                            nm.ctypes.data_as(up), pw.ctypes.data_as(dp))
        assert rc == 0
        km2, pw2 = np.full(nb * nb, -1.), np.full(nb * nb, -1.)
        assert e.lib.bchmc_measure_spectrum2d(e.h, 0, sig.ctypes.data_as(dp), nb, km2.ctypes.data_as(dp), None,
                                              pw2.ctypes.data_as(dp)) == 0  # nmode may be NULL
        assert np.array_equal(km, km2) and np.array_equal(pw, pw2)
        return km, nm, pw

    check_known_answers(measure, n, L, nb, KNOWN_M)
    e.close()


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("n", (16, 128))
def test_bitwise_repeatable(n, precision):
    """No atomics and a fixed order: two calls, a call after the tables were rebuilt for another n_bin, and a second
    handle all give the same bits in all three arrays."""
    f = fields_of(n)
    p = HamilParams(Nx=n, L=box_of(n))
    runs = []
    for _ in range(2):
        e = Engine(p, precision=precision)
        e.chain_set_state(f["q0"])
        for _ in range(2):
            runs.append([e.measure_spectrum2d(None, nb) + e.measure_spectrum2d(f["truth"], nb) for nb in (n, 7, n)])
        e.close()
    for other in runs:
        assert same(other[0], other[2])  # n_bin = n before and after n_bin = 7
        for a, b in zip(runs[0], other):
            assert same(a, b)
    compare("%d^3 repeat" % n, runs[-1][2][:3], restated(n, "q0", n), tol_of(precision))


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
            want = sr.spec2d(c.q0, 16, c.p.L, 16)
            for sig, src in ((None, "chain"), (c.truth, "host"), (None, "deltaX")):
                got = e.measure_spectrum2d(sig, 16, src)
                assert np.array_equal(got[1], want[1].reshape(16, 16))
            compare("chain, proposal pending", e.measure_spectrum2d(None, 16, "chain"), want, TOL_FIELD)
        after = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + (e.fetch("deltaX"),)
        assert same(before, after)
        e.chain_accept(1)
        assert np.array_equal(e.chain_get_state(), before[2])
        e.chain_set_momenta(0.9 * c.p0)
        dH, terms, done = e.chain_attempt(c.eps, 3)
        e.close()
        return dH, terms, done

    plain, meas = run(False), run(True)
    assert plain[0] == meas[0] and np.array_equal(plain[1], meas[1]) and plain[2] == meas[2] == 3


def test_refusals():
    n, nb = 16, 16
    L = box_of(n)
    f = fields_of(n)
    sig = np.array(f["truth"])
    want = restated(n, "truth", nb)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    km, pw, nm = np.zeros(4), np.zeros(4), np.zeros(4, dtype=np.uint64)
    out = (km.ctypes.data_as(dp), nm.ctypes.data_as(up), pw.ctypes.data_as(dp))
    s = sig.ctypes.data_as(dp)
    e = Engine(HamilParams(Nx=n, L=L))
    fn = e.lib.bchmc_measure_spectrum2d
    ARG, STATE = 1, 9
    refused = ((ARG, (e.h, 1, s, 2)), (ARG, (e.h, 2, s, 2)),          # a signal with a source that is not the host
               (ARG, (e.h, 0, None, 2)),                               # the host source without a signal
               (ARG, (e.h, 0, s, 0)), (ARG, (e.h, 0, s, 2049)),        # n_bin outside 1..2048
               (ARG, (e.h, 3, None, 2)),                               # an unknown source
               (STATE, (e.h, 1, None, 2)),                             # no chain state
               (STATE, (e.h, 2, None, 2)),                             # deltaX before any forward model
               (ARG, (None, 0, s, 2)))                                 # a null handle
    for code, args in refused:
        assert fn(*args, *out) == code, args[1:]
        assert not km.any() and not pw.any() and not nm.any()
        tag = "after refusal %d (source %d, %s signal, n_bin %d)" % (code, args[1], "a" if args[2] else "no", args[3])
        compare(tag, e.measure_spectrum2d(sig, nb), want, TOL_FIELD)
    assert fn(e.h, 0, s, 2, None, out[1], out[2]) == ARG and fn(e.h, 0, s, 2, out[0], out[1], None) == ARG
    with pytest.raises(BchmcError) as err:
        e.measure_spectrum2d(sig, 2049)
    assert err.value.code == ARG
    with pytest.raises(BchmcError) as err:
        e.measure_spectrum2d(None, 4, "deltaX")
    assert err.value.code == STATE
    e.close()


def test_non_finite_and_zero_fields():
    n, nb = 16, 16
    f = fields_of(n)
    want = restated(n, "truth", nb)
    e = Engine(HamilParams(Nx=n, L=box_of(n)))
    sig = np.array(f["truth"]).reshape(-1)
    sig[1234] = np.nan
    km, nm, pw = (a.ravel() for a in e.measure_spectrum2d(sig, nb))
    pop = want[1] > 0
    assert np.array_equal(nm, want[1]) and np.all(np.isnan(pw[pop])) and np.all(pw[~pop] == 0)
    assert np.max(np.abs(km - want[0]) / np.where(want[0] > 0, want[0], 1.)) <= TOL_RMODE
    km, nm, pw = (a.ravel() for a in e.measure_spectrum2d(np.zeros(n ** 3), nb))
    assert np.array_equal(nm, want[1]) and np.all(pw == 0)
    assert np.max(np.abs(km - want[0]) / np.where(want[0] > 0, want[0], 1.)) <= TOL_RMODE
    compare("after NaN and zero", e.measure_spectrum2d(f["truth"], nb), want, TOL_FIELD)
    e.close()


def test_shim_and_hamil_layers():
    """bchmc_shim::measure_spec2D and hamil.measure_spec2D return the engine's arrays (bit for bit: the sums are
    repeatable across handles); planepar = false raises upstream's text on both."""
    from barcode_amd.shim import ShimError, ShimHamil
    n, nb = 16, 16
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    e = c.engine()
    e.chain_set_state(c.q0)
    hd = ShimHamil(c.p, **c.arrays())
    hd.chain_set_state(c.q0)
    for sig, src in ((c.truth, None), (None, "chain")):
        km, nm, pw = e.measure_spectrum2d(sig, nb, src)
        got = hd.measure_spec2D(sig, nb)
        assert np.array_equal(got[0], km) and np.array_equal(got[1], pw)
    hd.chain_forward(1)
    e.chain_forward(1)
    km, nm, pw = e.measure_spectrum2d(None, nb, "deltaX")
    got = hd.measure_spec2D(None, nb, of_deltaX=True)
    assert np.array_equal(got[0], km) and np.max(np.abs(got[1] - pw)) <= TOL_FIELD * np.max(np.abs(pw))
    with pytest.raises(ShimError, match="non-plane-parallel option not yet implemented"):
        hd.measure_spec2D(c.truth, nb, planepar=False)
    hd.close()

    class View:  # what hamil.py's functions read of a HamilData
        engine = e
    assert same(hamil.measure_spec2D(View, c.truth, nb), e.measure_spectrum2d(c.truth, nb))
    assert same(hamil.measure_spec2D(View, None, nb, "deltaX"), e.measure_spectrum2d(None, nb, "deltaX"))
    assert hamil.measure_spec2D(View)[0].shape == (200, 200)
    with pytest.raises(RuntimeError, match="non-plane-parallel option not yet implemented"):
        hamil.measure_spec2D(View, c.truth, nb, planepar=False)
    e.close()


def test_tables_of_two_bin_counts_are_returned():
    """bchmc_live_resources counts the bin tables (four device buffers), sees them replaced by another n_bin's, not
    added to, and is back at its start after close()."""
    import gc
    gc.collect()
    start = engine_mod.live_resources()
    n = 16
    e = Engine(HamilParams(Nx=n, L=box_of(n)))
    e.chain_set_state(fields_of(n)["q0"])
    created = engine_mod.live_resources()
    e.measure_spectrum2d(None, 16)
    first = engine_mod.live_resources()
    print("live resources: start %s, created %s, measured %s" % (start, created, first))
    assert first[0] == created[0] + 4 and first[1] > created[1]  # idx, slices, part, out; nothing else from the chain
    e.measure_spectrum2d(None, 50)
    assert engine_mod.live_resources()[0] == first[0]
    e.close()
    assert engine_mod.live_resources() == start
