"""bchmc_measure_cross_spectrum on the device against the numpy restatement (tests/ensemble_restatement.py; its own
transforms are numpy.fft.rfftn in float64, its bin sums longdouble).  Every bin is compared, the empty ones included:

* nmode: equal.  A mode that changed its bin is a failure, not a tolerance.
* kmode: max relative difference <= 1e-14 over populated bins (the project's TOL_RMODE), empty bins exactly 0.
* power_a, power_b: max |engine - restatement| <= tol max |restatement|; cross: <= tol max sqrt(power_a power_b), the
  scale a cross term has (it may vanish itself); tol = TOL_FIELD on fp64 handles, TOL_F32_FIELD on fp32 handles.  Empty
  bins exactly 0.

The sums are float atomics, so nothing but nmode is compared bit for bit with another run.  The measured levels are
printed by every test (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

from barcode_amd import hamil, inputs
from barcode_amd.engine import BchmcError, Engine
from barcode_amd.params import HamilParams
from tests import ensemble_restatement as er
from tests.test_ensemble_restatement import KNOWN_M, KNOWN_N, KNOWN_NBIN, check_known_answers
from tests.test_gpu_parity import TOL_F32_FIELD
from tests.util import TOL_FIELD, Case

pytestmark = pytest.mark.gpu

TOL_RMODE = 1e-14
ARG, STATE = 1, 9
PREC = pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))


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
def restated(n, n_bin):
    """truth against q0, computed once and shared read-only by both precisions"""
    f = fields_of(n)
    res = er.cross_spectrum(f["truth"], f["q0"], n, box_of(n), n_bin)
    for a in res:
        a.setflags(write=False)
    return res


def compare(tag, got, want, tol):
    """(kmode, nmode, power_a, power_b, cross, coeff) of the engine against the restatement's, all bins."""
    km, nm, pa, pb, cr, co = (np.asarray(a).ravel() for a in got)
    km0, nm0, pa0, pb0, cr0, _ = (np.asarray(a).ravel() for a in want)
    assert nm.dtype == np.uint64 and np.array_equal(nm, nm0), "%s: %d bins differ in nmode" % (tag, int((nm != nm0).sum()))
    pop = nm0 > 0
    for a in (km, pa, pb, cr, co):
        assert np.all(a[~pop] == 0), tag
    lvl_k = float(np.max(np.abs(km[pop] - km0[pop]) / np.where(km0[pop] > 0, km0[pop], 1.)))
    lvl_a = float(np.max(np.abs(pa - pa0)) / np.max(np.abs(pa0)))
    lvl_b = float(np.max(np.abs(pb - pb0)) / np.max(np.abs(pb0)))
    lvl_c = float(np.max(np.abs(cr - cr0)) / np.max(np.sqrt(pa0 * pb0)))
    print("%s: %d bins (%d populated, %d modes), kmode rel %.2e, power_a %.2e, power_b %.2e of max, cross %.2e of max "
          "sqrt(power_a power_b)" % (tag, nm.size, int(pop.sum()), int(nm.sum()), lvl_k, lvl_a, lvl_b, lvl_c))
    assert lvl_k <= TOL_RMODE, (tag, lvl_k)
    assert lvl_a <= tol and lvl_b <= tol and lvl_c <= tol, (tag, lvl_a, lvl_b, lvl_c)
    assert np.array_equal(co, er.coeff_of(pa, pb, cr)), tag  # formed on the host from the three returned arrays


@PREC
@pytest.mark.parametrize("n", (4, 5, 9, 16, 128))
def test_host_field_against_chain_state(n, precision):
    """n = 4: the smallest grid; 5 and 9: odd, no Nyquist column; 16: unpadded rows; 128: padded rows (nhp != nh).
    Also power_a against measure_spectrum(source=...) of the same source, in the same bound."""
    f = fields_of(n)
    e = Engine(HamilParams(Nx=n, L=box_of(n)), precision=precision)
    e.chain_set_state(f["q0"])
    tol = tol_of(precision)
    for n_bin in ((n, 200) if n == 128 else (1, 2, n, 200)):
        tag = "%d^3 %s n_bin %d" % (n, "fp32" if precision else "fp64", n_bin)
        got = e.measure_cross_spectrum(f["truth"], None, n_bin)
        assert all(a.shape == (n_bin,) for a in got)
        compare(tag, got, restated(n, n_bin), tol)
        for side, (sig, src) in ((2, (f["truth"], "host")), (3, (None, "chain"))):
            km, pw = e.measure_spectrum(sig, n_bin, src)
            assert np.max(np.abs(got[side] - pw)) <= tol * np.max(np.abs(pw)), tag
    e.close()


@PREC
def test_the_largest_bin_count(precision):
    """n_bin = 2048: the workgroup's histogram is 80 KiB of LDS."""
    n = 16
    f = fields_of(n)
    e = Engine(HamilParams(Nx=n, L=box_of(n)), precision=precision)
    e.chain_set_state(f["q0"])
    compare("16^3 n_bin 2048", e.measure_cross_spectrum(f["truth"], None, 2048), restated(n, 2048), tol_of(precision))
    compare("16^3 n_bin 16 afterwards", e.measure_cross_spectrum(f["truth"], None, 16), restated(n, 16), tol_of(precision))
    e.close()


@PREC
def test_all_nine_source_pairs(precision):
    """An RSD case at 16^3: host, chain state and redshift-space deltaX on either side, each pair against the
    restatement of the two fields as the engine hands them out; identical sources correlate to 1."""
    n, nb = 16, 16
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    e = c.engine(precision=precision)
    e.chain_set_state(c.q0)
    e.chain_forward(1)
    field = dict(host=c.truth, chain=e.chain_get_state(), deltaX=e.fetch("deltaX"))
    tol = tol_of(precision)
    for sa in ("host", "chain", "deltaX"):
        for sb in ("host", "chain", "deltaX"):
            got = e.measure_cross_spectrum(c.truth if sa == "host" else None, c.truth if sb == "host" else None, nb, sa, sb)
            compare("%s x %s" % (sa, sb), got, er.cross_spectrum(field[sa], field[sb], n, c.p.L, nb), tol)
            if sa == sb:
                # the three fields have zero mean: bin 0 of 16 holds the k = 0 mode alone, its power may be exactly 0,
                # and coeff is then 0 by its own rule (compare() has checked that rule bin by bin)
                pop = (got[1] > 0) & (got[2] * got[3] != 0)
                assert pop[1:].all()
                assert np.max(np.abs(got[5][pop] - 1.)) <= TOL_FIELD, (sa, np.max(np.abs(got[5][pop] - 1.)))
    assert np.array_equal(e.fetch("deltaX"), field["deltaX"]) and np.array_equal(e.chain_get_state(), field["chain"])
    e.close()


def test_known_answers_through_the_c_abi():
    """The closed forms of tests/test_ensemble_restatement.py, with the arrays handed to the library directly."""
    n, nb = KNOWN_N, KNOWN_NBIN
    L = box_of(n)
    e = Engine(HamilParams(Nx=n, L=L))
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)

    def measure(a, b):
        a, b = (np.ascontiguousarray(x, dtype=np.float64) for x in (a, b))
        out = [np.full(nb, -1.) for _ in range(5)]
        nm = np.full(nb, 7, dtype=np.uint64)
        rc = e.lib.bchmc_measure_cross_spectrum(e.h, 0, a.ctypes.data_as(dp), 0, b.ctypes.data_as(dp), nb,
                                                out[0].ctypes.data_as(dp), nm.ctypes.data_as(up),
                                                *(o.ctypes.data_as(dp) for o in out[1:]))
        assert rc == 0
        out2 = [np.full(nb, -1.) for _ in range(5)]
        assert e.lib.bchmc_measure_cross_spectrum(e.h, 0, a.ctypes.data_as(dp), 0, b.ctypes.data_as(dp), nb,
                                                  out2[0].ctypes.data_as(dp), None,
                                                  *(o.ctypes.data_as(dp) for o in out2[1:])) == 0  # nmode may be NULL
        # float atomics: the second call agrees to rounding, not bit for bit
        assert np.max(np.abs(out[0] - out2[0])) <= TOL_RMODE * np.max(out[0])
        assert np.max(np.abs(out[1] - out2[1])) <= TOL_FIELD * np.max(out[1])
        return out[0], nm, out[1], out[2], out[3], out[4]

    check_known_answers(measure, fields_of(n)["truth"], n, L, nb, KNOWN_M)
    e.close()


def test_a_measurement_leaves_the_state_alone():
    """With a pending proposal: the chain state, the momenta, the proposal and deltaX are bit for bit what they were,
    chain_accept succeeds, and the next attempt returns the dH of a twin that did not measure."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)

    def run(measure):
        e = Engine(c.p, deterministic=1)
        e.upload(**c.arrays())
        e.chain_set_state(c.q0)
        e.chain_set_momenta(c.p0)
        e.chain_attempt(c.eps, 3)
        before = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + (e.fetch("deltaX"),)
        if measure:
            for sa, sb in (("chain", "deltaX"), ("host", "chain"), ("deltaX", "host")):
                got = e.measure_cross_spectrum(c.truth if sa == "host" else None, c.truth if sb == "host" else None, 16, sa, sb)
                field = dict(host=c.truth, chain=before[0], deltaX=before[4])
                compare("%s x %s, proposal pending" % (sa, sb), got, er.cross_spectrum(field[sa], field[sb], 16, c.p.L, 16),
                        TOL_FIELD)
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


def test_refusals_non_finite_fields_and_the_hamil_layer():
    n, nb = 16, 16
    f = fields_of(n)
    sig = np.array(f["truth"]).reshape(-1)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    arr = [np.zeros(4) for _ in range(5)]
    nm = np.zeros(4, dtype=np.uint64)
    out = (arr[0].ctypes.data_as(dp), nm.ctypes.data_as(up)) + tuple(a.ctypes.data_as(dp) for a in arr[1:])
    s = sig.ctypes.data_as(dp)
    e = Engine(HamilParams(Nx=n, L=box_of(n)))
    fn = e.lib.bchmc_measure_cross_spectrum
    refused = ((ARG, (e.h, 1, s, 0, s, 2)), (ARG, (e.h, 0, s, 2, s, 2)),      # a signal with a source that is not the host
               (ARG, (e.h, 0, None, 0, s, 2)), (ARG, (e.h, 0, s, 0, None, 2)),  # the host source without a signal
               (ARG, (e.h, 0, s, 0, s, 0)), (ARG, (e.h, 0, s, 0, s, 2049)),     # n_bin outside 1..2048
               (ARG, (e.h, 3, None, 0, s, 2)), (ARG, (e.h, 0, s, 3, None, 2)),  # an unknown source
               (STATE, (e.h, 1, None, 0, s, 2)), (STATE, (e.h, 0, s, 1, None, 2)),  # no chain state, on either side
               (STATE, (e.h, 2, None, 0, s, 2)), (STATE, (e.h, 0, s, 2, None, 2)),  # deltaX before any forward model
               (ARG, (None, 0, s, 0, s, 2)))                                    # a null handle
    want = er.cross_spectrum(sig, sig, n, box_of(n), nb)
    for code, args in refused:
        assert fn(*args, *out) == code, args[1:]
        assert not any(a.any() for a in arr) and not nm.any()
    compare("after the refusals", e.measure_cross_spectrum(sig, sig, nb), want, TOL_FIELD)
    for k in (0, 2, 3, 4, 5):  # every output but nmode is needed
        ptrs = list(out)
        ptrs[k] = None
        assert fn(e.h, 0, s, 0, s, 2, *ptrs) == ARG
    with pytest.raises(BchmcError) as err:
        e.measure_cross_spectrum(sig, sig, 2049)
    assert err.value.code == ARG
    with pytest.raises(BchmcError) as err:
        e.measure_cross_spectrum(sig, None, 4, source_b="deltaX")
    assert err.value.code == STATE
    # one NaN cell on one side: NaN in every populated bin of that side's power, of cross and of coeff, and nowhere else
    bad = sig.copy()
    bad[1234] = np.nan
    km, nmode, pa, pb, cross, coeff = e.measure_cross_spectrum(sig, bad, nb)
    pop = want[1] > 0
    assert np.array_equal(nmode, want[1]) and np.all(np.isnan(pb[pop])) and np.all(np.isnan(cross[pop]))
    assert np.all(np.isnan(coeff[pop])) and not np.isnan(pa).any()
    for a in (pa, pb, cross, coeff):
        assert np.all(a[~pop] == 0)
    zero = e.measure_cross_spectrum(sig, np.zeros(n ** 3), nb)
    assert not zero[3].any() and not zero[4].any() and not zero[5].any() and zero[2][1:].all()  # (bin 0: k = 0 alone)

    class View:  # what hamil.py's functions read of a HamilData
        engine = e
    e.chain_set_state(f["q0"])
    compare("hamil", hamil.measure_cross_spectrum(View, sig, None, nb), restated(n, nb), TOL_FIELD)
    e.close()
