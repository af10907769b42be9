"""bchmc_measure_corr / bchmc_measure_corr2d / bchmc_chain_forward on the device against the numpy restatement of the
reference's tools (tests/corr_restatement.py).  Every bin is compared, the empty ones included:

* nmode: equal.  A cell that changed its bin is a failure, not a tolerance.
* rmode: max relative difference <= 1e-14 over populated bins, empty bins exactly 0.
* corr: max |engine - restatement| <= TOL_FIELD max |restatement| on fp64 handles, TOL_F32_FIELD on fp32 handles.
  The restatement alone (float64 against long double transforms) sits at <= 2e-16 of max |corr|.

The measured levels are printed by every test (run with -s)."""
import ctypes as C

import numpy as np
import pytest

from barcode_amd import hamil, inputs, io
from barcode_amd.engine import BchmcError, Engine
from barcode_amd.params import HamilParams
from tests import corr_restatement as cr
from tests.test_corr_restatement import (check_constant, check_cosine, check_spike, known_constant, known_cosine,
                                         known_spike)
from tests.test_gpu_parity import TOL_F32_FIELD
from tests.util import TOL_FIELD, Case, rel_l2

pytestmark = pytest.mark.gpu

TOL_RMODE = 1e-14


def tol_of(precision):
    return TOL_F32_FIELD if precision else TOL_FIELD


def compare(tag, got, want, tol):
    """(rmode, nmode, corr) of the engine against the restatement's, all bins."""
    rm, nm, co = (np.asarray(a).ravel() for a in got)
    rm0, nm0, co0 = (np.asarray(a).ravel() for a in want[:3])
    assert nm.dtype == np.uint64 and np.array_equal(nm, nm0), "%s: %d bins differ in nmode" % (tag, int((nm != nm0).sum()))
    pop = nm0 > 0
    assert np.all(rm[~pop] == 0) and np.all(co[~pop] == 0)
    lvl_r = float(np.max(np.abs(rm[pop] - rm0[pop]) / np.where(rm0[pop] > 0, rm0[pop], 1.)))
    lvl_c = float(np.max(np.abs(co - co0)) / np.max(np.abs(co0)))
    print("%s: %d bins (%d populated, %d cells), rmode rel %.2e, corr %.2e of max" %
          (tag, nm.size, int(pop.sum()), int(nm.sum()), lvl_r, lvl_c))
    assert lvl_r <= TOL_RMODE, (tag, lvl_r)
    assert lvl_c <= tol, (tag, lvl_c)


def both(e, signal, n_bin, source=None):
    return e.measure_corr(signal, n_bin, source), e.measure_corr2d(signal, n_bin, source)


def restate(sig, n, L, n_bin):
    return cr.corr_grid(sig, n, L, n_bin), cr.corr2d(sig, n, L, n_bin)


def check_field(tag, e, sig, n, L, n_bin, tol, source=None, send=True):
    """Both functions of one field: through `source` (the field is sent only for the host source)."""
    got1, got2 = both(e, sig if send else None, n_bin, source)
    want1, want2 = restate(sig, n, L, n_bin)
    assert got1[0].shape == (n_bin,) and got2[0].shape == (n_bin, n_bin)
    compare(tag + " 1-D", got1, want1, tol)
    compare(tag + " 2-D", got2, want2, tol)
    return got1, got2


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("n", (16, 32, 64))
def test_corr_of_host_field_and_chain_state(n, precision):
    """n_bin = n (the bin-edge family: on the diagonal rtot / dr = 2 i n_bin / n is an integer in exact arithmetic),
    the automatic count, 200, 2048 and 1; a host field and the resident state, both functions.

    With n_bin = 1 the single 2-D bin holds every cell, so its corr is sum_r A(r) / N^2 = (mean delta)^2: for the
    zero-mean fields of make_fields that is rounding noise on both sides (measured at 16^3: restatement -1.0e-18, engine
    2.6e-18, against A(0) / N ~ 1e-3) and "of max |restatement|" bounds nothing.  The n_bin = 1 case therefore measures
    the same fields with a mean of 0.3 added, which makes the number it checks well conditioned."""
    L = 200. * n / 64.
    p = HamilParams(Nx=n, L=L)
    f = inputs.make_fields(p)
    e = Engine(p, precision=precision)
    e.chain_set_state(f["q0"])
    for n_bin in (n, cr.auto_nbin(n, L), 200, 2048, 1):
        tag = "%d^3 %s n_bin %d" % (n, "fp32" if precision else "fp64", n_bin)
        truth, q0 = f["truth"], f["q0"]
        if n_bin == 1:
            truth, q0 = truth + 0.3, q0 + 0.3
            e.chain_set_state(q0)
        check_field(tag + " host", e, truth, n, L, n_bin, tol_of(precision))
        check_field(tag + " chain", e, q0, n, L, n_bin, tol_of(precision), "chain", send=False)
    # n_bin = 1 on the make_fields field itself: nmode and rmode as everywhere, corr to tol x A(0) / N (the mean square
    # of the field, the scale of corr[0] at any finer binning) since the bin's own value is (mean delta)^2 ~ 0
    sig = f["truth"]
    for got, want in zip(both(e, sig, 1), restate(sig, n, L, 1)):
        nm, nm0 = np.asarray(got[1]).ravel(), np.asarray(want[1]).ravel()
        assert np.array_equal(nm, nm0)
        assert abs(float(np.ravel(got[0])[0]) - float(want[0][0])) <= TOL_RMODE * float(want[0][0])
        lvl = abs(float(np.ravel(got[2])[0]) - float(want[2][0])) / float(np.mean(sig * sig))
        print("%d^3 n_bin 1, zero-mean field: corr differs by %.2e of A(0)/N" % (n, lvl))
        assert lvl <= tol_of(precision)
    assert e.measure_corr(None, 0)[0].shape == (cr.auto_nbin(n, L),)  # n_bin = 0 on the host layer: the automatic count
    e.close()


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_all_sources_on_an_rsd_chain(precision):
    """The chain state after chain_set_state and again after an accepted attempt; deltaX after chain_forward(1) and
    chain_forward(0): the redshift-space and the real-space density of one sample, whose 2-D functions must differ."""
    n = 32
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    L, tol = c.p.L, tol_of(precision)
    e = c.engine(precision=precision)
    nbs = (n, cr.auto_nbin(n, L))
    e.chain_set_state(c.q0)
    for nb in nbs:
        check_field("set_state n_bin %d" % nb, e, c.q0, n, L, nb, tol, "chain", send=False)
    e.chain_set_momenta(c.p0)
    e.chain_attempt(c.eps, 3)
    e.chain_accept(True)
    q = e.chain_get_state()
    assert rel_l2(q, c.q0) > 1e-6
    for nb in nbs:
        check_field("accepted n_bin %d" % nb, e, q, n, L, nb, tol, "chain", send=False)
    two_d = {}
    for rsd in (1, 0):
        e.chain_forward(rsd)
        dX = e.fetch("deltaX")
        for nb in nbs:
            got = check_field("deltaX rsd %d n_bin %d" % (rsd, nb), e, dX, n, L, nb, tol, "deltaX", send=False)
            two_d[rsd, nb] = got[1][2]
        assert np.array_equal(e.fetch("deltaX"), dX)  # the measurement left it alone
    for nb in nbs:
        diff = np.max(np.abs(two_d[1, nb] - two_d[0, nb])) / np.max(np.abs(two_d[0, nb]))
        print("2-D corr, redshift space against real space, n_bin %d: %.2e of max" % (nb, diff))
        assert diff > 1e-3  # far above either tolerance: two different fields were measured
    e.close()


@pytest.mark.parametrize("two_d", (False, True), ids=("1d", "2d"))
def test_256_against_the_vectorised_restatement(two_d):
    n, L = 256, 800.
    rng = np.random.default_rng(11)
    x = np.arange(n) * (2 * np.pi / n)
    sig = (rng.standard_normal((n, n, n)) + 2. * np.cos(3 * x)[:, None, None] * np.cos(2 * x)[None, :, None] +
           1.5 * np.cos(5 * x)[None, None, :]).reshape(-1)
    nb = cr.auto_nbin(n, L)
    e = Engine(HamilParams(Nx=n, L=L))
    want = cr.corr2d(sig, n, L, nb) if two_d else cr.corr_grid(sig, n, L, nb)
    fn = e.measure_corr2d if two_d else e.measure_corr
    compare("256^3 host", fn(sig, nb), want, TOL_FIELD)
    e.chain_set_state(sig)
    compare("256^3 chain", fn(None, nb), want, TOL_FIELD)
    compare("256^3 chain, cached geometry", fn(None, nb), want, TOL_FIELD)
    e.close()


def test_known_answers_through_the_engine():
    """The three closed forms of tests/test_corr_restatement.py::test_known_answers_of_the_restatement."""
    n = 32
    L = 200. * n / 64.
    nb = cr.auto_nbin(n, L)
    e = Engine(HamilParams(Nx=n, L=L))
    check_constant(*both(e, known_constant(n, 1.7), nb), 1.7)
    check_spike(*both(e, known_spike(n, 2.5), nb), 2.5, float(n ** 3))
    check_cosine(e.measure_corr2d(known_cosine(n, 1.3, 3), nb), n, L, 1.3, 3)
    e.close()


def rows_per_perp_bin(n, L, n_bin):
    pos = cr._positions(n, L)
    _, dr = cr.rmax_dr(L, n_bin)
    p2 = pos * pos
    nperp = (np.sqrt(p2[:, None] + p2[None, :]) / dr).astype(np.uint64)
    return np.bincount(nperp[nperp < n_bin].astype(np.int64))


@pytest.mark.parametrize("n,n_bin,split", ((8, 200, False), (64, 1, True), (64, 7, True)))
def test_perp_bins_split_across_workgroups_or_not(n, n_bin, split):
    """A perp bin is cut into slices of max(8, min(64, n^2 / 2048)) rows, one workgroup each: cases where
    no bin is cut, where one bin holds every row, and where bins of very different size are cut."""
    L = 200. * n / 64.
    per = max(8, min(64, n * n // 2048))
    assert (rows_per_perp_bin(n, L, n_bin).max() > per) == split
    p = HamilParams(Nx=n, L=L)
    e = Engine(p)
    sig = inputs.make_fields(p)["truth"] + (0.3 if n_bin == 1 else 0.)  # n_bin 1: see the first test's docstring
    check_field("%d^3 n_bin %d" % (n, n_bin), e, sig, n, L, n_bin, TOL_FIELD)
    e.close()


@pytest.mark.parametrize("pad", ("0", "1"))
def test_padded_and_unpadded_rows(pad, monkeypatch):
    monkeypatch.setenv("BCHMC_FFT_PAD", pad)
    n, L = 16, 50.
    p = HamilParams(Nx=n, L=L)
    f = inputs.make_fields(p)
    e = Engine(p)
    e.chain_set_state(f["q0"])
    for nb in (n, cr.auto_nbin(n, L)):
        check_field("pad %s host" % pad, e, f["truth"], n, L, nb, TOL_FIELD)
        check_field("pad %s chain" % pad, e, f["q0"], n, L, nb, TOL_FIELD, "chain", send=False)
    e.close()


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_chain_forward_equals_forward_of_the_fetched_state(precision):
    """deltaX and pos* of chain_forward(r) against forward(chain_get_state(), r).  The two differ by one transform pair
    of the state in the handle's storage type, so the bound is the project's single-evaluation one for that type."""
    c = Case(Nx=32, likelihood=1, rsd_model=1)
    tol = tol_of(precision)
    e, e2 = c.engine(precision=precision), c.engine(precision=precision)
    e.chain_set_state(c.q0)
    q = e.chain_get_state()
    for rsd in (1, 0, -1):
        e.chain_forward(rsd)
        e2.forward(q, rsd)
        for k in ("deltaX", "posx", "posy", "posz"):
            lvl = rel_l2(e.fetch(k), e2.fetch(k))
            print("chain_forward(%d) %s: rel-L2 %.2e" % (rsd, k, lvl))
            assert lvl < tol
    assert np.array_equal(e.chain_get_state(), q)
    e.close()
    e2.close()


def chain_run(c, between=None, deterministic=1):
    """set_state, one accepted attempt, `between(engine)` if given, a second attempt from the carried gradient.  Without
    `between` nothing at all is called between the two attempts but the reads of the state and the momenta."""
    e = Engine(c.p, deterministic=deterministic)
    e.upload(**c.arrays())
    e.chain_set_state(c.q0)
    e.chain_set_momenta(c.p0)
    e.chain_attempt(c.eps, 3)
    e.chain_accept(True)
    extra = between(e) if between else None
    state, mom = e.chain_get_state(), e.chain_get_momenta()
    e.chain_set_momenta(0.9 * c.p0)
    dH, terms, done = e.chain_attempt(c.eps, 3)
    prop = e.chain_get_proposal()[0]
    e.close()
    return dict(state=state, mom=mom, dH=dH, terms=terms, prop=prop, extra=extra)


def test_measurements_change_nothing_else():
    """chain_get_state, fetch("deltaX"), the momenta and the six energy terms of a following attempt (which starts from
    the carried gradient and -log L) are bit for bit those of a run without the measurements, on deterministic handles.
    Both arms run one chain_forward first, so that there is a deltaX to measure and to compare; the run that calls
    nothing at all between the attempts is the baseline of the next test."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)

    def forward_only(e):
        e.chain_forward(-1)
        return e.fetch("deltaX")

    def measure(e):
        e.chain_forward(-1)
        out = []
        for nb in (16, 9):
            out += [both(e, None, nb, "chain"), both(e, None, nb, "deltaX"), both(e, c.truth, nb)]
        return e.fetch("deltaX"), out

    plain = chain_run(c, forward_only)
    meas = chain_run(c, measure)
    for k in ("state", "mom", "terms", "prop"):
        assert np.array_equal(plain[k], meas[k]), k
    assert plain["dH"] == meas["dH"] and np.array_equal(plain["extra"], meas["extra"][0])
    # and a second run gives the same measurements, bit for bit (1-D and 2-D, all three sources)
    again = chain_run(c, measure)
    for a, b in zip(meas["extra"][1], again["extra"][1]):
        for r1, r2 in zip(a, b):
            assert all(np.array_equal(x, y) for x, y in zip(r1, r2))


def test_chain_forward_and_measurements_keep_the_carried_gradient():
    """test_gradient_carried_across_attempts' observable: the attempt after chain_forward (real space, redshift space,
    in either order as the last call) and after measurements gives the dH, the six terms and the proposal of a chain
    that called NOTHING between its two attempts."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)
    plain = chain_run(c)
    arms = dict(fwd0=lambda e: e.chain_forward(0), fwd1=lambda e: e.chain_forward(1),
                fwd10=lambda e: (e.chain_forward(1), e.chain_forward(0)),
                meas=lambda e: (both(e, None, 16, "chain"), both(e, c.truth, 16), e.chain_forward(0),
                                both(e, None, 16, "deltaX")))
    for name, between in arms.items():
        run = chain_run(c, between)
        assert plain["dH"] == run["dH"] and np.array_equal(plain["terms"], run["terms"]), name
        for k in ("state", "mom", "prop"):
            assert np.array_equal(plain[k], run[k]), (name, k)


def test_a_pending_proposal_survives_a_measurement_but_not_chain_forward():
    c = Case(Nx=16, likelihood=1, rsd_model=1)
    e = c.engine()
    e.chain_set_state(c.q0)
    e.chain_set_momenta(c.p0)
    e.chain_attempt(c.eps, 3)
    q1 = e.chain_get_proposal()[0]
    both(e, None, 16, "chain"), both(e, c.truth, 16), both(e, None, 16, "deltaX")
    assert np.array_equal(e.chain_get_proposal()[0], q1)
    e.chain_accept(True)
    assert np.array_equal(e.chain_get_state(), q1)
    e.chain_set_momenta(c.p0)
    e.chain_attempt(c.eps, 3)
    e.chain_forward(0)
    with pytest.raises(BchmcError) as err:
        e.chain_accept(True)
    assert err.value.code == 9
    e.close()


@pytest.mark.parametrize("deterministic", (0, 1))
def test_repeatable(deterministic):
    """Two calls and two fresh handles: the 2-D results are array_equal on any handle (no atomics, fixed order); the
    1-D results on deterministic handles -- and, since its sums are integer, on the others too."""
    n = 32
    p = HamilParams(Nx=n, L=100.)
    f = inputs.make_fields(p)
    runs = []
    for _ in range(2):
        e = Engine(p, deterministic=deterministic)
        e.chain_set_state(f["q0"])
        for _ in range(2):
            runs.append([both(e, None, nb, "chain") + both(e, f["truth"], nb) for nb in (n, 5, 2048)])
        e.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            for r1, r2 in zip(a, b):
                assert all(np.array_equal(x, y) for x, y in zip(r1, r2))


def test_error_paths():
    n = 16
    p = HamilParams(Nx=n, L=50.)
    sig = inputs.make_fields(p)["truth"]
    e = Engine(p)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    rm, co, nm = np.zeros(4), np.zeros(4), np.zeros(4, dtype=np.uint64)
    args = (rm.ctypes.data_as(dp), nm.ctypes.data_as(up), co.ctypes.data_as(dp))
    s = sig.ctypes.data_as(dp)
    for fn in (e.lib.bchmc_measure_corr, e.lib.bchmc_measure_corr2d):
        assert fn(e.h, 0, s, 0, *args) == 1 and fn(e.h, 0, s, 2049, *args) == 1      # n_bin outside 1..2048
        assert fn(e.h, 0, None, 2, *args) == 1                                       # host source without a signal
        assert fn(e.h, 1, s, 2, *args) == 1 and fn(e.h, 2, s, 2, *args) == 1         # a signal with another source
        assert fn(e.h, 3, None, 2, *args) == 1                                       # unknown source
        assert fn(e.h, 1, None, 2, *args) == 9                                       # no chain state
        assert fn(e.h, 2, None, 2, *args) == 9                                       # no forward evaluation
        assert fn(e.h, 0, s, 2, None, args[1], args[2]) == 1
    assert e.lib.bchmc_chain_forward(e.h, 0) == 9 and e.lib.bchmc_chain_forward(None, 0) == 1
    assert not rm.any() and not co.any() and not nm.any()
    for meth in (e.measure_corr, e.measure_corr2d):
        with pytest.raises(BchmcError) as err:
            meth(sig, 2049)
        assert err.value.code == 1
        with pytest.raises(BchmcError) as err:
            meth(None, 4, "deltaX")
        assert err.value.code == 9
    with pytest.raises(BchmcError):
        e.chain_forward()
    # the handle still works
    compare("after the errors", e.measure_corr(sig, n), cr.corr_grid(sig, n, p.L, n), TOL_FIELD)
    e.close()


def test_shim_hamil_and_io_layers(tmp_path, monkeypatch):
    """bchmc_shim::measure_corr_grid / measure_corr2D / chain_forward and the hamil.py names equal the engine calls;
    planepar = false raises upstream's text; io.dump_deltas writes dump_deltas' three files of an RSD sample."""
    from barcode_amd.shim import ShimError, ShimHamil
    n = 16
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    e = c.engine()
    e.chain_set_state(c.q0)
    hd = ShimHamil(c.p, **c.arrays())
    hd.chain_set_state(c.q0)
    nb = cr.auto_nbin(n, c.p.L)
    for sig, src in ((c.truth, None), (None, "chain")):
        for got, want in ((hd.measure_corr_grid(sig, nb), e.measure_corr(sig, nb, src)),
                          (hd.measure_corr2D(sig, nb), e.measure_corr2d(sig, nb, src))):
            assert all(np.array_equal(x, y) for x, y in zip(got, want))
    for rsd in (1, 0):
        dX = hd.chain_forward(rsd).copy()
        e.chain_forward(rsd)
        assert rel_l2(dX, e.fetch("deltaX")) < TOL_FIELD
        got, want = hd.measure_corr2D(None, nb, of_deltaX=True), e.measure_corr2d(None, nb, "deltaX")
        assert np.array_equal(got[1], want[1]) and np.max(np.abs(got[2] - want[2])) <= TOL_FIELD * np.max(np.abs(want[2]))
        got, want = hd.measure_corr_grid(None, nb, of_deltaX=True), e.measure_corr(None, nb, "deltaX")
        assert np.array_equal(got[1], want[1]) and np.max(np.abs(got[2] - want[2])) <= TOL_FIELD * np.max(np.abs(want[2]))
    with pytest.raises(ShimError, match="non-plane-parallel option not yet implemented"):
        hd.measure_corr2D(c.truth, nb, planepar=False)
    hd.close()

    class View:  # what hamil.py's functions read of a HamilData
        engine = e
    assert all(np.array_equal(x, y) for x, y in zip(hamil.measure_corr_grid(View, c.truth, nb), e.measure_corr(c.truth, nb)))
    assert all(np.array_equal(x, y) for x, y in zip(hamil.measure_corr2D(View, None, 0), e.measure_corr2d(None, nb)))

    monkeypatch.chdir(tmp_path)  # a relative directory without a '.': write_array then appends ".dat"
    paths = io.dump_deltas(e, "", "_3")
    assert paths == ["deltaLAG_3.dat", "deltaRSS_3.dat", "deltaEUL_3.dat"]
    N = n ** 3
    assert np.array_equal(io.read_array(paths[0], N), e.chain_get_state())
    e.chain_forward(1)
    rss = e.fetch("deltaX")
    e.chain_forward(0)
    eul = e.fetch("deltaX")
    assert rel_l2(io.read_array(paths[1], N), rss) < TOL_FIELD and rel_l2(io.read_array(paths[2], N), eul) < TOL_FIELD
    assert rel_l2(rss, eul) > 1e-3
    e.close()
