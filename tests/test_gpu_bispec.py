"""bchmc_bispectrum on the device: B, ntri and the per-shell statistics against the enumerated definition of
tests/bispec_reference.py (n <= 16) or its float64 restatement (32^3 and 96^3) under the bounds of tests/bispec_bound.py,
exact counts, known answers, all three sources on fp64 and fp32 handles, the contraction kernel alone on chosen arrays
(libbchmc_fft_probe.so), bitwise repeatability, the cached table, the contracts of include/bchmc.h and the upper layers.
Grids: 4 (smallest), 5 and 9 (odd), 8, 12 and 16 (even), 32 once (256 tiles of the contraction) and 96 once (6912 tiles on
512 workgroups, and the grid-stride tail of the filter and statistics passes)."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

from barcode_amd import engine as engine_mod
from barcode_amd import hamil, io
from barcode_amd.engine import BchmcError, Engine
from barcode_amd.params import HamilParams
from tests import bispec_bound as bb
from tests import bispec_reference as br
from tests.test_bispec_bounds import CASES, both, ident
from tests.test_gpu_ensemble import samples_of
from tests.util import Case

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "barcode_amd", "libbchmc_fft_probe.so")
PREC = pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
DTYPE = (np.float64, np.float32)
KEYS = ("b", "ntri", "q", "kmean", "nmode", "power")


def engine_of(n, precision=0):
    return Engine(HamilParams(Nx=n, L=br.box_of(n)), precision=precision)


def check(res, x, L, k_min, dk, ns, dtype, tag, want=None):
    """Every output of one call against the reference of its source x (n, n, n).  want: the enumerated definition, or
    None -- then the reference is the float64 restatement, which obeys the float64 bound itself, so that bound is added."""
    n = x.shape[0]
    ref = br.restatement(x, L, k_min, dk, ns)
    bnd = bb.bounds(x, L, ref, dtype)
    if want is None:
        want = ref
        own = bb.bounds(x, L, ref, np.float64)
        bnd = {k: bnd[k] + own[k] for k in ("b", "ntri", "power", "kmean")}
    comp = ref["computed"]
    assert np.array_equal(res["triplets"], br.triplets(ns)), tag
    # exact integers
    assert res["nmode"].dtype == np.uint64 and np.array_equal(res["nmode"].astype(np.int64), np.asarray(want["nmode"]).astype(np.int64)), tag
    count = np.rint(np.asarray(want["ntri"], dtype=np.float64))
    if dtype is np.float64:
        assert np.array_equal(np.rint(res["ntri"]), count), tag
    fn = bb.fraction(np.abs(res["ntri"] - count), bnd["ntri"])
    fb = bb.fraction(np.abs(res["b"] - want["b"]).astype(np.float64), bnd["b"])
    fp = bb.fraction(np.abs(res["power"] - want["power"]).astype(np.float64), bnd["power"])
    fk = bb.fraction(np.abs(res["kmean"] - want["kmean"]), bnd["kmean"])
    print("%s: error / bound B %.3g, ntri %.3g, power %.3g, kmean %.3g" % (tag, fb, fn, fp, fk))
    assert fb <= 1.0 and fn <= 1.0 and fp <= 1.0 and fk <= 1.0, tag
    # B4: what is not computed is 0, and so is a triplet without a triangle
    assert np.all(res["b"][~comp] == 0) and np.all(res["ntri"][~comp] == 0), tag
    filled = comp & ~(res["ntri"] < 0.5)
    assert np.all(res["b"][~filled] == 0) and np.all(res["q"][~filled] == 0), tag
    # B6: Q is formed from the returned arrays
    assert np.array_equal(res["q"], br.reduced(res["b"], res["power"], filled)), tag
    return fb, fn, fp


# ---- against the definition ------------------------------------------------------------------------------------------------
@PREC
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_host_field_against_the_enumeration(case, precision):
    n, kmin_kf, dk_kf, ns = case
    x, L, _, want = both(case)
    k_min, dk = br.edges(n, kmin_kf, dk_kf)
    e = engine_of(n, precision)
    res = e.bispectrum(x, k_min=kmin_kf, dk=dk_kf, n_shell=ns, units="kf")
    check(res, x, L, k_min, dk, ns, DTYPE[precision], "host %s %s" % (ident(case), DTYPE[precision].__name__), want)
    # the same shells in h/Mpc are the same call
    again = e.bispectrum(x, k_min=k_min, dk=dk, n_shell=ns)
    assert all(np.array_equal(res[k], again[k]) for k in KEYS)
    e.close()


@pytest.mark.parametrize("case", ((32, 0.5, 2.0, 8), (96, 0.5, 3.0, 8)), ids=ident)
def test_host_field_against_the_restatement(case):
    """32^3: 256 tiles, one per workgroup, aliased triangles (upper edge 16.5 k_f).  96^3: 6912 tiles on 512 workgroups,
    13.5 per workgroup, every grid-stride kernel of the call in its second, partial trip; B4's rule active (24.5 <= 32)."""
    n, kmin_kf, dk_kf, ns = case
    x = br.field(n)
    L = br.box_of(n)
    k_min, dk = br.edges(n, kmin_kf, dk_kf)
    assert br.rule_active(n, L, k_min, dk, ns) == (n == 96)
    e = engine_of(n, 0)
    res = e.bispectrum(x, k_min=kmin_kf, dk=dk_kf, n_shell=ns, units="kf")
    check(res, x, L, k_min, dk, ns, np.float64, "host %s" % ident(case))
    if n == 96:
        assert np.count_nonzero(~br.computed(n, L, k_min, dk, ns)) > 0
    e.close()


# ---- known answers -----------------------------------------------------------------------------------------------------------
def counts_of(n, kmin_kf, dk_kf, ns):
    L = br.box_of(n)
    return br.sorted_table(br.enumerate_direct(n, L, *br.edges(n, kmin_kf, dk_kf), ns)[0])


@PREC
@pytest.mark.parametrize("n", (8, 9, 12))
def test_three_waves_that_close(n, precision):
    """x = a cos(k1 r) + b cos(k2 r) + c cos(k3 r), k1 + k2 + k3 = 0, in the shells 0, 2 and 3 of k_min = 0.5 k_f,
    dk = 0.7 k_f: x^(+-k1) = a N / 2 and so on, the closed triples with all factors non-zero are (k1, k2, k3) and its
    negative, so the sum over triangles is 2 abc N^3 / 8 and B(0, 2, 3) = L^6 abc / (4 ntri).  Every other triplet is 0
    within bound: no other three of the six modes close.

    Two of the three in one shell, k1 and k2 in shell 2 and k3 in shell 3: the ordered triples of shells (2, 2, 3) that
    close are (k1, k2, k3), (k2, k1, k3) and their negatives, four of them, so the sum doubles: B(2, 2, 3) =
    L^6 abc / (2 ntri)."""
    a, b, c = 1.5, -0.75, 2.0
    L = br.box_of(n)
    kmin_kf, dk_kf, ns = 0.5, 0.7, 4
    k_min, dk = br.edges(n, kmin_kf, dk_kf)
    cnt = counts_of(n, kmin_kf, dk_kf, ns)
    trip = [tuple(t) for t in br.triplets(ns)]
    e = engine_of(n, precision)
    for waves, shells, factor in ((((1, 0, 0), (1, 2, 0), (-2, -2, 0)), (0, 2, 3), 4.0),
                                  (((1, 2, 0), (2, -1, 0), (-3, -1, 0)), (2, 2, 3), 2.0)):
        sh = br.shells(n, L, k_min, dk, ns)
        assert tuple(sorted(int(sh[m]) for m in waves)) == shells
        x = br.cosines(n, list(zip((a, b, c), waves)))
        res = e.bispectrum(x, k_min=kmin_kf, dk=dk_kf, n_shell=ns, units="kf")
        t = trip.index(shells)
        want = np.zeros(len(trip))
        want[t] = L ** 6 * a * b * c / (factor * cnt[t])
        bnd = bb.bounds(x, L, br.restatement(x, L, k_min, dk, ns), DTYPE[precision])
        f = bb.fraction(np.abs(res["b"] - want), bnd["b"])
        print("three waves %d^3 %s %s: error / bound %.3g" % (n, shells, DTYPE[precision].__name__, f))
        assert f <= 1.0 and abs(res["b"][t]) > 100 * bnd["b"][t]
        if precision == 0:
            assert np.array_equal(np.rint(res["ntri"]), cnt * br.computed(n, L, k_min, dk, ns))
    e.close()


@PREC
def test_one_wave_and_a_constant(precision):
    """A single plane wave has no closed triple of non-zero modes: B = 0 everywhere within bound, and power only in its
    shell, L^3 a^2 / (2 nmode).  A constant lives in the mode k = 0, which belongs to no shell: all zeros, exactly."""
    n, a = 8, 1.25
    L = br.box_of(n)
    kmin_kf, dk_kf, ns = 0.0, 1.0, 4
    k_min, dk = br.edges(n, kmin_kf, dk_kf)
    e = engine_of(n, precision)
    x = br.cosines(n, [(a, (1, 2, 0))])  # |k| = 2.236 k_f: shell 2
    res = e.bispectrum(x, k_min=kmin_kf, dk=dk_kf, n_shell=ns, units="kf")
    ref = br.restatement(x, L, k_min, dk, ns)
    bnd = bb.bounds(x, L, ref, DTYPE[precision])
    assert bb.fraction(np.abs(res["b"]), bnd["b"]) <= 1.0
    want = np.zeros(ns)
    want[2] = L ** 3 * a * a / (2.0 * float(res["nmode"][2]))
    assert bb.fraction(np.abs(res["power"] - want), bnd["power"]) <= 1.0 and res["power"][2] > 0
    res = e.bispectrum(np.full((n, n, n), 3.0), k_min=kmin_kf, dk=dk_kf, n_shell=ns, units="kf")
    assert not res["b"].any() and not res["q"].any() and not res["power"].any()
    assert np.array_equal(res["nmode"].astype(np.int64), br.shell_stats_exact(n, L, k_min, dk, ns)[0])
    e.close()


# ---- every source --------------------------------------------------------------------------------------------------------------
@PREC
@pytest.mark.parametrize("case", ((9, 1.0, 0.5, 4), (16, 0.5, 1.5, 3)), ids=ident)
def test_chain_state_and_deltax(case, precision):
    """The chain state after chain_set_state, and deltaX after a forward model of it, against the definition of the
    field each stands for."""
    n, kmin_kf, dk_kf, ns = case
    c = Case(Nx=n, likelihood=1)
    e = c.engine(precision=precision)
    e.chain_set_state(c.q0)
    e.chain_forward(0)
    L = c.p.L
    kf = 2.0 * np.pi / L
    k_min, dk = kmin_kf * kf, dk_kf * kf
    for src, x in (("chain", c.q0), ("deltaX", e.fetch("deltaX"))):
        x = np.asarray(x, dtype=np.float64).reshape((n,) * 3)
        res = e.bispectrum(source=src, k_min=kmin_kf, dk=dk_kf, n_shell=ns, units="kf")
        check(res, x, L, k_min, dk, ns, DTYPE[precision], "%s %s %s" % (src, ident(case), DTYPE[precision].__name__),
              br.definition(x, L, k_min, dk, ns))
    e.close()


# ---- the contraction alone --------------------------------------------------------------------------------------------------
def probe_triple(prec, arrays, s3_end=None):
    lib = C.CDLL(PROBE)
    vp = C.c_void_p
    lib.fftp_bispec_triple.argtypes = [C.c_int, C.c_int, C.c_longlong, vp, vp, vp, vp]
    a = np.ascontiguousarray(arrays, dtype=DTYPE[prec])
    ns, M = a.shape
    out = np.full(ns * (ns + 1) * (ns + 2) // 6, -7.0)
    end = None if s3_end is None else np.ascontiguousarray(s3_end, dtype=np.uint8)
    rc = lib.fftp_bispec_triple(prec, ns, M, a.ctypes.data, None if end is None else end.ctypes.data, out.ctypes.data, None)
    assert rc == 0, rc
    return out


def exact_sums(arrays):
    a = np.asarray(arrays).astype(np.int64)
    return np.array([np.sum(a[s1] * a[s2] * a[s3]) for s1, s2, s3 in br.triplets(a.shape[0])], dtype=np.float64)


@PREC
def test_contraction_probe_is_exact_on_integers(precision):
    """Small integers, whose products and sums are exact in double, so every S must be exact.  One non-zero cell per
    tile of 128 at a random place, 600 tiles and 37 cells more (more tiles than workgroups, M no multiple of the tile);
    then every cell non-zero with 1, 5, 8, 9, 16, 17 and 32 shells (the three instantiations, a pair of rows without a
    partner, one and more than four waves of row pairs)."""
    rng = np.random.Generator(np.random.Philox(31))
    M = 128 * 600 + 37
    a = np.zeros((5, M), dtype=np.int64)
    where = np.arange(0, M, 128) + rng.integers(0, 128, size=601)
    where = where[where < M]
    a[:, where] = rng.integers(-3, 4, size=(5, where.size))
    assert np.array_equal(probe_triple(precision, a), exact_sums(a)) and exact_sums(a).any()
    for ns in (1, 5, 8, 9, 16, 17, 32):
        a = rng.integers(-3, 4, size=(ns, 1000))
        assert np.array_equal(probe_triple(precision, a), exact_sums(a)), ns
    # rows cut short (B4): the triplets below each row's end are the same numbers
    ns = 12
    a = rng.integers(-3, 4, size=(ns, 700))
    end = np.zeros((32, 32), dtype=np.uint8)
    for s1 in range(ns):
        for s2 in range(s1, ns):
            end[s1, s2] = min(ns, s1 + s2 + 2)
    got, want = probe_triple(precision, a, end), exact_sums(a)
    keep = np.array([s3 < end[s1, s2] for s1, s2, s3 in br.triplets(ns)])
    assert np.array_equal(got[keep], want[keep]) and not keep.all()


# ---- repeatability and the cached table ----------------------------------------------------------------------------------------
def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint64), np.asarray(b[k]).view(np.uint64)) for k in KEYS)


@PREC
def test_bitwise_repeatable(precision):
    """Two calls, a call across bchmc_bispec_release and two handles give identical bits, for a host field and for the
    chain state."""
    n = 16
    x = br.field(n)
    kw = dict(k_min=0.5, dk=1.0, n_shell=6, units="kf")
    e, f = engine_of(n, precision), engine_of(n, precision)
    e.chain_set_state(x)
    f.chain_set_state(x)
    for src in (dict(signal=x), dict(source="chain")):
        a = e.bispectrum(**src, **kw)
        assert same_bits(a, e.bispectrum(**src, **kw))
        e.bispec_release()
        assert same_bits(a, e.bispectrum(**src, **kw))
        assert same_bits(a, f.bispectrum(**src, **kw))
    e.close()
    f.close()


def test_table_is_kept_and_replaced_and_resources_are_counted():
    gc.collect()
    start = engine_mod.live_resources()
    n = 8
    N = n ** 3
    s = samples_of(n)
    e = engine_of(n)
    created = engine_mod.live_resources()
    a = e.bispectrum(s[0], k_min=0.5, dk=1.0, n_shell=3, units="kf")
    first = engine_mod.live_resources()
    # three real arrays, the partials, the table and the half-complex array of a host source
    assert first[0] == created[0] + 6 and first[2:] == created[2:]
    T = 10
    nhp_bytes = first[1] - created[1] - 3 * N * 8 - T * 8 - (max(4 * T, 2048 * 9) + 9 + T) * 8
    assert nhp_bytes >= 16 * n * n * (n // 2 + 1)
    b = e.bispectrum(s[1], k_min=0.5, dk=1.0, n_shell=3, units="kf")
    assert engine_mod.live_resources() == first
    assert np.array_equal(a["ntri"].view(np.uint64), b["ntri"].view(np.uint64)) and not np.array_equal(a["b"], b["b"])
    assert np.array_equal(a["nmode"], b["nmode"]) and np.array_equal(a["kmean"], b["kmean"])
    # other edges, the same n_shell: the table is rebuilt in place
    c = e.bispectrum(s[1], k_min=1.0, dk=1.0, n_shell=3, units="kf")
    assert engine_mod.live_resources() == first and not np.array_equal(c["ntri"], b["ntri"])
    assert np.array_equal(np.rint(c["ntri"]), br.sorted_table(br.enumerate_direct(n, br.box_of(n), *br.edges(n, 1.0, 1.0), 3)[0]))
    # fewer shells: the arrays beyond them go, the partials and the table are taken afresh
    d = e.bispectrum(s[1], k_min=0.5, dk=1.0, n_shell=2, units="kf")
    assert engine_mod.live_resources()[0] == created[0] + 5
    assert np.array_equal(d["ntri"].view(np.uint64), a["ntri"][[0, 1, 3, 6]].view(np.uint64))  # (0,0,0) (0,0,1) (0,1,1) (1,1,1)
    # back: the same bits as at first
    assert same_bits(b, e.bispectrum(s[1], k_min=0.5, dk=1.0, n_shell=3, units="kf"))
    e.bispec_release()
    assert engine_mod.live_resources() == created
    e.bispec_release()  # nothing held: a no-op
    e.chain_set_state(s[0])
    with_state = engine_mod.live_resources()
    e.bispectrum(source="chain", k_min=0.5, dk=1.0, n_shell=3, units="kf")  # the chain state needs no half-complex array
    assert engine_mod.live_resources()[0] == with_state[0] + 5
    e.close()
    assert engine_mod.live_resources() == start


# ---- contracts -----------------------------------------------------------------------------------------------------------
def test_refusals():
    n = 8
    N = n ** 3
    e = engine_of(n)
    created = engine_mod.live_resources()
    lib, dp = e.lib, C.POINTER(C.c_double)
    x = np.array(br.field(n)).ravel()
    xp = x.ctypes.data_as(dp)
    out = np.zeros(5984)
    op = out.ctypes.data_as(dp)
    kf = 2.0 * np.pi / br.box_of(n)

    def opts(k_min=0.5 * kf, dk=kf, ns=3):
        return C.byref(engine_mod.BispecOpts(k_min, dk, ns, 0))

    def call(src, sig, o, b=op):
        return lib.bchmc_bispectrum(e.h, src, sig, o, b, None, None, None, None, None)

    def refused(rc, code, word):
        assert rc == code and word in lib.bchmc_last_error(e.h).decode(), (rc, lib.bchmc_last_error(e.h))

    refused(call(0, xp, None), ARG, "opts")
    for k_min in (-1.0, np.nan, np.inf):
        refused(call(0, xp, opts(k_min=k_min)), ARG, "k_min")
    for dk in (0.0, -1.0, np.nan, np.inf):
        refused(call(0, xp, opts(dk=dk)), ARG, "dk")
    for ns in (0, -1, 33):
        refused(call(0, xp, opts(ns=ns)), ARG, "n_shell")
    refused(call(0, xp, opts(), None), ARG, "b is NULL")
    refused(call(1, xp, opts()), ARG, "signal")
    refused(call(0, None, opts()), ARG, "signal")
    refused(call(3, None, opts()), ARG, "source")
    refused(call(1, None, opts()), STATE, "chain state")
    refused(call(2, None, opts()), STATE, "forward evaluation")
    assert engine_mod.live_resources() == created and not out.any()  # nothing was taken or written
    for kw in (dict(n_shell=0), dict(n_shell=33), dict(k_min=-1.0)):  # and through the Engine
        with pytest.raises(BchmcError) as err:
            e.bispectrum(x, **kw)
        assert err.value.code == ARG
    with pytest.raises(ValueError):
        e.bispectrum(x, units="1/Mpc")
    assert call(0, xp, opts()) == 0 and out[:10].any()  # optional outputs all NULL
    e.close()


def test_a_call_leaves_the_chain_as_it_was():
    """A deterministic handle at 16^3: two attempts with bispectra of all three sources between them -- one set with the
    proposal pending -- give dH, terms and the proposal bit for bit as a twin that measured nothing."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)

    def run(measure):
        e = Engine(c.p, deterministic=1)
        e.upload(**c.arrays())
        e.chain_set_state(c.q0)
        e.chain_set_momenta(c.p0)
        out = [e.chain_attempt(c.eps, 3)]
        before = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + (e.fetch("deltaX"),)
        if measure:
            for kw in (dict(source="chain"), dict(source="deltaX"), dict(signal=c.truth)):
                e.bispectrum(k_min=0.5, dk=1.0, n_shell=5, units="kf", **kw)
        after = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + (e.fetch("deltaX"),)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        out.append(e.chain_get_proposal())
        e.chain_accept(1)
        if measure:
            e.bispectrum(source="chain", k_min=0.5, dk=1.0, n_shell=5, units="kf")
            assert np.array_equal(e.chain_get_state(), before[2])
        e.chain_set_momenta(0.9 * c.p0)
        out.append(e.chain_attempt(c.eps, 3))
        out.append(e.chain_get_proposal())
        e.close()
        return out

    plain, measured = run(False), run(True)
    for k in (0, 2):
        assert plain[k][0] == measured[k][0] and np.array_equal(plain[k][1], measured[k][1]) and plain[k][2] == measured[k][2] == 3
    for k in (1, 3):
        assert all(np.array_equal(x, y) for x, y in zip(plain[k], measured[k]))


@PREC
def test_non_finite_field(precision):
    """B8: NaN in B of every computed triplet that holds a triangle and in power of every populated shell, and nowhere
    else; nmode, kmean and ntri are those of a finite field, bit for bit."""
    n = 9
    x = np.array(br.field(n))
    e = engine_of(n, precision)
    kw = dict(k_min=1.0, dk=0.5, n_shell=4, units="kf")
    good = e.bispectrum(x, **kw)
    x[2, 3, 4] = np.nan
    bad = e.bispectrum(x, **kw)
    for k in ("nmode", "kmean", "ntri"):
        assert np.array_equal(np.asarray(good[k]).view(np.uint64), np.asarray(bad[k]).view(np.uint64)), k
    filled = ~(good["ntri"] < 0.5)
    assert filled.any() and not filled.all() and np.all(good["nmode"] > 0)
    assert np.all(np.isnan(bad["b"][filled])) and np.all(bad["b"][~filled] == 0)
    assert np.all(np.isnan(bad["q"][filled])) and np.all(bad["q"][~filled] == 0)
    assert np.all(np.isnan(bad["power"]))
    assert same_bits(good, e.bispectrum(np.array(br.field(n)), **kw))  # and nothing of it stays in the handle
    e.close()


# ---- upper layers ----------------------------------------------------------------------------------------------------------
def test_hamil_shim_and_io_layers(tmp_path, monkeypatch):
    from barcode_amd.shim import ShimHamil
    monkeypatch.chdir(tmp_path)
    n = 9
    c = Case(Nx=n, likelihood=1)
    e = c.engine()
    e.chain_set_state(c.q0)

    class View:  # what hamil.py's functions read of a HamilData
        engine = e
    kf = 2.0 * np.pi / c.p.L
    got = hamil.measure_bispectrum(View, c.truth, k_min=1.0, dk=0.5, n_shell=4, units="kf")
    assert set(got) == {"b", "ntri", "q", "kmean", "nmode", "power", "triplets"}
    assert got["triplets"].dtype == np.int32 and got["triplets"].shape == (20, 3)
    assert same_bits(got, e.bispectrum(c.truth, k_min=kf, dk=0.5 * kf, n_shell=4))
    assert same_bits(hamil.measure_bispectrum(View, k_min=1.0, dk=0.5, n_shell=4, units="kf"),
                     e.bispectrum(source="chain", k_min=1.0, dk=0.5, n_shell=4, units="kf"))
    path = io.dump_bispec(got, "", "deltaLAG")
    assert path == "deltaLAG_bispec.txt"
    back = io.read_bispec(path)
    assert np.array_equal(back["triplets"], got["triplets"]) and np.array_equal(back["kmean"], got["kmean"][got["triplets"]])
    for k in ("b", "ntri", "q"):
        assert np.array_equal(back[k], got[k])
    hd = ShimHamil(c.p, **c.arrays())
    b, ntri, q, km, nm, pw = hd.measure_bispectrum(c.truth, kf, 0.5 * kf, 4)
    for k, v in zip(KEYS, (b, ntri, q, km, nm, pw)):
        assert np.array_equal(v, got[k]), k
    hd.close()
    e.close()
