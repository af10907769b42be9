"""bchmc_density_particles on chosen catalogues: count / scan / fill / LDS scatter on the handle's tiles (n = 16, 8, 4) and the
direct kernel (n = 5, 9, and any grid whose origin is not 0), every masskernel, fp64 and fp32 handles, default and
deterministic ones.

Every cell is compared with the longdouble reference of tests/catalogue_reference.py under the bound of
tests/catalogue_bound.py (a cell the reference leaves empty must be exactly 0); each check prints its worst fraction of the
bound ("CAT mk.. <type> n=.. <set>: worst fraction of the bound ..").  The geometry has L = n, so d = 1 and every face is
exact in float32 and float64.  An fp32 handle converts the positions to float first: the catalogues are rounded to the
handle's type when they are built, so reference and engine see the same numbers.
"""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

from barcode_amd import engine as eng
from barcode_amd import inputs
from barcode_amd.engine import BchmcError, DensityOpts, DensityStats, Engine
from barcode_amd.params import HamilParams
from tests import catalogue_bound as cb
from tests import catalogue_reference as cr
from tests import pm_bound
from tests.util import Case

pytestmark = pytest.mark.gpu

LD = np.longdouble
DTYPE = {0: np.float64, 1: np.float32}
ZERO = (0.0, 0.0, 0.0)
MINS = (-1.5, 0.25, 3.0)      # NGP / CIC / TSC away from the origin (SPH refuses a negative min)
MINS_POS = (2.5, 0.25, 5.0)   # SPH away from the origin
KERNELS = ((0, None), (1, None), (2, None), (3, 1.0), (3, 1.3))  # (mk, h / d): SPH at h = d and at h = 1.3 d
ARG, UNSUPPORTED, STATE = 1, 5, 9

_ENGINES = {}


def engine_of(n, precision=0, deterministic=0, mins=ZERO, mk=3, rsd=0):
    """One handle per configuration for the whole module (the masskernel is an option of the call, not of the handle)."""
    key = (n, precision, deterministic, mins, mk, rsd)
    if key not in _ENGINES:
        p = HamilParams(Nx=n, L=float(n), mk=mk, calc_h=2 if mk == 3 else 1, rsd_model=rsd, min1=mins[0], min2=mins[1],
                        min3=mins[2])
        _ENGINES[key] = Engine(p, precision=precision, deterministic=deterministic)
    return _ENGINES[key]


def close_all():
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    close_all()


@functools.lru_cache(maxsize=None)
def catalogue(n, mins, precision, name, blob=60000):
    geo = cr.Geometry(n, float(n), mins)
    pos, w = cr.catalogue_sets(geo, DTYPE[precision], names=(name,), blob=blob)[name]
    for a in pos + ([] if w is None else [w]):
        a.setflags(write=False)
    return geo, pos, w


@functools.lru_cache(maxsize=None)
def reference(n, mins, precision, name, mk, h_rel, blob=60000):
    """The longdouble sums of one (catalogue, kernel), computed once and shared by the default and the deterministic case."""
    geo, pos, w = catalogue(n, mins, precision, name, blob)
    slack = cb.q_slack(DTYPE[precision], n, 1.0 / h_rel) if mk == 3 else 0.0
    return cr.density(mk, pos, w, geo, None if mk != 3 else h_rel * geo.d, slack)


def check(e, n, mins, precision, det, name, mk, h_rel, shuffle=None, blob=60000):
    """One call against the reference under the bound: every cell, the empty ones exactly 0, n_in / n_lost."""
    geo, pos, w = catalogue(n, mins, precision, name, blob)
    ref = reference(n, mins, precision, name, mk, h_rel, blob)
    if shuffle is not None:
        pos = [c[shuffle] for c in pos]
        w = None if w is None else w[shuffle]
    dtype = DTYPE[precision]
    d_h, w_norm = (1.0 / h_rel, 1.0 / np.pi / (h_rel * geo.d) ** 3) if mk == 3 else (1.0, 1.0)
    max_w = 1.0 if w is None else float(np.max(np.abs(w)))
    call = functools.partial(e.density_particles, pos[0], pos[1], pos[2], w, mk=mk,
                             kernel_h=0.0 if mk != 3 else h_rel * geo.d)
    if det:
        # the fixed point holds 2^16 maximal contributions (max|w| times the kernel's largest value) per cell; the
        # reference's absolute sums decide which side a catalogue is on, and none of the suite's is near the line
        load = float(ref.A.max()) / (max_w * w_norm) / 2.0 ** 16
        assert load < 1 / 1.5 or load > 1.5, load
        if load > 1:
            with pytest.raises(BchmcError) as err:
                call()
            assert err.value.code == STATE
            print("CAT mk%d <%s det> n=%d %s: %.3g x the fixed point's head-room, refused" % (mk, np.dtype(dtype).name, n,
                                                                                              name, load))
            return None, None
    rho, st = call()
    bound = cb.density_bound(ref, mk, dtype, n, d_h, w_norm, max_w, bool(det))
    f, i = cb.worst_fraction(rho, ref.S, bound)
    print("CAT mk%d%s <%s%s> n=%d mins=%s %s: worst fraction of the bound %.3f (cell %d, cnt %d, rho %.17g, reference %.17g), "
          "n_in %d, max_per_tile %d" % (mk, "" if mk != 3 else " h=%.1fd" % h_rel, np.dtype(dtype).name, " det" if det else "",
                                        n, mins, name, f, i, ref.cnt[i], rho[i], float(ref.S[i]), st["n_in"],
                                        st["max_per_tile"]))
    assert f <= 1
    assert not np.any(rho[ref.cnt == 0])
    assert st["n_in"] == ref.n_in and st["n_lost"] == len(pos[0]) - ref.n_in
    return rho, st


# ---- the error bound ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("det", (0, 1), ids=("default", "deterministic"))
@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("name", cr.SETS)
def test_every_cell_within_the_bound_on_tiles(name, precision, det):
    """n = 16: tiles of 8 x 8 x 16, four of them; the blob cuts its tiles into dozens of work items."""
    e = engine_of(16, precision, det)
    assert e.tile_info()["tiled"]
    for mk, h_rel in KERNELS:
        rho, st = check(e, 16, ZERO, precision, det, name, mk, h_rel)
        if rho is None:  # upstream's TSC weights of the particle at x == min + L: beyond a deterministic handle's range
            assert det and name == "faces" and mk == 2
            continue
        if name == "blob":
            assert st["max_per_tile"] > 40 * 256  # many times the 256 records of a work item: the tile was split
        if name == "faces":  # TSC keeps x == min + L, the others lose it
            assert st["n_lost"] > 0


def test_max_per_tile_is_the_largest_tile_population():
    e = engine_of(16)
    geo, pos, w = catalogue(16, ZERO, 0, "blob")
    c = [np.floor(x).astype(np.int64) % 16 for x in pos]
    tile = (c[0] // 8) * 2 + c[1] // 8  # tiles of 8 x 8 x 16: one along z
    rho, st = e.density_particles(pos[0], pos[1], pos[2], mk=0)
    assert st["max_per_tile"] == np.bincount(tile).max() and st["n_in"] == 60000


@pytest.mark.parametrize("n,precision,det", [(8, 0, 0), (8, 1, 1), (4, 0, 1), (4, 1, 0), (5, 0, 0), (5, 1, 1), (9, 0, 1),
                                             (9, 1, 0)])
def test_small_and_odd_grids(n, precision, det):
    """n = 8: tiles of 8^3 (the SPH image folds onto the grid); n = 4: one tile of 4^3; n = 5, 9: no tiles, the direct
    kernel."""
    e = engine_of(n, precision, det)
    assert bool(e.tile_info()["tiled"]) == (n in (4, 8))
    for name in ("uniform", "sparse", "faces", "corners", "weights"):
        for mk, h_rel in ((0, None), (1, None), (2, None), (3, 1.0)) + (((3, 1.3),) if n > 5 else ()):
            rho, st = check(e, n, ZERO, precision, det, name, mk, h_rel)
            if rho is None:
                assert det and name == "faces" and mk == 2
                continue
            assert (st["max_per_tile"] > 0) == (n in (4, 8) and st["n_in"] > 0)


@pytest.mark.parametrize("det", (0, 1), ids=("default", "deterministic"))
@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_grid_origin_away_from_zero(precision, det):
    """min != 0: the direct kernel.  NGP, CIC and TSC with a negative and two positive components; SPH (which does not
    subtract min from its cell index) with positive ones, and refused with a negative one."""
    e = engine_of(16, precision, det, MINS, mk=1)
    for name in ("uniform", "faces", "corners", "weights"):
        for mk in (0, 1, 2):
            rho, st = check(e, 16, MINS, precision, det, name, mk, None)
            if rho is None:
                assert det and name == "faces" and mk == 2
                continue
            assert st["max_per_tile"] == 0
    geo, pos, w = catalogue(16, MINS, precision, "sparse")
    with pytest.raises(BchmcError) as err:
        e.density_particles(pos[0], pos[1], pos[2], mk=3, kernel_h=1.0)
    assert err.value.code == UNSUPPORTED
    check(e, 16, MINS, precision, det, "sparse", 1, None)  # the handle is as usable as before
    e2 = engine_of(16, precision, det, MINS_POS)
    for name in ("uniform", "faces", "weights"):
        for h_rel in (1.0, 1.3):
            check(e2, 16, MINS_POS, precision, det, name, 3, h_rel)


# ---- more than one batch ------------------------------------------------------------------------------------------------

BATCH = 2 ** 20  # kCatBatch (barcode_amd/csrc/catalogue.hpp): particles staged per pass


@functools.lru_cache(maxsize=None)
def long_catalogue():
    """2^20 + 37 particles at n = 16: a full batch and a short one.  Uniform in a box a little larger than the domain, so
    both batches lose particles; the 37 of the second batch sit in two cells of which the first batch fills one."""
    n = 16
    rng = np.random.Generator(np.random.Philox(31))
    pos = rng.random((3, BATCH + 37)) * (n + 0.5) - 0.25
    pos[:, BATCH:] = np.array([3.25, 9.5, 15.75])[:, None] + 0.2 * rng.random((3, 37))
    pos[0, BATCH + 30:] = -0.125  # seven of the last batch are lost
    pos = [np.ascontiguousarray(c) for c in pos]
    geo = cr.Geometry(n, float(n))
    refs = {mk: cr.density(mk, pos, None, geo) for mk in (0, 1)}
    for a in pos:
        a.setflags(write=False)
    return geo, pos, refs


@pytest.mark.parametrize("det", (0, 1), ids=("default", "deterministic"))
def test_a_catalogue_longer_than_a_batch(det):
    """The batch loop beyond its first pass: the counts, cursors and work items start afresh, the field accumulates across
    the batches, n_in is their sum and max_per_tile their largest, the columns are read at the batch's offset and the
    last batch is short.  NGP and CIC against the reference; on the deterministic handle bitwise equal to the same
    catalogue shuffled across the batch boundary."""
    geo, pos, refs = long_catalogue()
    n_part = BATCH + 37
    e = engine_of(16, 0, det)
    perm = np.random.Generator(np.random.Philox(32)).permutation(n_part)
    for mk in (0, 1):
        ref = refs[mk]
        rho, st = e.density_particles(pos[0], pos[1], pos[2], mk=mk)
        bound = cb.density_bound(ref, mk, np.float64, 16, deterministic=bool(det))
        f, i = cb.worst_fraction(rho, ref.S, bound)
        print("CAT two batches mk%d%s: worst fraction of the bound %.3f, n_in %d of %d, max_per_tile %d" %
              (mk, " det" if det else "", f, st["n_in"], n_part, st["max_per_tile"]))
        assert f <= 1 and not np.any(rho[ref.cnt == 0])
        assert st["n_in"] == ref.n_in and st["n_lost"] == n_part - ref.n_in and 0 < st["n_lost"] < n_part // 8
        if mk == 0:
            assert np.array_equal(rho, ref.S.astype(np.float64))
            c = [np.floor(x[:BATCH]).astype(np.int64) for x in pos]
            ok = np.ones(BATCH, dtype=bool)
            for ci in c:
                ok &= (ci >= 0) & (ci < 16)
            first = np.bincount((c[0][ok] // 8) * 2 + c[1][ok] // 8).max()  # the first batch holds the largest tile
            assert st["max_per_tile"] == first
        rho2, st2 = e.density_particles(pos[0][perm], pos[1][perm], pos[2][perm], mk=mk)
        assert st2["n_in"] == st["n_in"]
        if det:
            assert np.array_equal(rho2, rho)
        else:
            assert cb.worst_fraction(rho2, ref.S, bound)[0] <= 1


def test_own_particles_of_a_grid_larger_than_a_batch():
    """BCHMC_PART_FORWARD at 128^3: two batches of the handle's 2^21 particles, the second from lattice index 2^20 on.
    Bitwise the field of the fetched positions as a host catalogue (deterministic handle), and every particle kept."""
    n = 128
    p = HamilParams(Nx=n, L=float(n), mk=1, calc_h=1)
    e = Engine(p, deterministic=1)
    rng = np.random.Generator(np.random.Philox(33))
    e.forward(0.3 * rng.standard_normal(p.N), 0)
    pos = [e.fetch(k) for k in ("posx", "posy", "posz")]
    fwd, st = e.density_particles(source="forward")
    host, st_h = e.density_particles(pos[0], pos[1], pos[2])
    assert st["n_in"] == st_h["n_in"] == p.N == 2 * BATCH and st["n_lost"] == 0 and st == st_h
    assert np.array_equal(fwd, host) and abs(fwd.sum() - p.N) < 1e-6 * p.N
    rho = e.fetch("rho")  # the handle's own CIC of the same particles
    assert np.max(np.abs(fwd - rho)) <= 1e-12 * np.max(rho)
    nobs_only, st_n = e.density_particles(source="forward", to_nobs=True, download=False)
    assert nobs_only is None and st_n == st and np.array_equal(e.fetch("nobs"), fwd)
    e.close()


# ---- fixed-point head-room ----------------------------------------------------------------------------------------------

def test_saturation_is_reported_by_the_call():
    """A deterministic handle holds 2^16 maximal contributions per cell.  NGP with unit weights adds exactly one maximal
    contribution per particle, so the reference's count decides: a blob that puts clearly more than 2^16 particles into
    one cell returns BCHMC_ERR_STATE from this very call and writes nothing; 20 000 particles succeed, and so do the
    same 200 000 on a default handle."""
    n = 16
    geo = cr.Geometry(n, float(n))
    rng = np.random.Generator(np.random.Philox(99))

    def blob(count):
        t = np.array([5.5, 9.5, 3.5])[:, None] + 0.3 * rng.standard_normal((3, count))
        return [np.mod(c, float(n)) for c in t]

    big, small = blob(200000), blob(20000)
    rb, rs = cr.ngp(big, None, geo), cr.ngp(small, None, geo)
    assert rb.cnt.max() > 1.5 * 2 ** 16 and rs.cnt.max() < 2 ** 16 / 1.5
    e = engine_of(n, 0, 1)
    good, _ = e.density_particles(*small, mk=0)
    assert np.array_equal(good, rs.S.astype(np.float64))
    opts, st = DensityOpts(0, 0, 0.0, -1, 0), DensityStats()
    out = np.full(geo.N, -7.0)
    dp = C.POINTER(C.c_double)
    cols = [np.ascontiguousarray(c) for c in big]
    rc = e.lib.bchmc_density_particles(e.h, 0, *[c.ctypes.data_as(dp) for c in cols], None, 200000, C.byref(opts),
                                       out.ctypes.data_as(dp), C.byref(st))
    assert rc == STATE and np.all(out == -7.0)
    again, _ = e.density_particles(*small, mk=0)
    assert np.array_equal(again, good)
    rho, st = engine_of(n, 0, 0).density_particles(*big, mk=0)  # float atomics have no such limit
    assert np.array_equal(rho, rb.S.astype(np.float64)) and st["max_per_tile"] >= rb.cnt.max()


# ---- the handle's own particles -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,det", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=("fp64", "fp64-det", "fp32", "fp32-det"))
@pytest.mark.parametrize("rsd", (0, 1), ids=("real", "rsd"))
@pytest.mark.parametrize("mk", (3, 1), ids=("sph", "cic"))
def test_own_particles_as_a_catalogue(mk, rsd, precision, det):
    """After bchmc_forward: the fetched positions as a host catalogue with the handle's mk give BCHMC_F_RHO within the sum
    of both kernels' bounds; BCHMC_PART_FORWARD gives the host catalogue's field within the bound, bitwise on
    deterministic handles.  On the SPH handle BCHMC_PART_FORWARD with mk = 1 is LAG2EULer's CIC density."""
    n = 16
    e = engine_of(n, precision, det, ZERO, mk, rsd)
    dtype = DTYPE[precision]
    geo = cr.Geometry(n, float(n))
    q = 0.5 * np.asarray(inputs.make_fields(HamilParams(Nx=n, L=float(n)))["truth"])
    e.forward(q, rsd)
    pos = [e.fetch(k) for k in ("posx", "posy", "posz")]
    rho_h = e.fetch("rho")
    h_rel = 1.0
    slack = cb.q_slack(dtype, n, 1.0) if mk == 3 else 0.0
    ref = cr.density(mk, pos, None, geo, geo.d * h_rel, slack)
    w_norm = 1.0 / np.pi if mk == 3 else 1.0
    b_cat = cb.density_bound(ref, mk, dtype, n, 1.0, w_norm, 1.0, bool(det))
    b_own = pm_bound.density_bound(ref.S, ref.cnt, dtype, n, 1.0, w_norm, bool(det), kind=cb.kind_of(mk))
    host, st = e.density_particles(pos[0], pos[1], pos[2], mk=None)
    assert st["n_in"] == ref.n_in
    f_ref, _ = cb.worst_fraction(host, ref.S, b_cat)
    f_own, _ = cb.worst_fraction(host, rho_h, b_cat + b_own)
    fwd, st2 = e.density_particles(source="forward")
    f_fwd, _ = cb.worst_fraction(fwd, ref.S, b_cat)
    print("CAT own particles mk%d rsd%d <%s%s>: host catalogue %.3f of its bound, against BCHMC_F_RHO %.3f of both, "
          "BCHMC_PART_FORWARD %.3f" % (mk, rsd, np.dtype(dtype).name, " det" if det else "", f_ref, f_own, f_fwd))
    assert f_ref <= 1 and f_own <= 1 and f_fwd <= 1 and st2 == st
    if det:
        assert np.array_equal(fwd, host)
    assert np.array_equal(e.fetch("rho"), rho_h) and all(np.array_equal(e.fetch(k), c) for k, c in zip(("posx", "posy", "posz"), pos))
    if mk == 3:  # LAG2EULer: CIC of the SPH handle's particles
        lag, _ = e.density_particles(source="forward", mk=1)
        rc = cr.cic(pos, None, geo)
        f, _ = cb.worst_fraction(lag, rc.S, cb.density_bound(rc, 1, dtype, n, deterministic=bool(det)))
        print("CAT LAG2EULer rsd%d <%s%s>: %.3f of the bound" % (rsd, np.dtype(dtype).name, " det" if det else "", f))
        assert f <= 1


def test_forward_source_needs_a_forward_model():
    e = Engine(HamilParams(Nx=8, L=8.0))
    with pytest.raises(BchmcError) as err:
        e.density_particles(source="forward")
    assert err.value.code == STATE
    rho, st = e.density_particles(np.array([0.5]), np.array([0.5]), np.array([0.5]), mk=0)
    assert rho[0] == 1 and rho.sum() == 1 and st == dict(n_in=1, n_lost=0, max_per_tile=1)
    e.close()


# ---- nobs, and what a call leaves alone ---------------------------------------------------------------------------------

def test_nobs_from_a_catalogue_is_an_uploaded_nobs():
    """dest = BCHMC_F_NOBS: the next energies are those of a twin that uploaded the same field from the host, bitwise on
    deterministic handles (and the field can be fetched back)."""
    c = Case(Nx=16, likelihood=1)
    geo = cr.Geometry(16, c.p.L)
    rng = np.random.Generator(np.random.Philox(5))
    pos = rng.random((3, 3 * c.p.N)) * c.p.L
    arrays = c.arrays()
    e = Engine(c.p, deterministic=1)
    e.upload(**{k: v for k, v in arrays.items() if k != "nobs"})
    with pytest.raises(BchmcError):
        e.energies(c.q0, c.p0)  # nobs was never uploaded
    rho, _ = e.density_particles(pos[0], pos[1], pos[2], mk=1, to_nobs=True)
    assert abs(rho.sum() - 3 * c.p.N) < 1e-6 and np.array_equal(e.fetch("nobs"), rho)
    got = e.energies(c.q0, c.p0)
    twin = Engine(c.p, deterministic=1)
    twin.upload(**dict(arrays, nobs=rho))
    want = twin.energies(c.q0, c.p0)
    assert np.array_equal(got, want)
    e.close()
    twin.close()


def test_a_call_leaves_the_state_alone():
    """dest = -1, with a proposal pending: the chain state, the momenta, the proposal, deltaX, rho and the positions are bit
    for bit what they were, and the next attempt returns the dH of a twin that never called."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)
    rng = np.random.Generator(np.random.Philox(6))
    pos = rng.random((3, 5000)) * c.p.L
    w = rng.standard_normal(5000)

    def run(call):
        e = Engine(c.p, deterministic=1)
        e.upload(**c.arrays())
        e.chain_set_state(c.q0)
        e.chain_set_momenta(c.p0)
        e.chain_attempt(c.eps, 3)
        keys = ("deltaX", "rho", "posx", "posy", "posz", "psix")
        before = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + tuple(e.fetch(k) for k in keys)
        info = e.tile_info()
        if call:
            for mk in (0, 1, 2, 3):
                e.density_particles(pos[0], pos[1], pos[2], w, mk=mk)
            e.density_particles(source="forward")
            e.catalogue_release()
        after = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + tuple(e.fetch(k) for k in keys)
        assert all(np.array_equal(a, b) for a, b in zip(before, after)) and e.tile_info() == info
        en = e.energies(c.q0, c.p0)
        e.chain_set_state(c.q0)
        e.chain_set_momenta(0.9 * c.p0)
        dH, terms, done = e.chain_attempt(c.eps, 3)
        e.close()
        return en, dH, terms, done

    plain, called = run(False), run(True)
    assert np.array_equal(plain[0], called[0]) and plain[1] == called[1] and np.array_equal(plain[2], called[2])
    assert plain[3] == called[3] == 3


# ---- repeatability ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_deterministic_results_are_bitwise_repeatable(precision):
    """Across two calls, across bchmc_catalogue_release, across a second handle and under a shuffled catalogue; a default
    handle stays within the bound under the shuffle."""
    e = engine_of(16, precision, 1)
    other = Engine(HamilParams(Nx=16, L=16.0, mk=1, calc_h=1), precision=precision, deterministic=1)
    for name in ("weights", "blob"):
        geo, pos, w = catalogue(16, ZERO, precision, name)
        perm = np.random.Generator(np.random.Philox(8)).permutation(len(pos[0]))
        for mk, h_rel in KERNELS:
            first, _ = check(e, 16, ZERO, precision, 1, name, mk, h_rel)
            second, _ = check(e, 16, ZERO, precision, 1, name, mk, h_rel)
            e.catalogue_release()
            third, _ = check(e, 16, ZERO, precision, 1, name, mk, h_rel)
            shuffled, _ = check(e, 16, ZERO, precision, 1, name, mk, h_rel, shuffle=perm)
            elsewhere, _ = other.density_particles(pos[0], pos[1], pos[2], w, mk=mk, kernel_h=h_rel or 0.0)
            for a in (second, third, shuffled, elsewhere):
                assert np.array_equal(first, a), (name, mk, h_rel)
            check(engine_of(16, precision, 0), 16, ZERO, precision, 0, name, mk, h_rel, shuffle=perm)
    other.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_leave_a_usable_handle():
    n = 16
    e = engine_of(n, 0, 1)
    geo, pos, w = catalogue(n, ZERO, 0, "weights")
    want, _ = e.density_particles(pos[0], pos[1], pos[2], w, mk=1)
    dp = C.POINTER(C.c_double)
    x, y, z = (np.ascontiguousarray(c).ctypes.data_as(dp) for c in pos)
    wp = np.ascontiguousarray(w).ctypes.data_as(dp)
    bad_w = np.array(w)
    bad_w[len(bad_w) // 2] = np.inf
    nan_w = np.array(w)
    nan_w[-1] = np.nan
    out = np.full(geo.N, -7.0)
    o = out.ctypes.data_as(dp)
    m = len(pos[0])
    fn = e.lib.bchmc_density_particles

    def opts(mk=1, weightmass=1, kernel_h=0.0, dest=-1):
        return C.byref(DensityOpts(mk, weightmass, kernel_h, dest, 0))

    fresh = Engine(HamilParams(Nx=n, L=float(n)), deterministic=1)  # no forward model has run on this one
    refused = (
        (ARG, (e.h, 0, None, y, z, wp, m, opts(), o, None)),                 # a NULL position column
        (ARG, (e.h, 0, x, None, z, wp, m, opts(), o, None)),
        (ARG, (e.h, 0, x, y, None, wp, m, opts(), o, None)),
        (ARG, (e.h, 0, x, y, z, None, m, opts(), o, None)),                  # weightmass = 1 without w
        (ARG, (e.h, 0, x, y, z, wp, m, opts(mk=-2), o, None)),               # mk outside -1..3
        (ARG, (e.h, 0, x, y, z, wp, m, opts(mk=4), o, None)),
        (ARG, (e.h, 0, x, y, z, wp, m, opts(mk=3, kernel_h=-1.0), o, None)),  # kernel_h negative, not finite, above L / 4
        (ARG, (e.h, 0, x, y, z, wp, m, opts(mk=3, kernel_h=np.nan), o, None)),
        (ARG, (e.h, 0, x, y, z, wp, m, opts(mk=3, kernel_h=np.inf), o, None)),
        (ARG, (e.h, 0, x, y, z, wp, m, opts(mk=3, kernel_h=n / 4 + 0.01), o, None)),
        (ARG, (e.h, 0, x, y, z, wp, m, opts(dest=0), o, None)),              # dest neither -1 nor BCHMC_F_NOBS
        (ARG, (e.h, 0, x, y, z, wp, m, opts(dest=4), o, None)),
        (ARG, (e.h, 0, x, y, z, wp, m, opts(), None, None)),                 # nowhere to put the field
        (ARG, (e.h, 0, x, y, z, wp, 2 ** 31, opts(), o, None)),              # n_part > 2^31 - 1
        (ARG, (e.h, 2, x, y, z, wp, m, opts(), o, None)),                    # an unknown source
        (ARG, (e.h, 1, x, y, z, None, m, opts(weightmass=0), o, None)),      # columns given with BCHMC_PART_FORWARD
        (ARG, (e.h, 0, x, y, z, bad_w.ctypes.data_as(dp), m, opts(), o, None)),   # a non-finite weight
        (ARG, (e.h, 0, x, y, z, nan_w.ctypes.data_as(dp), m, opts(), o, None)),
        (STATE, (fresh.h, 1, None, None, None, None, 0, opts(weightmass=0), o, None)),  # no forward model has run
        (ARG, (None, 0, x, y, z, wp, m, opts(), o, None)),                   # a null handle
        (ARG, (e.h, 0, x, y, z, wp, m, None, o, None)),                      # no options
    )
    for code, args in refused:
        assert fn(*args) == code, args[1:]
        assert np.all(out == -7.0)
        got, _ = e.density_particles(pos[0], pos[1], pos[2], w, mk=1)
        assert np.array_equal(got, want)
    fresh.close()
    zero, st = e.density_particles(np.empty(0), np.empty(0), np.empty(0), mk=3)  # n_part = 0: a zero field
    assert not zero.any() and st == dict(n_in=0, n_lost=0, max_per_tile=0)
    zero, st = e.density_particles(None, None, None, mk=2)
    assert not zero.any() and st["n_in"] == 0


# ---- resources ----------------------------------------------------------------------------------------------------------

def test_catalogue_buffers_are_counted_and_released():
    close_all()
    gc.collect()  # an engine some earlier test dropped without close() goes now, not between two readings
    start = eng.live_resources()  # (0, 0, 0, 0) unless another module of this process keeps a handle
    geo, pos, w = catalogue(16, ZERO, 0, "sparse")
    e = Engine(HamilParams(Nx=16, L=16.0))
    base = eng.live_resources()
    first, _ = e.density_particles(pos[0], pos[1], pos[2], mk=3)
    held = eng.live_resources()
    assert held[0] > base[0] and held[1] > base[1] and held[2] > base[2]
    second, _ = e.density_particles(pos[0], pos[1], pos[2], w, mk=1)
    assert eng.live_resources() == held
    e.catalogue_release()
    assert eng.live_resources() == base
    again, _ = e.density_particles(pos[0], pos[1], pos[2], mk=3)  # a later call rebuilds them
    assert eng.live_resources() == held and np.allclose(again, first, rtol=1e-13, atol=0)
    e.close()
    assert eng.live_resources() == start


# ---- the layers above ---------------------------------------------------------------------------------------------------

def test_shim_and_hamil_agree_with_the_c_abi(tmp_path):
    from barcode_amd import hamil, io, shim
    n = 16
    p = HamilParams(Nx=n, L=float(n))
    geo, pos, w = catalogue(n, ZERO, 0, "weights")
    e = engine_of(n, 0, 1)
    ones = np.ones(p.N)
    sh = shim.ShimHamil(p, signal_PS=ones, mass_f=ones)
    sh.hd.deterministic = 1
    hd = hamil.HamilData(p)
    for mk, h in ((0, 0.0), (1, 0.0), (2, 0.0), (3, 1.3)):
        want, _ = e.density_particles(pos[0], pos[1], pos[2], w, mk=mk, kernel_h=h)
        got = sh.getDensity(mk, pos[0], pos[1], pos[2], w, weightmass=True, kernel_h=h)
        assert np.array_equal(got, want), mk  # deterministic handles: bitwise across handles
        via, st = hamil.getDensity(hd, mk, pos[0], pos[1], pos[2], w, True, h)
        assert st["n_in"] == len(w) and np.allclose(via, want, rtol=0, atol=1e-9 * np.abs(want).max())
    unit, _ = e.density_particles(pos[0], pos[1], pos[2], mk=1)
    assert np.array_equal(sh.getDensity(1, pos[0], pos[1], pos[2], w, weightmass=False), unit)  # CIC ignores Par_mass then
    assert np.array_equal(sh.getDensity(0, pos[0], pos[1], pos[2]), e.density_particles(pos[0], pos[1], pos[2], mk=0)[0])
    with pytest.raises(shim.ShimError):
        sh.getDensity(3, pos[0], pos[1], pos[2], w, weightmass=True, kernel_h=0.0)  # upstream's SPH takes its own kernel_h
    path = io.dump_density(unit, str(tmp_path / "density"))
    assert np.array_equal(io.read_array(path, p.N), unit)
    sh.close()
    hd.engine.close()
