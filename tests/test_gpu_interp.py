"""bchmc_interp_particles on chosen catalogues: grid fields read at a free particle list by the tile kernel (count / scan /
fill / LDS gather on the handle's tiles) and by the direct kernel, CIC and TSC, one to four fields, fp64 and fp32 handles.

The criterion is bitwise equality with the numpy restatement of interpolate_CIC / interpolate_TSC / interpolate_TSC_multi
(tests/interp_restatement.py) applied to the same inputs -- for handle-resident sources, to what bchmc_chain_get_state /
bchmc_fetch return from the same handle at that moment.  There is no tolerance: nothing is accumulated across particles
and contraction is off on both sides.  A lost particle (TSC outside its domain, a non-finite coordinate) is NaN in every
field and counted in n_lost.  The one inequality is the adjointness with bchmc_density_particles, whose bound is the
rounding of the two orders of the same sum of products.
"""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

from barcode_amd import engine as eng
from barcode_amd.engine import BchmcError, Engine, InterpField, InterpOpts, InterpStats
from barcode_amd.params import HamilParams
from tests import interp_restatement as ir
from tests.util import Case

pytestmark = pytest.mark.gpu

DTYPE = {0: np.float64, 1: np.float32}
ARG, UNSUPPORTED, STATE = 1, 5, 9
BATCH = 1 << 20
# d = L / n is inexact in double for n = 5, 9 and 32 here
GRIDS = ((4, 4.0), (5, 3.0), (8, 8.0), (9, 1.0), (16, 50.0), (32, 1.1))

_ENGINES = {}


def engine_of(n, L, precision=0, deterministic=0):
    key = (n, L, precision, deterministic)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(HamilParams(Nx=n, L=L), precision=precision, deterministic=deterministic)
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
def grids_of(n, count=4, seed=11):
    rng = np.random.Generator(np.random.Philox(seed + n))
    f = rng.standard_normal((count, n ** 3))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def edge_catalogue(n, L):
    pos = ir.edge_set(n, L, seed=n, n_uniform=5000)
    for a in pos:
        a.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def edge_reference(n, L, kernel, precision, K):
    pos = edge_catalogue(n, L)
    return ir.interpolate(kernel, n, L, pos[0], pos[1], pos[2], grids_of(n)[:K], DTYPE[precision])


def same_bits(got, want):
    return np.array_equal(ir.bits(got), ir.bits(want))


def paths_of(e):
    return (0, 1) if e.tile_info()["tiled"] else (0,)


# ---- the edge set -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", (1, 3, 4))
@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("kernel", (ir.CIC, ir.TSC), ids=("cic", "tsc"))
@pytest.mark.parametrize("n,L", GRIDS)
def test_edge_positions_and_uniform_particles_are_the_restatement_bitwise(n, L, kernel, precision, K):
    e = engine_of(n, L, precision)
    pos = edge_catalogue(n, L)
    want, lost = edge_reference(n, L, kernel, precision, K)
    assert 0 < lost.sum() < lost.size  # NaN and infinities are lost under either kernel, the uniform ones never
    if n in (4, 8, 16, 32):
        assert 1 in paths_of(e)
    results = []
    for path in paths_of(e):
        got, st = e.interp_particles(pos[0], pos[1], pos[2], grids_of(n)[:K], kernel=kernel, path=path)
        bad = np.flatnonzero(np.any(ir.bits(got) != ir.bits(want), axis=0))
        print("ITP %s <%s> n=%d L=%g K=%d path %d: %d particles, %d lost, %d differ%s" % (
            "cic" if kernel == ir.CIC else "tsc", np.dtype(DTYPE[precision]).name, n, L, K, path, lost.size, lost.sum(),
            bad.size, "" if not bad.size else " (first %d at %r: %r, restatement %r)" % (
                bad[0], tuple(float(c[bad[0]]) for c in pos), got[:, bad[0]], want[:, bad[0]])))
        assert not bad.size
        assert np.array_equal(np.isnan(got), np.broadcast_to(lost, got.shape))
        assert st["n_lost"] == lost.sum() and st["n_in"] == lost.size - lost.sum() and st["path_used"] == path
        results.append(got)
    if len(results) == 2:
        assert same_bits(results[0], results[1])


def test_the_upper_face_of_a_nine_cell_unit_box_is_lost_under_tsc():
    """n = 9, L = 1: the double below 1.0 divided by d gives 9 -- x < L is not the domain."""
    n, L = 9, 1.0
    e = engine_of(n, L)
    top = np.nextafter(1.0, 0.0)
    assert top < L and top / (L / n) == 9.0
    x = np.array([top, 0.5, 0.5, 0.5])
    y = np.array([0.5, top, 0.5, 0.5])
    z = np.array([0.5, 0.5, top, 0.5])
    got, st = e.interp_particles(x, y, z, grids_of(n)[:1], kernel="tsc", path=0)
    assert np.array_equal(np.isnan(got[0]), [True, True, True, False]) and st["n_lost"] == 3
    cic, st = e.interp_particles(x, y, z, grids_of(n)[:1], kernel="cic", path=0)
    assert st["n_lost"] == 0 and same_bits(cic, ir.interpolate(ir.CIC, n, L, x, y, z, grids_of(n)[:1])[0])


# ---- crowded tiles, long catalogues -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", (ir.CIC, ir.TSC), ids=("cic", "tsc"))
def test_a_crowded_cell_is_cut_into_many_work_items(kernel):
    n, L, m = 16, 50.0, 50000
    e = engine_of(n, L)
    d = L / n
    rng = np.random.Generator(np.random.Philox(3))
    pos = (3 + rng.random((3, m))) * d  # cell (3, 3, 3): cell_index1 of CIC is 2 or 3, inside tile 0 either way
    want, lost = ir.interpolate(kernel, n, L, pos[0], pos[1], pos[2], grids_of(n)[:2])
    got, st = e.interp_particles(pos[0], pos[1], pos[2], grids_of(n)[:2], kernel=kernel, path=1)
    assert not lost.any() and st["n_in"] == m and st["max_per_tile"] == m and st["path_used"] == 1
    assert same_bits(got, want)
    direct, st0 = e.interp_particles(pos[0], pos[1], pos[2], grids_of(n)[:2], kernel=kernel, path=0)
    assert st0["max_per_tile"] == 0 and same_bits(direct, want)


@functools.lru_cache(maxsize=None)
def long_catalogue():
    rng = np.random.Generator(np.random.Philox(8))
    pos = rng.random((3, BATCH + 37)) * 50.0
    pos.setflags(write=False)
    return pos


@pytest.mark.parametrize("kernel", (ir.CIC, ir.TSC), ids=("cic", "tsc"))
def test_a_catalogue_longer_than_a_batch(kernel):
    n, L = 16, 50.0
    e = engine_of(n, L)
    pos = long_catalogue()
    want, lost = ir.interpolate(kernel, n, L, pos[0], pos[1], pos[2], grids_of(n)[:2])
    for path in (1, 0):
        got, st = e.interp_particles(pos[0], pos[1], pos[2], grids_of(n)[:2], kernel=kernel, path=path)
        assert st["n_in"] == BATCH + 37 - lost.sum() and st["n_lost"] == lost.sum()
        assert same_bits(got, want), path


def test_own_particles_of_a_grid_larger_than_a_batch():
    """BCHMC_PART_FORWARD at 128^3: two batches of the handle's 2^21 particles, deltaX as the field, against the
    restatement at the fetched positions on the fetched deltaX."""
    n = 128
    p = HamilParams(Nx=n, L=float(n), mk=1, calc_h=1)
    e = Engine(p)
    rng = np.random.Generator(np.random.Philox(33))
    e.forward(0.3 * rng.standard_normal(p.N), 0)
    pos = [e.fetch(k) for k in ("posx", "posy", "posz")]
    dx = e.fetch("deltaX")
    want, lost = ir.interpolate(ir.CIC, n, p.L, pos[0], pos[1], pos[2], [dx])
    for path in (0, 1):
        got, st = e.interp_particles(fields=["deltax"], kernel="cic", source="forward", path=path)
        assert got.shape == (1, p.N) and p.N == 2 * BATCH and st["n_in"] == p.N and not lost.any()
        assert same_bits(got, want), path
    # TSC on the tile kernel; its domain test decides what is lost, whatever the positions' fold left at the upper face
    want, lost = ir.interpolate(ir.TSC, n, p.L, pos[0], pos[1], pos[2], [dx])
    got, st = e.interp_particles(fields=["deltax"], kernel="tsc", source="forward", path=1)
    assert st["n_lost"] == lost.sum() and st["n_in"] == p.N - lost.sum() and st["path_used"] == 1
    assert same_bits(got, want)
    e.close()


# ---- order ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("det", (0, 1), ids=("default", "deterministic"))
def test_a_permuted_catalogue_gives_the_permuted_output(det):
    n, L = 16, 50.0
    e = engine_of(n, L, 0, det)
    pos = edge_catalogue(n, L)
    perm = np.random.Generator(np.random.Philox(4)).permutation(pos[0].size)
    for kernel in (ir.CIC, ir.TSC):
        for path in (0, 1):
            a, _ = e.interp_particles(pos[0], pos[1], pos[2], grids_of(n)[:3], kernel=kernel, path=path)
            b, _ = e.interp_particles(pos[0][perm], pos[1][perm], pos[2][perm], grids_of(n)[:3], kernel=kernel, path=path)
            assert same_bits(a[:, perm], b), (kernel, path)
    want, _ = edge_reference(n, L, ir.TSC, 0, 3)
    assert same_bits(b, want[:, perm])  # deterministic or not: the same bits


# ---- sources -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_handle_resident_sources(precision):
    c = Case(Nx=16, likelihood=1)
    n, L = 16, c.p.L
    e = Engine(c.p, precision=precision)
    e.upload(**c.arrays())
    e.chain_set_state(c.q0)
    e.chain_forward()
    pos = ir.edge_set(n, L, seed=5, n_uniform=2000)
    dt = DTYPE[precision]
    host = {"chain": e.chain_get_state(), "deltax": e.fetch("deltaX"), "psix": e.fetch("psix"), "psiy": e.fetch("psiy"),
            "psiz": e.fetch("psiz"), "window": e.fetch("window"), "nobs": e.fetch("nobs")}
    for kernel in (ir.CIC, ir.TSC):
        for path in (0, 1):
            for name, arr in host.items():
                got, _ = e.interp_particles(pos[0], pos[1], pos[2], [name], kernel=kernel, path=path)
                want, _ = ir.interpolate(kernel, n, L, pos[0], pos[1], pos[2], [arr], dt)
                assert same_bits(got, want), (kernel, path, name)
            mix = [grids_of(n)[0], "psiz", "deltax", "chain"]
            got, _ = e.interp_particles(pos[0], pos[1], pos[2], mix, kernel=kernel, path=path)
            want, _ = ir.interpolate(kernel, n, L, pos[0], pos[1], pos[2],
                                     [grids_of(n)[0], host["psiz"], host["deltax"], host["chain"]], dt)
            assert same_bits(got, want), (kernel, path, "mix")
    e.close()


# ---- adjointness with bchmc_density_particles ---------------------------------------------------------------------------

@pytest.mark.parametrize("path", (0, 1))
def test_cic_gather_is_the_adjoint_of_the_cic_scatter(path):
    """sum_p w_p interp(F)(x_p) == sum_c F_c density_CIC(w)(c): the same products F_c w_p W_pc in two orders, so the
    bound is rounding alone -- (8 n_part + N) 2^-53 n_part max|w| max|F| -- whatever the order of the scatter's atomics;
    a wrong cell or sign shows at O(1)."""
    n, L, m = 16, 50.0, 20000
    e = engine_of(n, L)
    rng = np.random.Generator(np.random.Philox(12))
    pos = rng.random((3, m)) * L
    w = rng.standard_normal(m)
    F = grids_of(n)[0]
    vals, _ = e.interp_particles(pos[0], pos[1], pos[2], [F], kernel="cic", path=path)
    rho, _ = e.density_particles(pos[0], pos[1], pos[2], w, mk=1)
    lhs, rhs = float(np.dot(w, vals[0])), float(np.dot(F, rho))
    bound = (8 * m + n ** 3) * 2.0 ** -53 * m * np.max(np.abs(w)) * np.max(np.abs(F))
    print("ITP adjoint path %d: gather side %.17g, scatter side %.17g, difference %.3g, bound %.3g" % (
        path, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound and abs(lhs) > 1e3 * bound


# ---- what a call leaves alone ---------------------------------------------------------------------------------------------

def test_a_call_leaves_the_state_alone():
    c = Case(Nx=16, likelihood=1, rsd_model=1)
    rng = np.random.Generator(np.random.Philox(6))
    pos = rng.random((3, 5000)) * c.p.L

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
            for kernel in ("cic", "tsc"):
                for path in (0, 1):
                    e.interp_particles(pos[0], pos[1], pos[2], ["chain", "deltax", "psix", c.window], kernel=kernel, path=path)
            e.interp_particles(fields=["deltax", "Vx"], source="forward")
            e.interp_release()
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


def test_the_carried_gradient_survives_a_call():
    """Fast attempts carry the gradient and -log L of the chain state; a call between two attempts changes neither."""
    c = Case(Nx=16, likelihood=1)
    rng = np.random.Generator(np.random.Philox(7))
    pos = rng.random((3, 3000)) * c.p.L

    def run(call):
        e = Engine(c.p, deterministic=1)
        e.upload(**c.arrays())
        e.chain_set_state(c.q0)
        e.chain_set_momenta(c.p0)
        first = e.chain_attempt(c.eps, 3)
        e.chain_accept(1)
        if call:
            e.interp_particles(pos[0], pos[1], pos[2], ["chain", c.noise], kernel="tsc", path=1)
        e.chain_set_momenta(0.8 * c.p0)
        second = e.chain_attempt(c.eps, 3)
        e.close()
        return first[0], second[0], second[1]

    plain, called = run(False), run(True)
    assert plain[0] == called[0] and plain[1] == called[1] and np.array_equal(plain[2], called[2])


# ---- refusals ------------------------------------------------------------------------------------------------------------

def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def raw(e, psrc, x, y, z, n_part, fields, n_fields, opts, out):
    fd = None
    if fields is not None:
        fd = (InterpField * len(fields))(*[InterpField(s, f, _dp(h)) for s, f, h in fields])
    st = InterpStats()
    return e.lib.bchmc_interp_particles(e.h, psrc, _dp(x), _dp(y), _dp(z), n_part, fd, n_fields,
                                        None if opts is None else C.byref(InterpOpts(*opts)), _dp(out), C.byref(st))


def test_refusals_leave_a_usable_handle():
    n, L = 16, 50.0
    c = Case(Nx=n, L=L, likelihood=1)
    e = Engine(c.p)
    N = n ** 3
    x = np.linspace(0.1, L - 0.1, 7)
    F = np.ascontiguousarray(grids_of(n)[0])
    out = np.full(4 * N, -7.0)
    host = [(0, 0, F)]
    ok = (1, 0)
    HANDLE = eng.INTERP_HANDLE_FIELD
    base = eng.live_resources()
    cases = [
        ("opts NULL", ARG, (0, x, x, x, 7, host, 1, None, out)),
        ("kernel 0", ARG, (0, x, x, x, 7, host, 1, (0, 0), out)),
        ("kernel 3", ARG, (0, x, x, x, 7, host, 1, (3, 0), out)),
        ("path -2", ARG, (0, x, x, x, 7, host, 1, (1, -2), out)),
        ("path 2", ARG, (0, x, x, x, 7, host, 1, (1, 2), out)),
        ("n_fields 0", ARG, (0, x, x, x, 7, host, 0, ok, out)),
        ("n_fields 5", ARG, (0, x, x, x, 7, host * 5, 5, ok, out)),
        ("fields NULL", ARG, (0, x, x, x, 7, None, 1, ok, out)),
        ("host field without its array", ARG, (0, x, x, x, 7, [(0, 0, None)], 1, ok, out)),
        ("array with the chain source", ARG, (0, x, x, x, 7, [(1, 0, F)], 1, ok, out)),
        ("array with a handle field", ARG, (0, x, x, x, 7, [(HANDLE, 5, F)], 1, ok, out)),
        ("unknown source", ARG, (0, x, x, x, 7, [(4, 0, None)], 1, ok, out)),
        ("negative source", ARG, (0, x, x, x, 7, [(-1, 0, None)], 1, ok, out)),
        ("unknown bchmc_field", ARG, (0, x, x, x, 7, [(HANDLE, 20, None)], 1, ok, out)),
        ("negative bchmc_field", ARG, (0, x, x, x, 7, [(HANDLE, -1, None)], 1, ok, out)),
        ("out NULL", ARG, (0, x, x, x, 7, host, 1, ok, None)),
        ("x NULL", ARG, (0, None, x, x, 7, host, 1, ok, out)),
        ("y NULL", ARG, (0, x, None, x, 7, host, 1, ok, out)),
        ("z NULL", ARG, (0, x, x, None, 7, host, 1, ok, out)),
        ("unknown position source", ARG, (2, x, x, x, 7, host, 1, ok, out)),
        ("a column with PART_FORWARD", ARG, (1, x, None, None, N, host, 1, ok, out)),
        ("n_part != N with PART_FORWARD", ARG, (1, None, None, None, 7, host, 1, ok, out)),
        ("n_part > 2^31 - 1", ARG, (0, x, x, x, 2 ** 31, host, 1, ok, out)),
        ("no chain state", STATE, (0, x, x, x, 7, [(1, 0, None)], 1, ok, out)),
        ("no forward evaluation for deltaX", STATE, (0, x, x, x, 7, [(2, 0, None)], 1, ok, out)),
        ("no forward evaluation for psix", STATE, (0, x, x, x, 7, [(HANDLE, 15, None)], 1, ok, out)),
        ("no forward evaluation for PART_FORWARD", STATE, (1, None, None, None, N, host, 1, ok, out)),
        ("a never-uploaded window", STATE, (0, x, x, x, 7, [(HANDLE, 5, None)], 1, ok, out)),
    ]
    want, _ = ir.interpolate(ir.TSC, n, L, x, x, x, [F])
    for what, code, args in cases:
        assert raw(e, *args) == code, what
        assert e.lib.bchmc_last_error(e.h), what
        assert np.all(out == -7.0), what           # nothing written
        assert eng.live_resources() == base, what  # nothing built
    got, st = e.interp_particles(x, x, x, [F], kernel="tsc", path=1)
    assert same_bits(got, want) and st["n_in"] == 7
    # n_part = 0 succeeds and writes nothing, with or without columns
    assert raw(e, 0, None, None, None, 0, host, 1, ok, None) == 0
    assert raw(e, 0, x, x, x, 0, host, 1, ok, out) == 0 and np.all(out == -7.0)
    empty, st = e.interp_particles(np.zeros(0), np.zeros(0), np.zeros(0), [F])
    assert empty.shape == (1, 0) and st["n_in"] == st["n_lost"] == 0
    e.close()
    for n_odd, L_odd in ((5, 3.0), (9, 1.0)):  # no tile partition: path = 1 is refused, the others run
        eo = engine_of(n_odd, L_odd)
        assert not eo.tile_info()["tiled"]
        xo = np.array([0.25 * L_odd])
        Fo = np.ascontiguousarray(grids_of(n_odd)[0])
        assert raw(eo, 0, xo, xo, xo, 1, [(0, 0, Fo)], 1, (1, 1), out) == UNSUPPORTED
        with pytest.raises(BchmcError) as err:
            eo.interp_particles(xo, xo, xo, [Fo], path="tile")
        assert err.value.code == UNSUPPORTED
        for path in (None, 0):
            got, st = eo.interp_particles(xo, xo, xo, [Fo], path=path)
            assert st["path_used"] == 0 and same_bits(got, ir.interpolate(ir.CIC, n_odd, L_odd, xo, xo, xo, [Fo])[0])


def test_the_engine_decides_the_path():
    """path = -1 (interp_plan.hpp): TSC of three fields or more at 64 particles per tile of the first batch takes the tile
    kernel; CIC, fewer fields, fewer particles, the handle's own particles and a handle without tiles the direct one.
    Either way the bits are the same."""
    n, L = 16, 50.0
    e = engine_of(n, L)
    pos = edge_catalogue(n, L)
    F = grids_of(n)
    assert e.tile_info()["tile_shape"] == (8, 8, 16) and pos[0].size >= 64 * 4
    want, _ = edge_reference(n, L, ir.TSC, 0, 3)
    got, st = e.interp_particles(pos[0], pos[1], pos[2], F[:3], kernel="tsc")
    assert st["path_used"] == 1 and st["max_per_tile"] > 0 and same_bits(got, want)
    few = [c[:255] for c in pos]
    got, st = e.interp_particles(few[0], few[1], few[2], F[:3], kernel="tsc")
    assert st["path_used"] == 0 and st["max_per_tile"] == 0 and same_bits(got, want[:, :255])
    assert e.interp_particles(pos[0], pos[1], pos[2], F[:2], kernel="tsc")[1]["path_used"] == 0
    assert e.interp_particles(pos[0], pos[1], pos[2], F[:4], kernel="tsc")[1]["path_used"] == 1
    assert e.interp_particles(pos[0], pos[1], pos[2], F[:4], kernel="cic")[1]["path_used"] == 0
    e.forward(0.1 * F[0], 0)
    assert e.interp_particles(fields=F[:3], kernel="tsc", source="forward")[1]["path_used"] == 0


# ---- resources -----------------------------------------------------------------------------------------------------------

def test_interpolation_buffers_are_counted_and_released():
    close_all()
    gc.collect()
    start = eng.live_resources()
    n, L = 16, 50.0
    pos = edge_catalogue(n, L)
    e = Engine(HamilParams(Nx=n, L=L))
    base = eng.live_resources()
    first, _ = e.interp_particles(pos[0], pos[1], pos[2], grids_of(n)[:2], kernel="tsc", path=1)
    held = eng.live_resources()
    assert held[0] > base[0] and held[1] > base[1] and held[2] > base[2]
    e.interp_particles(pos[0], pos[1], pos[2], grids_of(n)[:1], kernel="cic", path=0)
    assert eng.live_resources() == held  # fewer fields, another kernel and path: nothing new
    e.interp_release()
    assert eng.live_resources() == base
    again, _ = e.interp_particles(pos[0], pos[1], pos[2], grids_of(n)[:2], kernel="tsc", path=1)
    assert eng.live_resources() == held and same_bits(again, first)
    # beside the catalogue's buffers: each release frees its own, in either order
    for order in (("catalogue_release", "interp_release"), ("interp_release", "catalogue_release")):
        e.interp_release()
        e.catalogue_release()
        assert eng.live_resources() == base
        e.density_particles(pos[0][-5000:], pos[1][-5000:], pos[2][-5000:], mk=1)
        cat_only = eng.live_resources()
        e.interp_particles(pos[0], pos[1], pos[2], grids_of(n)[:2], kernel="tsc", path=1)
        both = eng.live_resources()
        assert both[0] - cat_only[0] == held[0] - base[0] and both[1] - cat_only[1] == held[1] - base[1]
        getattr(e, order[0])()
        mid = eng.live_resources()
        assert mid == (held if order[0] == "catalogue_release" else cat_only)
        if order[0] == "catalogue_release":  # the survivor still works, with the same bits
            assert same_bits(e.interp_particles(pos[0], pos[1], pos[2], grids_of(n)[:2], kernel="tsc", path=1)[0], first)
        else:
            e.density_particles(pos[0][-5000:], pos[1][-5000:], pos[2][-5000:], mk=1)
        assert eng.live_resources() == mid
        getattr(e, order[1])()
        assert eng.live_resources() == base
    e.close()
    assert eng.live_resources() == start


# ---- the layers above ----------------------------------------------------------------------------------------------------

def test_shim_and_hamil_agree_with_the_c_abi():
    from barcode_amd import hamil, shim
    n, L = 16, 50.0
    p = HamilParams(Nx=n, L=L)
    pos = edge_catalogue(n, L)
    F = grids_of(n)
    e = engine_of(n, L)
    ones = np.ones(p.N)
    sh = shim.ShimHamil(p, signal_PS=ones, mass_f=ones)
    hd = hamil.HamilData(p)
    cic, _ = e.interp_particles(pos[0], pos[1], pos[2], [F[0]], kernel="cic")
    tsc, _ = e.interp_particles(pos[0], pos[1], pos[2], [F[1]], kernel="tsc")
    multi, _ = e.interp_particles(pos[0], pos[1], pos[2], F[:3], kernel="tsc")
    assert same_bits(multi[1], tsc[0])  # one field or three: the same 27 terms
    assert same_bits(cic, edge_reference(n, L, ir.CIC, 0, 1)[0])
    assert same_bits(multi, edge_reference(n, L, ir.TSC, 0, 3)[0])
    assert same_bits(sh.interpolate_CIC(pos[0], pos[1], pos[2], F[0]), cic[0])
    assert same_bits(sh.interpolate_TSC(pos[0], pos[1], pos[2], F[1]), tsc[0])
    assert same_bits(sh.interpolate_TSC_multi(pos[0], pos[1], pos[2], F[:3]), multi)
    assert same_bits(hamil.interpolate_CIC(hd, pos[0], pos[1], pos[2], F[0]), cic[0])
    assert same_bits(hamil.interpolate_TSC(hd, pos[0], pos[1], pos[2], F[1]), tsc[0])
    assert same_bits(hamil.interpolate_TSC_multi(hd, pos[0], pos[1], pos[2], F[:3]), multi)
    with pytest.raises(shim.ShimError):
        sh.interpolate_TSC_multi(pos[0], pos[1], pos[2], [F[0]] * 5)
    sh.close()
    hd.engine.close()
