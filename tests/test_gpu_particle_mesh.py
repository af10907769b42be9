"""The particle-mesh kernels on chosen particle positions, through bchmc_probe_displacement: binning (k_bin_direct,
k_bin, k_scan_tiles, k_reorder, k_subsort), SPH scatter (k_scatter_tile81, k_scatter_tile, k_scatter_sph), NGP / CIC /
TSC (k_scatter_tile_low and the direct form) and the SPH adjoint gather (k_gather_tile81, k_gather_tile, k_gather_sph).

Every position is compared bitwise with tests/pm_reference.positions, every cell of rho and every particle of V with the
longdouble reference under the bound of tests/pm_bound.py (a cell or particle the reference leaves empty must be exactly
0), and the oracle's getDensity / likelihood_calc_V_SPH run as a second reference at TOL_FIELD / 10 TOL_FIELD.  Each
check prints its worst fraction of the bound ("PM <kernel family><type> n=.. <set>: worst fraction of the bound ..").

Not reachable through this entry point: k_zbin_direct, which takes Psi^ from k-space.  Its binning half is not
k_bin_direct's code but an implementation of its own (a hash table of 4 n slots on pairs of counters, two counts packed
in one 64-bit word, 64-bit global reservations); bchmc_probe_displacement_z reaches it and
tests/test_gpu_zbin_positions.py holds it to the same checks.  calc_h = 3's interpolation is covered at oracle precision only: its convolved fields cannot be fetched.
"""
import numpy as np
import pytest

from barcode_amd.engine import Engine
from barcode_amd.params import HamilParams
from oracle import oracle as orc
from tests import pm_bound
from tests import pm_reference as ref
from tests.util import TOL_FIELD, rel_l2

pytestmark = pytest.mark.gpu

LD = np.longdouble
DTYPE = {0: np.float64, 1: np.float32}
FP32_ORACLE_TOL = 2e-5  # the suite's fp32 tolerance against the double-precision oracle


def params(n, h_rel=1.0, mk=3, calc_h=2, rsd=0, mins=(0.0, 0.0, 0.0)):
    return HamilParams(Nx=n, L=200.0 * n / 64.0, likelihood=1, mk=mk, calc_h=calc_h, rsd_model=rsd,
                       particle_kernel_h_rel=h_rel, min1=mins[0], min2=mins[1], min3=mins[2])


def engine(p, precision=0, deterministic=0):
    e = Engine(p, precision=precision, deterministic=deterministic)
    ones = np.ones(p.N)
    e.upload(signal_PS=ones, mass_f=ones, mass_r=ones)
    return e


def rsd_scalars(p):
    hub = 100.0 * np.sqrt(p.OM / p.ascale ** 3 + p.OL + (1.0 - p.OM - p.OL) / p.ascale ** 2)
    return orc.c_pecvel(p.ascale, p.OM, p.OL), 1.0 / hub / p.ascale


def family(info, mk, n):
    if mk != 3:
        return "scatter_tile_low" if info["tiled"] else "scatter_low_order"
    return "tile81" if info["unrolled81"] else ("tile" if info["tiled"] else "sph")


def check_positions(e, p, psi, rsd, dtype):
    """Bitwise, NaN where the reference has NaN.  With RSD the two scalars come from two implementations: each may
    differ by an ulp, so z must be bitwise the reference's z for ONE of the nine combinations of neighbouring scalars
    (the allowance a 1-ulp change of each produces, and nothing else)."""
    geo = ref.Geometry(p.Nx, p.L)
    got = [e.fetch(k) for k in ("posx", "posy", "posz")]
    cp, vn = rsd_scalars(p) if rsd else (0.0, 0.0)
    want = ref.positions(psi, geo, rsd, dtype, cp, vn)
    for a in range(2 if rsd else 3):
        assert np.array_equal(got[a], want[a].astype(np.float64), equal_nan=True), "xyz"[a]
    if rsd:
        hits = []
        for c in (cp, np.nextafter(cp, 0), np.nextafter(cp, np.inf)):
            for v in (vn, np.nextafter(vn, 0), np.nextafter(vn, np.inf)):
                z = ref.positions(psi, geo, rsd, dtype, c, v)[2].astype(np.float64)
                hits.append(np.array_equal(got[2], z, equal_nan=True))
        assert any(hits)
    return got


def check_density(e, p, pos, dtype, label, deterministic=False):
    """rho against the longdouble reference under the bound, cell by cell; the oracle as second reference; the mean
    the tile kernels flushed (through deltaX) against the reference mean."""
    geo = ref.Geometry(p.Nx, p.L, (p.min1, p.min2, p.min3))
    n, info = p.Nx, e.tile_info()
    rho = e.fetch("rho")
    if p.mk == 3:
        d_h = 1.0 / p.particle_kernel_h_rel
        w_norm = 1.0 / np.pi / p.particle_kernel_h ** 3
        S, cnt, total = ref.sph_density(pos, geo, p.particle_kernel_h, pm_bound.q_slack(dtype, n, d_h), dtype)
        bound = pm_bound.density_bound(S, cnt, dtype, n, d_h, w_norm, deterministic)
    else:
        fn = (lambda q, g: ref.ngp_density(q, g, dtype), ref.cic_density, ref.tsc_density)[p.mk]
        S, cnt, total = fn(pos, geo)
        bound = pm_bound.density_bound(S, cnt, dtype, n, 1.0, 1.0, deterministic, kind="low")
        if p.mk == 0:
            assert np.array_equal(rho, S.astype(np.float64)), "NGP counts must be exact"
    f, i = pm_bound.worst_fraction(rho, S, bound)
    tname = np.dtype(dtype).name
    print("PM %s<%s> n=%d %s: worst fraction of the bound %.3f (cell %d = (%d, %d, %d), cnt %d, rho %.17g, reference "
          "%.17g)" % (family(info, p.mk, n), tname, n, label, f, i, i // (n * n), (i // n) % n, i % n, cnt[i], rho[i],
                      float(S[i])))
    assert f <= 1
    assert not np.any(rho[cnt == 0])
    finite = [np.where(np.isfinite(c), c, -1e30) for c in pos]  # the oracle drops what is outside the domain
    rho_o = orc.Oracle(p).getDensity(p.mk, *finite)
    assert rel_l2(rho, rho_o) < (TOL_FIELD if dtype is np.float64 else FP32_ORACLE_TOL)
    # sum(rho) as the likelihood sees it: deltaX = rho / mean - 1, so rho / (deltaX + 1) is the mean wherever deltaX is
    # well away from -1 (cells at half the mean or more: deltaX + 1 >= 1/2 carries the roundings of |deltaX| <= that)
    mean = total / geo.N
    if mean > 0:
        dX = e.fetch("deltaX")
        dense = rho >= 0.5 * float(mean)
        est = rho[dense].astype(LD) / (dX[dense].astype(LD) + 1)
        u = LD(pm_bound.unit_roundoff(dtype))
        tol = bound.sum() / geo.N + 3 * u * mean + geo.N * LD(2.0 ** -53) * mean
        assert dense.any() and np.max(np.abs(est - mean)) <= tol
    return rho


def upload_white_data(e, p, seed=11, impulse=None):
    """Gaussian likelihood data for which part_like = (nobs - Lambda) / sigma^2 is white with both signs wherever the
    window is open and the density positive; the window has holes.  impulse: open the window in that one cell only."""
    rng = np.random.Generator(np.random.Philox(seed))
    dX = e.fetch("deltaX")
    window = (rng.random(p.N) >= 0.2).astype(np.float64)
    if impulse is not None:
        window = np.zeros(p.N)
        window[impulse] = 1.0
    noise = np.full(p.N, 0.5)
    lam = window * p.rho_c * (1.0 + p.biasP * dX)
    nobs = lam + noise ** 2 * rng.standard_normal(p.N)
    e.upload(window=window, noise=noise, nobs=nobs)


def check_gather(e, p, pos, dtype, rsd, label, want_white=True):
    geo = ref.Geometry(p.Nx, p.L)
    n, info = p.Nx, e.tile_info()
    pl = e.fetch("part_like")
    V = np.array([e.fetch(k) for k in ("Vx", "Vy", "Vz")])
    if want_white:  # both signs among the open, occupied cells; holes
        nnz = np.count_nonzero(pl)
        assert nnz > 0 and (pl > 0).sum() >= nnz // 5 and (pl < 0).sum() >= nnz // 5 and (pl == 0).any()
    d_h = 1.0 / p.particle_kernel_h_rel
    f1 = orc.fgrow(p.ascale, p.OM, p.OL) if rsd else 0.0
    Vr, A, P, m = ref.sph_adjoint_gather(pos, pl, geo, p.particle_kernel_h, p.rho_c, bool(rsd), f1,
                                         pm_bound.q_slack(dtype, n, d_h), dtype)
    norm = 1.0 / (np.pi * p.particle_kernel_h ** 4)
    bound = pm_bound.gather_bound(A, P, m, dtype, n, d_h, norm, 1.0 + f1)
    f, i = pm_bound.worst_fraction(V, Vr, bound)
    fam = {"tile81": "gather_tile81", "tile": "gather_tile", "sph": "gather_sph"}[family(info, 3, n)]
    q = i % p.N
    print("PM %s<%s> n=%d %s: worst fraction of the bound %.3f (component %d of particle %d at (%.17g, %.17g, %.17g), %d "
          "cells, V %.17g, reference %.17g)" % (fam, np.dtype(dtype).name, n, label, f, i // p.N, q, pos[0][q], pos[1][q],
                                                pos[2][q], m[q], V.ravel()[i], float(Vr.ravel()[i])))
    assert f <= 1
    bad = ~(np.isfinite(pos[0]) & np.isfinite(pos[1]) & np.isfinite(pos[2]))
    assert not np.any(V[:, bad]) and not np.any(V[:, m == 0])
    ok = ~bad
    if ok.all():  # (the oracle indexes with the position: it is not given non-finite ones)
        Vo = orc.Oracle(p).likelihood_calc_V_SPH(pl, *pos)
        tol = 10 * TOL_FIELD if dtype is np.float64 else FP32_ORACLE_TOL
        assert rel_l2(V, np.array(Vo)) < tol
    return pl, V, bound


def run_sph(n, h_rel, precision, names, rsd=0, mins=(0.0, 0.0, 0.0), expect=None, deterministic=0, force=True,
            impulse_on=()):
    dtype = DTYPE[precision]
    p = params(n, h_rel, rsd=rsd, mins=mins)
    geo = ref.Geometry(n, p.L)
    sets = ref.position_sets(geo, dtype, names=names)
    e = engine(p, precision, deterministic)
    info = e.tile_info()
    if expect is not None:
        assert family(info, 3, n) == expect, info
    for name in names:
        psi = sets[name]
        e.probe_displacement(psi, rsd, False)
        pos = check_positions(e, p, psi, rsd, dtype)
        check_density(e, p, pos, dtype, name, bool(deterministic))
        if force:
            upload_white_data(e, p)
            e.probe_displacement(psi, rsd, True)
            check_gather(e, p, pos, dtype, rsd, name)
        if name in impulse_on:
            occupied = int(np.argmax(e.fetch("rho")))
            upload_white_data(e, p, impulse=occupied)
            e.probe_displacement(psi, rsd, True)
            pl, _, _ = check_gather(e, p, pos, dtype, rsd, name + " impulse", want_white=False)
            assert np.count_nonzero(pl) == 1
    e.close()


SPECIAL = ref.SPECIAL_SETS + ("upper_edge", "tiny_negative", "mixed")


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_every_position_set_on_the_unrolled_kernels(precision):
    """16^3, h = d: one 8 x 8 x 16 tile along z (the halo wraps onto the tile itself), every set of the issue; RSD on the
    second pass over the special sets for the gather's f1 factor."""
    run_sph(16, 1.0, precision, ref.ALL_SETS, expect="tile81", impulse_on=("uniform", "corners"))
    run_sph(16, 1.0, precision, ("mixed", "faces", "far_out"), rsd=1, expect="tile81")


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("h_rel,expect", ((0.8661, "tile81"), (1.0599, "tile81"), (0.866, "tile"), (0.85, "tile"),
                                          (1.3, "tile"), (0.8, "tile")))
def test_kernel_scales_at_the_ends_of_each_range(h_rel, expect, precision):
    """Both ends of the range the unrolled kernels accept (their branch classes and their hull are decided for
    0.8661 d <= h < 1.06 d; the decisive points are corners, edge midpoints and face centres), the generic tile kernel
    with the exact hull just below it, and the cube loop."""
    run_sph(16, h_rel, precision, SPECIAL, expect=expect)


@pytest.mark.parametrize("n,expect,names", ((32, "tile81", SPECIAL + ("collapse_inside", "collapse_corner", "sheet",
                                                                      "filament")),
                                            (48, "tile81", ("mixed", "corners")),
                                            (24, "tile", SPECIAL), (12, "tile", SPECIAL), (10, "sph", SPECIAL)))
def test_grid_and_tile_shapes(n, expect, names):
    """32^3; 48^3: three tiles along z; 24^3: 8 x 8 x 8 tiles; 12^3: 4 x 4 x 4 tiles; 10^3: no tile shape divides the
    grid, the direct kernels run."""
    run_sph(n, 1.0, 0, names, expect=expect)
    if n in (32, 10):
        run_sph(n, 1.0, 1, ("mixed", "collapse_corner") if n == 32 else ("mixed", "corners"), expect=expect)


# collapse_inside puts every particle around (3.6, 3.3, 5.4) d: outside the box at n = 4 and 5, where it would only be a
# second collapse_corner-like set after folding.  It is the one set left out, at those two sizes.
SMALL_BOX_SETS = tuple(s for s in ref.ALL_SETS if s != "collapse_inside")


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("n,h_rel,no_tiles,expect", ((4, 1.0, False, "tile"), (4, 0.87, False, "tile"), (4, 1.0, True, "sph"),
                                                     (5, 1.0, False, "sph"), (7, 1.0, False, "sph")),
                         ids=("n4_tile", "n4_tile_h0.87", "n4_direct", "n5_direct", "n7_direct"))
def test_smallest_and_odd_grids(n, h_rel, no_tiles, expect, precision, monkeypatch):
    """4^3: one 4 x 4 x 4 tile whose halo wraps onto the tile on every axis (every cell is in the image 8 times), at h = d
    and at h = 0.87 d; the direct kernels there (BCHMC_NO_TILES=1: stencil offsets -2 and +2 are one cell); 5^3 (the stencil
    is as wide as the box) and 7^3 on the direct kernels.  Every set but collapse_inside at 4 and 5 (SMALL_BOX_SETS), every
    set at 7; RSD on a second pass."""
    if no_tiles:
        monkeypatch.setenv("BCHMC_NO_TILES", "1")
    names = ref.ALL_SETS if n == 7 else SMALL_BOX_SETS
    run_sph(n, h_rel, precision, names, expect=expect, impulse_on=("uniform", "corners"))
    run_sph(n, h_rel, precision, ("mixed", "faces", "far_out"), rsd=1, expect=expect)


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("mk", (0, 1, 2), ids=("ngp", "cic", "tsc"))
def test_low_order_kernels_on_an_odd_grid(mk, precision):
    """NGP / CIC / TSC at 9^3: no tile shape divides it, the direct form runs."""
    dtype = DTYPE[precision]
    p = params(9, mk=mk, calc_h=1)
    geo = ref.Geometry(9, p.L)
    e = engine(p, precision)
    assert family(e.tile_info(), mk, 9) == "scatter_low_order"
    for name, psi in ref.position_sets(geo, dtype, names=ref.ALL_SETS).items():
        e.probe_displacement(psi, 0, False)
        pos = check_positions(e, p, psi, 0, dtype)
        check_density(e, p, pos, dtype, "mk=%d %s" % (mk, name))
    e.close()


def test_one_case_at_64():
    run_sph(64, 1.0, 0, ("mixed",), expect="tile81")


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_direct_kernels_without_tiles(precision, monkeypatch):
    monkeypatch.setenv("BCHMC_NO_TILES", "1")
    run_sph(16, 1.0, precision, ref.ALL_SETS, expect="sph")
    run_sph(16, 1.0, precision, ("mixed",), rsd=1, expect="sph")


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_domain_with_an_offset_corner(precision):
    """min1/2/3 != 0: positions stay in [0, L), the particles outside [min, min + L) are dropped from rho and still get
    a V (the gather does not know about the domain)."""
    d = 3.125
    for names in (("uniform", "mixed", "corners"),):
        dtype = DTYPE[precision]
        p = params(16, mins=(2 * d, -1.5 * d, 0.25 * d))
        geo = ref.Geometry(16, p.L)
        e = engine(p, precision)
        assert family(e.tile_info(), 3, 16) == "tile81"
        for name, psi in ref.position_sets(geo, dtype, names=names).items():
            e.probe_displacement(psi, 0, False)
            pos = check_positions(e, p, psi, 0, dtype)
            outside = ~ref.in_domain(pos, ref.Geometry(16, p.L, (p.min1, p.min2, p.min3)))
            assert outside.sum() > p.N // 10
            check_density(e, p, pos, dtype, name + " offset domain")
            upload_white_data(e, p)
            e.probe_displacement(psi, 0, True)
            _, V, _ = check_gather(e, p, pos, dtype, 0, name + " offset domain")
            assert np.count_nonzero(V[:, outside]) > 0
        e.close()


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_deterministic_mode_is_bitwise_repeatable_and_inside_the_bound(precision):
    dtype = DTYPE[precision]
    for n, names in ((16, ("mixed", "collapse_corner")), (32, ("filament",))):
        p = params(n)
        geo = ref.Geometry(n, p.L)
        sets = ref.position_sets(geo, dtype, names=names)
        runs = []
        for _ in range(2):
            e = engine(p, precision, deterministic=1)
            out = {}
            for name in names:
                e.probe_displacement(sets[name], 0, False)
                pos = check_positions(e, p, sets[name], 0, dtype)
                out[name] = check_density(e, p, pos, dtype, name + " deterministic", deterministic=True)
            runs.append(out)
            e.close()
        for name in names:
            assert np.array_equal(runs[0][name], runs[1][name]), name


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("mk", (0, 1, 2), ids=("ngp", "cic", "tsc"))
def test_low_order_kernels(mk, precision, monkeypatch):
    """NGP / CIC / TSC on the tile records, then the direct form (BCHMC_NO_TILES_LOW=1), then with an offset domain
    (direct kernels again: the records are keyed on floor(x / d))."""
    dtype = DTYPE[precision]

    def run(n, names, expect, mins=(0.0, 0.0, 0.0), deterministic=0):
        p = params(n, mk=mk, calc_h=1, mins=mins)
        geo = ref.Geometry(n, p.L)
        e = engine(p, precision, deterministic)
        assert family(e.tile_info(), mk, n) == expect
        for name, psi in ref.position_sets(geo, dtype, names=names).items():
            e.probe_displacement(psi, 0, False)
            pos = check_positions(e, p, psi, 0, dtype)
            check_density(e, p, pos, dtype, "mk=%d %s" % (mk, name), bool(deterministic))
        e.close()

    run(16, ref.ALL_SETS, "scatter_tile_low")
    run(32, ("mixed", "collapse_corner"), "scatter_tile_low")
    run(16, ("mixed",), "scatter_tile_low", deterministic=1)
    # (lower corners that are binary fractions below every position's ulp range: x - min is then exact in float32 as
    # in double, so the reference's storage-type cell and the kernel's double-precision one cannot differ)
    run(16, ("mixed", "corners"), "scatter_low_order", mins=(3.125, 6.25, 0.78125))
    monkeypatch.setenv("BCHMC_NO_TILES_LOW", "1")
    run(16, SPECIAL + ("collapse_inside",), "scatter_low_order")


@pytest.mark.parametrize("cap", ("0", "8", None), ids=("cap0", "cap8", "default"))
def test_sort_paths_with_small_chunks(cap, monkeypatch):
    """BCHMC_CHUNK=64: dozens of (tile, chunk) work items per tile at 16^3; BCHMC_SORT_CAP=0: two-pass sort only; 8: every
    segment overflows, the first evaluation runs two-pass sort + sub-cell ordering, the slots then grow."""
    monkeypatch.setenv("BCHMC_CHUNK", "64")
    if cap is not None:
        monkeypatch.setenv("BCHMC_SORT_CAP", cap)
    for precision in (0, 1):
        dtype = DTYPE[precision]
        p = params(16)
        geo = ref.Geometry(16, p.L)
        e = engine(p, precision)
        info = e.tile_info()
        assert info["tiled"] and info["unrolled81"] and info["one_pass"] == (cap != "0")
        if cap == "8":
            assert info["cap"] == 8
        for name, psi in ref.position_sets(geo, dtype, names=("mixed", "filament", "uniform", "mixed")).items():
            e.probe_displacement(psi, 0, False)
            pos = check_positions(e, p, psi, 0, dtype)
            check_density(e, p, pos, dtype, "%s chunk 64 cap %s" % (name, cap))
            upload_white_data(e, p)
            e.probe_displacement(psi, 0, True)
            check_gather(e, p, pos, dtype, 0, "%s chunk 64 cap %s" % (name, cap))
        if cap == "8":
            assert e.tile_info()["cap"] > 8
        e.close()


@pytest.mark.parametrize("name", ("collapse_inside", "collapse_corner"))
def test_a_real_overflow_at_the_default_cap(name):
    """32^3 collapsed into one point: the one real overflow.  The first evaluation must already be exact (through the
    two-pass sort), repeated calls stay exact while the slots grow until the one-pass path holds all of it, and a
    uniform set on the same handle is exact again."""
    n, dtype = 32, np.float64
    p = params(n)
    geo = ref.Geometry(n, p.L)
    sets = ref.position_sets(geo, dtype, names=(name, "uniform"))
    e = engine(p)
    before = e.tile_info()
    assert before["tiled"] and before["one_pass"] and before["unrolled81"]
    caps = [before["cap"]]
    for call in range(4):
        e.probe_displacement(sets[name], 0, False)
        pos = check_positions(e, p, sets[name], 0, dtype)
        check_density(e, p, pos, dtype, "%s call %d (slots per tile %d)" % (name, call, caps[-1]))
        caps.append(e.tile_info()["cap"])
    assert caps[1] > caps[0] and caps[-1] == caps[-2], caps  # grew after the overflow, then settled
    hc = [ref.home_cell(c, geo.d, dtype) % n for c in pos]
    tile_max = np.bincount((hc[0] // 8) * 8 + (hc[1] // 8) * 2 + hc[2] // 16).max()
    assert e.tile_info()["one_pass"] and caps[-1] >= tile_max // 8  # room for the fullest tile's fullest octant
    upload_white_data(e, p)
    e.probe_displacement(sets[name], 0, True)
    check_gather(e, p, pos, dtype, 0, name + " after the slots grew")
    e.probe_displacement(sets["uniform"], 0, False)
    pos = check_positions(e, p, sets["uniform"], 0, dtype)
    check_density(e, p, pos, dtype, "uniform after " + name)
    e.close()


def test_adjoint_identity_against_a_finite_difference():
    """sum_p V_p . e is rho_c d^3 times the derivative of sum_c part_like_c rho_c under a uniform shift of all particles
    along e.  The derivative is a longdouble central difference of pm_reference's density functional with step s =
    2^-20 d; its truncation error is estimated from the pair (s, s / 2): for an O(s^2) error the two differ by three
    times the error of the finer one, so |D(s) - D(s / 2)| bounds it with room.  On top comes the summed gather bound."""
    adjoint_identity(16)


def test_adjoint_identity_against_a_finite_difference_at_5():
    """The same identity where the stencil is as wide as the box (direct kernels)."""
    adjoint_identity(5)


def adjoint_identity(n):
    dtype = np.float64
    p = params(n)
    geo = ref.Geometry(n, p.L)
    psi = ref.position_sets(geo, dtype, names=("mixed",))["mixed"]
    e = engine(p)
    e.probe_displacement(psi, 0, False)
    pos = check_positions(e, p, psi, 0, dtype)
    upload_white_data(e, p)
    e.probe_displacement(psi, 0, True)
    pl, V, bound = check_gather(e, p, pos, dtype, 0, "mixed (adjoint identity)")
    e.close()
    normalize = LD(p.rho_c) * LD(p.L) ** 3 / LD(p.N)
    s = geo.d * 2.0 ** -20
    for axis in range(3):
        fine = ref.density_shift_derivative(pos, pl, geo, p.particle_kernel_h, axis, s / 2, dtype)
        coarse = ref.density_shift_derivative(pos, pl, geo, p.particle_kernel_h, axis, s, dtype)
        lhs = V[axis].astype(LD).sum()
        tol = normalize * abs(coarse - fine) + bound[axis].sum()
        print("PM adjoint identity axis %d: sum V = %.17g, rho_c d^3 dF/ds = %.17g, truncation estimate %.3g, summed "
              "bound %.3g" % (axis, float(lhs), float(normalize * fine), float(normalize * abs(coarse - fine)),
                              float(bound[axis].sum())))
        assert abs(lhs - normalize * fine) <= tol


def test_calc_h3_from_a_displacement_at_oracle_precision():
    """calc_h = 3 (convolution + TSC interpolation): the convolved fields cannot be fetched, so this path is covered at
    oracle precision only."""
    n = 16
    p = params(n, calc_h=3)
    geo = ref.Geometry(n, p.L)
    e = engine(p)
    for name, psi in ref.position_sets(geo, np.float64, names=("uniform", "mixed")).items():
        e.probe_displacement(psi, 0, False)
        pos = check_positions(e, p, psi, 0, np.float64)
        check_density(e, p, pos, np.float64, name + " calc_h 3")
        upload_white_data(e, p)
        e.probe_displacement(psi, 0, True)
        pl = e.fetch("part_like")
        Vo = orc.Oracle(p).likelihood_calc_V_SPH_fourier_TSC(pl, *pos)
        for k, want in zip(("Vx", "Vy", "Vz"), Vo):
            assert rel_l2(e.fetch(k), want) < 10 * TOL_FIELD
    e.close()


def test_entry_point_refuses_what_it_should():
    from barcode_amd.engine import BchmcError
    p = params(16)
    e = Engine(p)
    psi = np.zeros((3, p.N))
    with pytest.raises(BchmcError) as err:  # with_force needs the inputs
        e.probe_displacement(psi, 0, True)
    assert err.value.code == 9
    with pytest.raises(ValueError):
        e.probe_displacement(np.zeros(p.N), 0, False)
    e.probe_displacement(psi, 0, False)
    assert np.array_equal(e.fetch("psix"), np.zeros(p.N))
    e.close()
    e = Engine(HamilParams(Nx=16, L=50.0, planepar=0))
    with pytest.raises(BchmcError) as err:
        e.probe_displacement(psi, 1, False)
    assert err.value.code == 3
    e.close()


# ---- the last test of the file: a documented contract, checked once ------------------------------------------------------


@pytest.mark.parametrize("config", ("tile81", "tile", "direct", "two_pass", "cic"))
def test_non_finite_displacements_are_left_out(config, monkeypatch):
    """"Particles with a non-finite position are left out; the gather gives them V = 0" (tiles.hpp).  Every index the
    kernels form from a position is behind pos_ok / in_domain (k_bin_direct, k_bin, k_gather_sph, k_scatter_sph,
    k_scatter_low_order; the tile kernels only see binned records), so NaN, +inf and -inf in one component of a
    handful of particles -- the first and the last particle of a brick among them -- must cost exactly those particles:
    nothing in rho, V = 0, every other cell and particle inside the bound, no NaN anywhere else."""
    n, h_rel, mk = 16, 1.0, 3
    if config == "tile":
        n = 24
    if config == "direct":
        monkeypatch.setenv("BCHMC_NO_TILES", "1")
    if config == "two_pass":
        monkeypatch.setenv("BCHMC_SORT_CAP", "0")
    if config == "cic":
        mk = 1
    for precision in (0, 1):
        dtype = DTYPE[precision]
        p = params(n, h_rel, mk=mk, calc_h=2 if mk == 3 else 1)
        geo = ref.Geometry(n, p.L)
        psi = ref.position_sets(geo, dtype, names=("mixed",))["mixed"].copy()
        # a brick is 4 x 4 x 16 lattice sites when 16 divides n (else 256 consecutive ones): particle 0 is the first of
        # brick 0; (i, j, k) = (3, 3, 15) its last; N - 1 the last of the last brick
        victims = {0: (0, np.nan), 15 + n * (3 + n * 3): (1, np.inf), p.N - 1: (2, -np.inf), 255: (0, -np.inf),
                   256: (2, np.nan), p.N // 2 + 7: (1, np.nan), 1000: (0, np.inf)}
        for q, (axis, value) in victims.items():
            psi[axis, q] = value
        e = engine(p, precision)
        e.probe_displacement(psi, 0, False)
        pos = check_positions(e, p, psi, 0, dtype)
        bad = ~(np.isfinite(pos[0]) & np.isfinite(pos[1]) & np.isfinite(pos[2]))
        assert sorted(np.flatnonzero(bad)) == sorted(victims)
        rho = check_density(e, p, pos, dtype, "mixed with non-finite displacements (%s)" % config)
        assert np.all(np.isfinite(rho)) and np.all(np.isfinite(e.fetch("deltaX")))
        if mk == 3:
            upload_white_data(e, p)
            e.probe_displacement(psi, 0, True)
            _, V, _ = check_gather(e, p, pos, dtype, 0, "mixed with non-finite displacements (%s)" % config)
            assert np.all(np.isfinite(V)) and not np.any(V[:, bad]) and np.all(np.isfinite(e.fetch("part_like")))
        e.close()
