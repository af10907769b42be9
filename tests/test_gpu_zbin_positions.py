"""The fused z pass + binning kernel k_zbin_direct (barcode_amd/csrc/zpass.hpp) on chosen particle positions, through
bchmc_probe_displacement_z: the binning of every force evaluation at 256^3 and 512^3 (128^3 under BCHMC_ZBIN_128=1).  Its
binning half is an implementation of its own -- an LDS hash table of 4 n slots keyed on PAIRS of (tile, octant) counters,
the two counts of a pair packed into one 64-bit word, one 64-bit global reservation per pair, the table laid over the
transform tile -- and so gets what tests/test_gpu_particle_mesh.py gives k_bin_direct.

The entry sends psi / n through k_zr2c (tests/test_gpu_fft_passes.py) and the kernel transforms it back, so the kernel's
displacement is psi after a z round trip.  The stored Psi (store_psi = 1) is what the kernel used: it must be bitwise psi
for rows constant along z, inside the two-pass bound of tests/fft_bound.py per pair of rows otherwise, and every
reference below starts from it.  Per set:

1. positions bitwise tests/pm_reference.positions(Psi) (the nine-neighbour allowance for z under RSD);
2. rho over the whole grid against the C oracle's getDensity (its OpenMP build: 2 10^6 particles) at TOL_FIELD /
   FP32_ORACLE_TOL -- one lost or doubled particle among 2 10^6 moves this by about 1e-3 -- and exactly 0 in every cell
   no particle's stencil can reach;
3. rho per cell and V per particle under the unchanged bounds of tests/pm_bound.py against the longdouble reference on
   the subsets of tests/zbin_sets.py (>= 4096 cells: the 64 fullest, the box corners, a whole z row, a 16^3 block across
   tile boundaries; >= 4096 particles), printed as "PM zbin<type> n=.. <set>: worst fraction of the bound ..";
4. on a deterministic handle the k_bin_direct path from the same Psi gives bitwise the same pos*, rho, deltaX,
   part_like and V* (fixed-point sums do not depend on record order), and so does store_psi = 0 for rho and V*.

n = 128 (hash of 512 slots, odd log2 n) in fp64 and fp32 for every set; n = 256 (the benchmark instantiation) for
`mixed` and `scrambled`.  512^3 is left out: its host arrays alone (3 x 1 GiB of psi, the oracle's pass over 1.3 10^8
particles) take a test out of the seconds range; tests/test_gpu_large.py runs that instantiation on smooth fields.
"""
import os

import numpy as np
import pytest

from barcode_amd.engine import BchmcError, Engine
from oracle import oracle as orc
from tests import pm_bound, zbin_sets
from tests import pm_reference as ref
from tests.fft_bound import worst_ratio_roundtrip
from tests.test_gpu_particle_mesh import DTYPE, FP32_ORACLE_TOL, check_positions, params, upload_white_data
from tests.util import TOL_FIELD, rel_l2

pytestmark = pytest.mark.gpu

THREADS = max(1, min(8, os.cpu_count() or 1))
PSI = ("psix", "psiy", "psiz")
TWIN_FIELDS = ("posx", "posy", "posz", "rho", "deltaX", "part_like", "Vx", "Vy", "Vz")


@pytest.fixture
def engines(monkeypatch):
    """make(p, precision, deterministic) -> Engine with the spectra uploaded; every engine is closed afterwards."""
    monkeypatch.setenv("BCHMC_ZBIN_128", "1")
    made = []

    def make(p, precision=0, deterministic=0):
        e = Engine(p, precision=precision, deterministic=deterministic)
        made.append(e)
        ones = np.ones(p.N)
        e.upload(signal_PS=ones, mass_f=ones, mass_r=ones)
        info = e.tile_info()
        assert info["tiled"] and info["one_pass"] and info["unrolled81"] and min(info["tile_shape"]) > 0, info
        return e

    yield make
    for e in made:
        e.close()


def pairs(a, n):
    """(3, N) -> (3, n, n / 2, 2 n): the rows (i, j0) and (i, j0 + 1) of one packed transform side by side."""
    return np.asarray(a).reshape(3, n, n // 2, 2 * n)


def stored_psi(e, psi, n, dtype, exact, label):
    """Psi as the kernel stored it; bitwise psi (in the storage type) where the set is constant along z, inside the
    round-trip bound per pair of rows otherwise."""
    got = np.array([e.fetch(k) for k in PSI])
    want = np.asarray(psi, dtype=np.float64).reshape(3, -1).astype(dtype).astype(np.float64)
    if exact:
        assert np.array_equal(got, want), label
    else:
        f = worst_ratio_roundtrip(pairs(got, n), pairs(want, n), n, dtype)
        print("PM zbin<%s> n=%d %s: z round trip, worst fraction of the bound %.3f" % (np.dtype(dtype).name, n, label, f))
        assert f <= 1
    return got


def check_density(e, p, pos, dtype, label, tile_shape, deterministic=False, extra=None, reference=None):
    """Checks 2 and 3 for rho.  reference: a dict that keeps the longdouble sums between calls with the same positions."""
    geo = ref.Geometry(p.Nx, p.L, (p.min1, p.min2, p.min3))
    n, h = p.Nx, p.particle_kernel_h
    rho = e.fetch("rho")
    assert np.all(np.isfinite(rho))
    reference = {} if reference is None else reference
    if "S" not in reference:
        finite = [np.where(np.isfinite(c), c, -1e30) for c in pos]  # the oracle drops what is outside the domain
        reference["oracle"] = orc.Oracle(p, omp=True).getDensity(3, *finite)
        reference["reach"] = ref.reachable_cells(pos, geo, h, dtype)
        cells, hist = zbin_sets.cell_subset(pos, geo, tile_shape, dtype, extra)
        S, cnt = ref.sph_density_at(pos, geo, h, cells, pm_bound.q_slack(dtype, n, geo.d / h), dtype, threads=THREADS)
        reference.update(cells=cells, hist=hist, S=S, cnt=cnt)
    assert rel_l2(rho, reference["oracle"]) < (TOL_FIELD if dtype is np.float64 else FP32_ORACLE_TOL)
    assert not np.any(rho[~reference["reach"]])
    cells, S, cnt = reference["cells"], reference["S"], reference["cnt"]
    assert len(cells) >= 4096
    bound = pm_bound.density_bound(S, cnt, dtype, n, geo.d / h, 1.0 / np.pi / h ** 3, deterministic)
    f, i = pm_bound.worst_fraction(rho[cells], S, bound)
    c = int(cells[i])
    print("PM zbin<%s> n=%d %s: worst fraction of the bound %.3f (cell %d = (%d, %d, %d), cnt %d, rho %.17g, reference "
          "%.17g)" % (np.dtype(dtype).name, n, label, f, c, c // (n * n), (c // n) % n, c % n, cnt[i], rho[c], float(S[i])))
    assert f <= 1
    assert not np.any(rho[cells][cnt == 0])
    return rho, reference


def check_gather(e, p, pos, dtype, rsd, label, hist, extra=None):
    """Check 3 for V, on the particles of zbin_sets.particle_subset; V = 0 exactly for every non-finite position."""
    geo = ref.Geometry(p.Nx, p.L)
    n, h = p.Nx, p.particle_kernel_h
    pl = e.fetch("part_like")
    V = np.array([e.fetch(k) for k in ("Vx", "Vy", "Vz")])
    assert np.all(np.isfinite(pl)) and np.count_nonzero(pl) > 0
    parts = zbin_sets.particle_subset(pos, geo, dtype, hist, extra)
    assert len(parts) >= 4096
    f1 = orc.fgrow(p.ascale, p.OM, p.OL) if rsd else 0.0
    Vr, A, P, m = ref.sph_adjoint_gather_at(pos, pl, geo, h, p.rho_c, parts, bool(rsd), f1,
                                            pm_bound.q_slack(dtype, n, geo.d / h), dtype)
    bound = pm_bound.gather_bound(A, P, m, dtype, n, geo.d / h, 1.0 / (np.pi * h ** 4), 1.0 + f1)
    f, i = pm_bound.worst_fraction(V[:, parts], Vr, bound)
    q = int(parts[i % len(parts)])
    print("PM zbin gather<%s> n=%d %s: worst fraction of the bound %.3f (component %d of particle %d at (%.17g, %.17g, "
          "%.17g), %d cells, V %.17g, reference %.17g)" % (np.dtype(dtype).name, n, label, f, i // len(parts), q, pos[0][q],
                                                          pos[1][q], pos[2][q], m[i % len(parts)], V[i // len(parts), q],
                                                          float(Vr.ravel()[i])))
    assert f <= 1
    bad = ~(np.isfinite(pos[0]) & np.isfinite(pos[1]) & np.isfinite(pos[2]))
    assert np.all(np.isfinite(V)) and not np.any(V[:, bad]) and not np.any(V[:, parts][:, m == 0])
    return V


def run_set(engines, n, precision, name, rsd=0, mins=(0.0, 0.0, 0.0), load=None):
    """Checks 1 to 3 for one set on a default handle.  load: the set must give some workgroup at least this fraction of
    4 n distinct counter pairs (computed from the reference positions and the handle's tile shape)."""
    dtype = DTYPE[precision]
    p = params(n, rsd=rsd, mins=mins)
    geo = ref.Geometry(n, p.L)
    e = engines(p, precision)
    tile = e.tile_info()["tile_shape"]
    psi = zbin_sets.z_position_sets(geo, dtype, tile, (name,))[name]
    label = name + (" rsd" if rsd else "") + (" offset domain" if any(mins) else "")
    e.probe_displacement_z(psi, rsd, False, True)
    used = stored_psi(e, psi, n, dtype, name in zbin_sets.EXACT_SETS, label)
    pos = check_positions(e, p, used, rsd, dtype)
    key = zbin_sets.counter_keys(pos, geo, tile, dtype)
    per = zbin_sets.distinct_pairs_per_workgroup(key, n)
    print("PM zbin<%s> n=%d %s: distinct counter pairs per workgroup mean %.1f, largest %d of %d (load %.3f)"
          % (np.dtype(dtype).name, n, label, per.mean(), per.max(), 4 * n, per.max() / (4.0 * n)))
    if load is not None:
        assert per.max() >= load * 4 * n
    if name == "one_counter":
        assert np.all(per == 1) and len(np.unique(key)) == (n // 2) ** 2 and np.all(np.bincount(key)[np.unique(key)] == 4 * n)
    if name == "both_halves":
        _, even, odd = zbin_sets.pair_halves_per_workgroup(key, n)
        assert np.all(even + odd == 4 * tile[2]) and np.all(even > 0) and np.all(odd > 0)
    extra = None
    if any(mins):
        outside = ~ref.in_domain(pos, ref.Geometry(n, p.L, mins))
        assert outside.sum() > p.N // 200
        hc = [ref.home_cell(c[outside], geo.d, dtype) % n for c in pos]
        extra = np.unique(hc[2] + n * (hc[1] + n * hc[0]))  # every cell that holds a record with the no-scatter flag
    _, reference = check_density(e, p, pos, dtype, label, tile, extra=extra)
    upload_white_data(e, p)
    e.probe_displacement_z(psi, rsd, True, True)
    V = check_gather(e, p, pos, dtype, rsd, label, reference["hist"], extra=None if extra is None else np.flatnonzero(outside)[:2048])
    if any(mins):
        assert np.count_nonzero(V[:, outside]) > 0  # the gather does not know about the domain
    return e, psi, pos


EXACT = zbin_sets.EXACT_SETS
VARYING = ("uniform", "mixed", "scrambled", "one_counter")


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("name", EXACT + VARYING)
def test_position_sets_at_128(engines, name, precision):
    """Every set at 128^3: the z-constant ones (Psi bitwise as given: particles exactly on centres, corners, edges, faces,
    nextafter(L, 0), -ulp, many box lengths out, the boundary between the two counters of a pair) and the ones that vary
    along z; `scrambled` must fill some workgroup's table to >= 0.9, `one_counter` puts 4 n into one half of one word."""
    run_set(engines, 128, precision, name, load=0.9 if name == "scrambled" else None)


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_mixed_with_rsd_at_128(engines, precision):
    run_set(engines, 128, precision, "mixed", rsd=1)


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_mixed_in_an_offset_domain_at_128(engines, precision):
    """min1..3 != 0: the records of the particles outside [min, min + L) carry the no-scatter flag; they add nothing to
    rho (every cell that holds one is in the subset) and still get a V."""
    d = 400.0 / 128
    run_set(engines, 128, precision, "mixed", mins=(0.5 * d, -0.25 * d, 0.25 * d))


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("name", ("mixed", "scrambled"))
def test_benchmark_instantiation_at_256(engines, name, precision):
    """k_zbin_direct<T, 256>: 1024 slots, 3 waves per SIMD in fp64."""
    run_set(engines, 256, precision, name, load=0.9 if name == "scrambled" else None)


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("name", ("mixed", "uniform", "scrambled", "one_counter", "both_halves", "corners"))
def test_twin_paths_on_a_deterministic_handle(engines, name, precision):
    """Check 4: bchmc_probe_displacement (k_bin_direct) from the stored Psi against bchmc_probe_displacement_z, and the
    interior-step variant (store_psi = 0) against the storing one, bit for bit.  `mixed` puts 3 / 16 of the 2 10^6
    particles into one clump, more than the 2^16 maximal contributions per cell a deterministic handle accepts: there
    both paths must say so (BCHMC_ERR_STATE), which is all that can be compared."""
    n, dtype = 128, DTYPE[precision]
    p = params(n)
    geo = ref.Geometry(n, p.L)
    e = engines(p, precision, deterministic=1)
    psi = zbin_sets.z_position_sets(geo, dtype, e.tile_info()["tile_shape"], (name,))[name]
    if name == "mixed":
        for run in (lambda: e.probe_displacement_z(psi, 0, False, True), lambda: e.probe_displacement_z(psi, 0, False, False),
                    lambda: e.probe_displacement(psi, 0, False)):
            with pytest.raises(BchmcError) as err:
                run()
            assert err.value.code == 9 and "fixed-point range" in str(err.value)
        return
    e.probe_displacement_z(psi, 0, False, True)
    used = np.array([e.fetch(k) for k in PSI])
    upload_white_data(e, p)
    e.probe_displacement_z(psi, 0, True, True)
    z = {k: e.fetch(k) for k in TWIN_FIELDS}
    assert np.count_nonzero(z["Vx"]) > p.N // 2
    e.probe_displacement(used, 0, True)
    for k in TWIN_FIELDS:
        assert np.array_equal(e.fetch(k), z[k], equal_nan=True), k
    e.probe_displacement_z(psi, 0, True, False)
    for k in ("rho", "deltaX", "part_like", "Vx", "Vy", "Vz"):
        assert np.array_equal(e.fetch(k), z[k]), k + " (store_psi = 0)"


@pytest.mark.parametrize("store_psi", (1, 0), ids=("stored", "psi_only"))
@pytest.mark.parametrize("name", ("collapse_inside", "collapse_corner"))
def test_a_real_overflow_through_the_z_pass(engines, name, store_psi):
    """128^3 collapsed into one point at the default cap: a segment overflows, the evaluation must already be exact
    (through the two-pass sort, which with store_psi = 0 reads the Psi the PSI_ONLY launch wrote), repeated calls stay
    exact while bchmc_tile_info shows the slots grow and settle, and a uniform set on the same handle is exact again.
    The Psi the PSI_ONLY launch leaves must be bitwise the one stored on the way."""
    n, dtype = 128, np.float64
    p = params(n)
    geo = ref.Geometry(n, p.L)
    e = engines(p)
    tile = e.tile_info()["tile_shape"]
    sets = zbin_sets.z_position_sets(geo, dtype, tile, (name, "uniform"))
    caps = [e.tile_info()["cap"]]
    reference, used, pos = None, None, None
    for call in range(3):
        e.probe_displacement_z(sets[name], 0, False, bool(store_psi))
        caps.append(e.tile_info()["cap"])
        if call == 0:
            # Psi is in the handle either way: stored on the way, or written by the PSI_ONLY launch after the overflow
            used = stored_psi(e, sets[name], n, dtype, False, name)
            pos = check_positions(e, p, used, 0, dtype)
        _, reference = check_density(e, p, pos, dtype, "%s call %d (slots per tile %d, store_psi %d)"
                                     % (name, call, caps[-2], store_psi), tile, reference=reference)
    print("PM zbin<float64> n=%d %s: slots per tile %s" % (n, name, caps))
    assert caps[1] > caps[0] and caps[-1] == caps[-2], caps  # an overflow was seen; grew, then settled
    e.probe_displacement_z(sets[name], 0, False, True)
    assert np.array_equal(np.array([e.fetch(k) for k in PSI]), used)
    check_density(e, p, pos, dtype, name + " after the slots settled", tile, reference=reference)
    e.probe_displacement_z(sets["uniform"], 0, False, bool(store_psi))
    e.probe_displacement_z(sets["uniform"], 0, False, True)
    upos = check_positions(e, p, stored_psi(e, sets["uniform"], n, dtype, False, "uniform after " + name), 0, dtype)
    e.probe_displacement_z(sets["uniform"], 0, False, bool(store_psi))
    check_density(e, p, upos, dtype, "uniform after %s (store_psi %d)" % (name, store_psi), tile)


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_non_finite_displacements_cost_their_pairs_of_rows(engines, precision):
    """NaN and +-inf at single sites of a few rows of `mixed`.  The forward transform spreads one over its whole packed
    pair of rows (i, j0), (i, j0 + 1) of that component and over nothing else: exactly the poisoned pairs come back
    non-finite in the stored Psi, every other row is bitwise what the clean set gives.  Those particles add nothing to
    rho and get V = 0 exactly; every other cell and particle stays inside its bound."""
    n, dtype = 128, DTYPE[precision]
    p = params(n)
    geo = ref.Geometry(n, p.L)
    e = engines(p, precision)
    tile = e.tile_info()["tile_shape"]
    clean = zbin_sets.z_position_sets(geo, dtype, tile, ("mixed",))["mixed"]
    e.probe_displacement_z(clean, 0, False, True)
    clean_used = np.array([e.fetch(k) for k in PSI]).reshape(3, n, n, n)
    psi = clean.copy().reshape(3, n, n, n)
    victims = zbin_sets.nonfinite_victims(n)
    for site, value in victims.items():
        psi[site] = value
    psi = psi.reshape(3, -1)
    e.probe_displacement_z(psi, 0, False, True)
    used = np.array([e.fetch(k) for k in PSI])
    rows = zbin_sets.poisoned_rows(victims, n)
    u4 = used.reshape(3, n, n, n)
    assert not np.any(np.isfinite(u4[rows])) and np.array_equal(u4[~rows], clean_used[~rows])
    pos = check_positions(e, p, used, 0, dtype)
    bad = ~(np.isfinite(pos[0]) & np.isfinite(pos[1]) & np.isfinite(pos[2]))
    assert np.array_equal(bad.reshape(n, n, n), np.broadcast_to(rows.any(axis=0)[:, :, None], (n, n, n)))
    label = "mixed with non-finite displacements"
    _, reference = check_density(e, p, pos, dtype, label, tile)
    assert np.all(np.isfinite(e.fetch("deltaX")))
    upload_white_data(e, p)
    e.probe_displacement_z(psi, 0, True, True)
    check_gather(e, p, pos, dtype, 0, label, reference["hist"])


def test_entry_point_refuses_where_the_engine_would_not_take_this_path(monkeypatch):
    """BCHMC_ERR_UNSUPPORTED (5) naming the reason, nothing queued, the handle as before: the evaluation in it can still
    be fetched and is unchanged."""
    psi16 = np.zeros((3, 16 ** 3))
    e = Engine(params(16))
    try:
        e.probe_displacement(psi16 - 0.25, 0, False)
        before = [e.fetch(k) for k in ("posx", "rho", "psiz")]
        with pytest.raises(BchmcError) as err:
            e.probe_displacement_z(psi16, 0, False, True)
        assert err.value.code == 5 and "128, 256 and 512" in str(err.value)
        for k, b in zip(("posx", "rho", "psiz"), before):
            assert np.array_equal(e.fetch(k), b)
        with pytest.raises(ValueError):
            e.probe_displacement_z(np.zeros(5), 0, False, True)
    finally:
        e.close()
    p = params(128)
    psi = np.zeros((3, p.N))
    for env, cfg, word in ((None, {}, "BCHMC_ZBIN_128"), ("BCHMC_NO_ZBIN", {}, "BCHMC_NO_ZBIN"),
                           ("BCHMC_ZBIN_128", {"mk": 1, "calc_h": 1}, "masskernel"),
                           ("BCHMC_ZBIN_128", {}, None)):
        monkeypatch.delenv("BCHMC_ZBIN_128", raising=False)
        monkeypatch.delenv("BCHMC_NO_ZBIN", raising=False)
        if env:
            monkeypatch.setenv(env, "1")
            monkeypatch.setenv("BCHMC_ZBIN_128", "1")
        e = Engine(params(128, **cfg))
        try:
            if word is None:
                with pytest.raises(BchmcError) as err:  # with_force needs the inputs, as in bchmc_probe_displacement
                    e.probe_displacement_z(psi, 0, True, True)
                assert err.value.code == 9
                e.probe_displacement_z(psi, 0, False, True)
                assert not np.any(e.fetch("psix")) and np.all(e.fetch("rho") > 0)
            else:
                with pytest.raises(BchmcError) as err:
                    e.probe_displacement_z(psi, 0, False, True)
                assert err.value.code == 5 and word in str(err.value), str(err.value)
                with pytest.raises(BchmcError) as err:  # nothing was evaluated
                    e.fetch("rho")
                assert err.value.code == 9
        finally:
            e.close()
