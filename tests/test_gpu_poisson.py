"""bchmc_poisson_draw / _positions / _density / _release and bchmc_setup_random_test_poisson on the GPU.

Counts: equal to the numpy restatement (tests/poisson_restatement.py) in every cell whose restatement decision margin is
at least 1e-9 -- |u - s_k| in the inversion; |us - 0.07|, |us - 0.013|, |v - v_r|, |v - us|, |lhs - rhs| and the distance of
the floor's argument from an integer in PTRS.  Cells below that ("tight") are left out; they may be 1e-4 of the cells at
most, which pr.tight asserts on the restatement alone before the device is looked at.  Positions: bitwise the
restatement's (integer Philox and two uncontracted operations).  Density: the catalogue's own checks, with the sample
in the place of the host columns.
"""
import numpy as np
import pytest

from barcode_amd import engine as eng
from barcode_amd import inputs
from barcode_amd.engine import BchmcError, Engine
from barcode_amd.gsl_mt19937 import GslMT19937
from barcode_amd.params import HamilParams
from tests import catalogue_bound as cb
from tests import catalogue_reference as cr
from tests import mock_restatement as mr
from tests import poisson_restatement as pr
from tests.test_gpu_mt19937_draw import check_state
from tests.util import Case

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED, STATE = 1, 5, 9
HANDLES = ((0, 0), (0, 1), (1, 0), (1, 1))  # (precision, deterministic)
HANDLE_IDS = ("fp64", "fp64-det", "fp32", "fp32-det")
_ENGINES = {}


def engine_of(n, precision=0, deterministic=0):
    """One handle per configuration for the module: L = n, so d = 1 (a power of two) and CIC as the handle's kernel."""
    key = (n, precision, deterministic)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(HamilParams(Nx=n, L=float(n), mk=1, calc_h=1), precision=precision, deterministic=deterministic)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def mixed_rates(n_cells, seed):
    """lambda = 0, the double below 10, 10, 1e3, 1e6, negative values and a spread over both samplers, shuffled."""
    rng = np.random.Generator(np.random.Philox(seed))
    special = np.array([0.0, np.nextafter(10.0, 0.0), 10.0, 1e3, 1e6, -2.5, -0.0, 1e-3, 9.5, 10.5, 37.5])
    lam = np.concatenate([np.tile(special, max(1, n_cells // 44)), rng.uniform(0, 25, n_cells)])[:n_cells]
    lam[: special.size] = special  # every special value is there whatever the size
    rng.shuffle(lam)
    return lam


def compare_counts(got, r, st):
    """Device counts against a restatement result outside its tight cells, and the draw's stats."""
    t = pr.tight(r)
    diff = np.flatnonzero((got != r["counts"]) & ~t)
    print("POIS counts: %d cells, %d tight, %d differ, n_part %d, max %d, PTRS iterations <= %d" %
          (got.size, t.sum(), diff.size, st["n_part"], st["max_count"], r["iters"]))
    assert diff.size == 0, (diff[:8], got[diff[:8]], r["counts"][diff[:8]])
    assert st["n_part"] == int(got.sum()) and st["max_count"] == int(got.max()) and st["n_capped"] == 0
    assert not r["capped"].any()


# ---- counts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,precision,det", [(16,) + h for h in HANDLES] + [(9, 0, 0), (9, 1, 1), (4, 0, 1), (4, 1, 0)])
def test_counts_equal_the_restatement(n, precision, det):
    e = engine_of(n, precision, det)
    lam = mixed_rates(n ** 3, 100 + n)
    r = pr.counts(lam, 4242, 5)
    got, st = e.poisson_draw(lam, seed=4242, stream=5, scale=1.0, rate_mode=1)
    compare_counts(got, r, st)
    drew = lam > 0
    assert st["n_cells_drawn"] == drew.sum() and st["lambda_max"] == lam.max()
    assert not got[~drew].any()
    # rate_mode 0 with a scale: lambda = scale (1 + x), the product formed in double
    x = lam / 7.0 - 1.0
    r0 = pr.counts(pr.rate(x, 7.0, 0), 4242, 6)
    got0, st0 = e.poisson_draw(x, seed=4242, stream=6, scale=7.0)
    compare_counts(got0, r0, st0)
    # a 64-bit seed and another stream give other counts
    big, _ = e.poisson_draw(lam, seed=(1 << 63) + 4242, stream=5, scale=1.0, rate_mode=1)
    compare_counts(big, pr.counts(lam, (1 << 63) + 4242, 5), _)
    assert not np.array_equal(big, got) and not np.array_equal(got0, got)


def test_every_handle_draws_the_same_counts():
    lam = mixed_rates(16 ** 3, 7)
    out = [engine_of(16, p, d).poisson_draw(lam, seed=11, scale=1.0, rate_mode=1)[0] for p, d in HANDLES]
    for o in out[1:]:
        assert np.array_equal(o, out[0])


@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
def test_device_sources_are_read_in_the_storage_type(precision):
    """deltaX and the chain state as the handle holds them, widened: the restatement on what bchmc_fetch /
    bchmc_chain_get_state return."""
    n = 16
    e = engine_of(n, precision, 1)
    q = 0.5 * np.asarray(inputs.make_fields(HamilParams(Nx=n, L=float(n)))["truth"])
    e.forward(q)
    dx = e.fetch("deltaX")
    got, st = e.poisson_draw(source="deltaX", seed=3, scale=6.0)
    compare_counts(got, pr.counts(pr.rate(dx, 6.0), 3, 0), st)
    e.chain_set_state(q)
    qs = e.chain_get_state()
    got, st = e.poisson_draw(seed=3, stream=1, scale=12.0, n_in=n)
    compare_counts(got, pr.counts(pr.rate(qs, 12.0), 3, 1), st)


def test_a_coarser_rate_grid():
    e = engine_of(16)
    lam = mixed_rates(8 ** 3, 21)
    got, st = e.poisson_draw(lam, seed=8, scale=1.0, rate_mode=1)
    assert got.size == 512
    compare_counts(got, pr.counts(lam, 8, 0), st)


@pytest.mark.parametrize("window_type", (10, 23))
def test_windowed_cells_only(window_type):
    """The windows of setup_random_test: type 10 closes the first N / 2 cells, type 23 opens the few cells above a
    threshold -- long runs of empty cells for the positions' search."""
    n = 16
    e = engine_of(n, 0, 0)
    N = n ** 3
    x = np.random.Generator(np.random.Philox(window_type)).normal(0.0, 1.5, N)
    window = (np.arange(N) >= N // 2).astype(np.float64) if window_type == 10 else (x > 3).astype(np.float64)
    assert 0 < window.sum() < (N if window_type == 10 else N // 40)
    e.upload(window=window)
    lam = pr.rate(x, 9.0)
    r = pr.counts(lam, 77, 2, window=window)
    got, st = e.poisson_draw(x, seed=77, stream=2, scale=9.0, use_window=True)
    compare_counts(got, r, st)
    assert not got[window == 0].any() and st["n_cells_drawn"] == ((window > 0) & (lam > 0)).sum()
    pos = e.poisson_positions(0, st["n_part"])
    for a, b in zip(pos, pr.positions(got, 77, 2, n, float(n))):
        assert np.array_equal(a, b)
    # a NaN outside the window is not looked at
    x2 = x.copy()
    x2[np.flatnonzero(window == 0)[0]] = np.nan
    got2, _ = e.poisson_draw(x2, seed=77, stream=2, scale=9.0, use_window=True)
    assert np.array_equal(got2, got)


def test_both_levels_of_the_scan():
    """128^3 cells are 2048 workgroups of 1024: two groups of k_mock_scan, so an offset is the sum of all three levels.
    lambda = 0.01 keeps the sample small; every position pins its cell's offset."""
    n = 128
    e = Engine(HamilParams(Nx=n, L=float(n), mk=1, calc_h=1))
    lam = np.full(n ** 3, 0.01)
    r = pr.counts(lam, 5, 0)
    got, st = e.poisson_draw(lam, seed=5, scale=1.0, rate_mode=1)
    compare_counts(got, r, st)
    assert got[: 2 ** 20].sum() > 0 and got[2 ** 20:].sum() > 0
    pos = e.poisson_positions(0, st["n_part"])
    for a, b in zip(pos, pr.positions(got, 5, 0, n, float(n))):
        assert np.array_equal(a, b)
    e.close()


# ---- positions ------------------------------------------------------------------------------------------------------------

def test_positions_are_bitwise_the_restatements():
    n = 9
    e = engine_of(n, 1, 0)  # doubles on every handle: an fp32 one
    lam = mixed_rates(n ** 3, 3)
    lam[lam > 100] = 50.0
    got, st = e.poisson_draw(lam, seed=31, stream=9, scale=1.0, rate_mode=1)
    ref = pr.positions(got, 31, 9, n, float(n))
    whole = e.poisson_positions(0, st["n_part"])
    for a, b in zip(whole, ref):
        assert np.array_equal(a, b)
    d = 1.0
    cells = np.repeat(np.arange(n ** 3), got.astype(np.int64))
    assert np.array_equal(np.floor(whole[2] / d), cells % n) and np.array_equal(np.floor(whole[0] / d), cells // (n * n))
    # pieces that cut through cells
    cuts = [0, 1, 7, 300, 301, 2000, st["n_part"] - 1, st["n_part"]]
    for a, b in zip(cuts[:-1], cuts[1:]):
        piece = e.poisson_positions(a, b - a)
        for col, full in zip(piece, ref):
            assert np.array_equal(col, full[a:b])
    assert e.poisson_positions(st["n_part"], 0)[0].size == 0


def test_one_full_cell_and_an_empty_sample():
    n = 16
    e = engine_of(n)
    lam = np.zeros(n ** 3)
    cell = 5 + n * (11 + n * 3)
    lam[cell] = 1e5
    got, st = e.poisson_draw(lam, seed=1, scale=1.0, rate_mode=1)
    compare_counts(got, pr.counts(lam, 1, 0), st)
    assert st["n_part"] == got[cell] and st["n_cells_drawn"] == 1 and abs(got[cell] - 1e5) < 6 * np.sqrt(1e5)
    x, y, z = e.poisson_positions(0, st["n_part"])
    for a, b in zip((x, y, z), pr.positions(got, 1, 0, n, float(n))):
        assert np.array_equal(a, b)
    assert np.all(np.floor(x) == 3) and np.all(np.floor(y) == 11) and np.all(np.floor(z) == 5)
    rho, ds = e.poisson_density(mk=0)
    assert rho[cell] == got[cell] and ds["n_in"] == st["n_part"] and np.count_nonzero(rho) == 1
    empty, st = e.poisson_draw(np.full(n ** 3, -1.0), seed=1, scale=3.0)
    assert st["n_part"] == 0 and not empty.any() and st["n_cells_drawn"] == 0 and st["lambda_max"] == 0
    assert e.poisson_positions(0, 0)[0].size == 0
    rho, ds = e.poisson_density(mk=1)
    assert not rho.any() and ds == dict(n_in=0, n_lost=0, max_per_tile=0)


# ---- density --------------------------------------------------------------------------------------------------------------

def smooth_field(n, seed):
    """A lognormal-like overdensity: mean near 0, a few cells several times the mean."""
    g = np.random.Generator(np.random.Philox(seed)).normal(0.0, 0.8, n ** 3)
    return np.exp(g - 0.32) - 1.0


@pytest.mark.parametrize("precision,det", HANDLES, ids=HANDLE_IDS)
def test_ngp_of_the_sample_is_its_counts(precision, det):
    """n_in = Nx and d = 1: every particle of cell c lands in cell c, so NGP returns the counts exactly."""
    n = 16
    e = engine_of(n, precision, det)
    x = smooth_field(n, 40)
    got, st = e.poisson_draw(x, seed=90, scale=3.0)
    if precision == 1:  # D4: the position is rounded to float first; the seed is one where no rounding leaves the cell
        cells = np.repeat(np.arange(n ** 3), got.astype(np.int64))
        for col, idx in zip(pr.positions(got, 90, 0, n, float(n)), (cells // (n * n), (cells // n) % n, cells % n)):
            assert np.array_equal(np.floor(col.astype(np.float32).astype(np.float64)), idx)
    rho, ds = e.poisson_density(mk=0)
    assert np.array_equal(rho, got) and ds["n_in"] == st["n_part"] and ds["n_lost"] == 0


@pytest.mark.parametrize("precision,det", HANDLES, ids=HANDLE_IDS)
def test_cic_of_the_sample_is_the_catalogues(precision, det):
    """Deterministic handles: bit for bit bchmc_density_particles of the fetched positions.  The others: within the
    catalogue's own bound of the longdouble reference of those positions."""
    n = 16
    e = engine_of(n, precision, det)
    got, st = e.poisson_draw(smooth_field(n, 41), seed=91, scale=3.0)
    pos = e.poisson_positions(0, st["n_part"])
    rho, ds = e.poisson_density(mk=1)
    assert ds["n_in"] == st["n_part"]
    if det:
        host, hs = e.density_particles(*pos, mk=1)
        assert np.array_equal(rho, host) and hs == ds
        e.poisson_release()
        e.catalogue_release()
        e.poisson_draw(smooth_field(n, 41), seed=91, scale=3.0, counts=False)
        assert np.array_equal(e.poisson_density(mk=1)[0], rho)
    dtype = np.float32 if precision else np.float64
    seen = [c.astype(dtype).astype(np.float64) for c in pos]
    ref = cr.density(1, seen, None, cr.Geometry(n, float(n)))
    f, i = cb.worst_fraction(rho, ref.S, cb.density_bound(ref, 1, dtype, n, deterministic=bool(det)))
    print("POIS CIC <%s%s>: worst fraction of the bound %.3f (cell %d)" % (np.dtype(dtype).name, " det" if det else "", f, i))
    assert f <= 1


def test_a_sample_longer_than_a_batch():
    """32^3 at lambda = 40: 1.3 million particles, so a cell straddles the edge of the first batch of 2^20."""
    n = 32
    e = Engine(HamilParams(Nx=n, L=float(n), mk=1, calc_h=1), deterministic=1)
    lam = np.full(n ** 3, 40.0)
    r = pr.counts(lam, 17, 0)
    got, st = e.poisson_draw(lam, seed=17, scale=1.0, rate_mode=1)
    compare_counts(got, r, st)
    off = pr.offsets(got)
    edge = int(np.searchsorted(off, 2 ** 20, side="right")) - 1
    assert st["n_part"] > 2 ** 20 and off[edge] < 2 ** 20 < off[edge + 1]  # the cell that straddles
    rho, ds = e.poisson_density(mk=0)
    assert np.array_equal(rho, got) and ds["n_in"] == st["n_part"]
    a, b = 2 ** 20 - 500, 2 ** 20 + 500
    piece = e.poisson_positions(a, b - a)
    for col, full in zip(piece, pr.positions(got, 17, 0, n, float(n), first=a, m=b - a)):
        assert np.array_equal(col, full)
    pos = e.poisson_positions(0, st["n_part"])
    cic, _ = e.poisson_density(mk=1)
    assert np.array_equal(cic, e.density_particles(*pos, mk=1)[0])
    e.close()


def test_up_resolving_conserves_the_particles():
    """n_in = 8 into Nx = 16, CIC (poisson_upres.cc end to end): every particle's eight weights add to 1 up to their
    roundings and the 2^-46 of the fixed point, so |sum - n_part| <= n_part 2^-40 with room to spare."""
    n = 16
    e = engine_of(n, 0, 1)
    field = smooth_field(8, 42)
    got, st = e.poisson_draw(field, seed=92, scale=8.0)
    assert got.size == 512
    compare_counts(got, pr.counts(pr.rate(field, 8.0), 92, 0), st)
    rho, ds = e.poisson_density(mk=1)
    assert ds["n_in"] == st["n_part"] and ds["n_lost"] == 0
    assert abs(rho.sum() - st["n_part"]) <= st["n_part"] * 2.0 ** -40
    x, y, z = e.poisson_positions(0, st["n_part"])
    for a, b in zip((x, y, z), pr.positions(got, 92, 0, 8, float(n))):
        assert np.array_equal(a, b)


def test_hamil_names_follow_the_engine():
    from barcode_amd import hamil
    n = 16
    hd = hamil.HamilData(HamilParams(Nx=n, L=float(n), mk=1, calc_h=1))
    field = smooth_field(8, 43)
    x, y, z, st = hamil.discrete_poisson_sample(hd, field, 4.0, 55)
    cnt = pr.counts(pr.rate(field, 4.0), 55, 0)["counts"]
    assert st["n_part"] == cnt.sum() == x.size
    for a, b in zip((x, y, z), pr.positions(cnt, 55, 0, 8, float(n))):
        assert np.array_equal(a, b)
    rho, st2 = hamil.poisson_upres(hd, field, 4.0, 55)
    # float atomics in double: every weight and every add is within 2^-53 relative, far inside the bound of
    # test_up_resolving_conserves_the_particles
    assert st2["n_in"] == st["n_part"] and abs(rho.sum() - st["n_part"]) <= st["n_part"] * 2.0 ** -40
    hd.engine.close()


def test_cpp_shim_follows_the_engine():
    """bchmc_shim::discrete_poisson_sample / poisson_upres / setup_random_test with its seed: the engine's numbers."""
    from barcode_amd import shim
    n = 16
    p = HamilParams(Nx=n, L=float(n), mk=1, calc_h=1)
    ones = np.ones(p.N)
    sh = shim.ShimHamil(p, signal_PS=ones, mass_f=ones)
    sh.hd.deterministic = 1
    field = smooth_field(8, 44)
    lam = pr.rate(field, 5.0)
    cnt = pr.counts(lam, 66, 1)["counts"]
    xyz = sh.discrete_poisson_sample(lam, 66, stream=1)
    assert xyz.shape == (cnt.sum(), 3)
    for col, ref in zip(xyz.T, pr.positions(cnt, 66, 1, 8, float(n))):
        assert np.array_equal(col, ref)
    e = engine_of(n, 0, 1)
    e.poisson_draw(field, seed=66, stream=1, scale=5.0, counts=False)
    assert np.array_equal(sh.poisson_upres(field, 5.0, 66, stream=1), e.poisson_density(mk=1)[0])
    assert np.array_equal(sh.poisson_upres(field, 5.0, 66, mk=0, stream=1), e.poisson_density(mk=0)[0])
    with pytest.raises(shim.ShimError):
        sh.discrete_poisson_sample(np.zeros(17 ** 3), 1)
    sh.close()
    # the mock: the engine's arrays, and the caller's copies of window / nobs / noise receive them
    pm = mr.params(n, likelihood=0)
    P = mr.power(pm)
    own = {k: np.full(pm.N, -7.) for k in ("window", "nobs", "noise")}
    hs = shim.ShimHamil(pm, signal_PS=P, mass_f=inputs.inverse_power_mass(P), **own)
    hs.hd.deterministic = 1
    ep = Engine(pm, deterministic=1)
    ep.upload(signal_PS=P, mass_f=inputs.inverse_power_mass(P))
    r1, r2 = GslMT19937(8), GslMT19937(8)
    with pytest.raises(shim.ShimError, match="Poissonian"):
        hs.setup_random_test(r1)  # without the seed: refused as before
    dl, de = hs.setup_random_test(r1, poisson_seed=21, poisson_stream=4)
    _, dl_e, de_e = ep.setup_random_test_poisson(r2, 21, stream=4)
    assert np.array_equal(dl, dl_e) and np.array_equal(de, de_e)
    assert r1.get_state()[1] == r2.get_state()[1] and np.array_equal(r1.get_state()[0], r2.get_state()[0])
    kept = hs._keep
    assert np.array_equal(kept["nobs"], ep.fetch("nobs")) and kept["nobs"].sum() > 0
    assert np.array_equal(kept["window"], np.ones(pm.N)) and not kept["noise"].any()
    hs.close(), ep.close()


# ---- state ----------------------------------------------------------------------------------------------------------------

def test_draw_and_density_leave_the_state_alone():
    """D6 across draw and density, with a proposal pending: chain state, momenta, proposal, deltaX and the rest bit for
    bit, and the next attempt returns the dH of a twin that never called."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)

    def run(call):
        e = Engine(c.p, deterministic=1)
        e.upload(**c.arrays())
        e.chain_set_state(c.q0)
        e.chain_set_momenta(c.p0)
        e.chain_attempt(c.eps, 3)
        keys = ("deltaX", "rho", "posx", "posy", "posz", "psix", "nobs", "window")
        before = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + tuple(e.fetch(k) for k in keys)
        info = e.tile_info()
        if call:
            _, st = e.poisson_draw(c.truth, seed=5, scale=2.0)
            e.poisson_draw(source="chain", seed=5, scale=2.0, use_window=True)
            e.poisson_draw(source="deltaX", seed=5, scale=2.0)
            for mk in (0, 1, 2, 3):
                e.poisson_density(mk=mk)
            e.poisson_positions(0, 10)
            e.poisson_release()
        after = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + tuple(e.fetch(k) for k in keys)
        assert all(np.array_equal(a, b) for a, b in zip(before, after)) and e.tile_info() == info
        e.chain_accept(True)
        e.chain_set_momenta(0.9 * c.p0)
        dH, terms, done = e.chain_attempt(c.eps, 3)
        e.close()
        return dH, terms, done

    plain, called = run(False), run(True)
    assert plain[0] == called[0] and np.array_equal(plain[1], called[1]) and plain[2] == called[2] == 3


def test_buffers_are_counted_released_and_the_sample_reproduced():
    e = engine_of(16, 0, 1)
    lam = np.minimum(mixed_rates(16 ** 3, 9), 100.0)  # some 1e5 particles: their columns pass 1 MiB
    # the handle's transfer staging (pinned chunks and their events) is taken by its first transfer above 1 MiB and kept:
    # one fetch of this size beforehand, so that what is counted below is the feature's own
    e.poisson_positions(0, e.poisson_draw(lam, seed=2, scale=1.0, rate_mode=1)[1]["n_part"])
    e.poisson_release()
    e.catalogue_release()
    start = eng.live_resources()
    got, st = e.poisson_draw(lam, seed=2, scale=1.0, rate_mode=1)
    held = eng.live_resources()
    assert held[0] > start[0] and held[1] >= start[1] + 8 * (16 ** 3 + 1)
    pos = e.poisson_positions(0, st["n_part"])
    assert eng.live_resources()[0] == held[0] + 1  # the batch of positions, taken by the first fetch
    e.poisson_draw(lam[:512], seed=2, scale=1.0, rate_mode=1)  # another n_in replaces the scan's buffers
    e.poisson_release()
    assert eng.live_resources() == start
    with pytest.raises(BchmcError) as err:
        e.poisson_positions(0, 1)
    assert err.value.code == STATE
    again, st2 = e.poisson_draw(lam, seed=2, scale=1.0, rate_mode=1)
    assert np.array_equal(again, got) and st2 == st
    for a, b in zip(e.poisson_positions(0, st["n_part"]), pos):
        assert np.array_equal(a, b)
    e.poisson_release()
    assert eng.live_resources() == start


def test_nobs_from_a_draw_is_an_uploaded_nobs():
    c = Case(Nx=16, likelihood=0)
    e, twin = (Engine(c.p, deterministic=1) for _ in range(2))
    arrays = c.arrays()
    for h in (e, twin):
        h.upload(**arrays)
    got, _ = e.poisson_draw(c.truth, seed=12, scale=c.p.rho_c, to_nobs=True)
    assert np.array_equal(e.fetch("nobs"), got)
    twin.upload(nobs=got)
    assert np.array_equal(e.gradient(c.q0), twin.gradient(c.q0))
    e.close(), twin.close()


# ---- the Poissonian mock ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window_type,rsd", ((1, False), (10, True), (23, False)))
def test_poissonian_mock(window_type, rsd):
    """Truth, forward model, window and the generator: bchmc_setup_random_test's on a Gaussian handle from the same seed.
    nobs: the restatement on the fetched deltaX.  noise: 0.  Then an attempt runs on the likelihood = 0 handle."""
    n, seed = 16, 2
    pg, pp = mr.params(n, likelihood=1), mr.params(n, likelihood=0)
    P = mr.power(pp)
    mass_f = inputs.inverse_power_mass(P)
    eg, ep = Engine(pg, deterministic=1), Engine(pp, deterministic=1)
    for h in (eg, ep):
        h.upload(signal_PS=P, mass_f=mass_f)
    rg, rp = GslMT19937(seed), GslMT19937(seed)
    rg.raw(5), rp.raw(5)
    before = rp.copy()
    _, dl_g, de_g = eg.setup_random_test(rg, window_type=window_type, random_test_rsd=rsd)
    used, dl, de = ep.setup_random_test_poisson(rp, 1234, stream=3, window_type=window_type, random_test_rsd=rsd)
    assert np.array_equal(dl, dl_g) and np.array_equal(de, de_g)
    window = ep.fetch("window")
    assert np.array_equal(window, eg.fetch("window"))
    check_state(before, used, rp)  # the generator advanced by the truth's words only ...
    twin = before.copy()
    assert eg.make_initial_guess(twin, 2) == used  # ... which are create_GARFIELD's 2 N Gaussians
    dx = ep.fetch("deltaX")
    assert np.array_equal(dx, de)
    r = pr.counts(pr.rate(dx, pp.rho_c), 1234, 3, window=window)
    nobs = ep.fetch("nobs")
    t = pr.tight(r)
    assert np.array_equal(nobs[~t], r["counts"][~t]) and not nobs[window == 0].any()
    assert nobs.sum() > 0 and not ep.fetch("noise").any()
    ep.chain_set_state(0.5 * dl)
    ep.chain_draw_momenta(7, 0)
    dH, terms, done = ep.chain_attempt(0.02 * pp.eps_heuristic(), 3)
    assert np.isfinite(dH) and np.all(np.isfinite(terms)) and done == 3
    eg.close(), ep.close()


def test_mock_module_takes_the_seed():
    from barcode_amd import hamil, mock
    p = mr.params(16, likelihood=0)
    P = mr.power(p)
    hd = hamil.HamilData(p, signal_PS=P, mass_f=inputs.inverse_power_mass(P))
    rng = GslMT19937(4)
    state = rng.get_state()
    with pytest.raises(BchmcError) as err:  # without the seed: refused as before
        mock.load_initial_fields(hd, rng, mock.MockParams(likelihood=0))
    assert err.value.code == UNSUPPORTED and "Poissonian" in str(err.value)
    assert rng.get_state()[1] == state[1] and np.array_equal(rng.get_state()[0], state[0])
    mock.load_initial_fields(hd, rng, mock.MockParams(likelihood=0, poisson_seed=99))
    nobs = hd.engine.fetch("nobs")
    r = pr.counts(pr.rate(hd.engine.fetch("deltaX"), p.rho_c), 99, 0)
    t = pr.tight(r)
    assert np.array_equal(nobs[~t], r["counts"][~t])
    hd.engine.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------

def refused(code, call, *a, **kw):
    with pytest.raises(BchmcError) as err:
        call(*a, **kw)
    assert err.value.code == code, str(err.value)
    return str(err.value)


def test_refusals_leave_a_usable_handle():
    n = 16
    N = n ** 3
    e = Engine(HamilParams(Nx=n, L=float(n), mk=1, calc_h=1))
    lam = np.full(N, 2.0)
    refused(STATE, e.poisson_positions, 0, 0)
    refused(STATE, e.poisson_density, mk=1)
    refused(STATE, e.poisson_draw, seed=1)                       # no chain state
    refused(STATE, e.poisson_draw, source="deltaX", seed=1)      # no forward model
    refused(STATE, e.poisson_draw, lam, seed=1, use_window=True)  # no window
    refused(ARG, e.poisson_draw, lam, seed=1, source="chain")    # a signal with a device source
    refused(ARG, e.poisson_draw, lam, seed=1, stream=1 << 31)
    refused(ARG, e.poisson_draw, lam, seed=1, rate_mode=2)
    refused(ARG, e.poisson_draw, lam, seed=1, scale=np.inf)
    refused(ARG, e.poisson_draw, np.zeros(17 ** 3), seed=1)      # n_in > Nx
    dp = eng.C.POINTER(eng.C.c_double)
    o = eng.PoissonOpts(1, 0, 1, 1.0, 0, -1)
    assert e.lib.bchmc_poisson_draw(e.h, 0, lam.ctypes.data_as(dp), 0, eng.C.byref(o), None, None) == ARG  # n_in = 0, host
    assert "n_in = 0" in e.lib.bchmc_last_error(e.h).decode()
    assert e.lib.bchmc_poisson_draw(e.h, 0, None, n, eng.C.byref(o), None, None) == ARG  # a host source without its signal
    assert "signal" in e.lib.bchmc_last_error(e.h).decode()
    e.upload(window=np.ones(N))
    refused(ARG, e.poisson_draw, lam[:512], seed=1, use_window=True)  # n_in != Nx
    refused(ARG, e.poisson_draw, lam[:512], seed=1, to_nobs=True)
    e.chain_set_state(np.zeros(N))
    refused(ARG, e.poisson_draw, seed=1, n_in=8)                 # a device source is Nx^3
    o = eng.PoissonOpts(1, 0, 0, 1.0, 0, 2)
    assert e.lib.bchmc_poisson_draw(e.h, 1, None, 0, eng.C.byref(o), None, None) == ARG   # dest
    assert e.lib.bchmc_poisson_draw(e.h, 1, None, 0, None, None, None) == ARG             # opts
    # a rate that cannot be drawn: the first such cell is named, nothing is kept or made nobs
    good, st = e.poisson_draw(lam, seed=1, scale=1.0, rate_mode=1)
    e.upload(nobs=np.full(N, 7.0))
    for badval in (np.nan, np.inf, 2.0 ** 30 * 1.001):
        bad = lam.copy()
        bad[[3000, 1234]] = badval
        counts = np.full(N, -5.0)
        dp = eng.C.POINTER(eng.C.c_double)
        o = eng.PoissonOpts(1, 0, 1, 1.0, 0, eng.F_NOBS)
        rc = e.lib.bchmc_poisson_draw(e.h, 0, bad.ctypes.data_as(dp), n, eng.C.byref(o), counts.ctypes.data_as(dp), None)
        assert rc == ARG and "cell 1234" in e.lib.bchmc_last_error(e.h).decode()
        assert np.all(counts == -5.0) and np.all(e.fetch("nobs") == 7.0)
        refused(STATE, e.poisson_positions, 0, 0)
    bad = lam.copy()
    bad[5] = -np.inf  # lambda <= 0: a count of 0, as GSL
    got, _ = e.poisson_draw(bad, seed=1, scale=1.0, rate_mode=1)
    assert got[5] == 0 and np.array_equal(np.delete(got, 5), np.delete(good, 5))
    # positions and density
    refused(ARG, e.poisson_positions, 0, int(got.sum()) + 1)
    refused(ARG, e.poisson_positions, int(got.sum()), 1)
    assert e.lib.bchmc_poisson_positions(e.h, 0, 1, None, None, None) == ARG
    for kw in (dict(mk=4), dict(kernel_h=-1.0), dict(kernel_h=n)):
        refused(ARG, e.poisson_density, **kw)
    dopts = eng.DensityOpts(1, 1, 0.0, -1, 0)
    out = np.empty(N)
    assert e.lib.bchmc_poisson_density(e.h, eng.C.byref(dopts), out.ctypes.data_as(eng.C.POINTER(eng.C.c_double)), None) == ARG
    assert "weightmass" in e.lib.bchmc_last_error(e.h).decode()
    dopts = eng.DensityOpts(1, 0, 0.0, -1, 0)
    assert e.lib.bchmc_poisson_density(e.h, eng.C.byref(dopts), None, None) == ARG  # nowhere to put the field
    # the existing entry point still refuses the internal source
    assert e.lib.bchmc_density_particles(e.h, 2, None, None, None, None, 0, eng.C.byref(dopts),
                                         out.ctypes.data_as(eng.C.POINTER(eng.C.c_double)), None) == ARG
    rho, ds = e.poisson_density(mk=0)  # and the handle works
    assert np.array_equal(rho, got)
    e.close()


def test_a_sample_beyond_32_bits():
    """Three cells at lambda = 2^30 hold more than 2^31 particles: the scan and stats.n_part are 64-bit, a position past
    2^32 is the restatement's, and bchmc_poisson_density refuses the sample (the catalogue's n_part <= 2^31 - 1) and
    leaves the handle usable."""
    n = 16
    e = engine_of(n, 0, 1)
    lam = np.full(n ** 3, 0.5)
    lam[[7, 2000, 4095]] = 2.0 ** 30
    lam[[8, 4000]] = 2.0 ** 30 - 1e3
    r = pr.counts(lam, 13, 0)
    got, st = e.poisson_draw(lam, seed=13, scale=1.0, rate_mode=1)
    compare_counts(got, r, st)
    assert st["n_part"] > 2 ** 32 and st["max_count"] > 2 ** 30 - 10 ** 6 and st["lambda_max"] == 2.0 ** 30
    for first in (2 ** 31 - 3, 2 ** 32 - 3, st["n_part"] - 6):  # slices across 2^31, 2^32 and the end
        piece = e.poisson_positions(first, 6)
        for col, ref in zip(piece, pr.positions(got, 13, 0, n, float(n), first=first, m=6)):
            assert np.array_equal(col, ref)
    assert "2^31 - 1" in refused(ARG, e.poisson_density, mk=1)
    small, st = e.poisson_draw(np.minimum(lam, 3.0), seed=13, scale=1.0, rate_mode=1)
    rho, ds = e.poisson_density(mk=0)
    assert np.array_equal(rho, small) and ds["n_in"] == st["n_part"]


def test_mock_refusals_are_those_of_setup_random_test():
    n = 16
    for like, kw, code, text in ((1, dict(), ARG, "likelihood = 1"), (2, dict(), ARG, "likelihood = 2"),
                                 (0, dict(window_type=2), ARG, "window_type"), (0, dict(stream=1 << 31), ARG, "stream")):
        p = mr.params(n, likelihood=like)
        e = Engine(p)
        e.upload(signal_PS=mr.power(p))
        rng = GslMT19937(3)
        rng.raw(17)
        before = rng.get_state()
        assert text in refused(code, e.setup_random_test_poisson, rng, 1, **kw)
        after = rng.get_state()
        assert before[1] == after[1] and np.array_equal(before[0], after[0])  # the caller's generator is untouched
        e.close()
    p = mr.params(n, likelihood=0)
    e = Engine(p)
    assert "signal_PS" in refused(STATE, e.setup_random_test_poisson, GslMT19937(3), 1)
    o = eng.MockOpts(1, 1, 0, 0, 1.0, 0.0)  # data_model 1
    mt, mti = GslMT19937(3).get_state()
    mt = np.ascontiguousarray(mt, dtype=np.uint32)
    m = eng.C.c_int32(int(mti))
    rc = e.lib.bchmc_setup_random_test_poisson(e.h, eng.C.byref(o), mt.ctypes.data_as(eng.C.POINTER(eng.C.c_uint32)),
                                               eng.C.byref(m), None, 1, 0, None, None)
    assert rc == ARG and "data_model = 1" in e.lib.bchmc_last_error(e.h).decode()
    e.close()
    odd = Engine(mr.params(9, likelihood=0))
    odd.upload(signal_PS=mr.power(mr.params(9, likelihood=0)))
    assert "even Nx" in refused(UNSUPPORTED, odd.setup_random_test_poisson, GslMT19937(3), 1)
    odd.close()
