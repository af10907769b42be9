"""Every cell of every tile image, written by a flush and read by a gather: the index arithmetic of the tile kernels'
fills and flushes (barcode_amd/csrc/tile_walk.hpp; tests/test_tile_walk_cpu.py proves the walker itself on the CPU).

One particle sits in every cell of the grid, at a seeded offset inside the cell.  Every image cell of every tile -- the
halo included, across all six periodic faces -- then receives mass that its flush must put into the right global cell,
and is a part_like value that its fill must have fetched from the right global cell.  Through
bchmc_probe_displacement, against the longdouble reference of tests/pm_reference.py under the bounds of
tests/pm_bound.py (their derivation is there; nothing is added to them here):

    16^3, 32^3, 48^3    k_scatter_tile81 / k_gather_tile81, float64 and float32 (16^3: the halo wraps onto the tile)
    24^3                k_scatter_tile / k_gather_tile (8 x 8 x 8 tiles)
    32^3 with mk = 1    k_scatter_tile_low (CIC; the 10 x 10 x 18 image)
    12^3                k_scatter_tile / k_gather_tile (4 x 4 x 4 tiles, 27 of them)
    4^3                 the same with ONE 4 x 4 x 4 tile, float64 and float32: the halo (R = 2) wraps onto the tile on all
                        three axes, the 8 x 8 x 8 image is (2 n)^3 and holds every global cell 8 times; and with mk = 1

rho cell by cell and V particle by particle must be under the bound, what the reference leaves empty must be exactly 0,
and with deterministic=1 two fresh handles must give identical rho and V.  The reference density of a case is computed
once and shared by its tests.
"""
import functools

import numpy as np
import pytest

from barcode_amd.engine import Engine
from barcode_amd.params import HamilParams
from tests import pm_bound
from tests import pm_reference as ref

pytestmark = pytest.mark.gpu

DTYPE = {0: np.float64, 1: np.float32}
# (n, mk, precision, kernel family)
CASES = [(16, 3, 0, "tile81"), (16, 3, 1, "tile81"), (32, 3, 0, "tile81"), (32, 3, 1, "tile81"), (48, 3, 0, "tile81"),
         (48, 3, 1, "tile81"), (24, 3, 0, "tile"), (32, 1, 0, "tile_low"),
         (4, 3, 0, "tile"), (4, 3, 1, "tile"), (12, 3, 0, "tile"), (4, 1, 0, "tile_low")]
IDS = ["n%d-mk%d-%s" % (n, mk, ("fp64", "fp32")[pr]) for n, mk, pr, _ in CASES]


def params(n, mk):
    return HamilParams(Nx=n, L=200.0 * n / 64.0, likelihood=1, mk=mk, calc_h=2 if mk == 3 else 1, rsd_model=0,
                       particle_kernel_h_rel=1.0)


def engine(p, precision, deterministic=0):
    e = Engine(p, precision=precision, deterministic=deterministic)
    ones = np.ones(p.N)
    e.upload(signal_PS=ones, mass_f=ones, mass_r=ones)
    return e


def family(info, mk):
    if mk != 3:
        return "tile_low" if info["tiled"] else "direct"
    return "tile81" if info["unrolled81"] else ("tile" if info["tiled"] else "direct")


@functools.lru_cache(maxsize=None)
def one_per_cell(n):
    """psi (3, N): particle p = k + n (j + n i) goes to (i + u, j + v, k + w) d with u, v, w in [0.05, 0.95): inside its
    own cell in float32 as in float64, well away from the faces."""
    rng = np.random.Generator(np.random.Philox(1000 + n))
    d = 200.0 / 64.0
    psi = (0.05 + 0.9 * rng.random((3, n ** 3)) - 0.5) * d
    psi.setflags(write=False)
    return psi


@functools.lru_cache(maxsize=None)
def reference_density(n, mk, precision):
    """(pos, S, cnt) of the case: the positions in the storage type (the engine's are compared bitwise with them), the
    exact density and the per-cell particle counts.  Read-only, shared."""
    dtype = DTYPE[precision]
    p = params(n, mk)
    geo = ref.Geometry(n, p.L)
    pos = [c.astype(np.float64) for c in ref.positions(one_per_cell(n), geo, 0, dtype)]
    hc = [ref.home_cell(c, geo.d, dtype) for c in pos]
    assert np.array_equal(hc[2] + n * (hc[1] + n * hc[0]), np.arange(geo.N)), "one particle in every cell"
    if mk == 3:
        S, cnt, _ = ref.sph_density(pos, geo, p.particle_kernel_h, pm_bound.q_slack(dtype, n, 1.0), dtype)
    else:
        S, cnt, _ = ref.cic_density(pos, geo)
    for a in pos + [S, cnt]:
        a.setflags(write=False)
    return pos, S, cnt


def density_bound(p, S, cnt, dtype, deterministic):
    if p.mk == 3:
        w_norm = 1.0 / np.pi / p.particle_kernel_h ** 3
        return pm_bound.density_bound(S, cnt, dtype, p.Nx, 1.0, w_norm, deterministic)
    return pm_bound.density_bound(S, cnt, dtype, p.Nx, 1.0, 1.0, deterministic, kind="low")


def upload_white_data(e, p, seed=11):
    """The white-data recipe of tests/test_gpu_particle_mesh.py: Gaussian likelihood data for which part_like = (nobs -
    Lambda) / sigma^2 is white with both signs wherever the window is open; the window has holes."""
    rng = np.random.Generator(np.random.Philox(seed))
    dX = e.fetch("deltaX")
    window = (rng.random(p.N) >= 0.2).astype(np.float64)
    noise = np.full(p.N, 0.5)
    lam = window * p.rho_c * (1.0 + p.biasP * dX)
    nobs = lam + noise ** 2 * rng.standard_normal(p.N)
    e.upload(window=window, noise=noise, nobs=nobs)


def run(n, mk, precision, fam, deterministic):
    """One fresh handle: (rho, V or None, part_like or None), positions checked bitwise on the way."""
    p = params(n, mk)
    pos, _, _ = reference_density(n, mk, precision)
    psi = one_per_cell(n)
    e = engine(p, precision, deterministic)
    assert family(e.tile_info(), mk) == fam, e.tile_info()
    e.probe_displacement(psi, 0, False)
    for k, want in zip(("posx", "posy", "posz"), pos):
        assert np.array_equal(e.fetch(k), want), k
    rho = e.fetch("rho")
    V = pl = None
    if mk == 3:
        upload_white_data(e, p)
        e.probe_displacement(psi, 0, True)
        pl = e.fetch("part_like")
        V = np.array([e.fetch(k) for k in ("Vx", "Vy", "Vz")])
    e.close()
    return rho, V, pl


def check_rho(n, mk, precision, rho, deterministic, label):
    dtype = DTYPE[precision]
    p = params(n, mk)
    _, S, cnt = reference_density(n, mk, precision)
    f, i = pm_bound.worst_fraction(rho, S, density_bound(p, S, cnt, dtype, deterministic))
    print("tile image %s n=%d mk=%d %s: rho worst fraction of the bound %.3f (cell %d = (%d, %d, %d), cnt %d, rho %.17g, "
          "reference %.17g)" % (label, n, mk, np.dtype(dtype).name, f, i, i // (n * n), (i // n) % n, i % n, cnt[i],
                                rho[i], float(S[i])))
    assert f <= 1
    assert not np.any(rho[cnt == 0])
    if mk == 3:
        assert np.all(cnt > 0)  # every cell, so every image cell of every tile, was flushed into


def check_V(n, precision, V, pl, label):
    dtype = DTYPE[precision]
    p = params(n, 3)
    geo = ref.Geometry(n, p.L)
    pos, _, _ = reference_density(n, 3, precision)
    nnz = np.count_nonzero(pl)  # both signs among the open cells; holes
    assert nnz > 0 and (pl > 0).sum() >= nnz // 5 and (pl < 0).sum() >= nnz // 5 and (pl == 0).any()
    Vr, A, P, m = ref.sph_adjoint_gather(pos, pl, geo, p.particle_kernel_h, p.rho_c, False, 0.0,
                                         pm_bound.q_slack(dtype, n, 1.0), dtype)
    bound = pm_bound.gather_bound(A, P, m, dtype, n, 1.0, 1.0 / (np.pi * p.particle_kernel_h ** 4), 1.0)
    f, i = pm_bound.worst_fraction(V, Vr, bound)
    q = i % p.N
    print("tile image %s n=%d %s: V worst fraction of the bound %.3f (component %d of particle %d, %d cells, V %.17g, "
          "reference %.17g)" % (label, n, np.dtype(dtype).name, f, i // p.N, q, m[q], V.ravel()[i], float(Vr.ravel()[i])))
    assert f <= 1
    assert not np.any(V[:, m == 0])


@pytest.mark.parametrize("n,mk,precision,fam", CASES, ids=IDS)
def test_every_image_cell_is_flushed_and_gathered_inside_the_bound(n, mk, precision, fam):
    rho, V, pl = run(n, mk, precision, fam, 0)
    check_rho(n, mk, precision, rho, False, fam)
    if mk == 3:
        check_V(n, precision, V, pl, fam)


@pytest.mark.parametrize("n,mk,precision,fam", CASES, ids=IDS)
def test_deterministic_mode_repeats_bitwise_on_fresh_handles(n, mk, precision, fam):
    a = run(n, mk, precision, fam, 1)
    b = run(n, mk, precision, fam, 1)
    check_rho(n, mk, precision, a[0], True, fam + " deterministic")
    assert np.array_equal(a[0], b[0]), "rho"
    if mk == 3:
        assert np.array_equal(a[2], b[2]), "part_like"
        assert np.array_equal(a[1], b[1]), "V"
        assert np.all(np.isfinite(a[1])) and np.any(a[1])
