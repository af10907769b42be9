"""Host side of tests/test_gpu_zbin_positions.py, kept apart so that tests/test_pm_bounds.py can check it without a GPU:
which counter of k_zbin_direct (zpass.hpp) a position falls into, how many distinct counter pairs a workgroup meets, the
position sets made for that kernel's hash table, and the cells and particles the longdouble reference is evaluated on.

A workgroup of k_zbin_direct owns the 2 x 2 x n column (i0 + f, j0 + e, :) of the Lagrangian lattice, 4 n particles.  A
particle's counter is key = tile * 8 + octant (tile of its home cell, tile sides from bchmc_tile_info; octant: position of
the three "upper half of the cell" bits b = 4 bx + 2 by + bz in the Gray sequence, b ^ (b >> 1) ^ (b >> 2)); the kernel's
table is keyed on the pair key >> 1, whose two counters differ in bz only, and has 4 n slots.
"""
import numpy as np

from tests import pm_reference as ref


def z_constant(psi, n):
    """The displacement of the plane k = 0 repeated along z: constant along every z row."""
    p = np.asarray(psi, dtype=np.float64).reshape(3, n, n, n)
    return np.ascontiguousarray(np.broadcast_to(p[:, :, :, :1], p.shape)).reshape(3, -1)


def workgroup_index(n):
    """Workgroup (i // 2) (n / 2) + j // 2 of every particle p = k + n (j + n i)."""
    i, j, _ = ref.lattice_index(n)
    return (i // 2) * (n // 2) + j // 2


def counter_keys(pos, geo, tile_shape, dtype):
    """tile * 8 + octant per particle as k_zbin_direct forms it, -1 for a non-finite position.  The home cell is
    pm_reference's; the sub-cell bits are those of x * (1 / d) in the storage type."""
    n = geo.n
    T = np.dtype(dtype).type
    tx, ty, tz = tile_shape
    fin = np.isfinite(pos[0]) & np.isfinite(pos[1]) & np.isfinite(pos[2])
    key = np.full(len(pos[0]), -1, dtype=np.int64)
    x = [np.asarray(c, dtype=np.float64)[fin] for c in pos]
    hc = [ref.home_cell(c, geo.d, dtype) % n for c in x]
    tile = (hc[2] // tz) + (n // tz) * ((hc[1] // ty) + (n // ty) * (hc[0] // tx))
    inv_d = T(1) / T(geo.d)
    b = np.zeros(len(tile), dtype=np.int64)
    for c, bit in zip(x, (4, 2, 1)):
        f = c.astype(dtype) * inv_d
        b |= np.where(f - np.floor(f) >= T(0.5), bit, 0)
    key[fin] = tile * 8 + (b ^ (b >> 1) ^ (b >> 2))
    return key


def distinct_pairs_per_workgroup(key, n):
    """Number of distinct counter pairs key >> 1 among the binned particles (key >= 0) of each of the (n / 2)^2
    workgroups."""
    wg = workgroup_index(n)
    ok = key >= 0
    npair = int(key.max()) // 2 + 1 if ok.any() else 1
    both = np.unique(wg[ok] * npair + (key[ok] >> 1))
    return np.bincount(both // npair, minlength=(n // 2) ** 2)


def pair_halves_per_workgroup(key, n):
    """(workgroup * npair + pair, particles in the even counter, particles in the odd one) for every pair a workgroup
    uses."""
    wg = workgroup_index(n)
    ok = key >= 0
    npair = int(key.max()) // 2 + 1
    code = wg[ok] * npair + (key[ok] >> 1)
    pairs, inv = np.unique(code, return_inverse=True)
    odd = (key[ok] & 1).astype(bool)
    return pairs, np.bincount(inv[~odd], minlength=len(pairs)), np.bincount(inv[odd], minlength=len(pairs))


# the sets whose rows are constant along z: they pass both z transforms exactly (tests/fft_bound.py)
EXACT_SETS = ("lattice",) + ref.SPECIAL_SETS + ("upper_edge_zc", "tiny_negative_zc", "far_out_zc", "both_halves")
VARYING_SETS = ("uniform", "mixed", "scrambled", "one_counter", "collapse_inside", "collapse_corner")


def z_position_sets(geo, dtype, tile_shape, names, seed=77):
    """name -> psi (3, N).  pm_reference's sets under their names, `<set>_zc` and the four SPECIAL_SETS in the z-constant
    form (`faces` picks its axis from the particle index, which runs along z), and the sets of this file:

    lattice      no displacement;
    scrambled    every particle to an independent uniform position in the box: a workgroup's 4 n particles meet about
                 4 n distinct counter pairs;
    one_counter  the 4 n particles of workgroup w go into the central cell of tile w mod ntiles, sub-cell octant bits
                 w div ntiles, spread over 0.3 d inside that octant: one counter per workgroup, no two alike;
    both_halves  the four rows of a workgroup share one (x, y) of their own, stay in their z cells, and sit on z = the cell
                 centre, the boundary between the two counters of a pair (rows j even: on it, the upper counter; rows j
                 odd: 2^-10 d below it): every pair a workgroup uses holds 2 tz particles in either half."""
    n, d, L, N = geo.n, geo.d, geo.L, geo.N
    tx, ty, tz = tile_shape
    rng = np.random.Generator(np.random.Philox(seed))
    c0 = np.array(ref.lattice_centres(geo, np.float64))
    i, j, _ = ref.lattice_index(n)
    wg = workgroup_index(n)
    nwg = (n // 2) ** 2
    out = {}
    for name in names:
        if name == "lattice":
            psi = np.zeros((3, N))
        elif name in ref.SPECIAL_SETS:
            psi = z_constant(ref.position_sets(geo, dtype, names=(name,))[name], n)
        elif name.endswith("_zc"):
            psi = z_constant(ref.position_sets(geo, dtype, names=(name[:-3],))[name[:-3]], n)
        elif name == "scrambled":
            psi = rng.random((3, N)) * L - c0
        elif name == "one_counter":
            ntiles = (n // tx) * (n // ty) * (n // tz)
            assert nwg <= 8 * ntiles
            w = np.arange(nwg)
            t, b = w % ntiles, w // ntiles
            cell = [((t // ((n // tz) * (n // ty))) * tx + tx // 2), (((t // (n // tz)) % (n // ty)) * ty + ty // 2),
                    ((t % (n // tz)) * tz + tz // 2)]
            psi = np.empty((3, N))
            for a, bit in enumerate((4, 2, 1)):
                lo = (cell[a] + 0.1 + 0.5 * ((b & bit) != 0)) * d
                psi[a] = lo[wg] + 0.3 * d * rng.random(N) - c0[a]
        elif name == "both_halves":
            xy = (rng.integers(0, n, size=(2, nwg)) + 0.2 + 0.6 * rng.random((2, nwg))) * d
            psi = np.zeros((3, N))
            psi[0] = xy[0][wg] - c0[0]
            psi[1] = xy[1][wg] - c0[1]
            psi[2, j % 2 == 1] = -d * 2.0 ** -10
        else:
            psi = ref.position_sets(geo, dtype, names=(name,))[name]
        out[name] = psi
    return out


def nonfinite_victims(n):
    """(component, i, j, k) -> value: NaN and +-inf at single sites of a few rows -- the first and the last row of the
    lattice, both rows of one pair, the even and the odd row of others, k at both ends and inside."""
    return {(0, 0, 0, 0): np.nan, (1, n - 1, n - 1, n - 1): np.inf, (2, 5, 8, n // 2): -np.inf, (0, 5, 9, 3): np.inf,
            (1, 64, 31, 1): np.nan, (2, 77, 100, n - 2): np.inf, (0, n - 2, 2, 17): -np.inf}


def poisoned_rows(victims, n):
    """Boolean (3, n, n): the z rows (component, i, j) of the pairs (i, j0), (i, j0 + 1), j0 even, that hold a victim."""
    rows = np.zeros((3, n, n), dtype=bool)
    for (c, i, j, _k) in victims:
        rows[c, i, (j // 2) * 2] = rows[c, i, (j // 2) * 2 + 1] = True
    return rows


def cell_subset(pos, geo, tile_shape, dtype, extra=None):
    """Flat indices of the cells the longdouble density is evaluated on: the 64 fullest home cells, the 2 x 2 x 2 cells
    at each box corner, one whole z row (it crosses every tile boundary along z), a 16^3 block that straddles tile
    boundaries on all three axes (4096 cells), and `extra`."""
    n = geo.n
    tx, ty, tz = tile_shape
    ok = ref.in_domain(pos, geo)
    hc = [ref.home_cell(np.asarray(c, dtype=np.float64)[ok], geo.d, dtype) % n for c in pos]
    hist = np.bincount(hc[2] + n * (hc[1] + n * hc[0]), minlength=geo.N)
    chosen = np.zeros((n, n, n), dtype=bool)
    chosen.reshape(-1)[np.argsort(hist, kind="stable")[-64:]] = True
    ends = np.array([0, 1, n - 2, n - 1])
    chosen[np.ix_(ends, ends, ends)] = True
    chosen[n // 3, n // 5, :] = True
    b = [np.arange(t // 2, t // 2 + 16) % n for t in (tx, ty, tz)]
    chosen[np.ix_(*b)] = True
    if extra is not None:
        chosen.reshape(-1)[np.asarray(extra, dtype=np.int64)] = True
    return np.flatnonzero(chosen.reshape(-1)), hist


def particle_subset(pos, geo, dtype, hist, extra=None, per_cell=64):
    """Particles V is evaluated for: up to `per_cell` from each of the 64 fullest home cells, a 16^3 block of the lattice
    (4096), one whole z row, the eight lattice corners, every particle with a non-finite position, and `extra`."""
    n = geo.n
    take = np.zeros(geo.N, dtype=bool)
    fin = np.isfinite(pos[0]) & np.isfinite(pos[1]) & np.isfinite(pos[2])
    take[~fin] = True
    idx = np.flatnonzero(fin)
    hc = [ref.home_cell(np.asarray(c, dtype=np.float64)[idx], geo.d, dtype) % n for c in pos]
    cell = hc[2] + n * (hc[1] + n * hc[0])
    top = np.argsort(hist, kind="stable")[-64:]
    crowd = np.flatnonzero(np.isin(cell, top))
    for c in top:
        take[idx[crowd[cell[crowd] == c][:per_cell]]] = True
    lat = take.reshape(n, n, n)
    lat[3:19, 5:21, 9:25] = True
    lat[n // 2 + 1, n // 2, :] = True
    ends = np.array([0, n - 1])
    lat[np.ix_(ends, ends, ends)] = True
    if extra is not None:
        take[np.asarray(extra, dtype=np.int64)] = True
    return np.flatnonzero(take)
