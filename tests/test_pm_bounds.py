"""CPU: the bound of tests/pm_bound.py is met by numpy restatements of the particle-mesh kernels' arithmetic and is
missed by wrong ones.

The restatements follow the kernels operation by operation in the storage type (float32 / float64 numpy arrays: every
operation rounded once, no fused multiply-add, 1 / sqrt correctly rounded):

  generic   k_scatter_tile / k_gather_tile: dx = x - (cc + i d), r^2 = (dx^2 + dy^2) + dz^2, q = (r^2 rsqrt(r^2 + tiny))
            / h, W_4 and dW/dq / q with folded coefficients; the cube for the scatter, the hull columns with the running
            z offset for the gather.
  tile81    k_scatter_tile81 / k_gather_tile81: offsets from the home centre in h units, q^2 = X[a] + Y[b] + Z[c] with
            tiny_pos in X, the cut-off on q^2, sqrt_rsq, and the three branch classes fixed at unroll time (home cell:
            inner spline only; a cell two away along any axis: outer only; the other 26: select), on the 81-cell hull.

Accumulation: np.add.at in double (one serial order), rounded to float32 once for the float32 case, which is what one
work item of a float32 handle does.

Measured worst fractions of the bound at C = 1 over all position sets of pm_reference.position_sets at n = 16 and 32,
h = d (this file prints them; pm_bound.MEASURED records them and test_c_is_the_measurement_times_four checks that):

    scatter  float32 0.0259 (generic, n = 16, mixed set)      float64 0.0478 (the same case)
    gather   float32 0.4283 (tile81, n = 16, h = 0.8661 d, one impulse of part_like seen from uniform positions)
             float64 0.4964 (generic and tile81, n = 16, h = 1.0599 d, likewise); white part_like: <= 0.18
    low      float32 0.0269 (CIC, n = 16, mixed set)          float64 0.5326 (CIC, n = 32, tiny_negative set)
    (the fully collapsed 32^3, cnt_c up to 32766: 0.002-0.003 of the scatter's bound)

The same measurement at n = 4 and 5 (test_c_covers_the_smallest_grids; h = d, and h = 0.87 d for the gather at 4), where one
stencil covers the box -- at 4 the offsets -2 and +2 are one cell, which is then charged twice and counted twice -- for the
generic restatement, the only one whose kernels run there (k_scatter_tile / k_gather_tile at 4; the direct kernels at 5
evaluate the same expressions with IEEE sqrt and divide).  Cells and particles collect fewer terms than at 16, so single
roundings average less and three figures (both of the scatter, float32 of low) are above the ones recorded above; all stay below C = 4 x those, which is what
the test asserts, and C is not changed:

    scatter  float32 0.0436 (n = 4, corners set)              float64 0.1210 (n = 4, edges set)
    gather   float32 0.3067 (n = 4, impulse seen from uniform) float64 0.1816 (n = 5, likewise)
    low      float32 0.0489 (CIC, n = 4, upper_edge set)      float64 0.2395 (CIC, n = 5, mixed set)

Mutants (every one must exceed the bound with the final C): stencil cells that wrap are dropped; cut-off at q <= 1.9; a
weight off by 1e-9 relative (float64 only: it is below float32's unit round-off); one particle of a crowded cell left
out; the home cell of a particle on a face taken one lower (NGP and CIC: caught.  SPH: NOT caught, and rightly so --
the density does not depend on which cell the stencil is centred on as long as the stencil still covers the sphere, and
a particle on a face is half a cell from either centre, so cube and 81-cell hull cover it from both and the branch
classes (|offset| <= d / 2 per axis) still hold; the test asserts that the SPH mutant stays inside the bound).
"""
import numpy as np
import pytest

from tests import pm_bound
from tests import pm_reference as ref

LD = np.longdouble
TINY = {np.dtype(np.float32): np.float32(1e-30), np.dtype(np.float64): np.float64(1e-280)}
SETS = {16: ref.ALL_SETS, 32: ref.ALL_SETS}


def geometry(n):
    return ref.Geometry(n, 200.0 * n / 64.0)


def zw81(a, b):
    i1, i2 = abs(a - 2), abs(b - 2)
    return -1 if (i1 == 2 and i2 == 2) else (1 if (i1 == 2 or i2 == 2) else 2)


def _home(x, d, dtype, mutant):
    hc = ref.home_cell(x, d, dtype)
    if mutant == "home_low":
        quot = x / dtype(d)
        hc = np.where(quot == np.trunc(quot), hc - 1, hc)
    return hc


def _finish(acc, dtype):
    return acc.astype(dtype)  # float32: the work item's one flush; float64: no-op


def _w_folded(q, q2, w, dtype, mutant):
    T = dtype
    c34w, c32w, c14w = T(0.75) * w, T(-1.5) * w, T(0.25) * w
    inner = q2 * (c34w * q + c32w) + w
    t = np.maximum(T(2) - q, T(0))
    outer = (c14w * t) * (t * t)
    return inner, outer


def scatter_generic(pos, geo, h, dtype, mutant=None, skip=None):
    T = np.dtype(dtype).type
    n, d = geo.n, T(geo.d)
    x = [np.asarray(c, dtype=dtype) for c in pos]
    keep = ref.in_domain(x, geo) if skip is None else (ref.in_domain(x, geo) & ~skip)
    x = [c[keep] for c in x]
    hc = [_home(c, geo.d, T, mutant) for c in x]
    cc = [(i.astype(dtype) + T(0.5)) * d for i in hc]
    h_inv, w = T(1.0 / h), T(1.0 / np.pi / h ** 3)
    r2_lim = T(4.0 * h * h * (1 + (1e-5 if T is np.float32 else 1e-12)))
    qcut = T(1.9) if mutant == "cutoff" else T(2)
    reach = int(2 * h / geo.d) + 1
    acc = np.zeros(geo.N, dtype=np.float64)
    for i1 in range(-reach, reach + 1):
        dx = x[0] - (cc[0] + T(i1) * d)
        for i2 in range(-reach, reach + 1):
            dy = x[1] - (cc[1] + T(i2) * d)
            r2ab = dx * dx + dy * dy
            for i3 in range(-reach, reach + 1):
                dz = x[2] - (cc[2] + T(i3) * d)
                r2 = r2ab + dz * dz
                m = np.flatnonzero(r2 <= r2_lim)
                if not len(m):
                    continue
                r2m = r2[m]
                q = (r2m * (T(1) / np.sqrt(r2m + TINY[np.dtype(dtype)]))) * h_inv
                inner, outer = _w_folded(q, q * q, w, T, mutant)
                val = np.where(q <= T(1), inner, outer)
                if mutant == "weight":
                    val = val * T(1 + 1e-9)
                ok = q <= qcut
                cx, cy, cz = hc[0][m] + i1, hc[1][m] + i2, hc[2][m] + i3
                if mutant == "nowrap":
                    ok &= (cx >= 0) & (cx < n) & (cy >= 0) & (cy < n) & (cz >= 0) & (cz < n)
                idx = (cz % n) + n * ((cy % n) + n * (cx % n))
                np.add.at(acc, idx[ok], val[ok].astype(np.float64))
    return _finish(acc, dtype)


def scatter_tile81(pos, geo, h, dtype, mutant=None, skip=None):
    T = np.dtype(dtype).type
    n, d = geo.n, T(geo.d)
    x = [np.asarray(c, dtype=dtype) for c in pos]
    keep = ref.in_domain(x, geo) if skip is None else (ref.in_domain(x, geo) & ~skip)
    x = [c[keep] for c in x]
    hc = [_home(c, geo.d, T, mutant) for c in x]
    h_inv, w = T(1.0 / h), T(1.0 / np.pi / h ** 3)
    d_h = d * h_inv
    q2_lim = T(4.0 * h * h * (1 + (1e-5 if T is np.float32 else 1e-12)) * (1.0 / h) * (1.0 / h))
    u = [(c - (i.astype(dtype) + T(0.5)) * d) * h_inv for c, i in zip(x, hc)]
    tiny = TINY[np.dtype(dtype)]
    X = [(u[0] - T(a - 2) * d_h) ** 2 + tiny for a in range(5)]
    Y = [(u[1] - T(a - 2) * d_h) ** 2 for a in range(5)]
    Z = [(u[2] - T(a - 2) * d_h) ** 2 for a in range(5)]
    qcut2 = T(1.9 * 1.9) if mutant == "cutoff" else None
    acc = np.zeros(geo.N, dtype=np.float64)
    for a in range(5):
        for b in range(5):
            zw = zw81(a, b)
            if zw < 0:
                continue
            q2ab = X[a] + Y[b]
            for c in range(2 - zw, 2 + zw + 1):
                q2 = q2ab + Z[c]
                m = np.flatnonzero(q2 <= q2_lim)
                if not len(m):
                    continue
                q2m = q2[m]
                q = np.sqrt(q2m)
                inner, outer = _w_folded(q, q2m, w, T, mutant)
                far = a in (0, 4) or b in (0, 4) or c in (0, 4)
                home = (a, b, c) == (2, 2, 2)
                val = inner if home else (outer if far else np.where(q2m <= T(1), inner, outer))
                if mutant == "weight":
                    val = val * T(1 + 1e-9)
                ok = np.ones(len(m), dtype=bool) if qcut2 is None else (q2m <= qcut2)
                cx, cy, cz = hc[0][m] + a - 2, hc[1][m] + b - 2, hc[2][m] + c - 2
                if mutant == "nowrap":
                    ok &= (cx >= 0) & (cx < n) & (cy >= 0) & (cy < n) & (cz >= 0) & (cz < n)
                idx = (cz % n) + n * ((cy % n) + n * (cx % n))
                np.add.at(acc, idx[ok], val[ok].astype(np.float64))
    return _finish(acc, dtype)


def gather_generic(pos, plike, geo, h, rho_c, dtype):
    T = np.dtype(dtype).type
    n = geo.n
    x = [np.asarray(c, dtype=dtype) for c in pos]
    pl = np.asarray(plike, dtype=dtype)
    hc = [ref.home_cell(c, geo.d, T) for c in x]
    h_inv = T(1.0 / h)
    d_h = T(geo.d * (1.0 / h))
    norm = T(1.0 / (np.pi * (h * h) * (h * h)))
    dpc = [c * h_inv - (i.astype(dtype) + T(0.5)) * d_h for c, i in zip(x, hc)]
    v = [np.zeros(geo.N, dtype=dtype) for _ in range(3)]
    tiny = TINY[np.dtype(dtype)]
    for i1, i2, lo, hi in ref.hull_columns(h, geo.d):
        xh = dpc[0] - T(i1) * d_h
        yh = dpc[1] - T(i2) * d_h
        r2ab = xh * xh + yh * yh
        row = n * (((hc[1] + i2) % n) + n * ((hc[0] + i1) % n))
        zh = dpc[2] - T(lo) * d_h
        for i3 in range(lo, hi + 1):
            q_sq = r2ab + zh * zh
            m = (r2ab <= T(4)) & (q_sq <= T(4))
            rq = T(1) / np.sqrt(q_sq + tiny)
            q = q_sq * rq
            inner = (T(2.25) * norm) * q + T(-3) * norm
            qm2 = q - T(2)
            outer = ((qm2 * qm2) * (T(-0.75) * norm)) * rq
            common = pl[row + (hc[2] + i3) % n] * np.where(q_sq > T(1), outer, inner)
            for e, comp in enumerate((xh, yh, zh)):
                v[e] = np.where(m, v[e] + common * comp, v[e])
            zh = zh - d_h
    normalize = T(rho_c * geo.L ** 3 / geo.N)
    return np.array([c * normalize for c in v])


def gather_tile81(pos, plike, geo, h, rho_c, dtype):
    T = np.dtype(dtype).type
    n = geo.n
    x = [np.asarray(c, dtype=dtype) for c in pos]
    pl = np.asarray(plike, dtype=dtype)
    hc = [ref.home_cell(c, geo.d, T) for c in x]
    h_inv = T(1.0 / h)
    d_h = T(geo.d * (1.0 / h))
    norm = T(1.0 / (np.pi * (h * h) * (h * h)))
    dpc = [c * h_inv - (i.astype(dtype) + T(0.5)) * d_h for c, i in zip(x, hc)]
    c225n, c3n, c34n, c3p = T(2.25) * norm, T(-3) * norm, T(-0.75) * norm, T(3) * norm
    tiny = TINY[np.dtype(dtype)]
    v = [np.zeros(geo.N, dtype=dtype) for _ in range(3)]
    yh = [dpc[1] - T(a - 2) * d_h for a in range(5)]
    zh = [dpc[2] - T(a - 2) * d_h for a in range(5)]
    for a in range(5):
        xh = dpc[0] - T(a - 2) * d_h
        X = xh * xh + tiny
        for b in range(5):
            zw = zw81(a, b)
            if zw < 0:
                continue
            r2ab = yh[b] * yh[b] + X
            row = n * (((hc[1] + b - 2) % n) + n * ((hc[0] + a - 2) % n))
            for c in range(2 - zw, 2 + zw + 1):
                q_sq = zh[c] * zh[c] + r2ab
                m = (r2ab <= T(4)) & (q_sq <= T(4))
                q = np.sqrt(q_sq)
                rq = T(1) / q
                inner = c225n * q + c3n
                outer = c3n * rq + (c34n * q + c3p)
                far = a in (0, 4) or b in (0, 4) or c in (0, 4)
                home = (a, b, c) == (2, 2, 2)
                gr = inner if home else (outer if far else np.where(q_sq > T(1), outer, inner))
                common = pl[row + (hc[2] + c - 2) % n] * gr
                for e, comp in enumerate((xh, yh[b], zh[c])):
                    v[e] = np.where(m, v[e] + common * comp, v[e])
    normalize = T(rho_c * geo.L ** 3 / geo.N)
    return np.array([c * normalize for c in v])


def low_order(pos, geo, mk, dtype, mutant=None):
    """k_scatter_tile_low's expressions for NGP, CIC and TSC: double arithmetic on the stored position, every weight
    rounded to the storage type, double accumulation, one rounding at the end.  mutant "home_low": the cell of a
    particle that sits exactly on a face (x / d integral) is taken one lower, the weights follow from it."""
    n, d, L = geo.n, geo.d, geo.L
    x = [np.asarray(c, dtype=np.float64) for c in pos]
    acc = np.zeros(geo.N)
    on_face = [(a / d == np.floor(a / d)) if mutant == "home_low" else np.zeros(len(a), dtype=bool) for a in x]
    if mk == 0:
        c = [(np.floor(a / d).astype(np.int64) - f) % n for a, f in zip(x, on_face)]
        np.add.at(acc, c[2] + n * (c[1] + n * c[0]), 1.0)
    elif mk == 1:
        c1, dx = [], []
        for a, f in zip(x, on_face):
            q = ref.pacman(a - 0.5 * d, L)
            i = (q / d).astype(np.int64) - f
            c1.append((i + n) % n)
            dx.append(q / d - i)
        for a in (0, 1):
            for b in (0, 1):
                for e in (0, 1):
                    w = 1.0 * (dx[0] if a else 1 - dx[0]) * (dx[1] if b else 1 - dx[1]) * (dx[2] if e else 1 - dx[2])
                    idx = ((c1[2] + e) % n) + n * (((c1[1] + b) % n) + n * ((c1[0] + a) % n))
                    np.add.at(acc, idx, w.astype(dtype).astype(np.float64))
    else:
        ci, w = [], []
        for a, f in zip(x, on_face):
            quot = a / d
            i = np.floor(quot).astype(np.int64) - f
            dd = quot - (i + 0.5)
            ci.append(i)
            w.append([0.5 * (0.5 - dd) * (0.5 - dd), 0.75 - dd * dd, 0.5 * (0.5 + dd) * (0.5 + dd)])
        for a in range(3):
            for b in range(3):
                for e in range(3):
                    idx = ((ci[2] + e - 1) % n) + n * (((ci[1] + b - 1) % n) + n * ((ci[0] + a - 1) % n))
                    np.add.at(acc, idx, (1.0 * w[0][a] * w[1][b] * w[2][e]).astype(dtype).astype(np.float64))
    return acc.astype(dtype)


# ---- cases ----------------------------------------------------------------------------------------------------------

_cache = {}


def case(n, dtype, name):
    """positions of one set in the storage type, and the reference density of them (cached: the reference is the
    expensive part)."""
    key = (n, np.dtype(dtype).name, name)
    if key not in _cache:
        geo = geometry(n)
        psi = ref.position_sets(geo, dtype, names=(name,))[name]
        pos = ref.positions(psi, geo, False, dtype)
        slack = pm_bound.q_slack(dtype, n, 1.0)
        S, cnt, _ = ref.sph_density([c.astype(np.float64) for c in pos], geo, geo.d, q_slack=slack, dtype=dtype)
        _cache[key] = (geo, pos, S, cnt)
    return _cache[key]


def scatter_fraction(n, dtype, name, kernel, mutant=None, skip=None, c=1.0):
    geo, pos, S, cnt = case(n, dtype, name)
    got = kernel(pos, geo, geo.d, dtype, mutant=mutant, skip=skip)
    w_norm = 1.0 / np.pi / geo.d ** 3
    return pm_bound.worst_fraction(got, S, pm_bound.density_bound(S, cnt, dtype, n, 1.0, w_norm, c=c))


KERNELS = {"generic": scatter_generic, "tile81": scatter_tile81}
LOW_REF = {0: None, 1: ref.cic_density, 2: ref.tsc_density}
DTYPES = (np.float32, np.float64)


def white_plike(geo, dtype, seed=7):
    rng = np.random.Generator(np.random.Philox(seed))
    pl = rng.standard_normal(geo.N)
    pl[rng.random(geo.N) < 0.2] = 0.0  # the holes of a window
    return pl.astype(dtype).astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: np.dtype(t).name)
def test_position_sets_hit_their_targets(dtype):
    """pm_reference.positions (the storage-type sequence) lands the special sets exactly where they are meant to be."""
    for n in (16, 32):
        geo = geometry(n)
        d, L = geo.d, geo.L
        sets = ref.position_sets(geo, dtype)
        idx = ref.lattice_index(n)
        pos = {k: ref.positions(v, geo, False, dtype) for k, v in sets.items()}
        cen = ref.lattice_centres(geo, np.float64)
        for a in range(3):
            assert np.array_equal(pos["centres"][a], cen[a])
            assert np.array_equal(pos["corners"][a], idx[a] * d)
        on_face = sum((pos["faces"][a] / d == np.round(pos["faces"][a] / d)).astype(int) for a in range(3))
        assert np.all(on_face == 1)
        on_face = sum((pos["edges"][a] / d == np.round(pos["edges"][a] / d)).astype(int) for a in range(3))
        assert np.all(on_face == 2)
        T = np.dtype(dtype).type
        plane = idx[0] == 0
        assert np.all(pos["upper_edge"][0][plane] == np.nextafter(T(L), T(0)))
        plane = idx[1] == 0
        assert np.all(pos["tiny_negative"][1][plane] == 0)  # -ulp + L rounded to L, folded to 0
        psi_t = sets["tiny_negative"].astype(dtype)
        raw = cen[1].astype(dtype) + psi_t[1]
        assert np.all(raw[plane] < 0) and np.all(raw[plane] + T(L) == T(L))
        for name in ("collapse_inside", "collapse_corner"):
            p = np.array(pos[name], dtype=np.float64)
            centre = np.array([3.6, 3.3, 5.4]) * d if name == "collapse_inside" else np.zeros(3)
            sep = (p - centre[:, None] + L / 2) % L - L / 2
            assert np.all(np.sqrt((sep ** 2).sum(0)) <= 0.3 * d * (1 + 1e-6))
        for name, p in pos.items():
            for a in range(3):
                assert np.all((p[a] >= 0) & (p[a] < T(L))), name
        # the crowding the sort paths are meant to meet: a few tiles with >= 8x the mean occupancy, many empty
        tiles = (8, 8, 16)
        tid = [(ref.home_cell(pos["filament"][a], d, dtype) % n) // tiles[a] for a in range(3)]
        occ = np.bincount(tid[2] + (n // 16) * (tid[1] + (n // 8) * tid[0]), minlength=(n // 8) ** 2 * (n // 16))
        if n >= 32:  # 16^3 has four tiles: nothing can hold more than 4x the mean there
            assert occ.max() >= 8 * occ.mean() and (occ == 0).sum() >= len(occ) // 2


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: np.dtype(t).name)
def test_home_cell_follows_the_storage_type_division(dtype):
    T = np.dtype(dtype).type
    d = T(3.125)
    x = np.array([0.0, 3.125, np.nextafter(T(3.125), T(0)), 46.875, np.nextafter(T(50), T(0))], dtype=dtype)
    assert ref.home_cell(x, 3.125, dtype).tolist() == [0, 1, 0, 15, 15]


@pytest.mark.parametrize("n", (16, 32))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_scatter_restatements_meet_the_bound(kernel, dtype, n):
    worst = 0.0
    for name in SETS[n]:
        f, i = scatter_fraction(n, dtype, name, KERNELS[kernel])
        print("PMCPU scatter_%s<%s> n=%d %s: worst fraction of the bound at C = 1: %.4f (cell %d)"
              % (kernel, np.dtype(dtype).name, n, name, f, i))
        worst = max(worst, f)
    assert worst <= pm_bound.MEASURED["scatter"][np.dtype(dtype).name]


def _gather_case(n, dtype, name, impulse=None, h_rel=1.0):
    geo, pos, _, _ = case(n, dtype, name)
    pl = white_plike(geo, dtype)
    if impulse is not None:  # one non-zero cell: V of every particle near it is ONE kernel-gradient evaluation
        pl = np.zeros(geo.N)
        pl[impulse] = -1.75
    h = h_rel * geo.d
    slack = pm_bound.q_slack(dtype, n, 1.0 / h_rel)
    V, A, P, m = ref.sph_adjoint_gather([c.astype(np.float64) for c in pos], pl, geo, h, 1.0, q_slack=slack, dtype=dtype)
    norm = 1.0 / (np.pi * h ** 4)
    return geo, pos, pl, h, V, pm_bound.gather_bound(A, P, m, dtype, n, 1.0 / h_rel, norm, c=1.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("kernel", ("generic", "tile81"))
def test_gather_restatements_meet_the_bound(kernel, dtype):
    fn = gather_generic if kernel == "generic" else gather_tile81
    worst = 0.0
    # impulses: nothing averages there, and cells far from the origin see the largest coordinate roundings
    cases = [(n, name, None) for n, name in ((16, "mixed"), (16, "corners"), (16, "centres"), (16, "edges"),
                                              (16, "faces"), (16, "collapse_corner"), (32, "mixed"), (16, "upper_edge"),
                                              (16, "tiny_negative"))]
    cases += [(16, "uniform", c) for c in (0, 803, 1911, 2730, 3003, 3583, 4095)]
    cases += [(16, "mixed", c) for c in (1638, 4095)] + [(32, "uniform", c) for c in (32767, 21845)]
    cases = [c + (1.0,) for c in cases]
    # both ends of the unrolled kernels' range of h: d / h is no longer 1, so (i + 1/2) d / h is rounded as well
    cases += [(16, "uniform", c, h_rel) for h_rel in (0.8661, 1.0599) for c in (3583, 4095)]
    cases += [(16, "mixed", None, h_rel) for h_rel in (0.8661, 1.0599)]
    for n, name, impulse, h_rel in cases:
        geo, pos, pl, h, V, bound = _gather_case(n, dtype, name, impulse, h_rel)
        got = fn(pos, pl, geo, h, 1.0, dtype)
        f, i = pm_bound.worst_fraction(got, V, bound)
        print("PMCPU gather_%s<%s> n=%d %s%s: worst fraction of the bound at C = 1: %.4f (element %d)"
              % (kernel, np.dtype(dtype).name, n, name + ("" if h_rel == 1.0 else " h = %g d" % h_rel),
                 "" if impulse is None else " impulse at %d" % impulse, f, i))
        worst = max(worst, f)
    assert worst <= pm_bound.MEASURED["gather"][np.dtype(dtype).name]


# (collapse_inside needs a box of more than 5.4 d: left out at 4 and 5, as in tests/test_gpu_particle_mesh.py)
SMALL_BOX_SETS = tuple(s for s in ref.ALL_SETS if s != "collapse_inside")


@pytest.mark.parametrize("n", (4, 5))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: np.dtype(t).name)
def test_c_covers_the_smallest_grids(dtype, n):
    """The measurement of the tests above at n = 4 and 5 (module docstring): the worst fraction at C = 1 of the generic
    scatter and gather and of NGP / CIC / TSC must be below the C in force, pm_bound.constant(kind, dtype)."""
    tname = np.dtype(dtype).name
    worst = 0.0
    for name in SMALL_BOX_SETS:
        f, i = scatter_fraction(n, dtype, name, scatter_generic)
        print("PMCPU scatter_generic<%s> n=%d %s: worst fraction of the bound at C = 1: %.4f (cell %d)" % (tname, n, name, f, i))
        worst = max(worst, f)
    assert worst <= pm_bound.constant("scatter", dtype)
    cases = [(name, None, 1.0) for name in ("mixed", "corners", "uniform", "collapse_corner", "edges", "faces")]
    cases += [("uniform", c, 1.0) for c in (0, n ** 3 // 3, n ** 3 // 2, n ** 3 - 1)]
    cases += [("mixed", None, 0.87), ("uniform", n ** 3 // 3, 0.87)] if n == 4 else []
    worst = 0.0
    for name, impulse, h_rel in cases:
        geo, pos, pl, h, V, bound = _gather_case(n, dtype, name, impulse, h_rel)
        f, i = pm_bound.worst_fraction(gather_generic(pos, pl, geo, h, 1.0, dtype), V, bound)
        print("PMCPU gather_generic<%s> n=%d %s%s: worst fraction of the bound at C = 1: %.4f (element %d)"
              % (tname, n, name + ("" if h_rel == 1.0 else " h = %g d" % h_rel),
                 "" if impulse is None else " impulse at %d" % impulse, f, i))
        worst = max(worst, f)
    assert worst <= pm_bound.constant("gather", dtype)
    worst = 0.0
    for mk in (0, 1, 2):
        for name in SMALL_BOX_SETS:
            geo, pos, _, _ = case(n, dtype, name)
            p64 = [c.astype(np.float64) for c in pos]
            S, cnt, _ = ref.ngp_density(p64, geo, dtype) if mk == 0 else LOW_REF[mk](p64, geo)
            got = low_order(pos, geo, mk, dtype)
            if mk == 0:
                assert np.array_equal(got.astype(np.float64), S.astype(np.float64)), name
            f, i = pm_bound.worst_fraction(got, S, pm_bound.density_bound(S, cnt, dtype, n, 1.0, 1.0, c=1.0))
            print("PMCPU low mk=%d<%s> n=%d %s: worst fraction of the bound at C = 1: %.4f (cell %d)" % (mk, tname, n, name, f, i))
            worst = max(worst, f)
    assert worst <= pm_bound.constant("low", dtype)


def test_c_is_the_measurement_times_four():
    assert pm_bound.MARGIN == 4.0
    for kind, per_type in pm_bound.MEASURED.items():
        for t, f in per_type.items():
            assert pm_bound.constant(kind, np.dtype(t)) == 4.0 * f > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_mutants_of_the_scatter_exceed_the_bound(kernel, dtype):
    fn, C = KERNELS[kernel], pm_bound.constant("scatter", dtype)
    name32 = np.dtype(dtype).name
    # stencil cells that wrap past n dropped: every set has particles next to the box faces
    for name in ("uniform", "corners", "collapse_corner", "mixed"):
        f, _ = scatter_fraction(16, dtype, name, fn, mutant="nowrap", c=C)
        print("PMCPU mutant nowrap %s<%s> %s: %.3g x the bound" % (kernel, name32, name, f))
        assert f > 1
    # cut-off at q <= 1.9: wherever a particle has a cell in the shell (the lattice sets have none at h = d: from a
    # centre the cells sit at q^2 = 0, 1, 2, 3, 4, from a corner at 0.75, 2.75, from a face centre at <= 3.25, from an
    # edge midpoint at <= 3.5)
    for name in ("uniform", "filament", "sheet", "mixed"):
        f, _ = scatter_fraction(16, dtype, name, fn, mutant="cutoff", c=C)
        print("PMCPU mutant cutoff %s<%s> %s: %.3g x the bound" % (kernel, name32, name, f))
        assert f > 1
    # a weight off by 1e-9 relative
    if np.dtype(dtype) == np.dtype(np.float64):
        for name in ("uniform", "centres", "mixed"):
            f, _ = scatter_fraction(16, dtype, name, fn, mutant="weight", c=C)
            print("PMCPU mutant weight %s<%s> %s: %.3g x the bound" % (kernel, name32, name, f))
            assert f > 1
    # one particle of a crowded cell left out: the clump of the mixed set
    geo, pos, S, cnt = case(16, dtype, "mixed")
    crowded = int(np.argmax(cnt))
    centre = (np.array([crowded // geo.n ** 2, (crowded // geo.n) % geo.n, crowded % geo.n]) + 0.5) * geo.d
    r = np.sqrt(sum((np.asarray(c, dtype=np.float64) - x0) ** 2 for c, x0 in zip(pos, centre)))
    assert cnt[crowded] >= 50 and r.min() < geo.d
    skip = np.zeros(geo.N, dtype=bool)
    skip[int(np.argmin(r))] = True
    f, i = scatter_fraction(16, dtype, "mixed", fn, skip=skip, c=C)
    print("PMCPU mutant dropped particle %s<%s>: %.3g x the bound (cell %d, cnt %d)" % (kernel, name32, f, i, cnt[i]))
    assert f > 1
    # home cell of a particle on a face one lower: not an error for SPH (see the module docstring)
    for name in ("corners", "faces", "mixed"):
        f, _ = scatter_fraction(16, dtype, name, fn, mutant="home_low", c=C)
        print("PMCPU mutant home_low %s<%s> %s: %.3g x the bound" % (kernel, name32, name, f))
        assert f <= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("mk", (0, 1, 2))
def test_low_order_restatements_and_their_home_cell_mutant(mk, dtype):
    """NGP / CIC / TSC as the tile kernel evaluates them: NGP exact, CIC and TSC within (1) with w_norm = 1, h = d; and
    the home cell of a particle on a face taken one lower is caught for NGP and CIC."""
    name32, worst = np.dtype(dtype).name, 0.0
    for n in (16, 32):
        for name in ref.ALL_SETS:
            geo, pos, _, _ = case(n, dtype, name)
            p64 = [c.astype(np.float64) for c in pos]
            S, cnt, _ = ref.ngp_density(p64, geo, dtype) if mk == 0 else LOW_REF[mk](p64, geo)
            got = low_order(pos, geo, mk, dtype)
            if mk == 0:
                assert np.array_equal(got.astype(np.float64), S.astype(np.float64)), name
            f, i = pm_bound.worst_fraction(got, S, pm_bound.density_bound(S, cnt, dtype, n, 1.0, 1.0, c=1.0))
            print("PMCPU low mk=%d<%s> n=%d %s: worst fraction of the bound at C = 1: %.4f (cell %d)"
                  % (mk, name32, n, name, f, i))
            worst = max(worst, f)
            # (TSC's weights are continuous across the face like SPH's: with the cell one lower the particle sits at
            # dd = +1/2 instead of -1/2 and the same two cells get 1/2 each, so there is nothing to catch)
            if n == 16 and mk < 2 and name in ("faces", "mixed", "edges"):
                bound = pm_bound.density_bound(S, cnt, dtype, n, 1.0, 1.0, kind="low")
                f, _ = pm_bound.worst_fraction(low_order(pos, geo, mk, dtype, mutant="home_low"), S, bound)
                print("PMCPU mutant home_low mk=%d<%s> %s: %.3g x the bound" % (mk, name32, name, f))
                assert f > 1
    assert worst <= pm_bound.MEASURED["low"][name32]


# ---- the host side of tests/test_gpu_zbin_positions.py -------------------------------------------------------------------

from tests import zbin_sets  # noqa: E402


@pytest.mark.parametrize("name", ("mixed", "collapse_corner"))
def test_subset_evaluators_are_bitwise_the_full_reference(name):
    """sph_density_at / sph_adjoint_gather_at on chosen cells and particles against the full evaluation at 32^3, with an
    offset domain so that dropped particles are among the neighbours."""
    n, dtype = 32, np.float64
    geo = ref.Geometry(n, 100.0, (0.5 * 3.125, -0.25 * 3.125, 0.25 * 3.125))
    psi = ref.position_sets(geo, dtype, names=(name,))[name]
    psi[0, 5], psi[2, 777] = np.nan, np.inf
    pos = [c.astype(np.float64) for c in ref.positions(psi, geo, 0, dtype)]
    h, slack = geo.d, pm_bound.q_slack(dtype, n, 1.0)
    cells, hist = zbin_sets.cell_subset(pos, geo, (8, 8, 16), dtype, extra=[17, 30000])
    assert len(cells) >= 4096 and hist.sum() == ref.in_domain(pos, geo).sum()
    S, cnt, _ = ref.sph_density(pos, geo, h, slack, dtype)
    Sa, cnta = ref.sph_density_at(pos, geo, h, cells, slack, dtype)
    assert np.array_equal(Sa, S[cells]) and np.array_equal(cnta, cnt[cells])
    assert np.array_equal(np.sort(np.argsort(hist, kind="stable")[-64:]), np.intersect1d(cells, np.argsort(hist, kind="stable")[-64:]))
    assert not np.any(cnt[~ref.reachable_cells(pos, geo, h, dtype)])
    parts = zbin_sets.particle_subset(pos, geo, dtype, hist, extra=[123])
    assert len(parts) >= 4096 and {5, 777, 123, 0, geo.N - 1} <= set(parts.tolist())
    plike = np.random.default_rng(3).standard_normal(geo.N)
    full = ref.sph_adjoint_gather(pos, plike, geo, h, 1.3, True, 0.4, slack, dtype)
    sub = ref.sph_adjoint_gather_at(pos, plike, geo, h, 1.3, parts, True, 0.4, slack, dtype)
    for a, b in zip(full, sub):
        assert np.array_equal(a[..., parts], b)


def test_reachable_cells_leave_out_exactly_the_far_ones():
    """One particle: the cells farther than the stencil from its home cell, and only those, are unreachable; every
    cell with cnt > 0 is reachable wherever the particle sits in its home cell."""
    n = 16
    geo = ref.Geometry(n, 50.0)
    for frac in ((0.0, 0.0, 0.0), (0.999, 0.999, 0.999), (0.5, 0.0, 0.999)):
        pos = [np.array([(5 + f) * geo.d]) for f in frac]
        reach = ref.reachable_cells(pos, geo, geo.d)
        _, cnt, _ = ref.sph_density(pos, geo, geo.d)
        assert not np.any(cnt[~reach]) and reach.sum() < 7 ** 3 and cnt.sum() > 0
    corners = sum((ref.sph_density([np.array([(5 + a) * geo.d * (1 - 1e-12) if a else 5 * geo.d]) for a in f], geo, geo.d)[1] > 0)
                  for f in np.ndindex(2, 2, 2))
    assert np.array_equal(corners > 0, ref.reachable_cells([np.array([5.5 * geo.d])] * 3, geo, geo.d) & (corners > 0))


def test_counter_pairs_of_a_hand_made_case():
    """n = 4, tiles of 2 x 2 x 2: workgroup 0 owns the rows (0..1, 0..1, :).  Its 16 particles are put into known
    counters; every other particle goes to one far counter."""
    n = 4
    geo = ref.Geometry(n, 4.0)  # d = 1
    tile = (2, 2, 2)
    pos = [np.full(geo.N, 3.25), np.full(geo.N, 3.25), np.full(geo.N, 3.25)]  # tile 7, bits 000: key 56, pair 28
    i, j, k = ref.lattice_index(n)
    wg0 = np.flatnonzero((i < 2) & (j < 2))
    assert len(wg0) == 16
    # four particles each: cell (0, 0, 0) lower z half (key 0), the same cell upper z half (key 1: the other half of pair
    # 0), cell (0, 0, 2) = tile 1 with x upper (b = 4: octant 7, pair 7 of tile 1 = pair 7), and a NaN
    for m, p in enumerate(wg0):
        x, y, z = ((0.25, 0.25, 0.25), (0.25, 0.25, 0.75), (0.75, 0.25, 2.25), (np.nan, 0.0, 0.0))[m // 4]
        pos[0][p], pos[1][p], pos[2][p] = x, y, z
    key = zbin_sets.counter_keys(pos, geo, tile, np.float64)
    assert sorted(set(key[wg0].tolist())) == [-1, 0, 1, 15]
    assert set(key[np.setdiff1d(np.arange(geo.N), wg0)].tolist()) == {56}
    per = zbin_sets.distinct_pairs_per_workgroup(key, n)
    assert per.tolist() == [2, 1, 1, 1]
    pairs, even, odd = zbin_sets.pair_halves_per_workgroup(key, n)
    assert pairs.tolist()[:2] == [0, 7] and even.tolist()[:2] == [4, 0] and odd.tolist()[:2] == [4, 4]
    assert np.array_equal(zbin_sets.workgroup_index(n)[wg0], np.zeros(16, dtype=np.int64))


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("fp32", "fp64"))
def test_zbin_sets_do_what_they_are_for(dtype):
    """32^3 with 8 x 8 x 16 tiles: one_counter gives every workgroup one counter of its own, both_halves fills both halves
    of every pair alike, the z-constant sets are constant along z, scrambled meets many pairs (the 0.9 of the GPU test
    needs the tile count of 128^3: here 256 pairs for 128 particles)."""
    n, tile = 32, (8, 8, 16)
    geo = ref.Geometry(n, 100.0)
    names = ("one_counter", "both_halves", "scrambled", "faces", "far_out_zc", "tiny_negative_zc", "upper_edge_zc")
    sets = zbin_sets.z_position_sets(geo, dtype, tile, names)
    keys = {}
    for name in names:
        pos = [c.astype(np.float64) for c in ref.positions(sets[name], geo, 0, dtype)]
        keys[name] = zbin_sets.counter_keys(pos, geo, tile, dtype)
        if name in zbin_sets.EXACT_SETS:
            q = sets[name].reshape(3, n, n, n)
            assert np.array_equal(q, np.broadcast_to(q[..., :1], q.shape)), name
    wg = zbin_sets.workgroup_index(n)
    one = keys["one_counter"]
    assert np.all(zbin_sets.distinct_pairs_per_workgroup(one, n) == 1)
    first = one[np.unique(wg, return_index=True)[1]]
    assert np.array_equal(one, first[wg]) and len(np.unique(first)) == (n // 2) ** 2
    pairs, even, odd = zbin_sets.pair_halves_per_workgroup(keys["both_halves"], n)
    assert np.all(even == 2 * tile[2]) and np.all(odd == 2 * tile[2]) and len(pairs) == (n // 2) ** 2 * (n // tile[2])
    assert zbin_sets.distinct_pairs_per_workgroup(keys["scrambled"], n).max() >= 0.55 * 4 * n
    faces = ref.positions(sets["faces"], geo, 0, dtype)
    on_face = [np.mean(np.fmod(c.astype(np.float64), geo.d) == 0) for c in faces]
    assert all(0.2 < f < 0.5 for f in on_face)


def test_scrambled_fills_the_table_of_the_128_instantiation():
    """The GPU test asserts >= 0.9 * 4 n distinct pairs in the fullest workgroup; here the same count on the host for the
    positions as given (before the z round trip), 128^3 with 8 x 8 x 16 tiles."""
    n, tile, dtype = 128, (8, 8, 16), np.float64
    geo = ref.Geometry(n, 400.0)
    psi = zbin_sets.z_position_sets(geo, dtype, tile, ("scrambled",))["scrambled"]
    pos = [c.astype(np.float64) for c in ref.positions(psi, geo, 0, dtype)]
    per = zbin_sets.distinct_pairs_per_workgroup(zbin_sets.counter_keys(pos, geo, tile, dtype), n)
    print("scrambled 128^3: distinct pairs per workgroup mean %.1f, largest %d of %d" % (per.mean(), per.max(), 4 * n))
    assert per.max() >= 0.9 * 4 * n
