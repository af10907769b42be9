"""Plain high-precision reference of the particle-mesh stage, written from the upstream definitions (not from the
kernels): particle_pos + pacman_coordinate (disp_part.cc, pacman.cpp:20-28), overdens and getDensity_NGP / _CIC / _TSC /
_SPH with SPH_kernel_3D (massFunctions.cc:30-47, 49-364, 366-495; getCICcells / getCICweights interpolate_grid.cpp:27-79),
likelihood_calc_V_SPH with its inner loop (HMC_models.cc:77-128, 200-303) and grad_SPH_kernel_3D_h_units
(SPH_kernel.cpp:148-208).

Two kinds of function:

* `positions` and `home_cell` work IN THE STORAGE TYPE, operation by operation, each operation rounded once (numpy scalars
  and arrays of float32 / float64 do exactly that; there is no fused multiply-add in numpy).  The engine promises this
  sequence, so they are compared bitwise.
* the densities and the adjoint gather take positions that are exact in double (the fetched ones) and evaluate the
  DEFINITION in numpy longdouble (64-bit mantissa): every cell whose centre is within 2 h of the particle, periodic wrap,
  particles outside [min, min + L) dropped.  Next to each sum they return what tests/pm_bound.py needs to bound the
  error of a storage-type evaluation of the same sum.

Also here: the position sets both test files use (`position_sets`), built as targets; psi = target - lattice centre.
"""
import numpy as np

LD = np.longdouble


class Geometry:
    """Cubic grid: n cells of size d = L / n per axis, lower corner `mins` of the mass-assignment domain."""

    def __init__(self, n, L, mins=(0.0, 0.0, 0.0)):
        self.n, self.L, self.d, self.N = int(n), float(L), float(L) / int(n), int(n) ** 3
        self.mins = tuple(float(m) for m in mins)


def lattice_index(n):
    """(i, j, k) of particle p = k + n (j + n i)."""
    p = np.arange(n ** 3)
    return p // (n * n), (p // n) % n, p % n


def lattice_centres(geo, dtype=np.float64):
    """d * i + 0.5 * d in `dtype` (two products, one sum, each rounded): where particle_pos starts from."""
    T = np.dtype(dtype).type
    d = T(geo.d)
    return [d * idx.astype(dtype) + T(0.5) * d for idx in lattice_index(geo.n)]


def pacman(x, L):
    """pacman_coordinate (pacman.cpp:20-28) on an array of the storage type: a negative x becomes fmod(x, L) + L, and
    then -- in this order -- anything >= L (which x + L may have rounded to) becomes fmod(x, L)."""
    x = np.array(x, copy=True)
    T = x.dtype.type
    L = T(L)
    with np.errstate(invalid="ignore"):
        neg = x < 0
        x[neg] = np.fmod(x[neg], L) + L
        big = x >= L
        x[big] = np.fmod(x[big], L)
    return x


def positions(psi, geo, rsd, dtype, cpecvel=0.0, v_norm=0.0):
    """particle_pos + pacman in the storage type: x = d i + d / 2 + psi_x, folded; with RSD (plane-parallel, rsd.cc:28-68)
    z += (cpecvel * psi_z) * v_norm, folded again.  psi: (3, N) doubles, converted to `dtype` first like the engine does.
    Returns [x, y, z] in `dtype`."""
    T = np.dtype(dtype).type
    psi = np.asarray(psi, dtype=np.float64).reshape(3, -1).astype(dtype)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for c0, ps in zip(lattice_centres(geo, dtype), psi):
            out.append(pacman(c0 + ps, geo.L))
        if rsd:
            vz = T(cpecvel) * psi[2]
            out[2] = pacman(out[2] + vz * T(v_norm), geo.L)
    return out


def home_cell(x, d, dtype):
    """(ULONG)(x / d) with the division done in the storage type (massFunctions.cc:434-436, HMC_models.cc:264-266).
    x must be finite and >= 0."""
    T = np.dtype(dtype).type
    return np.trunc(np.asarray(x, dtype=dtype) / T(d)).astype(np.int64)


def in_domain(pos, geo, closed=False):
    """The domain test of the mass assignments (massFunctions.cc:75, 116, 426; :195 for TSC is closed above), evaluated
    on the exact positions; non-finite positions fail it."""
    ok = np.ones(len(pos[0]), dtype=bool)
    with np.errstate(invalid="ignore"):
        for x, m in zip(pos, geo.mins):
            ok &= np.isfinite(x) & (x >= m) & ((x <= m + geo.L) if closed else (x < m + geo.L))
    return ok


def sph_w(q, w_norm):
    """SPH_kernel_3D, Monaghan's W_4 (massFunctions.cc:366-384), 0 beyond q = 2."""
    q = np.asarray(q, dtype=LD)
    inner = 1 - LD(1.5) * q * q + LD(0.75) * q * q * q
    outer = LD(0.25) * (2 - q) ** 3
    return w_norm * np.where(q <= 1, inner, np.where(q <= 2, outer, 0))


def _accumulate(S, cnt, idx, w, near=None):
    np.add.at(S, idx, w)
    np.add.at(cnt, idx, 1 if near is None else near.astype(np.int64))


def sph_density(pos, geo, h, q_slack=0.0, dtype=np.float64, skip=None, cells=None):
    """getDensity_SPH.  pos: [x, y, z] exact in double.  Every particle in the domain adds W_4(r / h) / (pi h^3) to every
    cell whose centre is at r / h <= 2, searched in the (2 reach + 1)^3 cube around its home cell (reach = int(2 h / d) + 1
    covers the sphere from any point of the home cell), indices wrapped periodically.  The home cell is the storage-type
    one (`dtype`); the distances are exact.
    Returns (S, cnt, total): per cell the sum and the number of particles with q <= 2 + q_slack (a storage-type
    evaluation may find such a particle on either side of the cut-off; pm_bound charges it like a contributing one),
    and the sum over all cells.  skip: boolean mask of particles to leave out (mutants).  cells: flat indices; S and cnt
    are then kept for these cells only, in this order (what lands elsewhere is dropped before it is added)."""
    n, d = geo.n, LD(geo.d)
    h = LD(h)
    w_norm = 1 / _pi() / (h * h * h)
    ok = in_domain(pos, geo)
    if skip is not None:
        ok &= ~skip
    sel = np.flatnonzero(ok)
    x = [np.asarray(c, dtype=np.float64)[sel] for c in pos]
    hc = [home_cell(c, geo.d, dtype) for c in x]
    xl = [c.astype(LD) for c in x]
    slot = None
    if cells is not None:
        slot = np.full(geo.N, -1, dtype=np.int64)
        slot[cells] = np.arange(len(cells))
    S = np.zeros(geo.N if slot is None else len(cells), dtype=LD)
    cnt = np.zeros(len(S), dtype=np.int64)
    reach = int(2 * float(h) / geo.d) + 1
    lim = (2 + LD(q_slack)) ** 2 * h * h
    for i1 in range(-reach, reach + 1):
        dx = xl[0] - (hc[0] + i1 + LD(0.5)) * d
        dx2 = dx * dx
        mx = dx2 <= lim
        if not mx.any():
            continue
        for i2 in range(-reach, reach + 1):
            dy = xl[1] - (hc[1] + i2 + LD(0.5)) * d
            r2ab = dx2 + dy * dy
            mxy = mx & (r2ab <= lim)
            if not mxy.any():
                continue
            m2 = np.flatnonzero(mxy)
            row = n * (((hc[1][m2] + i2) % n) + n * ((hc[0][m2] + i1) % n))
            for i3 in range(-reach, reach + 1):
                dz = xl[2][m2] - (hc[2][m2] + i3 + LD(0.5)) * d
                r2 = r2ab[m2] + dz * dz
                m3 = r2 <= lim
                if not m3.any():
                    continue
                idx = row[m3] + (hc[2][m2][m3] + i3) % n
                r2 = r2[m3]
                if slot is not None:
                    idx = slot[idx]
                    r2, idx = r2[idx >= 0], idx[idx >= 0]
                q = np.sqrt(r2) / h
                _accumulate(S, cnt, idx, sph_w(q, w_norm))
    return S, cnt, S.sum()


def sph_density_at(pos, geo, h, cells, q_slack=0.0, dtype=np.float64, threads=1):
    """S and cnt of sph_density on the chosen cells (flat indices), from the particles that can reach them: those whose
    home cell is within the search cube's reach of a chosen cell.  The particles left out add nothing to a chosen cell and
    the others keep their order, so every chosen cell sees the same additions in the same order as in the full
    evaluation: bitwise its values (tests/test_pm_bounds.py).  threads > 1: the particles are split into that many
    runs, evaluated side by side (numpy's longdouble loops release the interpreter lock) and the partial sums added in
    longdouble -- the same sums in another order, 2^-64 relative apart.  Returns (S[cells], cnt[cells])."""
    n = geo.n
    cells = np.asarray(cells, dtype=np.int64)
    reach = int(2 * float(h) / geo.d) + 1
    chosen = np.zeros((n, n, n), dtype=bool)
    chosen.reshape(-1)[cells] = True
    grown = chosen.copy()
    for axis in range(3):  # the cube of side 2 reach + 1 around every chosen cell, periodic
        acc = grown.copy()
        for s in range(1, min(reach, n // 2) + 1):
            acc |= np.roll(grown, s, axis) | np.roll(grown, -s, axis)
        grown = acc
    ok = in_domain(pos, geo)
    idx = np.flatnonzero(ok)
    hc = [home_cell(np.asarray(c, dtype=np.float64)[idx], geo.d, dtype) % n for c in pos]
    near = idx[grown[hc[0], hc[1], hc[2]]]

    def run(part):
        take = np.ones(geo.N, dtype=bool)
        take[part] = False
        return sph_density(pos, geo, h, q_slack, dtype, skip=take, cells=cells)[:2]

    if threads <= 1 or len(near) < 4096 * threads:
        return run(near)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(run, np.array_split(near, threads)))
    return sum(p[0] for p in parts), sum(p[1] for p in parts)


def reachable_cells(pos, geo, h, dtype=np.float64):
    """Boolean (N): the cells that can have a particle within 2 h of their centre -- the home cells of the particles in
    the domain, grown by every offset whose nearest approach to a point of the home cell, max(0, |i| - 1/2) d per axis,
    is within 2 h (taken 1e-6 wider).  A cell outside it has cnt_c = 0 wherever the particles sit inside their home cells:
    it must be exactly 0."""
    n = geo.n
    ok = in_domain(pos, geo)
    hc = [home_cell(np.asarray(c, dtype=np.float64)[ok], geo.d, dtype) % n for c in pos]
    occ = np.zeros((n, n, n), dtype=bool)
    occ[hc[0], hc[1], hc[2]] = True
    out = np.zeros_like(occ)
    reach = int(2 * float(h) / geo.d) + 1
    gap = [max(0.0, abs(i) - 0.5) * geo.d for i in range(-reach, reach + 1)]
    lim = (2 * float(h)) ** 2 * (1 + 1e-6)
    for a, i1 in enumerate(range(-reach, reach + 1)):
        for b, i2 in enumerate(range(-reach, reach + 1)):
            ks = [i3 for c, i3 in enumerate(range(-reach, reach + 1)) if gap[a] ** 2 + gap[b] ** 2 + gap[c] ** 2 <= lim]
            if not ks:
                continue
            col = np.roll(occ, (i1, i2), (0, 1))
            for i3 in ks:
                out |= np.roll(col, i3, 2)
    return out.reshape(-1)


def _pi():
    return LD("3.14159265358979323846264338327950288")


def _cells_of(x, geo):
    """floor((x - min) / d) mod n, exact quotient (d = L / n is a binary fraction in the suite's geometry)."""
    return [np.floor((c.astype(LD) - LD(m)) / LD(geo.d)).astype(np.int64) for c, m in zip(x, geo.mins)]


def ngp_density(pos, geo, dtype=np.float64):
    """getDensity_NGP: one unit into the cell floor((x - min) / d) mod n, the subtraction and the division done in the
    storage type like upstream's real_prec expression.  Returns (S, cnt, total); S is integral."""
    T = np.dtype(dtype).type
    ok = in_domain(pos, geo)
    x = [np.asarray(c, dtype=np.float64)[ok] for c in pos]
    c = [np.floor((ci.astype(dtype) - T(m)) / T(geo.d)).astype(np.int64) % geo.n for ci, m in zip(x, geo.mins)]
    S = np.zeros(geo.N, dtype=LD)
    cnt = np.zeros(geo.N, dtype=np.int64)
    _accumulate(S, cnt, c[2] + geo.n * (c[1] + geo.n * c[0]), LD(1))
    return S, cnt, S.sum()


def cic_density(pos, geo):
    """getDensity_CIC: the coordinate shifted by half a cell and folded (getCICcells), split linearly between the cell
    it falls into and the next one (getCICweights)."""
    n, d, L = geo.n, LD(geo.d), LD(geo.L)
    ok = in_domain(pos, geo)
    c1, dx = [], []
    for c in pos:
        q = np.asarray(c, dtype=np.float64)[ok].astype(LD) - d / 2
        q = np.where(q < 0, q + L, q)  # positions are in [0, L): one fold suffices
        q = np.where(q >= L, q - L, q)
        i = np.floor(q / d).astype(np.int64)
        c1.append(i % n)
        dx.append(q / d - i)
    S = np.zeros(geo.N, dtype=LD)
    cnt = np.zeros(geo.N, dtype=np.int64)
    for a in (0, 1):
        for b in (0, 1):
            for e in (0, 1):
                w = (dx[0] if a else 1 - dx[0]) * (dx[1] if b else 1 - dx[1]) * (dx[2] if e else 1 - dx[2])
                idx = ((c1[2] + e) % n) + n * (((c1[1] + b) % n) + n * ((c1[0] + a) % n))
                _accumulate(S, cnt, idx, w, near=np.ones(len(w), dtype=bool))
    return S, cnt, S.sum()


def tsc_density(pos, geo):
    """getDensity_TSC: quadratic spline weights from the distance to the home cell centre, 27 cells.  Its domain test
    is closed above (massFunctions.cc:195), which only matters for x == min + L."""
    n, d = geo.n, LD(geo.d)
    ok = in_domain(pos, geo, closed=True)
    x = [np.asarray(c, dtype=np.float64)[ok] for c in pos]
    ci = _cells_of(x, geo)
    w = []
    for c, i, m in zip(x, ci, geo.mins):
        dd = (c.astype(LD) - LD(m)) / d - (i + LD(0.5))
        w.append([LD(0.5) * (LD(0.5) - dd) ** 2, LD(0.75) - dd * dd, LD(0.5) * (LD(0.5) + dd) ** 2])
    S = np.zeros(geo.N, dtype=LD)
    cnt = np.zeros(geo.N, dtype=np.int64)
    for a in range(3):
        for b in range(3):
            for e in range(3):
                idx = ((ci[2] + e - 1) % n) + n * (((ci[1] + b - 1) % n) + n * ((ci[0] + a - 1) % n))
                _accumulate(S, cnt, idx, w[0][a] * w[1][b] * w[2][e], near=np.ones(len(idx), dtype=bool))
    return S, cnt, S.sum()


def sph_grad_over_q(q, norm):
    """dW_4/dq / q / (pi h^4) in h units (grad_SPH_kernel_3D_h_units): (2.25 q - 3) for q <= 1, -0.75 (q - 2)^2 / q up
    to q = 2, 0 beyond."""
    q = np.asarray(q, dtype=LD)
    safe = np.where(q > 0, q, 1)
    return norm * np.where(q <= 1, LD(2.25) * q - 3, np.where(q <= 2, LD(-0.75) * (q - 2) ** 2 / safe, 0))


def hull_columns(h, d):
    """The stencil of likelihood_calc_V_SPH: the cells of SPH_kernel_3D_cells (SPH_kernel.cpp:62-102: every offset whose
    per-axis distance (|i| - 1/2) d from the home cell's centre, squared and summed, is within (2 h)^2), reduced by
    SPH_kernel_3D_cells_hull_1 (:110-139) to (i, j) columns with an inclusive k range.  Returns [(i, j, k_begin,
    k_last)]."""
    reach = int(2 * h / d) + 1
    cols = {}
    for i1 in range(-reach, reach + 1):
        for i2 in range(-reach, reach + 1):
            for i3 in range(-reach, reach + 1):
                r2 = sum(((abs(i) - 0.5) * d) ** 2 for i in (i1, i2, i3))
                if r2 <= (2 * h) ** 2:
                    lo, hi = cols.get((i1, i2), (i3, i3))
                    cols[(i1, i2)] = (min(lo, i3), max(hi, i3))
    return [(i1, i2, lo, hi) for (i1, i2), (lo, hi) in cols.items()]


def sph_adjoint_gather(pos, plike, geo, h, rho_c, rsd=False, f1=0.0, q_slack=0.0, dtype=np.float64):
    """likelihood_calc_V_SPH: V_p = rho_c d^3 sum_c part_like_c g(q_pc) x_pc / h over the cells of the stencil hull around
    the particle's home cell (`hull_columns`; g vanishes beyond q = 2, and for h = d the hull holds every cell that can
    be within it) (x_pc: particle minus cell centre), V_z (1 + f1) under RSD.  Particles with a non-finite position get 0.
    Returns (V, A, P, ncell): V (3, N); A (3, N) = sum_c |part_like_c g x / h| with the same factors as V; P (N) = sum of
    |part_like_c| over the cells with q <= 2 + q_slack, times rho_c d^3; ncell (N) = number of those cells."""
    fin = np.ones(geo.N, dtype=bool)
    for c in pos:
        fin &= np.isfinite(c)
    sel = np.flatnonzero(fin)
    V = np.zeros((3, geo.N), dtype=LD)
    A = np.zeros((3, geo.N), dtype=LD)
    P = np.zeros(geo.N, dtype=LD)
    ncell = np.zeros(geo.N, dtype=np.int64)
    V[:, sel], A[:, sel], P[sel], ncell[sel] = _gather_of(pos, plike, geo, h, rho_c, sel, rsd, f1, q_slack, dtype)
    return V, A, P, ncell


def sph_adjoint_gather_at(pos, plike, geo, h, rho_c, particles, rsd=False, f1=0.0, q_slack=0.0, dtype=np.float64):
    """sph_adjoint_gather for the chosen particles only (index array), at the cost of those particles: the gather is a
    sum per particle, so these are the same operations in the same order.  Returns (V, A, P, ncell) of shapes (3, m),
    (3, m), (m), (m) in the order of `particles`; a particle with a non-finite position gets zeros."""
    particles = np.asarray(particles, dtype=np.int64)
    fin = np.ones(len(particles), dtype=bool)
    for c in pos:
        fin &= np.isfinite(np.asarray(c)[particles])
    V = np.zeros((3, len(particles)), dtype=LD)
    A = np.zeros((3, len(particles)), dtype=LD)
    P = np.zeros(len(particles), dtype=LD)
    ncell = np.zeros(len(particles), dtype=np.int64)
    V[:, fin], A[:, fin], P[fin], ncell[fin] = _gather_of(pos, plike, geo, h, rho_c, particles[fin], rsd, f1, q_slack,
                                                          dtype)
    return V, A, P, ncell


def _gather_of(pos, plike, geo, h, rho_c, sel, rsd, f1, q_slack, dtype):
    """The sums of sph_adjoint_gather for the particles `sel` (all with finite positions), compact."""
    n, d = geo.n, LD(geo.d)
    h = LD(h)
    norm = 1 / (_pi() * h ** 4)
    normalize = LD(rho_c) * LD(geo.L) ** 3 / LD(geo.N)
    plike = np.asarray(plike, dtype=np.float64)
    x = [np.asarray(c, dtype=np.float64)[sel] for c in pos]
    hc = [home_cell(c, geo.d, dtype) for c in x]
    xl = [c.astype(LD) for c in x]
    V = np.zeros((3, len(sel)), dtype=LD)
    A = np.zeros((3, len(sel)), dtype=LD)
    P = np.zeros(len(sel), dtype=LD)
    ncell = np.zeros(len(sel), dtype=np.int64)
    lim = (2 + LD(q_slack)) ** 2
    for i1, i2, lo, hi in hull_columns(float(h), geo.d):
        xh = (xl[0] - (hc[0] + i1 + LD(0.5)) * d) / h
        yh = (xl[1] - (hc[1] + i2 + LD(0.5)) * d) / h
        r2ab = xh * xh + yh * yh
        m2 = np.flatnonzero(r2ab <= lim)
        if not len(m2):
            continue
        row = n * (((hc[1][m2] + i2) % n) + n * ((hc[0][m2] + i1) % n))
        for i3 in range(lo, hi + 1):
            zh = (xl[2][m2] - (hc[2][m2] + i3 + LD(0.5)) * d) / h
            q2 = r2ab[m2] + zh * zh
            m3 = np.flatnonzero(q2 <= lim)
            if not len(m3):
                continue
            p = m2[m3]
            pl = plike[row[m3] + (hc[2][m2][m3] + i3) % n].astype(LD)
            g = pl * sph_grad_over_q(np.sqrt(q2[m3]), norm)
            for e, comp in enumerate((xh[m2[m3]], yh[m2[m3]], zh[m3])):
                V[e, p] += g * comp  # p has no duplicates within one offset
                A[e, p] += np.abs(g * comp)
            P[p] += np.abs(pl)
            ncell[p] += 1
    fz = normalize * (1 + LD(f1)) if rsd else normalize
    for arr in (V, A):
        arr[0] *= normalize
        arr[1] *= normalize
        arr[2] *= fz
    return V, A, P * normalize, ncell


def density_shift_derivative(pos, plike, geo, h, axis, step, dtype=np.float64):
    """Central difference of sum_c part_like_c rho_c under a uniform shift of all particles along `axis` (longdouble).
    The home cells are those of the unshifted positions: the density does not depend on which cell the cube is
    centred on, so the difference is that of a smooth function as long as no particle crosses the domain boundary."""
    plike = np.asarray(plike, dtype=np.float64).astype(LD)
    vals = []
    for s in (step, -step):
        # shift in longdouble: done on the coordinates fed to the exact evaluation, not on the stored doubles
        vals.append(_sph_functional(pos, plike, geo, h, axis, LD(s), dtype))
    return (vals[0] - vals[1]) / (2 * LD(step))


def _sph_functional(pos, plike, geo, h, axis, shift, dtype):
    n, d = geo.n, LD(geo.d)
    h = LD(h)
    w_norm = 1 / _pi() / (h * h * h)
    ok = in_domain(pos, geo)
    x = [np.asarray(c, dtype=np.float64)[ok] for c in pos]
    hc = [home_cell(c, geo.d, dtype) for c in x]
    xl = [c.astype(LD) for c in x]
    xl[axis] = xl[axis] + shift
    reach = int(2 * float(h) / geo.d) + 2  # one more than the cube: the shifted particle may reach one cell farther
    total = LD(0)
    for i1 in range(-reach, reach + 1):
        dx = xl[0] - (hc[0] + i1 + LD(0.5)) * d
        for i2 in range(-reach, reach + 1):
            dy = xl[1] - (hc[1] + i2 + LD(0.5)) * d
            r2ab = dx * dx + dy * dy
            m2 = np.flatnonzero(r2ab <= 4 * h * h)
            if not len(m2):
                continue
            row = n * (((hc[1][m2] + i2) % n) + n * ((hc[0][m2] + i1) % n))
            for i3 in range(-reach, reach + 1):
                dz = xl[2][m2] - (hc[2][m2] + i3 + LD(0.5)) * d
                r2 = r2ab[m2] + dz * dz
                m3 = r2 <= 4 * h * h
                if not m3.any():
                    continue
                w = sph_w(np.sqrt(r2[m3]) / h, w_norm)
                total += np.sum(w * plike[row[m3] + (hc[2][m2][m3] + i3) % n])
    return total


# ---- position sets -----------------------------------------------------------------------------------------------------

SPECIAL_SETS = ("centres", "corners", "edges", "faces")
ALL_SETS = SPECIAL_SETS + ("uniform", "collapse_inside", "collapse_corner", "sheet", "filament", "upper_edge",
                           "tiny_negative", "far_out", "mixed")


def position_sets(geo, dtype=np.float64, seed=2024, names=ALL_SETS):
    """name -> psi (3, N) doubles for the position sets of the particle-mesh tests, psi = target - lattice centre.
    d = L / n is a binary fraction in the suite's geometry (L = 200 n / 64), so centres, faces, edges and corners are
    exactly representable and hit exactly in float32 and float64.  `dtype` matters for the two sets made of
    neighbouring floating-point numbers (upper_edge, tiny_negative)."""
    n, d, L, N = geo.n, geo.d, geo.L, geo.N
    rng = np.random.Generator(np.random.Philox(seed))
    c0 = np.array(lattice_centres(geo, np.float64))  # exact: multiples of d / 2
    T = np.dtype(dtype).type
    out = {}

    def from_targets(t):
        return np.asarray(t, dtype=np.float64).reshape(3, N) - c0

    for name in names:
        if name == "centres":
            psi = np.zeros((3, N))
        elif name == "corners":      # the lower corner of the own cell: on three faces at once
            psi = np.full((3, N), -0.5 * d)
        elif name == "edges":        # midpoint of an edge: on two faces
            psi = np.zeros((3, N))
            psi[0], psi[1] = -0.5 * d, -0.5 * d
            psi[:, N // 2:] = np.array([0.0, -0.5 * d, -0.5 * d])[:, None]
        elif name == "faces":        # centre of a face, a different axis for each third of the particles
            psi = np.zeros((3, N))
            third = np.arange(N) % 3
            for a in range(3):
                psi[a, third == a] = -0.5 * d
        elif name == "uniform":
            psi = from_targets(rng.random((3, N)) * L)
        elif name in ("collapse_inside", "collapse_corner"):
            # every particle within 0.3 d of one point: inside a tile, or on the box corner (a tile corner whose halo
            # wraps on all three axes)
            centre = np.array([3.6, 3.3, 5.4]) * d if name == "collapse_inside" else np.zeros(3)
            t = centre[:, None] + (rng.random((3, N)) * 2 - 1) * (0.3 / np.sqrt(3.0)) * d
            psi = t - c0
        elif name == "sheet":        # one cell thick in x
            t = rng.random((3, N)) * L
            t[0] = (n // 2 + rng.random(N)) * d
            psi = from_targets(t)
        elif name == "filament":     # one cell wide in x and y
            t = rng.random((3, N)) * L
            t[0] = (n // 2 + rng.random(N)) * d
            t[1] = (1 + rng.random(N)) * d
            psi = from_targets(t)
        elif name == "upper_edge":   # the plane i = 0 goes to x = nextafter(L, 0) of the storage type
            psi = from_targets(rng.random((3, N)) * L)
            plane = lattice_index(n)[0] == 0
            psi[0, plane] = float(np.nextafter(T(L), T(0))) - c0[0, plane]
        elif name == "tiny_negative":  # the plane j = 0 goes to y = -ulp(d / 2): y + L rounds to L and is folded to 0
            psi = from_targets(rng.random((3, N)) * L)
            plane = lattice_index(n)[1] == 0
            psi[1, plane] = -float(np.nextafter(T(0.5 * d), T(L)))
        elif name == "far_out":      # many box lengths out on every axis, both signs: the fmod branch of pacman
            t = rng.random((3, N)) * L + rng.integers(-7, 8, size=(3, N)) * L * 3
            psi = t - c0
        elif name == "mixed":        # every special point inside one random field
            psi = from_targets(rng.random((3, N)) * L)
            kind = rng.integers(0, 16, size=N)
            for a in range(3):
                psi[a, kind == 1] = 0.0                                  # centres
                psi[a, kind == 2] = -0.5 * d                             # corners
            psi[0, kind == 3] = -0.5 * d                                 # faces
            psi[1, kind == 4] = -0.5 * d
            psi[2, kind == 5] = -0.5 * d
            psi[0, kind == 6], psi[2, kind == 6] = -0.5 * d, -0.5 * d    # edges
            psi[1, kind == 6] = 0.0
            psi[0, kind == 7] = float(np.nextafter(T(L), T(0))) - c0[0, kind == 7]
            low = (kind == 8) & (lattice_index(n)[2] == 0)               # only the lowest plane can hit -ulp exactly
            psi[2, low] = -float(np.nextafter(T(0.5 * d), T(L)))
            far = kind == 9
            psi[:, far] += rng.integers(-5, 6, size=(3, int(far.sum()))) * L * 2
            blob = kind >= 13                                            # a clump: a few crowded cells
            psi[:, blob] = (np.array([1.3, 6.7, 9.2])[:, None] * d + rng.random((3, int(blob.sum()))) * 0.6 * d
                            - c0[:, blob])
        else:
            raise KeyError(name)
        out[name] = psi
    return out
