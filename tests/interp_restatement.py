"""numpy restatement of the reference's grid interpolators for a free particle list: ``interpolate_CIC`` (array form,
barlib/src/interpolate_grid.cpp:108-120 with :82-103 and getCICcells / getCICweights :27-79), ``interpolate_TSC``
(:194-202 with :134-191) and ``interpolate_TSC_multi`` (:271-286 with :207-268) -- each statement for statement as a
literal loop over the particles (Python floats: IEEE double, no contraction) and in vectorised form, in which every
numpy operation is one IEEE double operation per element, so the results are the loop's bits.

What the engine adds to the reference is carried here too:

* the storage type of an fp32 handle: a position is converted to float first (the domain test, the cells and the weights
  see the float's value), a field value is read as float and widened; the arithmetic stays double;
* the domain: CIC folds every finite coordinate; TSC upstream casts ``xp / d`` to unsigned without a test, and the engine
  keeps a particle only if ``0 <= x`` and ``(unsigned)(x / d) < n`` on every axis -- stated here as ``x / d < n``, the
  same set wherever the cast is defined; a non-finite coordinate is lost under either kernel.  A lost particle's values
  are quiet NaNs.

The slip of :166-167 (``wx[2]`` and ``wy[2]`` computed from ``dz``) is kept.  ``mutant`` switches one property off, for
the tests that show the edge set tells the restatement from each wrong version:
``"no_slip"``, ``"no_half_shift"``, ``"no_second_fold"``, ``"domain_x_lt_L"``.
"""
import math

import numpy as np

CIC, TSC = 1, 2
KERNELS = dict(cic=CIC, tsc=TSC)
MUTANTS = ("no_slip", "no_half_shift", "no_second_fold", "domain_x_lt_L")
CIC_ORDER = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


def storage(a, dtype):
    """A double array as a handle of storage type ``dtype`` holds it, widened again."""
    with np.errstate(over="ignore"):  # a double beyond the float range becomes an infinity, as on the device
        return np.ascontiguousarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


# ---- literal loops --------------------------------------------------------------------------------------------------
def _pacman(x, L, mutant=None):
    """pacman_coordinate, pacman.cpp:20-28"""
    if x < 0.:
        x = math.fmod(x, L)
        x += L
    if x >= L and mutant != "no_second_fold":
        x = math.fmod(x, L)
    return x


def cic_one(n, L, d, xp, yp, zp, fields, mutant=None):
    """interpolate_CIC, interpolate_grid.cpp:82-103, for every field of ``fields`` ([K][n, n, n]).  None: lost."""
    if not (math.isfinite(xp) and math.isfinite(yp) and math.isfinite(zp)):
        return None
    c1, c2, dx, tx = [], [], [], []
    for p in (xp, yp, zp):
        pos = p - 0.5 * d if mutant != "no_half_shift" else p  # getCICcells :31-33, getCICweights :60-62
        pos = _pacman(pos, L, mutant)
        c = int(pos / d)          # :39-41
        c = (c + n) % n           # :43-45
        c1.append(c)
        c2.append((c + 1) % n)    # :47-49
        dx.append(pos / d - float(c))  # :72-74
        tx.append(1. - dx[-1])         # :76-78
    cell = (c1, c2)
    w = (tx, dx)
    out = []
    for f in fields:
        o = None
        for (a, b, c) in CIC_ORDER:  # :92-99
            term = float(f[cell[a][0], cell[b][1], cell[c][2]]) * w[a][0] * w[b][1] * w[c][2]
            o = term if o is None else o + term
        out.append(o)
    return out


def tsc_one(n, L, d, xp, yp, zp, fields, mutant=None):
    """interpolate_TSC_multi for one particle, interpolate_grid.cpp:207-268 (one field: interpolate_TSC, :134-191)."""
    kern = []
    for p in (xp, yp, zp):
        if math.isnan(p) or math.isinf(p):
            return None
        q = p / d  # :217-219
        if mutant == "domain_x_lt_L":
            if not (0. <= p < L):
                return None
        elif not (p >= 0. and q < float(n)):
            return None
        kern.append(q)
    cell = [int(q) for q in kern]                               # :221-223
    dd = [q - (float(c) + 0.5) for q, c in zip(kern, cell)]     # :225-231
    w = [[0.] * 3 for _ in range(3)]
    for a in range(3):
        w[a][1] = 0.75 - dd[a] * dd[a]                          # :235-237
        t = 1.5 - abs(dd[a] + 1)
        w[a][0] = 0.5 * (t * t)                                 # :238-240
        t = 1.5 - abs((dd[a] if mutant == "no_slip" else dd[2]) - 1)
        w[a][2] = 0.5 * (t * t)                                 # :241-243, wx[2] and wy[2] from dz
    ix = [[(c - 1 + n) % n, c % n if mutant == "domain_x_lt_L" else c, (c + 1) % n] for c in cell]  # :246-255
    out = [0.] * len(fields)
    for i in range(3):
        for j in range(3):
            for k in range(3):
                for m, f in enumerate(fields):
                    out[m] += w[0][i] * w[1][j] * w[2][k] * float(f[ix[0][i], ix[1][j], ix[2][k]])  # :265
    return out


def interpolate_loops(kernel, n, L, x, y, z, fields, dtype=np.float64, mutant=None):
    """The array forms (:108-120, :194-202, :271-286) as loops.  Returns (values[K, n_part], lost[n_part])."""
    d = L / float(n)
    xs, ys, zs = (storage(a, dtype) for a in (x, y, z))
    fs = [storage(f, dtype).reshape(n, n, n) for f in fields]
    one = cic_one if kernel == CIC else tsc_one
    out = np.full((len(fs), xs.size), np.nan)
    lost = np.zeros(xs.size, dtype=bool)
    for p in range(xs.size):
        v = one(n, L, d, float(xs[p]), float(ys[p]), float(zs[p]), fs, mutant)
        if v is None:
            lost[p] = True
        else:
            out[:, p] = v
    return out, lost


# ---- vectorised -----------------------------------------------------------------------------------------------------
def _pacman_v(x, L, mutant=None):
    with np.errstate(invalid="ignore"):
        neg = x < 0.
        x = np.where(neg, np.fmod(x, L) + L, x)
        if mutant != "no_second_fold":
            x = np.where(x >= L, np.fmod(x, L), x)
    return x


def interpolate(kernel, n, L, x, y, z, fields, dtype=np.float64, mutant=None):
    """The same as ``interpolate_loops``, vectorised over the particles: the same operations in the same order."""
    d = L / float(n)
    pos = [storage(a, dtype) for a in (x, y, z)]
    fs = [storage(f, dtype).reshape(n, n, n) for f in fields]
    m = pos[0].size
    finite = np.isfinite(pos[0]) & np.isfinite(pos[1]) & np.isfinite(pos[2])
    out = np.full((len(fs), m), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        if kernel == CIC:
            keep = finite
            p = [np.where(keep, a, 0.) for a in pos]
            cell, w = [[], []], [[], []]
            for a in p:
                q = a - 0.5 * d if mutant != "no_half_shift" else a
                q = _pacman_v(q, L, mutant)
                c = (q / d).astype(np.int64)
                c = (c + n) % n
                dx = q / d - c.astype(np.float64)
                cell[0].append(c)
                cell[1].append((c + 1) % n)
                w[0].append(1. - dx)
                w[1].append(dx)
            for k, f in enumerate(fs):
                o = None
                for (a, b, c) in CIC_ORDER:
                    term = ((f[cell[a][0], cell[b][1], cell[c][2]] * w[a][0]) * w[b][1]) * w[c][2]
                    o = term if o is None else o + term
                out[k] = o
        else:
            if mutant == "domain_x_lt_L":
                keep = finite & np.all([(a >= 0.) & (a < L) for a in pos], axis=0)
            else:
                keep = finite & np.all([(a >= 0.) & (a / d < float(n)) for a in pos], axis=0)
            p = [np.where(keep, a, 0.) for a in pos]
            kern = [a / d for a in p]
            cell = [q.astype(np.int64) for q in kern]
            dd = [q - (c.astype(np.float64) + 0.5) for q, c in zip(kern, cell)]
            w = [[None] * 3 for _ in range(3)]
            for a in range(3):
                w[a][1] = 0.75 - dd[a] * dd[a]
                t = 1.5 - np.abs(dd[a] + 1)
                w[a][0] = 0.5 * (t * t)
                t = 1.5 - np.abs((dd[a] if mutant == "no_slip" else dd[2]) - 1)
                w[a][2] = 0.5 * (t * t)
            ix = [[(c - 1 + n) % n, c % n if mutant == "domain_x_lt_L" else c, (c + 1) % n] for c in cell]
            for k, f in enumerate(fs):
                o = np.zeros(m)
                for i in range(3):
                    for j in range(3):
                        for kk in range(3):
                            o = o + ((w[0][i] * w[1][j]) * w[2][kk]) * f[ix[0][i], ix[1][j], ix[2][kk]]
                out[k] = o
    out[:, ~keep] = np.nan
    return out, ~keep


def interpolate_CIC(n, L, x, y, z, field, dtype=np.float64):
    return interpolate(CIC, n, L, x, y, z, [field], dtype)[0][0]


def interpolate_TSC(n, L, x, y, z, field, dtype=np.float64):
    return interpolate(TSC, n, L, x, y, z, [field], dtype)[0][0]


def interpolate_TSC_multi(n, L, x, y, z, fields, dtype=np.float64):
    return interpolate(TSC, n, L, x, y, z, fields, dtype)[0]


def bits(a):
    """The bit patterns of a double array, every NaN as one pattern (the engine writes the quiet NaN 0x7ff8...)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7ff8000000000000)
    return b


# ---- the positions that decide ----------------------------------------------------------------------------------------
def edge_values(n, L, tile=(8, 8, 16)):
    """Coordinates along one axis at which an interpolator can go wrong on an n-cell grid of side L."""
    d = L / float(n)
    na = np.nextafter
    v = [0., -0., d / 2, na(d / 2, 0.), na(d / 2, L), na(L, 0.), L, na(L, 2 * L), L - d / 2, na(L - d / 2, 0.),
         na(L - d / 2, L), -d / 4, -d / 2, -L / 3, -L, -1.75 * L, -1e-300, -1e300, 1.25 * L, 2 * L, 2.5 * L, 7.3 * L, 1e300,
         np.nan, np.inf, -np.inf, L * (1 - 2.0 ** -30), d * 0.999999, 4294967296.0 * d, 4294967297.5 * d]
    for k in range(n + 1):  # cell faces and their neighbours in double
        v += [k * d, na(k * d, -1.), na(k * d, 2 * L), (k + 0.5) * d]
    for t in set(tile):     # tile faces
        for k in range(0, n + 1, t):
            v += [k * d, na(k * d, -1.), k * d + d / 2, na(k * d + d / 2, -1.), k * d - d / 2]
    return np.array(v)


def edge_set(n, L, seed=0, tile=(8, 8, 16), n_uniform=0):
    """A few hundred positions: every edge value on one axis against a spread of values on the other two, the edge values
    on all three axes at once (tile corners among them), and ``n_uniform`` uniform particles in [0, L)."""
    rng = np.random.default_rng(seed)
    v = edge_values(n, L, tile)
    ok = rng.uniform(0., L, size=(3, v.size))
    cols = [[], [], []]
    for axis in range(3):       # one edge coordinate, the others inside
        for a in range(3):
            cols[a].append(v if a == axis else ok[a])
    for a in range(3):          # three at once, and permuted against each other
        cols[a].append(v)
        cols[a].append(rng.permutation(v))
    if n_uniform:
        u = rng.uniform(0., L, size=(3, n_uniform))
        for a in range(3):
            cols[a].append(u[a])
    return tuple(np.concatenate(c) for c in cols)
