"""Input sets for the real-space ALPT kernels and the calc_h 0 / 3 kernels (tests/test_rs_bounds.py, tests/test_gpu_rs.py).
Every array is in the storage type T of `prec` and indexed [i, j, k]; the box length is 1.25 n, so that fac = n / (2 L) is not
1 / 2 and kfac is not 2 pi / n.

phi_sets (k_alpt_grad; through the reference's first pass also the g3 of k_alpt_sources, and dX of k_findif_mul):
- white: white Gaussian;  offset: 1e6 plus white noise of 1e-3, which maximises cancellation in the differences;
- axes: f(i) + 10 g(j) + 100 h(k) with distinct f, g, h, so that swapped axes or strides show;
- impulse_*: one unit impulse at the origin, the far corner (n-1, n-1, n-1), an edge cell (0, n-1, n/2) and an interior cell;
- wave_x / _y / _z: cos(2 pi m c / n + 0.3) along one axis (closed-form response: wave_response);
- nonfinite: the white set with one NaN and one +inf.

delta1_special: the delta(1) values of k_alpt_sources around the branch edge and the extremes, for D1 = 0.62.
"""
import numpy as np

from tests import pm_reference as pm
from tests.kstep_inputs import box, row_stride, types

D1, D2 = 0.62, -0.21  # tests/offdefault.py: OFF
SIZES = (4, 5, 8, 9, 16, 24, 83, 88)
FULL = 16


def rng_for(n, seed):
    return np.random.default_rng(seed + 1000 * n)


def impulse_cells(n):
    return {"origin": (0, 0, 0), "corner": (n - 1, n - 1, n - 1), "edge": (0, n - 1, n // 2), "interior": (n // 2, 1, n - 2)}


def wave(n, axis, m=1):
    c = np.arange(n, dtype=np.float64)
    shape = [1, 1, 1]
    shape[axis] = n
    return np.cos(2 * np.pi * m * c / n + 0.3).reshape(shape) + np.zeros((n, n, n))


def wave_response(n, L, axis, m=1):
    """gradfindif of cos(theta c + 0.3), theta = 2 pi m / n:  -fac ((4/3)(cos(th (c-1)) - cos(th (c+1))) - (1/6)(cos(th (c-2)) -
    cos(th (c+2)))) = -fac sin(theta c + 0.3) ((8/3) sin theta - (1/3) sin 2 theta)."""
    LDT = np.longdouble
    pi = LDT("3.14159265358979323846264338327950288")
    th = 2 * pi * m / n
    c = np.arange(n).astype(LDT)
    shape = [1, 1, 1]
    shape[axis] = n
    fac = LDT(n) / (2 * LDT(L))
    return (-fac * np.sin(th * c + LDT(0.3)) * ((LDT(8) / 3) * np.sin(th) - (LDT(1) / 3) * np.sin(2 * th))).reshape(shape)


def phi_sets(n, prec, full=True):
    """[(name, phi)]; full = False: the white set and the impulses."""
    rdt = types(prec)[0]
    rng = rng_for(n, 11)
    out = [("white", rng.standard_normal((n, n, n)).astype(rdt))]
    for name, at in impulse_cells(n).items():
        a = np.zeros((n, n, n), rdt)
        a[at] = 1
        out.append(("impulse_" + name, a))
    if not full:
        return out
    out.append(("offset", (1e6 + 1e-3 * rng.standard_normal((n, n, n))).astype(rdt)))
    f, g, h = rng.standard_normal(n), rng.standard_normal(n) ** 2, np.cos(np.arange(n) * 1.7)
    out.append(("axes", (f[:, None, None] + 10 * g[None, :, None] + 100 * h[None, None, :]).astype(rdt)))
    for axis, nm in enumerate("xyz"):
        out.append(("wave_" + nm, wave(n, axis).astype(rdt)))
    return out


def nonfinite(n, prec):
    """(clean, dirty, cells): the white set, the same with NaN and +inf put in, where they went."""
    clean = phi_sets(n, prec, False)[0][1]
    dirty = clean.copy()
    cells = ((1, n - 1, 0), (n - 2, 2, n // 2))
    dirty[cells[0]] = np.nan
    dirty[cells[1]] = np.inf
    return clean, dirty, cells


def delta1_special(prec):
    """delta(1) in T with D1 delta = 1.5 to the last representable value below, at and above; 10; -1e6; 0; +-1e-12; NaN, +-inf."""
    T = types(prec)[0]
    edge = T(1.5 / D1)
    v = [np.nextafter(edge, T(0)), edge, np.nextafter(edge, T(10)), np.nextafter(np.nextafter(edge, T(0)), T(0)),
         np.nextafter(np.nextafter(edge, T(10)), T(10)), T(10 / D1), T(-1e6 / D1), T(0), T(1e-12), T(-1e-12), T(np.nan),
         T(np.inf), T(-np.inf)]
    return np.array(v, T)


def sources_inputs(phi, n, prec, special=True, seed=5):
    """g3 = the reference's first derivatives of phi rounded once to T (exact inputs of the second pass), delta(1) white
    with the special values in the first cells of row (1, 2)."""
    from tests import rs_reference as ref
    rdt = types(prec)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        g3 = ref.alpt_grad(phi, n, box(n))["g3"].astype(rdt)
    d1 = (0.5 * rng_for(n, seed).standard_normal((n, n, n))).astype(rdt)
    if np.count_nonzero(phi) == 1:   # an impulse: delta(1) = 0, so that a is -D2 m2v alone
        d1[:] = 0
    elif special:
        s = delta1_special(prec)
        flat = d1.reshape(-1)
        flat[n * n + 2 * n: n * n + 2 * n + len(s)] = s
    return g3, d1


def kspace_white(n, prec, seed=3):
    """White half-complex data with NaN in the row padding (rows padded to whole 128-byte lines)."""
    rdt, cdt = types(prec)
    nhp, nh = row_stride(n, rdt, True), n // 2 + 1
    rng = rng_for(n, seed)
    a = (rng.standard_normal((n, n, nhp)) + 1j * rng.standard_normal((n, n, nhp))).astype(cdt)
    a[:, :, nh:] = np.nan
    return a


def kspace_impulses(n, prec):
    """Impulses (1 - 0.5 i) on DC, on the three Nyquist planes (index n / 2, integer division, and its partner at odd n),
    on an edge of them and on ordinary modes, all in one array: the kernels are element-wise."""
    rdt, cdt = types(prec)
    nhp, h = row_stride(n, rdt, True), n // 2
    a = np.zeros((n, n, nhp), cdt)
    for at in ((0, 0, 0), (h, 1, 1), (1, h, 1), (1, 1, h), (h, h, 0), (n - h, 1, 0), (1, n - h, 0), (h, n - h, 0), (1, 2, 1),
               (n - 1, 2, 0), (2, n - 1, h - 1 if h > 1 else 0)):
        a[at] = 1 - 0.5j
    return a


def conv_table(n, prec, seed=9):
    """F (doubles) with a wide range, zeros and negative entries; finite in the row padding."""
    nhp = row_stride(n, types(prec)[0], True)
    rng = rng_for(n, seed)
    F = rng.standard_normal((n, n, nhp)) * 10.0 ** rng.uniform(-3, 3, (n, n, nhp))
    F[rng.random((n, n, nhp)) < 0.1] = 0.0
    return F


LN_RHO_C, LN_DELTA_MIN = 1.7, -0.75  # delta_min exact in float32 too: a neighbour can sit exactly on the clamp


def findif_inputs(n, prec, likelihood, seed=21):
    """dX white (for the log-normal code with neighbours at delta_min, one representable value either side, far below)
    and part_like with zeros and negative entries."""
    rdt = types(prec)[0]
    rng = rng_for(n, seed)
    dX = (0.6 * rng.standard_normal((n, n, n))).astype(rdt)
    if likelihood == 2:
        T = rdt
        dm = T(LN_DELTA_MIN)   # the clamp value as the storage type holds it; the kernel compares with the double
        s = np.array([dm, np.nextafter(dm, T(0)), np.nextafter(dm, T(-2)), T(-5.0), T(-0.999999), dm, T(3.0)], rdt)
        dX.reshape(-1)[n * n + n: n * n + n + len(s)] = s
        dX[n - 1, n - 1, n - 1], dX[0, 0, 0] = dm, np.nextafter(dm, T(-2))
    pl = rng.standard_normal((n, n, n)).astype(rdt)
    pl[rng.random((n, n, n)) < 0.1] = 0
    return dX, pl


TSC_SETS = ("centres", "corners", "faces", "upper_edge", "far_out", "mixed")
TSC_POS = dict(cpecvel=0.9, v_norm=0.013)
TSC_F1 = 0.52


def tsc_inputs(n, prec, names=TSC_SETS, seed=31):
    """[(name, psi (3, N) in T)] from the position sets of tests/pm_reference.py, the last particles of each set NaN / inf,
    and conv (3, n, n, n) that depends on i, j and k separately (so that taking dz for the upper x and y weights shows)."""
    rdt = types(prec)[0]
    geo = pm.Geometry(n, box(n))
    rng = rng_for(n, seed)
    sets = []
    for name, psi in pm.position_sets(geo, rdt, names=names).items():
        psi = psi.astype(rdt)
        psi[0, -1], psi[1, -2], psi[2, -3] = np.nan, np.inf, -np.inf
        sets.append((name, psi))
    f, g, h = rng.standard_normal((3, n)), rng.standard_normal((3, n)), rng.standard_normal((3, n))
    conv = np.array([f[c][:, None, None] + 10 * g[c][None, :, None] + 100 * h[c][None, None, :] for c in range(3)]).astype(rdt)
    return geo, sets, conv


COLLAPSE_SCALE = 2.0


def collapse_case(nx):
    """(case, delta(1)): the suite's seeded ALPT case at the OFF scalars and its initial field times COLLAPSE_SCALE, which
    puts D1 delta(1) >= 1.5 -- the spherical-collapse branch of k_alpt_sources -- in about 12 % of the cells and keeps
    every cell 1e-6 away from the branch edge (tests/test_rs_bounds.py: test_collapse_case_reaches_the_branch)."""
    from tests.offdefault import OFF
    from tests.util import Case
    c = Case(Nx=nx, likelihood=1, rsd_model=0, sfmodel=2, **OFF)
    return c, COLLAPSE_SCALE * c.q0
