"""The bounds the generic trajectory's real-space mass and GRF kernels are held to, cell by cell, the value sets both test
files use, and float64 / float32-storage restatements of the kernels' operation order with the wrong kernels the checker has
to reject (tests/test_massrs_bounds.py on the CPU, tests/test_gpu_massrs.py on the device; reference:
tests/massrs_reference.py).

Notation.  u_d = 2^-53: the kernels compute in double on every handle.  u_T: the rounding of a double to the storage type
at a store, 2^-24 on fp32 handles and 0 on fp64 handles (a double is stored as it is).  sub_T: the smallest subnormal of T.

The bounds are counted from the operation lists, one u per rounded operation, and are used as they stand (no constant, no
margin):

  k_div_mass_r   out = (T)(p * (1 / m)) where m > 0, else 0:  1 / m, the product, the store
                     (2 u_d + u_T) |ref|  +  sub_T  +  |p| 2^-1075 where 1 / m < 2^-1022
                 The last term is a correction of the count: on fp64 handles the largest finite mass has 1 / m = 5.6e-309, a
                 subnormal double, whose rounding is absolute (half a subnormal of double) and reaches the output times |p|
                 -- 500 subnormals of the result at |p| = 1e3.  A cell with m <= 0 or NaN has bound 0: exactly 0.
  k_grf_grad     out = (T)((q - nobs) / (s * s)) where w > 0, else 0:  difference, square, quotient, store
                     (3 u_d + u_T) |ref|  +  sub_T
                 sub_T corrects the count for the store's underflow (a huge noise on an fp32 handle: 1e-60 is stored as 0).
  k_add_r        out = a + b in T: one rounding of T's own arithmetic, u(T) |ref| with u(T) = 2^-24 or 2^-53 (here alone the
                 fp64 handle has a rounding: the sum is taken in double).  Sums in the subnormal range are exact.
  k_scale_c      per component (T)(x * s):  (u_d + u_T) |ref|  +  sub_T
  k_kin_rs       term = (0.5 p) ((1 / m) p): three roundings (0.5 p is exact), 3 u_d |term|
  k_grf_loglike  term = 0.5 (t t), t = (q - nobs) / s: t carries 2 u_d, its square 4 u_d and one more, 5 u_d |term|
  both sums      a thread adds its k terms one after the other (k = the turns of the grid-stride loop that reach its block),
                 the workgroup adds the 256 thread sums in 6 + 2 tree levels (block_sum: wave_sum over 64 lanes, then over
                 the 4 wave sums; the other 60 lanes add exact zeros):
                     |partial^ - partial|  <=  (c + k + 8) u_d  sum |term|  +  cells 2^-1074 (1 + |p| + p^2 / 2)
                 over exactly the cells the block owns, c = 3 or 5.  The last term stands for intermediates in double's
                 subnormal range (1 / m of the largest mass, the square of a tiny t; p = 0 in the GRF sum); it is 1e-318 per
                 cell and only cells whose guard is open have it.  A block that owns no cell, or only masked ones, has bound 0.
                 The total (the longdouble sum of the 1024 partials: the host's own addition is not under test) has the sum
                 of the partials' bounds.  It follows from the partials and adds a check of sign and bias only; on the
                 "confined" sets it is non-finite beyond a few hundred cells and judged by class, on the "moderate" sets
                 (no extremes, every term finite) by value at every size.
  Non-finite     where the reference is NaN, +inf or -inf the result must be that class (tests/like_bound.py::worst_fraction).

No cell is excluded from any comparison.  The kernels decide nothing except m > 0 and w > 0, and the sets put values ON those
edges (+0, -0, NaN, the smallest subnormal) and nowhere near them otherwise; the same holds for the edges of double's and T's
range (massrs_reference.near_edge).

MEASURED: the worst fraction of its bound every kernel reaches over all sets, restatement (rounded up to two digits) and
MI355X (four digits).  The restatement rounds every operation once and the device may contract multiply-adds, yet the worst
cells are the same on both and agree to the four digits: a single rounding that uses its half ulp up (fractions near 1 where
an output is one rounded value stored once), and sums whose errors add up like a random walk, far below their counted sum.
"""
import functools

import numpy as np

from tests import like_bound as lb
from tests import massrs_reference as ref

LD = np.longdouble
UD = LD(2.0) ** -53
TINY_D = LD(2.0) ** -1074
FILL = -7.25
TREE_LEVELS = 8
TERM_ROUNDINGS = {"kin_rs": 3, "grf_loglike": 5}

# kernel -> storage type -> (restatement, device); asserted by tests/test_massrs_bounds.py (restatement) and printed by
# tests/test_gpu_massrs.py (device)
MEASURED = {
    "div_mass_r": {"float32": (1.0, 0.9994), "float64": (0.98, 0.9733)},
    "kin_rs": {"float32": (0.44, 0.4382), "float64": (0.35, 0.3428)},
    "grf_grad": {"float32": (1.0, 0.9993), "float64": (0.91, 0.9079)},
    "grf_loglike": {"float32": (0.33, 0.3264), "float64": (0.34, 0.3314)},
    "scale_c": {"float32": (1.0, 0.9985), "float64": (1.0, 0.999)},
    "add_r": {"float32": (1.0, 1.0), "float64": (1.0, 1.0)},
}

FULL = ref.RED_BLOCKS * ref.RED_THREADS
COUNTS = (1, 255, 256, 257, 729, 4096, 2048 * 256 + 3)   # the last: past nblk_stride's cap, the stride loop turns
SUM_COUNTS = COUNTS[:-1] + (FULL + 3, COUNTS[-1])        # FULL + 3: three threads of block 0 take a second cell
ENTRY_N = (8, 9, 16)
JASCHE_EPS_SCALE = 0.1   # Case's own Gaussian-likelihood step: the masked Jasche mass is as well conditioned (measured in
                         # tests/test_massrs_bounds.py::test_oracle_conditioning)


def u_store(dtype):
    return LD(2.0) ** -24 if np.dtype(dtype) == np.float32 else LD(0)


def u_arith(dtype):
    return LD(2.0) ** -24 if np.dtype(dtype) == np.float32 else UD


def sub(dtype):
    return LD(np.finfo(dtype).smallest_subnormal)


# ---- the value sets ---------------------------------------------------------------------------------------------------------
SUM_SETS = ("confined", "moderate")


def _wide_ok(count, confined):
    """Where the extreme values may stand: everywhere (False), or, for the two sums, only in the cells of blocks 1, 5, 9, ...
    ("confined" or True), so that an infinite or NaN term spoils one partial in four and the others are judged by value, or
    nowhere ("moderate"): every term is finite -- the guard values and the window cycle stay -- and the total is judged by
    value at every size."""
    if confined == "moderate":
        return np.zeros(count, dtype=bool)
    return (ref.owner_block(count) % 4 == 1) if confined else np.ones(count, dtype=bool)


def _decades(dtype):
    return (-300.0, 300.0) if np.dtype(dtype) == np.float64 else (-37.0, 38.0)


def mass_inputs(count, dtype, confined=False):
    """p, mass_r.  mass_r: positives over the decades T holds (moderate decades outside the confined blocks), every seventh
    cell one of +0, -0, -1, NaN, +inf, every eleventh (where extremes may stand) the smallest subnormal or the largest finite
    value of T.  p: both signs over six decades, every fifth cell an exact zero of either sign -- cell 5 (mod 55) has p = 0
    under the smallest subnormal mass, whose 1 / m is infinite in double on an fp64 handle: 0 * inf."""
    dtype = np.dtype(dtype)
    rng = np.random.Generator(np.random.Philox(3000 + count))
    i = np.arange(count)
    ok = _wide_ok(count, confined)
    lo, hi = _decades(dtype)
    m = np.where(ok, 10.0 ** rng.uniform(lo, hi, count), 10.0 ** rng.uniform(-3, 3, count)).astype(dtype)
    guard = np.array([0.0, -0.0, -1.0, np.nan, np.inf], dtype=dtype)
    g = i % 7 == 3
    m[g] = guard[(i[g] // 7) % guard.size]
    ext = np.array([np.finfo(dtype).smallest_subnormal, np.finfo(dtype).max], dtype=dtype)
    x = (i % 11 == 5) & ok
    m[x] = ext[(i[x] // 11) % 2]
    p = (rng.standard_normal(count) * 10.0 ** rng.uniform(-3, 3, count)).astype(dtype)
    p[i % 5 == 0] = 0.0
    p[i % 10 == 5] = -0.0
    return p, m


def grf_inputs(count, dtype, confined=False):
    """q, nobs, noise, window.  window cycles through 1, 0, 1, -0.0, 1, -1, 0.5, NaN, 1, the smallest subnormal; q == nobs in
    every sixth cell and q = 0 in every fifth; noise is 10^U(-2, 2) with, in every thirteenth cell (where extremes may stand),
    0, a tiny, a huge, a tinier and a huger value: on fp64 handles 1e-150 and 1e150 (squares inside double's range), 1e-170
    and 1e170 (squares that leave it); on fp32 handles 1e-30, 1e30, the smallest subnormal and the largest finite float.
    Cell 4 (mod 390) has q == nobs over noise == 0 under an open window: 0 / 0."""
    dtype = np.dtype(dtype)
    rng = np.random.Generator(np.random.Philox(5000 + count))
    i = np.arange(count)
    ok = _wide_ok(count, confined)
    q = (rng.standard_normal(count) * 10.0 ** rng.uniform(-3, 3, count)).astype(dtype)
    q[i % 5 == 0] = 0.0
    nobs = (rng.standard_normal(count) * 10.0 ** rng.uniform(-3, 3, count)).astype(dtype)
    same = i % 6 == 4
    nobs[same] = q[same]
    wcycle = np.array([1.0, 0.0, 1.0, -0.0, 1.0, -1.0, 0.5, np.nan, 1.0, np.finfo(dtype).smallest_subnormal], dtype=dtype)
    window = wcycle[i % wcycle.size]
    noise = (10.0 ** rng.uniform(-2, 2, count)).astype(dtype)
    if dtype == np.float64:
        special = np.array([0.0, 1e-150, 1e150, 1e-170, 1e170])
    else:
        special = np.array([0.0, 1e-30, 1e30, np.finfo(dtype).smallest_subnormal, np.finfo(dtype).max], dtype=dtype)
    s = (i % 13 == 4) & ok
    noise[s] = special[(i[s] // 13) % special.size]
    return q, nobs, noise, window


def scale_inputs(count, dtype):
    """Complex values over the decades of T with zeros of either sign, and the scale 1 / 729 (the generic path's 1 / N)."""
    dtype = np.dtype(dtype)
    rng = np.random.Generator(np.random.Philox(7000 + count))
    lo, hi = _decades(dtype)
    z = np.empty((count, 2), dtype=dtype)
    for c in range(2):
        z[:, c] = (rng.standard_normal(count) * 10.0 ** rng.uniform(lo + 2, hi - 2, count)).astype(dtype)
    z[::5, 0] = 0.0
    z[3::7, 1] = -0.0
    ct = np.complex128 if dtype == np.float64 else np.complex64
    return np.ascontiguousarray(z).view(ct).ravel(), 1.0 / 729.0


def add_inputs(count, dtype):
    """a, b: both signs over six decades; every fourth cell b = -a (an exact zero), every ninth both the largest finite T
    (an infinity), every tenth two subnormals."""
    dtype = np.dtype(dtype)
    rng = np.random.Generator(np.random.Philox(9000 + count))
    a = (rng.standard_normal(count) * 10.0 ** rng.uniform(-3, 3, count)).astype(dtype)
    b = (rng.standard_normal(count) * 10.0 ** rng.uniform(-3, 3, count)).astype(dtype)
    b[::4] = -a[::4]
    a[4::9] = b[4::9] = np.finfo(dtype).max
    a[7::10], b[7::10] = 3 * np.finfo(dtype).smallest_subnormal, 5 * np.finfo(dtype).smallest_subnormal
    return a, b


def entry_mass_r(c, seed=515):
    """The real-space mass of the entry-point cases: Case's (|GRF| + 0.5, rounded to float so that fp32 handles hold it
    exactly) with 20 % zeros, 5 % negatives and 2 % NaN."""
    rng = np.random.Generator(np.random.Philox(seed))
    m = np.asarray(c.mass_r, dtype=np.float64).astype(np.float32).astype(np.float64)
    r = rng.random(m.shape)
    m[r < 0.20] = 0.0
    neg = (r >= 0.20) & (r < 0.25)
    m[neg] = -m[neg]
    m[(r >= 0.25) & (r < 0.27)] = np.nan
    return m


@functools.lru_cache(maxsize=None)
def entry_case(kind, n):
    """The entry-point cases both test files use: "mass0" / "mass5" (Gaussian likelihood, mass_type 0 / 5, entry_mass_r in
    the case and in its oracle) and "grf" (likelihood 3 with 30 % of the window zero)."""
    from tests.util import Case
    if kind == "grf":
        return Case(Nx=n, likelihood=3, window_zero_fraction=0.3)
    c = Case(Nx=n, likelihood=1, mass_type={"mass0": 0, "mass5": 5}[kind])
    c.mass_r = entry_mass_r(c)
    c.oracle.set(mass_r=c.mass_r)
    return c


# ---- the checks: (worst fraction of the bound, flat index) ----------------------------------------------------------------------
def _abs_fin(x):
    return np.abs(np.where(np.isfinite(x), x, LD(0)))


def check_div_mass_r(got, p, m, dtype):
    want = ref.as_storage(ref.div_mass_r(p, m), dtype)
    inv = ref.inv_mass(m)
    b = (2 * UD + u_store(dtype)) * _abs_fin(want) + sub(dtype) + np.where(inv < LD(2.0) ** -1022, np.abs(ref.ld(p)) * TINY_D / 2, 0)
    b = np.where(ref.ld(m) > 0, b, LD(0))
    return lb.worst_fraction(got, want, b)


def check_grf_grad(got, q, nobs, noise, window, dtype):
    want = ref.as_storage(ref.grf_grad(q, nobs, noise, window), dtype)
    b = np.where(ref.ld(window) > 0, (3 * UD + u_store(dtype)) * _abs_fin(want) + sub(dtype), LD(0))
    return lb.worst_fraction(got, want, b)


def check_scale_c(got, z, s, dtype):
    """got, z: complex arrays; the worse of the two components."""
    got = np.asarray(got).ravel()
    worst = (0.0, 0)
    for want, g in zip(ref.scale_c(z, s), (got.real, got.imag)):
        want = ref.as_storage(want, dtype)
        worst = max(worst, lb.worst_fraction(g, want, (UD + u_store(dtype)) * _abs_fin(want) + sub(dtype)))
    return worst


def check_add_r(got, a, b, dtype):
    want = ref.as_storage(ref.add_r(a, b), dtype)
    return lb.worst_fraction(got, want, u_arith(dtype) * _abs_fin(want))


def _check_sum(kernel, partials, terms, open_cells, p_abs):
    """Every partial against the longdouble sum of its block's cells, then the total; index RED_BLOCKS means the total."""
    partials = np.asarray(partials, dtype=np.float64).ravel()
    if partials.size != ref.RED_BLOCKS:
        return np.inf, -1
    want = ref.as_double(ref.block_sums(terms))
    tiny = TINY_D * np.where(open_cells, 1 + p_abs + p_abs * p_abs / 2, LD(0))
    k = ref.trips(terms.size).astype(LD)
    b = (TERM_ROUNDINGS[kernel] + k + TREE_LEVELS) * UD * ref.block_sums(_abs_fin(terms)) + ref.block_sums(tiny)
    f, at = lb.worst_fraction(partials, want, b)
    with np.errstate(invalid="ignore", over="ignore"):
        ft, _ = lb.worst_fraction(np.array([np.sum(partials.astype(LD))]), np.array([np.sum(want)]), np.array([np.sum(b)]))
    return (ft, ref.RED_BLOCKS) if ft > f else (f, at)


def check_kin_rs(partials, p, m):
    return _check_sum("kin_rs", partials, ref.kin_terms(p, m), ref.ld(m) > 0, np.abs(ref.ld(p)))


def check_grf_loglike(partials, q, nobs, noise, window):
    return _check_sum("grf_loglike", partials, ref.grf_terms(q, nobs, noise, window), ref.ld(window) > 0, LD(0) * ref.ld(q))


# ---- restatements of the kernels' operation order: float64 arithmetic, `dtype` storage -------------------------------------------
MASS_MUTANTS = ("m_ge_0", "m_ne_0", "fabs_m", "no_guard", "inverse_twice")
KIN_MUTANTS = MASS_MUTANTS + ("half_dropped",)
WINDOW_MUTANTS = ("w_ne_0", "w_times")
GRAD_MUTANTS = WINDOW_MUTANTS + ("noise_not_squared", "sign_flipped")
LOGLIKE_MUTANTS = WINDOW_MUTANTS + ("square_over_sigma",)
SUM_MUTANTS = ("second_trip_dropped", "idle_blocks_unwritten")


def _f64(*arrays):
    return [np.ascontiguousarray(a).ravel().astype(np.float64) for a in arrays]


def _inv_mass64(m, mut):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mut == "fabs_m":
            m = np.abs(m)
        on = {"m_ge_0": m >= 0, "m_ne_0": m != 0, "no_guard": np.ones(m.shape, dtype=bool)}.get(mut, m > 0)
        return on, 1.0 / m


def div_mass_r64(p, m, dtype, mut=None):
    p, m = _f64(p, m)
    on, inv = _inv_mass64(m, mut)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = p * inv
        if mut == "inverse_twice":
            v = v * inv
        return np.where(on, v, 0.0).astype(dtype)


def kin_terms64(p, m, mut=None):
    p, m = _f64(p, m)
    on, inv = _inv_mass64(m, mut)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        inv = np.where(on, inv, 0.0)
        if mut == "inverse_twice":
            inv = inv * inv
        return ((1.0 if mut == "half_dropped" else 0.5) * p) * (inv * p)


def _window64(w, mut):
    with np.errstate(invalid="ignore"):
        return (w != 0) if mut == "w_ne_0" else (w > 0)


def grf_grad64(q, nobs, noise, window, dtype, mut=None):
    q, nobs, s, w = _f64(q, nobs, noise, window)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        d = (nobs - q) if mut == "sign_flipped" else (q - nobs)
        v = d / (s if mut == "noise_not_squared" else s * s)
        if mut == "w_times":
            return np.where(w != 0, w * v, 0.0).astype(dtype)
        return np.where(_window64(w, mut), v, 0.0).astype(dtype)


def grf_terms64(q, nobs, noise, window, mut=None):
    q, nobs, s, w = _f64(q, nobs, noise, window)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if mut == "square_over_sigma":
            v = 0.5 * ((q - nobs) * (q - nobs) / s)
        else:
            t = (q - nobs) / s
            v = 0.5 * (t * t)
        if mut == "w_times":
            return np.where(w != 0, w * v, 0.0)
        return np.where(_window64(w, mut), v, 0.0)


def block_sum64(terms, mut=None):
    """The 1024 partials as the kernels form them: a thread adds its cells turn by turn, block_sum's tree adds the threads."""
    terms = np.asarray(terms, dtype=np.float64).ravel()
    turns = -(-terms.size // FULL)
    pad = np.zeros(turns * FULL)
    pad[:terms.size] = terms
    pad = pad.reshape(turns, ref.RED_BLOCKS, 4, 64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.zeros(pad.shape[1:])
        for j in range(1 if mut == "second_trip_dropped" else turns):
            v = v + pad[j]
        off = 32
        while off:
            v[..., :off] = v[..., :off] + v[..., off:2 * off]
            off //= 2
        r = v[..., 0]
        out = (r[:, 0] + r[:, 2]) + (r[:, 1] + r[:, 3])
    if mut == "idle_blocks_unwritten":
        out[ref.trips(terms.size) == 0] = FILL
    return out


def scale_c64(z, s, dtype):
    z = np.ascontiguousarray(z).ravel()
    with np.errstate(over="ignore", under="ignore"):
        out = np.empty((z.size, 2), dtype=dtype)
        out[:, 0] = (z.real.astype(np.float64) * s).astype(dtype)
        out[:, 1] = (z.imag.astype(np.float64) * s).astype(dtype)
    return out.view(np.complex128 if np.dtype(dtype) == np.float64 else np.complex64).ravel()


def add_r64(a, b, dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, dtype=dtype) + np.asarray(b, dtype=dtype)).astype(dtype)
