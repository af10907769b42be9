"""The error bounds the Philox momentum draw is held to, value by value (tests/test_draw_bounds.py measures the constants
on the CPU and shows that the checker rejects wrong draws, tests/test_gpu_draw.py applies the bounds to the kernels and to
bchmc_chain_draw_momenta; tests/draw_restatement.py supplies the longdouble reference).

u = 2^-53 throughout (both kernels compute in double on every handle), u_T is the unit round-off of the storage type.

(1) White noise, per value.  g = rad cos(theta) s or rad sin(theta) s with rad = sqrt(-2 ln u1), theta = 2 pi u2, s = sqrt(var)
    or 1; u1, u2 are exact inputs.  log, sqrt and the product cost a few u of rad; theta is 2 pi (rounded) times u2 (one
    rounding): an absolute error of about u theta in the angle, which moves cos / sin by as much, plus their own u; s is one
    sqrt; the store rounds once to the storage type:

        |g^ - g|  <=  C_w u rad (1 + theta) s  +  u_T |g|

    var <= 0 must give exactly 0 and rad = 0 exactly 0; a value whose reference is +-inf (var = +inf) must be that infinity.

(2) Colouring, per real and per imaginary part.  out = w a [+ old], a = 1 / sqrt(wM) (sqrt, division, product, sum: each
    one rounding), stored once:

        |out^ - out|  <=  C_c u (|w| a + |old|)  +  u_T |out|

    wM <= 0 must give exactly old (or 0).

(3) The whole draw, p = irfftn(rfftn(w0) a) + sqrt(mass_r) w1 through bchmc_chain_get_momenta (the device carries the second
    part through a transform pair as well).  A transform of N = n^3 points loses C log2(N) u_T of its input's norm
    (tests/fft_bound.py); the forward transform's error is scaled by the colouring before it comes back, so the scale is

        S  =  max_k a_k ||w0||_2  +  ||sqrt(mass_r) w1||_2           (not ||p||: a is far from flat)

        max |p^ - p|  <=  C_e log2(N) u_T S      and      ||p^ - p||_2  <=  C_e log2(N) u_T S

    A part the mass type does not have contributes nothing to S and nothing to p.

No element is excluded from any comparison: the draw decides nothing from its data except var > 0 and wM > 0, and those are
taken on exact inputs.

The constants are measured, not chosen.  tests/test_draw_bounds.py evaluates the float64 and the float32-storage
restatement of the kernels' operation order against the longdouble reference on the sets of tests/test_gpu_draw.py (SETS
below) and finds the worst fraction of (1), (2), (3) at C = 1: MEASURED.  Every C is its figure times 4, the margin of
tests/pm_bound.py and tests/fft_bound.py, for what the restatement does not do: the device's log / sincos / sqrt (a few ulp
where glibc's are correctly rounded or nearly so), fused multiply-adds, and rocFFT's operation order against pocketfft's.

As fractions of the bounds the tests apply (C = 4 x MEASURED), restatement / MI355X: (1) 0.436 / 0.436 in float64 and 0.9995 /
1.000 in float32, (2) 0.431 / 0.431 and 1.000 / 1.000, (3) 0.248 / 0.237 and 0.248 / 0.585 -- the kernels' double arithmetic has
its worst values where the restatement has them, and rocFFT's float32 transforms show 2.4 times pocketfft's error.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53

# worst fraction at C = 1 reached by the restatements over SETS (tests/test_draw_bounds.py asserts that none is exceeded)
# float64: white 1.815, colouring 1.576, the whole draw 0.584.  float32: (1) and (2) sit at 0.9995 and 1.0000 of the store's own half ulp, which C does not multiply -- the double
# arithmetic in front of it is nine digits below; the whole draw 0.129 (float32 transforms on float32 data).
MEASURED = {"white": {"float32": 1.0, "float64": 1.82}, "color": {"float32": 1.0, "float64": 1.58},
            "draw": {"float32": 0.13, "float64": 0.59}}
MARGIN = 4.0
C = {kind: {t: MARGIN * f for t, f in per_type.items()} for kind, per_type in MEASURED.items()}

UNIT_ROUNDOFF = {np.dtype(np.float32): LD(2.0) ** -24, np.dtype(np.float64): LD(2.0) ** -53}

# ---- the sets, shared by the CPU measurement and the GPU tests ----------------------------------------------------------
SEED = 0x9E3779B97F4A7C15                    # a non-zero high word
WHITE_N = (1, 2, 3, 729, 4096, 2 * 2048 * 256 + 3)   # the last: second stride iteration of a 2048 x 256 grid, odd tail
WHITE_ATTEMPTS = (0, 1, 2 ** 32 - 1)
WHITE_STREAMS = (0, 1)
COLOR_NH = (1, 257, 2048 * 256 + 5)
DRAW_N = (8, 9, 16)
DRAW_MASS_TYPES = (1, 0, 5)                  # Fourier only, real-space only, both
DRAW_SEED, DRAW_ATTEMPT = 0x1234567800000011, 7


def white_params(n):
    """(attempt, stream, with_var) of the runs at size n: the full product, thinned at the largest size to one run per
    attempt, the two streams and the two var variants each met (its reference alone takes a second to compute)."""
    if n < 100000:
        return [(a, s, v) for a in WHITE_ATTEMPTS for s in WHITE_STREAMS for v in (False, True)]
    return [(0, 0, False), (1, 1, True), (2 ** 32 - 1, 0, True)]


def white_var(n, dtype):
    """The var array of the sets: positive values over many decades with zeros, a negative, a denormal and 1e300 (in
    float32 that is +inf, so the largest finite float32 is there as well) at fixed places, whatever n allows."""
    dtype = np.dtype(dtype)
    rng = np.random.Generator(np.random.Philox(1000 + n))
    with np.errstate(over="ignore"):
        v = (10.0 ** rng.uniform(-6, 6, n)).astype(dtype)
        tiny = np.finfo(dtype).smallest_subnormal
        special = [0.0, -1.5, tiny, 1e300, -0.0, float(np.finfo(dtype).max), 0.0]
        for k, x in enumerate(special):
            # spread over the array: head, odd and even places, the tail
            for pos in (k, n - 1 - k, (n // 2 + 3 * k) | 1):
                if 0 <= pos < n:
                    v[pos] = dtype.type(x)
    return v


def color_inputs(nh, dtype):
    """wk, wM (zeros and negatives among positives over many decades), old: complex / float64 arrays of the set.  The
    float64 set also holds a denormal and 1e300; in float32 their quotients leave the type's range, where (2) says nothing."""
    ct = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    rng = np.random.Generator(np.random.Philox(2000 + nh))
    wk = (rng.standard_normal(nh) + 1j * rng.standard_normal(nh)).astype(ct) * ct(30.0)
    old = (rng.standard_normal(nh) + 1j * rng.standard_normal(nh)).astype(ct)
    wM = 10.0 ** rng.uniform(-8, 8, nh)
    wM[::5] = 0.0
    wM[3::7] = -wM[3::7]
    if nh > 16:
        wM[nh - 1] = -0.0
        if np.dtype(dtype) == np.float64:
            wM[1], wM[2] = 5e-324, 1e300
    return wk, wM, old


# ---- the checks ---------------------------------------------------------------------------------------------------------
def constant(kind, dtype):
    return C[kind][np.dtype(dtype).name]


def _fraction(err, bound):
    """max err / bound with 0 / 0 = 0 and anything / 0 = inf; returns (fraction, flat index)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    i = int(np.argmax(f))
    return float(f[i]), i


def white_fraction(got, ref, dtype, c=None):
    """Worst fraction of (1) over all values of `got` (storage type array of exactly the reference's length) and where.
    ref: tests.draw_restatement.white_ref's dict."""
    c = constant("white", dtype) if c is None else c
    got = np.asarray(got).ravel()
    g = ref["g"]
    if got.size != g.size:
        return np.inf, -1
    fin = np.isfinite(g)
    wrong_class = (~fin & (got.astype(LD) != g)) | (fin & ~np.isfinite(got))
    if wrong_class.any():
        return np.inf, int(np.flatnonzero(wrong_class)[0])
    gz = np.where(fin, g, 0)
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(np.where(fin, got.astype(LD), 0) - gz), 0)
        bound = np.where(fin, LD(c) * U * ref["rad"] * (1 + ref["theta"]) * np.where(fin, ref["s"], 0)
                         + UNIT_ROUNDOFF[np.dtype(dtype)] * np.abs(gz), 1)
    return _fraction(err, bound)


def color_fraction(got, ref, wk, a, old, dtype, c=None):
    """Worst fraction of (2) over the real and imaginary parts of every element.  old: None without accumulate."""
    c = constant("color", dtype) if c is None else c
    got = np.asarray(got).ravel()
    if got.size != ref.size or not np.all(np.isfinite(got.view(got.real.dtype))):
        return np.inf, -1
    worst = (0.0, 0)
    for part in ("real", "imag"):
        w = np.abs(getattr(np.asarray(wk), part).astype(LD).ravel())
        o = 0 if old is None else np.abs(getattr(np.asarray(old), part).astype(LD).ravel())
        r = getattr(ref, part).ravel()
        err = np.abs(getattr(got, part).astype(LD) - r)
        bound = LD(c) * U * (w * a.ravel() + o) + UNIT_ROUNDOFF[np.dtype(dtype)] * np.abs(r)
        f = _fraction(err, bound)
        worst = max(worst, f)
    return worst


def draw_fractions(got, ref, n, dtype, c=None, scale=1.0):
    """(max |p^ - p|, ||p^ - p||_2) as fractions of (3) (times `scale`).  ref: draw_ref's dict (p and S), or (p, S)."""
    c = constant("draw", dtype) if c is None else c
    p, S = (ref["p"], ref["S"]) if isinstance(ref, dict) else ref
    got = np.asarray(got).ravel()
    if got.size != p.size or not np.all(np.isfinite(got)):
        return np.inf, np.inf
    d = np.abs(got.astype(LD) - p)
    bound = LD(scale) * LD(c) * np.log2(LD(n) ** 3) * UNIT_ROUNDOFF[np.dtype(dtype)] * S
    if bound == 0:
        return (0.0, 0.0) if not d.any() else (np.inf, np.inf)
    return float(d.max() / bound), float(np.sqrt(np.sum(d * d)) / bound)
