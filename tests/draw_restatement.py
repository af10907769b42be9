"""The Philox momentum draw of include/bchmc.h (the comment above bchmc_chain_draw_momenta) restated from its definitions:
the counter map, the two 53-bit uniforms, Box-Muller, the scaling by sqrt(var), the colouring by 1 / sqrt(wM) and the whole
draw p = irfftn(rfftn(w0) sqrt(mass_f N / L^3)) + sqrt(mass_r) w1 -- in numpy.longdouble (2 pi, log, sqrt, cos, sin and
the transforms), which is what tests/test_gpu_draw.py compares the device with.  Only philox4x32_10 and u53 are shared
(tests/poisson_restatement.py; they reproduce the Random123 known answers on the CPU, tests/test_poisson_cpu.py).

The *_storage functions are another thing: float64 arithmetic in the kernels' own operation order (rng.hpp, chain_draw in
bchmc.hip), rounded to the storage type where the kernels round.  Their only purpose is to measure the constants of
tests/draw_bound.py, and -- through `mut`, one named deviation at a time -- to show that the checker rejects a wrong draw
(tests/test_draw_bounds.py).
"""
import numpy as np

from tests.poisson_restatement import M32, philox4x32_10, u53

LD = np.longdouble
TWO_PI = LD(8) * np.arctan(LD(1))
DOMAIN = np.uint64(0x80000000)  # bit 31 of the second counter word: the momentum draw's domain
FOURIER, REAL = 0, 1            # the white-noise arrays (counter word 3)

MUTANTS = ("swap_attempt_stream", "no_domain", "pair_plus_one", "swap_u", "swap_sincos", "shift12", "no_half", "var_not_sqrt",
           "inv_wM_not_sqrt", "no_accumulate", "one_stream", "odd_tail")


def counters(pair, attempt, stream, mut=None):
    """The four counter words of pair index `pair` (any uint64 array) of white-noise array `stream` of `attempt`."""
    i = np.asarray(pair, dtype=np.uint64)
    if mut == "pair_plus_one":
        i = i + np.uint64(1)
    hi = i >> np.uint64(32)
    assert not np.any(hi & DOMAIN), "a pair index stays below 2^63"
    c1 = hi if mut == "no_domain" else hi | DOMAIN
    c2 = np.full(i.shape, int(attempt), dtype=np.uint64)
    c3 = np.full(i.shape, int(stream), dtype=np.uint64)
    assert int(attempt) < 2 ** 32 and int(stream) < 2 ** 32
    if mut == "swap_attempt_stream":
        c2, c3 = c3, c2
    return i & M32, c1, c2, c3


def poisson_counters(cell, j_or_kk, stream, positions):
    """The Poisson sampler's counter words (P1: counts, iteration j; P5: positions, index kk within the cell)."""
    c = np.asarray(cell, dtype=np.uint64)
    assert int(stream) < 2 ** 31
    return (c & M32, c >> np.uint64(32), np.full(c.shape, int(j_or_kk), dtype=np.uint64),
            np.full(c.shape, 2 * int(stream) + (1 if positions else 0), dtype=np.uint64))


def uniforms(pair, seed, attempt, stream, mut=None):
    """u1, u2 (float64, exact values of the definition) of the given pair indices."""
    seed = int(seed)
    r = philox4x32_10(*counters(pair, attempt, stream, mut), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    if mut in ("shift12", "no_half"):
        sh, half = (12, 0.5) if mut == "shift12" else (11, 0.0)

        def u(hi, lo):
            return ((((hi << np.uint64(32)) | lo) >> np.uint64(sh)).astype(np.float64) + half) * 2.0 ** -53
    else:
        u = u53
    u1, u2 = u(r[0], r[1]), u(r[2], r[3])
    return (u2, u1) if mut == "swap_u" else (u1, u2)


def _interleave(a, b, n):
    out = np.empty(2 * a.size, dtype=a.dtype)
    out[0::2], out[1::2] = a, b
    return out[:n]


def _root_where_positive(v):
    """sqrt(v) where v > 0, else 0, in v's precision."""
    v = np.asarray(v)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.sqrt(np.where(v > 0, v, 1)), 0).astype(v.dtype)


# ---- the longdouble reference -------------------------------------------------------------------------------------------
def white_ref(n, seed, attempt, stream, var=None):
    """The n values of one white-noise array: dict g (longdouble; +-inf where var is +inf), rad, theta, s (per value)."""
    n = int(n)
    u1, u2 = uniforms(np.arange((n + 1) // 2, dtype=np.uint64), seed, attempt, stream)
    rad = np.sqrt(LD(-2) * np.log(u1.astype(LD)))
    theta = TWO_PI * u2.astype(LD)
    g = _interleave(rad * np.cos(theta), rad * np.sin(theta), n)
    s = np.ones(n, dtype=LD) if var is None else _root_where_positive(np.asarray(var).astype(LD).ravel())
    assert s.size == n
    with np.errstate(invalid="ignore"):
        gs = np.where(s == 0, LD(0), g * s)  # 0 times anything is the kernel's 0, too: its g is finite
    return dict(g=gs, rad=_interleave(rad, rad, n), theta=_interleave(theta, theta, n), s=s)


def color_ref(wk, wM=None, old=None, accumulate=0):
    """[old +] wk / sqrt(wM) per element (complex longdouble), 0 in place of the quotient where wM <= 0.  Returns
    (ref, a) with a = 1 / sqrt(wM) (1 without wM)."""
    w = np.asarray(wk).astype(np.clongdouble)
    if wM is None:
        a = np.ones(w.shape, dtype=LD)
    else:
        m = np.asarray(wM).astype(LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(m > 0, LD(1) / np.sqrt(np.where(m > 0, m, 1)), LD(0))
    ref = w * a
    if accumulate:
        ref = ref + np.asarray(old).astype(np.clongdouble)
    return ref, a


def draw_ref(n, L, seed, attempt, mass_f=None, mass_r=None):
    """The whole draw on an n^3 grid of box side L.  mass_f: the full n^3 grid of the Fourier-space mass or None;
    mass_r: the real-space mass or None.  Returns dict p (longdouble, n^3 flat), S (the scale of the whole-draw bound:
    max_k a_k ||w0||_2 + ||sqrt(mass_r) w1||_2), pf and pr (the two parts)."""
    n, N = int(n), int(n) ** 3
    pf = pr = np.zeros(N, dtype=LD)
    S = LD(0)
    if mass_f is not None:
        w0 = white_ref(N, seed, attempt, FOURIER)["g"]
        mf = np.asarray(mass_f, dtype=np.float64).reshape(n, n, n)[:, :, : n // 2 + 1].astype(LD)
        a = _root_where_positive(mf * LD(N) / LD(L) ** 3)
        wk = np.fft.rfftn(w0.reshape(n, n, n))
        assert wk.dtype == np.clongdouble
        pf = np.fft.irfftn(wk * a, s=(n, n, n), axes=(0, 1, 2)).ravel()
        S = S + a.max() * np.sqrt(np.sum(w0 * w0))
    if mass_r is not None:
        pr = white_ref(N, seed, attempt, REAL, var=np.asarray(mass_r, dtype=np.float64).ravel())["g"]
        S = S + np.sqrt(np.sum(pr * pr))
    return dict(p=pf + pr, S=S, pf=pf, pr=pr)


# ---- the kernels' operation order in float64, stored as `dtype` (constants and mutants only) ------------------------------
def white_storage(out, n, seed, attempt, stream, var, dtype, mut=None):
    """k_white_noise: writes into out[0 .. n) (an array of `dtype` with at least n + 1 elements, so that a write past the
    end is seen).  var: array of `dtype` or None."""
    n = int(n)
    assert out.dtype == np.dtype(dtype) and out.size >= n + 1
    pairs = (n + 1) // 2
    u1, u2 = uniforms(np.arange(pairs, dtype=np.uint64), seed, attempt, stream, mut)
    with np.errstate(divide="ignore"):
        rad = np.sqrt(-2.0 * np.log(u1))
    ang = 6.283185307179586476925 * u2
    cs, sn = np.cos(ang), np.sin(ang)
    if mut == "swap_sincos":
        cs, sn = sn, cs
    g = np.empty(2 * pairs, dtype=np.float64)
    g[0::2], g[1::2] = rad * cs, rad * sn
    m = n + 1 if (mut == "odd_tail" and n & 1) else n
    if var is not None:
        assert var.dtype == np.dtype(dtype)
        v = var.astype(np.float64).ravel()
        s = np.where(v > 0, v, 0) if mut == "var_not_sqrt" else _root_where_positive(v)
        with np.errstate(over="ignore", invalid="ignore"):
            g[:n] = g[:n] * s
    with np.errstate(over="ignore"):
        out[:m] = g[:m].astype(dtype)


def _prepare_mult(mass_f, n, L):
    """k_prepare_mult on the half-complex layout: normFS / mass_f, 0 where mass_f <= 0 (float64)."""
    c = np.asarray(mass_f, dtype=np.float64).reshape(n, n, n)[:, :, : n // 2 + 1]
    norm_fs = L * L * L / float(n ** 3)
    with np.errstate(divide="ignore"):
        return np.where(c > 0, norm_fs / np.where(c > 0, c, 1), 0.0)


def color_storage(wk, wM, old, accumulate, dtype, mut=None):
    """k_color_momenta: wk, old complex arrays of the storage type's complex twin; returns the new pk in that type."""
    ct = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    assert np.asarray(wk).dtype == ct
    vx, vy = wk.real.astype(np.float64), wk.imag.astype(np.float64)
    if wM is not None:
        m = np.asarray(wM, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if mut == "inv_wM_not_sqrt":
                a = np.where(m > 0, 1.0 / np.where(m > 0, m, 1), 0.0)
            else:
                a = np.where(m > 0, 1.0 / np.sqrt(np.where(m > 0, m, 1)), 0.0)
        vx, vy = vx * a, vy * a
    if accumulate and mut != "no_accumulate":
        assert old.dtype == ct
        vx, vy = vx + old.real.astype(np.float64), vy + old.imag.astype(np.float64)
    out = np.empty(vx.shape, dtype=ct)
    out.real, out.imag = vx.astype(dtype), vy.astype(dtype)
    return out


def draw_storage(n, L, seed, attempt, mass_f, mass_r, dtype, mut=None):
    """chain_draw followed by bchmc_chain_get_momenta on a handle of storage type `dtype`: white noise, R2C, colouring,
    [white noise times sqrt(mass_r), R2C, accumulate], scaling by 1 / N, C2R, widening.  numpy's transforms keep the type."""
    n, N = int(n), int(n) ** 3
    dtype = np.dtype(dtype)
    ct = np.complex64 if dtype == np.float32 else np.complex128
    cp = np.zeros((n, n, n // 2 + 1), dtype=ct)
    if mass_f is not None:
        w = np.empty(N + 1, dtype=dtype)
        white_storage(w, N, seed, attempt, FOURIER, None, dtype, mut)
        wk = np.fft.rfftn(w[:N].reshape(n, n, n))
        assert wk.dtype == ct
        cp = color_storage(wk, _prepare_mult(mass_f, n, L), None, 0, dtype, mut)
    if mass_r is not None:
        w = np.empty(N + 1, dtype=dtype)
        var = np.asarray(mass_r, dtype=np.float64).ravel().astype(dtype)  # an upload rounds mass_r to the storage type
        white_storage(w, N, seed, attempt, FOURIER if mut == "one_stream" else REAL, var, dtype, mut)
        wk = np.fft.rfftn(w[:N].reshape(n, n, n))
        cp = color_storage(wk, None, cp, 1, dtype, mut)
    scaled = np.empty_like(cp)
    scaled.real = (cp.real.astype(np.float64) * (1.0 / float(N))).astype(dtype)
    scaled.imag = (cp.imag.astype(np.float64) * (1.0 / float(N))).astype(dtype)
    p = np.fft.irfftn(scaled, s=(n, n, n), axes=(0, 1, 2), norm="forward")
    assert p.dtype == dtype
    return p.ravel().astype(np.float64)
