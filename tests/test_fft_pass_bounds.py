"""The FFT-pass error bound of tests/fft_bound.py on the CPU: achievable, and able to fail.

xfft_inplace (barcode_amd/csrc/step_boundary_x.hpp) is restated here in numpy, operation by operation in the storage
type: bit-reversed fill, a radix-2 first stage when log2 n is odd, radix-4 passes with tw[r t1] and tw[r t2] and the
+-i rotation of the odd pair, the host twiddle table of fft_host.hpp (computed in double, rounded once).  The real
transforms of the z passes are restated around it: k_zbin_direct's C2R packing of two half-complex rows into one
complex column and k_zr2c's R2C unpacking.

(a) The restatement meets the bound against a longdouble np.fft for every n and direction, in float32 and float64:
    this is where C comes from.
(b) The same checker rejects each of four plausible kernel bugs: float64 twiddles rounded to float32, the second-stage
    twiddle conjugated in one direction, one twiddle index off by one, the n / 2 term of the C2R packing dropped.
    Without (b) nobody would know whether tests/test_gpu_fft_passes.py can fail.
(c) The z round trip of bchmc_probe_displacement_z (x / n through k_zr2c, back through k_zbin_direct's inverse) at
    n = 128, 256, 512: the constant of fft_bound's two-pass form is measured here, rows that are constant along z come
    back bit for bit, and the two-pass checker rejects a conjugate taken with the wrong sign in the R2C unpacking and
    the k = n / 2 element taken from the wrong row of the pair.
"""
import numpy as np
import pytest

from tests.fft_bound import MEASURED_ROUNDTRIP, MARGIN_ROUNDTRIP, C_ROUNDTRIP, worst_ratio, worst_ratio_roundtrip

NS = [32, 64, 128, 256, 512]
DTYPES = [np.float32, np.float64]


def twiddles(n, dtype):
    """fft_twiddles<T>(n): exp(-2 pi i r / n), r < n / 2, from double cos / sin rounded once to T."""
    ang = -2.0 * np.pi * np.arange(n // 2, dtype=np.float64) / n
    return np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)


def bitrev(n):
    l2 = n.bit_length() - 1
    return np.array([int(format(i, "0%db" % l2)[::-1], 2) for i in range(n)])


def xfft(re, im, inverse, dtype, mutation=None):
    """xfft_inplace on columns: re, im of shape (n, cols) in NATURAL order (the bit-reversed fill is done here).
    Returns (re, im) in natural order.  Every operation rounds to `dtype` as the kernel's does (no fused
    multiply-adds)."""
    n = re.shape[0]
    log2n = n.bit_length() - 1
    twr, twi = twiddles(n, dtype)
    if mutation == "twiddle_fp32":
        twr, twi = twr.astype(np.float32).astype(dtype), twi.astype(np.float32).astype(dtype)
    br = bitrev(n)
    s_re = np.empty_like(re, dtype=dtype)
    s_im = np.empty_like(im, dtype=dtype)
    s_re[br] = re.astype(dtype)
    s_im[br] = im.astype(dtype)
    st = 1
    if log2n & 1:  # stage 1: half = 1, twiddle 1
        ar, ai, xr, xi = s_re[0::2].copy(), s_im[0::2].copy(), s_re[1::2].copy(), s_im[1::2].copy()
        s_re[0::2], s_im[0::2] = ar + xr, ai + xi
        s_re[1::2], s_im[1::2] = ar - xr, ai - xi
        st = 2
    bf = np.arange(n // 4)
    while st < log2n:  # stages st and st + 1
        half = 1 << (st - 1)
        t1, t2 = n >> st, n >> (st + 1)
        r = bf & (half - 1)
        grp = bf >> (st - 1)
        j = (grp << (st + 1)) + r
        i1, i2 = r * t1, r * t2
        if mutation == "twiddle_index":
            i1 = np.where(r == 1, i1 + 1, i1)
        w1r, w1i = twr[i1][:, None], twi[i1][:, None]
        w2r, w2i = twr[i2][:, None], twi[i2][:, None]
        if inverse:
            w1i, w2i = -w1i, -w2i
        if mutation == "conj_w2" and not inverse:
            w2i = -w2i
        e0r, e0i = s_re[j], s_im[j]
        e1r, e1i = s_re[j + half], s_im[j + half]
        e2r, e2i = s_re[j + 2 * half], s_im[j + 2 * half]
        e3r, e3i = s_re[j + 3 * half], s_im[j + 3 * half]
        m1r, m1i = w1r * e1r - w1i * e1i, w1r * e1i + w1i * e1r
        m3r, m3i = w1r * e3r - w1i * e3i, w1r * e3i + w1i * e3r
        a0r, a0i = e0r + m1r, e0i + m1i
        a1r, a1i = e0r - m1r, e0i - m1i
        a2r, a2i = e2r + m3r, e2i + m3i
        a3r, a3i = e2r - m3r, e2i - m3i
        n2r, n2i = w2r * a2r - w2i * a2i, w2r * a2i + w2i * a2r
        n3r, n3i = w2r * a3r - w2i * a3i, w2r * a3i + w2i * a3r
        if inverse:
            r3r, r3i = -n3i, n3r
        else:
            r3r, r3i = n3i, -n3r
        s_re[j], s_im[j] = a0r + n2r, a0i + n2i
        s_re[j + 2 * half], s_im[j + 2 * half] = a0r - n2r, a0i - n2i
        s_re[j + half], s_im[j + half] = a1r + r3r, a1i + r3i
        s_re[j + 3 * half], s_im[j + 3 * half] = a1r - r3r, a1i - r3i
        st += 2
    return s_re, s_im


def zc2r(A, B, dtype, mutation=None):
    """k_zbin_direct's transform: half-complex rows A, B (shape (n/2 + 1, cols), complex) -> real rows a, b (n, cols)
    through one inverse complex transform of Z = A + i B (k <= n/2), Z[n - k] = conj(A[k]) + i conj(B[k]).  The
    imaginary parts of A, B at k = 0 and n / 2 do not enter."""
    n = 2 * (A.shape[0] - 1)
    ar, ai = A.real.astype(dtype), A.imag.astype(dtype)
    br_, bi = B.real.astype(dtype), B.imag.astype(dtype)
    zr = np.zeros((n,) + A.shape[1:], dtype)
    zi = np.zeros_like(zr)
    zr[0], zi[0] = ar[0], br_[0]
    if mutation != "drop_nyquist":
        zr[n // 2], zi[n // 2] = ar[n // 2], br_[n // 2]
    k = np.arange(1, n // 2)
    zr[k], zi[k] = ar[k] - bi[k], ai[k] + br_[k]
    zr[n - k], zi[n - k] = ar[k] + bi[k], br_[k] - ai[k]
    return xfft(zr, zi, True, dtype, mutation)


def zr2c(a, b, dtype, mutation=None):
    """k_zr2c's transform: real rows a, b (n, cols) -> half-complex A, B (n/2 + 1, cols) from one forward complex
    transform of a + i b: A[k] = (Z[k] + conj(Z[n - k])) / 2, B[k] = (Z[k] - conj(Z[n - k])) / (2 i)."""
    n = a.shape[0]
    zr, zi = xfft(a.astype(dtype), b.astype(dtype), False, dtype, mutation)
    k = np.arange(n // 2 + 1)
    km = (n - k) & (n - 1)
    h = dtype(0.5)
    Ar, Ai = h * (zr[k] + zr[km]), h * (zi[k] - zi[km])
    Br, Bi = h * (zi[k] + zi[km]), dtype(-0.5) * (zr[k] - zr[km])
    if mutation == "unpack_conj_sign":  # conj(Z[n - k]) taken as Z[n - k] in A's imaginary part
        Ai = h * (zi[k] + zi[km])
    Ar[n // 2], Ai[n // 2], Br[n // 2], Bi[n // 2] = zr[n // 2], 0, zi[n // 2], 0
    if mutation == "nyquist_wrong_row":  # the k = n / 2 terms of the two rows of the pair swapped
        Ar[n // 2], Br[n // 2] = zi[n // 2], zr[n // 2]
    return (Ar.astype(np.float64) + 1j * Ai.astype(np.float64), Br.astype(np.float64) + 1j * Bi.astype(np.float64))


def columns(n, cols, seed):
    """White complex Gaussian columns followed by unit impulses at 0, 1, n/2 - 1, n/2, n/2 + 1, n - 1."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, cols)) + 1j * rng.standard_normal((n, cols))
    imp = np.zeros((n, 6), complex)
    for c, i in enumerate([0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1]):
        imp[i, c] = 1.0
    return np.concatenate([x, imp], axis=1)


def ref_c2c(x, inverse):
    xl = x.astype(np.clongdouble)
    return np.fft.ifft(xl, axis=0, norm="forward") if inverse else np.fft.fft(xl, axis=0)


def rounded(x, dtype):
    """x as the kernel holds it: rounded to the storage type (the reference transforms the rounded values)."""
    if np.iscomplexobj(x):
        return x.real.astype(dtype).astype(np.float64) + 1j * x.imag.astype(dtype).astype(np.float64)
    return x.astype(dtype).astype(np.float64)


def c2c_ratio(n, dtype, inverse, mutation=None, seed=1):
    x = rounded(columns(n, 16, seed), dtype)
    yr, yi = xfft(x.real, x.imag, inverse, dtype, mutation)
    return worst_ratio(yr.astype(np.float64) + 1j * yi.astype(np.float64), ref_c2c(x, inverse), n, dtype, axis=0)


def c2r_ratio(n, dtype, mutation=None, seed=2):
    rng = np.random.default_rng(seed)
    nh = n // 2 + 1
    A = rng.standard_normal((nh, 8)) + 1j * rng.standard_normal((nh, 8))
    B = rng.standard_normal((nh, 8)) + 1j * rng.standard_normal((nh, 8))
    A[:, 7] = 0
    A[n // 2, 7] = 1.0 + 0.5j  # a lone Nyquist term (its imaginary part must not enter)
    A, B = rounded(A, dtype), rounded(B, dtype)
    a, b = zc2r(A, B, dtype, mutation)
    ra = np.fft.irfft(A.astype(np.clongdouble), n, axis=0, norm="forward")
    rb = np.fft.irfft(B.astype(np.clongdouble), n, axis=0, norm="forward")
    got = np.concatenate([a, b], axis=0).astype(np.float64)  # a column = the pair of rows of one complex transform
    return worst_ratio(got, np.concatenate([ra, rb], axis=0), n, dtype, axis=0)


def r2c_ratio(n, dtype, mutation=None, seed=3):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, 8))
    b = rng.standard_normal((n, 8))
    a[:, 7] = 0
    a[n // 2, 7] = 1.0
    a, b = rounded(a, dtype), rounded(b, dtype)
    A, B = zr2c(a, b, dtype, mutation)
    ra = np.fft.rfft(a.astype(np.longdouble), axis=0)
    rb = np.fft.rfft(b.astype(np.longdouble), axis=0)
    return worst_ratio(np.concatenate([A, B], axis=0), np.concatenate([ra, rb], axis=0), n, dtype, axis=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", NS)
def test_restatement_meets_the_bound(n, dtype):
    """(a) every n, both directions, the complex transform and both real-transform packings."""
    ratios = [c2c_ratio(n, dtype, False), c2c_ratio(n, dtype, True), c2r_ratio(n, dtype), r2c_ratio(n, dtype)]
    print("n %d %s: worst fraction of the bound %s" % (n, np.dtype(dtype).name, " ".join("%.3f" % r for r in ratios)))
    assert max(ratios) <= 1.0


def test_restatement_is_the_dft():
    """The restatement is a DFT at all (and not only within the bound): float64 against np.fft at round-off."""
    x = columns(64, 4, 9)
    yr, yi = xfft(x.real, x.imag, False, np.float64)
    assert np.allclose(yr + 1j * yi, np.fft.fft(x, axis=0), rtol=0, atol=1e-12)
    yr, yi = xfft(x.real, x.imag, True, np.float64)
    assert np.allclose(yr + 1j * yi, np.fft.ifft(x, axis=0, norm="forward"), rtol=0, atol=1e-12)


@pytest.mark.parametrize("n", NS)
def test_bound_rejects_fp32_twiddles_in_fp64(n):
    """(b) a float64 pass whose twiddle table was rounded to float32."""
    assert c2c_ratio(n, np.float64, False, "twiddle_fp32") > 1.0
    assert c2c_ratio(n, np.float64, True, "twiddle_fp32") > 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", NS)
def test_bound_rejects_conjugated_second_stage_twiddle(n, dtype):
    """(b) the second-stage twiddle conjugated in the forward direction only (the inverse stays right)."""
    assert c2c_ratio(n, dtype, False, "conj_w2") > 1.0
    assert c2c_ratio(n, dtype, True, "conj_w2") <= 1.0
    assert r2c_ratio(n, dtype, "conj_w2") > 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", NS)
def test_bound_rejects_twiddle_index_off_by_one(n, dtype):
    """(b) first-stage twiddle index r t1 + 1 instead of r t1 for r = 1 (one table entry per radix-4 pass)."""
    assert c2c_ratio(n, dtype, False, "twiddle_index") > 1.0
    assert c2c_ratio(n, dtype, True, "twiddle_index") > 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", NS)
def test_bound_rejects_dropped_nyquist_term_of_the_c2r(n, dtype):
    """(b) k_zbin_direct's packing without Z[n/2] = A[n/2] + i B[n/2]."""
    assert c2r_ratio(n, dtype, "drop_nyquist") > 1.0


# ---- (c) the z round trip ----------------------------------------------------------------------------------------------

RT_NS = [128, 256, 512]


def roundtrip(a, b, dtype, mutation=None):
    """Rows a, b (n, cols): scaled by 1 / n (exact), k_zr2c, then k_zbin_direct's inverse.  Returns (a', b')."""
    n = a.shape[0]
    s = dtype(1) / dtype(n)
    A, B = zr2c(a.astype(dtype) * s, b.astype(dtype) * s, dtype, mutation)
    return zc2r(A, B, dtype)


def roundtrip_rows(n, seed=4):
    """White rows, rows many box lengths out mixed with small ones, an impulse against a zero partner, a constant pair."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, 12))
    b = rng.standard_normal((n, 12))
    a[:, 8] += 1e3 * rng.integers(-7, 8, n)
    b[:, 9] *= 1e-3
    a[:, 10], b[:, 10] = 0, 0
    a[n // 2 + 1, 10] = 1.0
    a[:, 11], b[:, 11] = -1.5625, 0.3
    return a, b


def roundtrip_ratio(n, dtype, mutation=None):
    a, b = roundtrip_rows(n)
    a, b = rounded(a, dtype), rounded(b, dtype)
    ga, gb = roundtrip(a, b, dtype, mutation)
    got = np.concatenate([ga, gb], axis=0).astype(np.float64)
    return worst_ratio_roundtrip(got, np.concatenate([a, b], axis=0), n, dtype, axis=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_roundtrip_constant_is_the_measured_one(dtype):
    """The worst fraction of log2(n) u ||x|| the restated round trip reaches is the figure fft_bound records (rounded
    up to two digits), and the constant in use is four times it."""
    name = np.dtype(dtype).name
    worst = max(roundtrip_ratio(n, dtype) for n in RT_NS) * C_ROUNDTRIP[name]
    print("z round trip %s: worst fraction of log2(n) u ||x|| %.3f" % (name, worst))
    assert 0.8 * MEASURED_ROUNDTRIP[name] <= worst <= MEASURED_ROUNDTRIP[name]
    assert C_ROUNDTRIP[name] == MARGIN_ROUNDTRIP * MEASURED_ROUNDTRIP[name] and MARGIN_ROUNDTRIP == 4.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", RT_NS)
def test_rows_constant_along_z_survive_the_roundtrip_bitwise(n, dtype):
    """Every non-trivial twiddle meets an exact zero and the remaining butterflies are doublings: cell fractions,
    nextafter(L, 0) - d / 2, -ulp, many box lengths, a pair of very different sizes."""
    T = np.dtype(dtype).type
    L = 200.0 * n / 64.0
    vals = np.array([0.0, -0.5 * L / n, float(np.nextafter(T(L), T(0))) - 0.5 * L / n,
                     -float(np.nextafter(T(0.5 * L / n), T(L))), 17 * L + 0.3, -21 * L - 1e-3, 1e-30, 3.0])
    a = np.broadcast_to(vals.astype(dtype)[None, :], (n, len(vals))).copy()
    b = np.broadcast_to(vals.astype(dtype)[None, ::-1], (n, len(vals))).copy()
    ga, gb = roundtrip(a, b, dtype)
    assert np.array_equal(ga, a) and np.array_equal(gb, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", RT_NS)
@pytest.mark.parametrize("mutation", ["unpack_conj_sign", "nyquist_wrong_row"])
def test_roundtrip_bound_rejects_wrong_unpacking(mutation, n, dtype):
    assert roundtrip_ratio(n, dtype) <= 1.0
    assert roundtrip_ratio(n, dtype, mutation) > 1.0
