"""The engine's own FFT passes, each run alone on the GPU through libbchmc_fft_probe.so (barcode_amd/csrc/fft_probe.hip:
the kernels of kernels.hpp with the engine's launches) and compared with numpy's DFT per transformed column, at the
bound of tests/fft_bound.py.

- xfft_inplace (the radix-4 core of k_step_boundary_x, k_ypass, k_zbin_direct, k_zr2c) at n = 32 .. 512, with the
  interleave KB of the x / y passes (8 fp64, 16 fp32) and of the z passes (6), both directions;
- k_ypass inverse at 128 / 256 / 512 and forward at 512 over three whole n^2 nhp components;
- k_zr2c<T, 512>, the z R2C of the planes-mode forward transform at 512^3, and <T, 128> / <T, 256>, which only
  bchmc_probe_displacement_z launches (tests/test_gpu_zbin_positions.py stands on them);
- k_zbin_direct<T, NZ, true> (the overflow fallback, *ovf set), the z C2R of three components at 128 / 256 / 512.

Inputs: white complex Gaussian data in every column, unit impulses at 0, 1, n/2 - 1, n/2, n/2 + 1, n - 1 in the first
and the last lane of a k-group and in the last k-group (the one holding the row padding), non-zero imaginary parts at
kz = 0 and kz = n/2 of the C2R input (they must not enter, as in numpy's irfft and rocFFT's C2R), NaN in the row
padding k in [n/2 + 1, nhp) (no output outside it may be NaN; k_zr2c must leave it as it was).  The probe checks a
canary after every device array.  Reference: longdouble np.fft up to n = 256; at 512, float64 over the whole array
plus longdouble on a sample of columns that includes the edge columns.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests.fft_bound import worst_ratio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "barcode_amd", "libbchmc_fft_probe.so")
PREC = {"fp64": (0, np.float64, np.complex128), "fp32": (1, np.float32, np.complex64)}


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the process-wide HIP runtime first, as barcode_amd.engine does)
    assert os.path.exists(PROBE), "%s not built (make -C barcode_amd/csrc)" % PROBE
    L = C.CDLL(PROBE)
    vp, i = C.c_void_p, C.c_int
    L.fftp_row_stride.argtypes = [i, i]
    L.fftp_xfft.argtypes = [i, i, i, i, i, vp]
    L.fftp_ypass.argtypes = [i, i, i, vp]
    L.fftp_zr2c.argtypes = [i, i, vp, vp]
    L.fftp_zc2r.argtypes = [i, i, vp, vp]
    return L


def ptr(a):
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


def check_status(st):
    assert st == 0, {-1: "arguments outside the engine's instantiations", -2: "HIP error"}.get(
        st, "canary after device array %d overwritten" % st)


def impulses(n):
    return [0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1]


def report(name, ratio):
    print("\nFFTPASS %s worst fraction of the bound %.3f" % (name, ratio))
    assert ratio <= 1.0


def white(rng, shape, cdtype):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdtype)


# ---- xfft_inplace --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", ["fwd", "inv"])
@pytest.mark.parametrize("kb", ["kb6", "kbx"])
@pytest.mark.parametrize("n", [32, 64, 128, 256, 512])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_xfft_inplace(lib, prec, n, kb, direction):
    """Workgroups of n x KB interleaved columns: two of white data, then one per impulse position with the impulse
    in the first and the last lane (white data in between)."""
    p, rdt, cdt = PREC[prec]
    kbv = 6 if kb == "kb6" else 128 // (2 * np.dtype(rdt).itemsize)
    inverse = direction == "inv"
    rng = np.random.default_rng(100 + n + kbv)
    idx = impulses(n)
    x = white(rng, (2 + len(idx), n, kbv), cdt)
    for g, i in enumerate(idx):
        for lane in (0, kbv - 1):
            x[2 + g, :, lane] = 0
            x[2 + g, i, lane] = 1
    y = x.copy()
    check_status(lib.fftp_xfft(p, n, kbv, int(inverse), x.shape[0], ptr(y)))
    xl = x.astype(np.clongdouble)
    ref = np.fft.ifft(xl, axis=1, norm="forward") if inverse else np.fft.fft(xl, axis=1)
    report("xfft_inplace<%s> n=%d KB=%d %s" % (prec, n, kbv, direction), worst_ratio(y, ref, n, rdt, axis=1))


# ---- k_ypass -------------------------------------------------------------------------------------------------------

def planes_input(lib, p, rdt, cdt, n, seed):
    """Three components (3, n, n, nhp): white data for k <= n/2, NaN in the row padding."""
    nhp = lib.fftp_row_stride(n, p)
    nh = n // 2 + 1
    assert nhp > nh  # padded rows at n >= 128: the last k-group holds padding
    rng = np.random.default_rng(seed)
    x = np.empty((3, n, n, nhp), cdt)
    for c in range(3):
        x[c, :, :, :nh] = white(rng, (n, n, nh), cdt)
    x[..., nh:] = np.nan + 1j * np.nan
    return x, nh, nhp


def sample_rows(rng, n, m=16):
    """(component, plane) pairs for the longdouble check at 512: the edges and m random ones."""
    rows = [(0, 0), (0, n - 1), (2, 0), (2, n - 1), (1, n // 2)]
    rows += [(int(c), int(i)) for c, i in zip(rng.integers(0, 3, m), rng.integers(0, n, m))]
    return rows


@pytest.mark.parametrize("case", ["inv128", "inv256", "inv512", "fwd512"])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_k_ypass(lib, prec, case):
    """k_ypass<T, NT, PER> in place over the y columns (c, i, :, k) of three components."""
    p, rdt, cdt = PREC[prec]
    n, inverse = int(case[3:]), case.startswith("inv")
    x, nh, nhp = planes_input(lib, p, rdt, cdt, n, 200 + n)
    kbv = 128 // (2 * np.dtype(rdt).itemsize)
    lanes = [0, kbv - 1, n // 2 - 1, n // 2]  # first / last lane of a k-group; the last k-group (padding) and its neighbour
    for m, j in enumerate(impulses(n)):
        for c, i in ((0, m), (2, n - 1 - m)):
            x[c, i, :, lanes] = 0
            x[c, i, j, lanes] = 1
    y = x.copy()
    check_status(lib.fftp_ypass(p, n, int(inverse), ptr(y)))
    assert not np.isnan(y[..., :nh]).any()
    assert np.isnan(y[..., nh:]).all()  # padding columns are transformed like data: NaN stays in them

    def ref(a):
        return np.fft.ifft(a, axis=-2, norm="forward") if inverse else np.fft.fft(a, axis=-2)

    worst = 0.0
    for c in range(3):
        if n <= 256:
            worst = max(worst, worst_ratio(y[c, :, :, :nh], ref(x[c, :, :, :nh].astype(np.clongdouble)), n, rdt, axis=1))
        else:
            worst = max(worst, worst_ratio(y[c, :, :, :nh], ref(x[c, :, :, :nh].astype(np.complex128)), n, rdt, axis=1))
    if n > 256:
        for c, i in sample_rows(np.random.default_rng(7), n):
            worst = max(worst, worst_ratio(y[c, i, :, :nh], ref(x[c, i, :, :nh].astype(np.clongdouble)), n, rdt, axis=0))
    report("k_ypass<%s> n=%d %s" % (prec, n, "inverse" if inverse else "forward"), worst)


# ---- z passes ------------------------------------------------------------------------------------------------------
# A column of a z pass is the pair of rows (c, i, 2 p) and (c, i, 2 p + 1) that goes through one complex transform
# (as real and imaginary part): the k_zr2c workgroup (i0, j0) packs lane 2 c + f = rows (i0 + f, j0) + i (i0 + f, j0 + 1).

def pairs(a):
    """(3, n, n, L) -> (3, n, n/2, 2 L): the two rows of each complex column side by side."""
    s = a.shape
    return a.reshape(s[0], s[1], s[2] // 2, 2 * s[3])


def z_impulse_rows(n):
    """Per impulse position m: (first lane: component 0, even i, pair j = 0, 1, impulse in the real row) and (last
    lane: component 2, odd i, pair j = n - 2, n - 1, impulse in the imaginary row)."""
    for m, k in enumerate(impulses(n)):
        yield k, (0, 2 * m, 0), (0, 2 * m, 1)          # impulse row, zero partner row
        yield k, (2, n - 1 - 2 * m, n - 1), (2, n - 1 - 2 * m, n - 2)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_k_zr2c_512(lib, prec):
    """k_zr2c<T, 512>: V (3, n, n, n) real -> half-complex (3, n, n, nhp); every k <= n/2 written (the output array
    goes in as NaN), the row padding returned bit for bit."""
    check_k_zr2c(lib, prec, 512)


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_k_zr2c(lib, prec, n):
    """k_zr2c<T, 128> and <T, 256>, the instantiations bchmc_probe_displacement_z feeds k_zbin_direct through: the same
    inputs and the same bound as at 512."""
    check_k_zr2c(lib, prec, n)


def check_k_zr2c(lib, prec, n):
    p, rdt, cdt = PREC[prec]
    rng = np.random.default_rng(300)
    V = rng.standard_normal((3, n, n, n)).astype(rdt)
    for k, row, partner in z_impulse_rows(n):
        V[row] = 0
        V[partner] = 0
        V[row][k] = 1
    nhp = lib.fftp_row_stride(n, p)
    nh = n // 2 + 1
    ck = np.full((3, n, n, nhp), np.nan + 1j * np.nan, cdt)
    pad_bits = ck[..., nh:].copy().view(np.uint8)
    check_status(lib.fftp_zr2c(p, n, ptr(V), ptr(ck)))
    assert not np.isnan(ck[..., :nh]).any()
    assert np.array_equal(ck[..., nh:].copy().view(np.uint8), pad_bits)
    worst = 0.0
    for c in range(3):
        ref = np.fft.rfft(V[c].astype(np.float64), axis=-1)
        worst = max(worst, worst_ratio(pairs(ck[c:c + 1, :, :, :nh]), pairs(ref[None]), n, rdt, axis=-1))
        del ref
    for c, i in sample_rows(np.random.default_rng(8), n):
        ref = np.fft.rfft(V[c, i].astype(np.longdouble), axis=-1)
        worst = max(worst, worst_ratio(pairs(ck[None, c, i:i + 1, :, :nh]), pairs(ref[None, None]), n, rdt, axis=-1))
    report("k_zr2c<%s,%d>" % (prec, n), worst)


@pytest.mark.parametrize("n", [128, 256, 512])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_k_zbin_direct_psi_only(lib, prec, n):
    """k_zbin_direct<T, n, true> with *ovf set: half-complex (3, n, n, nhp) -> Psi (3, n, n, n) real.  The input has
    non-zero imaginary parts at kz = 0 and n/2 everywhere (white data), and impulse rows whose kz = 0 / n/2 terms
    carry one too; NaN in the row padding must not reach Psi."""
    p, rdt, cdt = PREC[prec]
    x, nh, nhp = planes_input(lib, p, rdt, cdt, n, 400 + n)
    for k, row, partner in z_impulse_rows(n):
        if k > n // 2:
            continue  # beyond the half-complex row
        x[row][:nh] = 0
        x[partner][:nh] = 0
        x[row][k] = 1 + 0.75j
    assert (x[..., 0].imag != 0).mean() > 0.99 and (x[..., n // 2].imag != 0).mean() > 0.99
    psi = np.empty((3, n, n, n), rdt)
    check_status(lib.fftp_zc2r(p, n, ptr(x), ptr(psi)))
    assert not np.isnan(psi).any()
    worst = 0.0
    for c in range(3):
        ck = x[c, :, :, :nh].astype(np.clongdouble if n <= 256 else np.complex128)
        ref = np.fft.irfft(ck, n, axis=-1, norm="forward")
        worst = max(worst, worst_ratio(pairs(psi[c:c + 1]), pairs(ref[None]), n, rdt, axis=-1))
        del ck, ref
    if n > 256:
        for c, i in sample_rows(np.random.default_rng(9), n):
            ref = np.fft.irfft(x[c, i, :, :nh].astype(np.clongdouble), n, axis=-1, norm="forward")
            worst = max(worst, worst_ratio(pairs(psi[None, c, i:i + 1]), pairs(ref[None, None]), n, rdt, axis=-1))
    report("k_zbin_direct<%s,%d,true>" % (prec, n), worst)
