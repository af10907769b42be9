"""The error bound the engine's own FFT passes are held to (tests/test_fft_pass_bounds.py derives it and shows that it
can fail, tests/test_gpu_fft_passes.py applies it to the kernels).

Per transformed column y (length n, computed ŷ):

    ||ŷ - y||_2  <=  C log2(n) u_T ||y||_2     and     max |ŷ - y|  <=  C log2(n) u_T ||y||_2

u_T is the unit round-off of the storage type T.  The second inequality follows from the first; it is checked on its
own so that a failure names the worst single element.  A column is what one complex transform of the pass sees: a y
column of k_ypass, an interleaved column of xfft_inplace, and for the z passes the PAIR of real rows that
k_zr2c / k_zbin_direct pack into one complex transform (the round-off of one row leaks into the other, so the pair's
norm is the scale).

C: the numpy restatement of xfft_inplace (test_fft_pass_bounds.py) reaches at most 0.32 (float32) / 0.49 (float64)
of log2(n) u_T ||y|| over n = 32 .. 512, both directions, white and impulse data, with and without the real-transform
packing (float64 sits higher: the angle -2 pi r / n of the double twiddle table is itself rounded, which costs a few
u in cos / sin).  C = 2 leaves a factor of 4 for the GPU's fused multiply-adds; a float64 pass with a twiddle table
rounded to float32 misses it by seven orders of magnitude, a conjugated twiddle by six, one twiddle index off by one
by four.

Two passes (the z round trip of bchmc_probe_displacement_z: x / n through k_zr2c, back through the inverse inside
k_zbin_direct, both unnormalised).  With F the DFT matrix, ||F v|| = sqrt(n) ||v||.  The forward pass returns
X^ = F (x / n) + e1 with ||e1|| <= C1 log2(n) u ||F x / n|| = C1 log2(n) u ||x|| / sqrt(n) (the single-pass form above; the
scaling by 1 / n, a power of two, is exact).  The inverse pass returns conj(F) X^ + e2 = x + conj(F) e1 + e2 with
||conj(F) e1|| = sqrt(n) ||e1|| <= C1 log2(n) u ||x|| and ||e2|| <= C1 log2(n) u ||x|| (1 + O(u log n)).  So, per pair of rows,

    ||x^ - x||_2  <=  C_rt log2(n) u_T ||x||_2     and     max |x^ - x|  <=  C_rt log2(n) u_T ||x||_2,      C_rt <= 2 C1,

and a pair that is zero comes back exactly zero.  The two errors are not aligned, so the restated round trip
(test_fft_pass_bounds.py, float32 and float64, n = 128 .. 512, white rows, rows many box lengths out, an impulse against
a zero partner) reaches less than twice the single-pass figure: MEASURED_ROUNDTRIP below; C_rt is 4 times it, the
margin every constant here has.  The same checker rejects a conjugate with the wrong sign in the R2C unpacking and
the k = n / 2 element taken from the other row of the pair.
"""
import numpy as np

C = 2.0

# worst fraction of log2(n) u_T ||x|| the restated z round trip reaches (tests/test_fft_pass_bounds.py asserts it)
MEASURED_ROUNDTRIP = {"float32": 0.40, "float64": 0.40}
MARGIN_ROUNDTRIP = 4.0
C_ROUNDTRIP = {t: MARGIN_ROUNDTRIP * f for t, f in MEASURED_ROUNDTRIP.items()}

UNIT_ROUNDOFF = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def unit_roundoff(dtype):
    """u_T of a real or complex storage type."""
    return UNIT_ROUNDOFF[np.dtype(np.empty(0, dtype).real.dtype)]


def worst_ratio_roundtrip(xhat, x, n, dtype, axis=-1):
    """worst_ratio for the two-pass form: x^ the pair of rows after the z round trip, x the pair that went in."""
    return worst_ratio(xhat, x, n, dtype, axis, c=C_ROUNDTRIP[np.dtype(dtype).name])


def worst_ratio(yhat, y, n, dtype, axis=-1, c=C):
    """Largest of ||ŷ - y||_2 / bound and max|ŷ - y| / bound over the columns along `axis` (the check passes when it is
    <= 1).  NaN anywhere in ŷ gives inf.  `y` may be longdouble; the difference is taken in its precision."""
    yhat = np.asarray(yhat)
    y = np.asarray(y)
    if np.isnan(yhat).any():
        return np.inf
    d = np.abs(yhat.astype(y.dtype) - y)
    scale = c * np.log2(n) * unit_roundoff(dtype) * np.sqrt(np.sum(np.abs(y) ** 2, axis=axis))
    e2 = np.sqrt(np.sum(d ** 2, axis=axis))
    emax = np.max(d, axis=axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        # a zero column must come out exactly zero
        r2 = np.where(scale > 0, e2 / np.where(scale > 0, scale, 1), np.where(e2 > 0, np.inf, 0))
        rmax = np.where(scale > 0, emax / np.where(scale > 0, scale, 1), np.where(emax > 0, np.inf, 0))
    return float(max(np.max(r2), np.max(rmax)))
