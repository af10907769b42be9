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
"""
import numpy as np

C = 2.0

UNIT_ROUNDOFF = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def unit_roundoff(dtype):
    """u_T of a real or complex storage type."""
    return UNIT_ROUNDOFF[np.dtype(np.empty(0, dtype).real.dtype)]


def worst_ratio(yhat, y, n, dtype, axis=-1):
    """Largest of ||ŷ - y||_2 / bound and max|ŷ - y| / bound over the columns along `axis` (the check passes when it is
    <= 1).  NaN anywhere in ŷ gives inf.  `y` may be longdouble; the difference is taken in its precision."""
    yhat = np.asarray(yhat)
    y = np.asarray(y)
    if np.isnan(yhat).any():
        return np.inf
    d = np.abs(yhat.astype(y.dtype) - y)
    scale = C * np.log2(n) * unit_roundoff(dtype) * np.sqrt(np.sum(np.abs(y) ** 2, axis=axis))
    e2 = np.sqrt(np.sum(d ** 2, axis=axis))
    emax = np.max(d, axis=axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        # a zero column must come out exactly zero
        r2 = np.where(scale > 0, e2 / np.where(scale > 0, scale, 1), np.where(e2 > 0, np.inf, 0))
        rmax = np.where(scale > 0, emax / np.where(scale > 0, scale, 1), np.where(emax > 0, np.inf, 0))
    return float(max(np.max(r2), np.max(rmax)))
