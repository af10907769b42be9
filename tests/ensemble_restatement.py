"""numpy float64 restatement of the engine's ensemble accumulators (Welford's update, Chan, Golub & LeVeque's pairwise
merge, variance and standard deviation) and of its cross-spectrum, in the operand orders include/bchmc.h states.

numpy contracts nothing into fused multiply-adds and its divide and sqrt are IEEE, so the accumulator functions are the
bit-exact twins of the kernels in barcode_amd/csrc/ensemble.hpp: tests compare them with ``numpy.array_equal``.

The cross-spectrum is measure_spectrum (field_statistics.cpp:20-90) on two transforms at once: ``numpy.fft.rfftn``, the
Hermitian weight of the half grid (1 for k = 0 and the Nyquist column of an even n, 2 otherwise: the full-grid sum bin by
bin), measure_spectrum's bin expression ``(ULONG)(ktot / dk)`` with dk = |k|_max / n_bin, modes with a bin index >=
n_bin dropped (the corner mode), NORM = L^3 / N^2.  The per-bin sums run in ``numpy.longdouble``, so their own rounding
stays far inside the bounds they are compared at; the engine's sums are float atomics and are compared by tolerance.
"""
import math

import numpy as np

from tests import spec2d_restatement as sr


# ---- the accumulators ------------------------------------------------------------------------------------------
class Welford:
    """count, mean, m2 after every ``add``; ``merge`` is the pairwise update."""

    def __init__(self, size):
        self.count = 0
        self.mean = np.zeros(size)
        self.m2 = np.zeros(size)

    def add(self, x):
        x = np.asarray(x, dtype=np.float64).ravel()
        c = float(self.count + 1)
        with np.errstate(invalid="ignore", over="ignore"):
            d = x - self.mean
            self.mean = self.mean + d / c
            self.m2 = self.m2 + d * (x - self.mean)
        bad = ~np.isfinite(x)  # E4: a sample cell that is not finite makes the cell NaN
        self.mean[bad] = np.nan
        self.m2[bad] = np.nan
        self.count += 1
        return self

    def merge(self, count_b, mean_b, m2_b):
        nb = int(count_b)
        if nb == 0:
            return self
        mean_b, m2_b = np.asarray(mean_b, dtype=np.float64).ravel(), np.asarray(m2_b, dtype=np.float64).ravel()
        na = self.count
        if na == 0:
            self.mean, self.m2 = mean_b.copy(), m2_b.copy()
        else:
            w = float(nb) / float(na + nb)
            c = float(na) * float(nb) / float(na + nb)
            with np.errstate(invalid="ignore", over="ignore"):
                d = mean_b - self.mean
                self.mean = self.mean + d * w
                self.m2 = (self.m2 + m2_b) + (d * d) * c
        self.count = na + nb
        return self

    def variance(self):
        assert self.count >= 2
        return self.m2 / float(self.count - 1)

    def std(self):
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.m2 / float(self.count - 1))

    def export(self):
        return self.count, self.mean.copy(), self.m2.copy()


def two_pass(samples):
    """The reference the one-pass updates are held to: mean and ddof = 1 variance in two passes in longdouble."""
    s = np.asarray(samples, dtype=np.longdouble)
    mean = s.sum(axis=0) / s.shape[0]
    var = ((s - mean) ** 2).sum(axis=0) / (s.shape[0] - 1)
    return mean, var


# ---- the cross-spectrum ------------------------------------------------------------------------------------------
def spectrum_dk(n, L, n_bin):
    """field_statistics.cpp:37-39"""
    knyq = sr.kfac_of(L) * float(n // 2)
    return math.sqrt(knyq * knyq + knyq * knyq + knyq * knyq) / float(n_bin)


def spectrum_norm(n, L):
    """FOURIER_DEF_2, field_statistics.cpp:73-75, in the engine's order"""
    N = float(n ** 3)
    return L * L * L / N / N


def cross_spectrum_of_transforms(A, B, n, L, n_bin):
    """(kmode, nmode, power_a, power_b, cross, coeff) of two half-complex transforms [n, n, n / 2 + 1]."""
    nh = n // 2 + 1
    kv = sr.kvals(n, L)
    k2 = kv * kv
    ktot = np.sqrt((k2[:, None, None] + k2[None, :, None]) + k2[None, None, :nh])
    nbin = (ktot / spectrum_dk(n, L, n_bin)).astype(np.uint64)
    hw = np.broadcast_to(sr.hermitian_weight(n)[None, None, :], nbin.shape)
    keep = nbin < np.uint64(n_bin)
    paa = A.real * A.real + A.imag * A.imag
    pbb = B.real * B.real + B.imag * B.imag
    pab = A.real * B.real + A.imag * B.imag
    nmode, (ksum, saa, sbb, sab) = sr._bin_sums(nbin[keep], hw[keep], (ktot[keep], paa[keep], pbb[keep], pab[keep]), n_bin)
    pop = nmode > 0
    cnt = nmode[pop].astype(np.float64)
    norm = spectrum_norm(n, L)
    kmode, pa, pb, cross = (np.zeros(n_bin) for _ in range(4))
    kmode[pop] = ksum[pop] / cnt
    for o, s in ((pa, saa), (pb, sbb), (cross, sab)):
        o[pop] = s[pop] / cnt * norm
    return kmode, nmode, pa, pb, cross, coeff_of(pa, pb, cross)


def coeff_of(power_a, power_b, cross):
    """cross / sqrt(power_a power_b); 0 where the product is 0 (an empty bin among them), NaN where it is NaN."""
    pp = np.asarray(power_a) * np.asarray(power_b)
    coeff = np.zeros(pp.shape)
    with np.errstate(invalid="ignore"):
        nz = pp != 0.
        coeff[nz] = np.asarray(cross)[nz] / np.sqrt(pp[nz])
    return coeff


def cross_spectrum(a, b, n, L, n_bin):
    shape = (n, n, n)
    A = np.fft.rfftn(np.asarray(a, dtype=np.float64).reshape(shape))
    B = np.fft.rfftn(np.asarray(b, dtype=np.float64).reshape(shape))
    return cross_spectrum_of_transforms(A, B, n, L, n_bin)


def spectrum_full_grid(a, n, L, n_bin):
    """measure_spectrum as the vectorised full-grid sum of tests/test_oracle_cpu.py -> (kmode, power, count)."""
    F = np.fft.fftn(np.asarray(a, dtype=np.float64).reshape(n, n, n))
    kv = sr.kvals(n, L)
    k2 = kv * kv
    kt = np.sqrt((k2[:, None, None] + k2[None, :, None]) + k2[None, None, :])
    b = (kt / spectrum_dk(n, L, n_bin)).astype(np.int64).ravel()
    ok = b < n_bin
    cnt = np.bincount(b[ok], minlength=n_bin)
    ks = np.bincount(b[ok], weights=kt.ravel()[ok], minlength=n_bin)
    ps = np.bincount(b[ok], weights=(F.real * F.real + F.imag * F.imag).ravel()[ok], minlength=n_bin)
    has = cnt > 0
    kmode, power = np.zeros(n_bin), np.zeros(n_bin)
    kmode[has] = ks[has] / cnt[has]
    power[has] = ps[has] / cnt[has] * spectrum_norm(n, L)
    return kmode, power, cnt.astype(np.uint64)
