"""numpy restatement of the reference's ``measure_spec2D`` (tools/2D_powspec.cc:25-110, plane-parallel, line of sight
= z): as the literal triple loop over the full complex grid (small grids), and vectorised on the Hermitian-weighted half
grid of ``numpy.fft.rfftn``.  Both return flat arrays of n_bin^2 (kmode, nmode, power), element ``par + n_bin * perp``.

Four properties of the tool are restated as they are:

* S1: ``NORM = L^3 / (4 pi) / N^2`` carries a 1 / (4 pi) that measure_spectrum's does not (upstream: "TODO: check").
* S2: ``dk = kmax / (N_bin - 1)``.  k_perp <= sqrt(2) k_Ny and k_par <= k_Ny are below kmax = sqrt(3) k_Ny, so the bound
  test never fires, every mode is binned and the top perp and par bins are empty.  ``N_bin = 1``: the C++ division by 0.
  gives +inf and every mode lands in bin 0; Python's ``/ 0`` raises, so that case is spelled out in ``kmax_dk``.
* S3: ky comes from calc_kz(j, L2, N2), the same number on a cubic box.
* S4: kmode is the mean 3-D |k| of a bin.

A mode and its conjugate partner (-i, -j, -k) share k_perp, k_par and |k|, so the half-grid sum with the weight hw(k)
-- 1 for k = 0 and for k = n / 2 of an even n, 2 otherwise -- is the full-grid sum bin by bin.  The per-bin sums of the
vectorised form run in ``numpy.longdouble``, so that its own summation error stays far inside the bounds it is compared
at.
"""
import math

import numpy as np


def kfac_of(L):
    return 2. * math.pi / L


def calc_ki(i, L, n):
    """scale_space.cpp:41-51"""
    kfac = kfac_of(L)
    return kfac * float(i) if i <= n // 2 else -kfac * float(n - i)


def kmax_dk(n, L, n_bin):
    """2D_powspec.cc:40-43: kmax = sqrt(k_squared(N/2, N/2, N/2)), dk = kmax / (N_bin - 1); +inf for N_bin = 1 (S2)."""
    knyq = calc_ki(n // 2, L, n)
    kmax = math.sqrt(knyq * knyq + knyq * knyq + knyq * knyq)
    return kmax, (kmax / float(n_bin - 1) if n_bin > 1 else math.inf)


def norm_of(n, L):
    """2D_powspec.cc:32 (S1)"""
    N = float(n ** 3)
    return L * L * L / (4. * math.pi) / (N * N)


def bin_of(kval, dk):
    """static_cast<ULONG>(k / dk)"""
    return int(kval / dk)


def _normalise(ksum, psum, nmode, n, L):
    """2D_powspec.cc:102-109"""
    kmode, power = np.zeros(nmode.shape), np.zeros(nmode.shape)
    pop = nmode > 0
    cnt = nmode[pop].astype(np.float64)
    kmode[pop] = ksum[pop] / cnt
    power[pop] = norm_of(n, L) * psum[pop] / cnt
    return kmode, power


# ---- the literal loop -------------------------------------------------------------------------------------------
def spec2d_loops(signal, n, L, n_bin):
    """2D_powspec.cc:37-109 statement for statement on the full complex grid."""
    assert n <= 16, "the literal loop is for small grids"
    S = np.fft.fftn(np.asarray(signal, dtype=np.float64).reshape(n, n, n))
    _, dk = kmax_dk(n, L, n_bin)
    sq = n_bin * n_bin
    kmode, power, nmode = np.zeros(sq), np.zeros(sq), np.zeros(sq, dtype=np.uint64)
    for i in range(n):
        for j in range(n):
            for k in range(n):
                kx, ky, kz = calc_ki(i, L, n), calc_ki(j, L, n), calc_ki(k, L, n)
                ktot = math.sqrt(kx * kx + ky * ky + kz * kz)
                kpar = math.sqrt(kz * kz)
                kperp = math.sqrt(kx * kx + ky * ky)
                nbin_perp, nbin_par = bin_of(kperp, dk), bin_of(kpar, dk)
                if nbin_perp < n_bin and nbin_par < n_bin:
                    ii = nbin_par + n_bin * nbin_perp
                    s = S[i, j, k]
                    kmode[ii] += 1 * ktot
                    power[ii] += s.real * s.real + s.imag * s.imag
                    nmode[ii] += 1
    kmode, power = _normalise(kmode, power, nmode, n, L)
    return kmode, nmode, power


# ---- vectorised, on the half grid ------------------------------------------------------------------------------
def kvals(n, L):
    ix = np.arange(n)
    kfac = kfac_of(L)
    return np.where(ix <= n // 2, kfac * ix, -kfac * (n - ix))


def hermitian_weight(n):
    """Full-grid modes a column k of the half grid stands for."""
    hw = np.full(n // 2 + 1, 2, dtype=np.uint64)
    hw[0] = 1
    if n % 2 == 0:
        hw[n // 2] = 1
    return hw


def bin_indices(n, L, n_bin):
    """(nbin_perp [n, n], nbin_par [n / 2 + 1]) in the tool's expressions."""
    kv = kvals(n, L)
    k2 = kv * kv
    _, dk = kmax_dk(n, L, n_bin)
    nperp = (np.sqrt(k2[:, None] + k2[None, :]) / dk).astype(np.uint64)
    npar = (np.sqrt(k2[:n // 2 + 1]) / dk).astype(np.uint64)
    return nperp, npar


def rows_per_perp_bin(n, L, n_bin):
    nperp, _ = bin_indices(n, L, n_bin)
    return np.bincount(nperp.ravel().astype(np.int64), minlength=n_bin).astype(np.uint64)


def weight_per_par_bin(n, L, n_bin):
    _, npar = bin_indices(n, L, n_bin)
    return np.bincount(npar.astype(np.int64), weights=hermitian_weight(n).astype(np.float64),
                       minlength=n_bin).astype(np.uint64)


def _bin_sums(bins, weights, values, n_bins):
    """Per-bin sum of the weights (exact, integer) and float64 roundings of the longdouble sums of weights * values."""
    b = bins.ravel()
    order = np.argsort(b, kind="stable")
    bs = b[order]
    starts = np.flatnonzero(np.r_[True, bs[1:] != bs[:-1]])
    ub = bs[starts].astype(np.int64)
    w = weights.ravel()[order]
    nmode = np.zeros(n_bins, dtype=np.uint64)
    nmode[ub] = np.add.reduceat(w, starts)
    sums = []
    for v in values:
        full = np.zeros(n_bins)
        full[ub] = np.add.reduceat(v.ravel()[order].astype(np.longdouble) * w.astype(np.longdouble), starts)
        sums.append(full)
    return nmode, sums


def spec2d_of_transform(S, n, L, n_bin):
    """measure_spec2D of a half-complex transform S [n, n, n / 2 + 1] (unnormalised, like FFT3dR2C's)."""
    nh = n // 2 + 1
    kv = kvals(n, L)
    k2 = kv * kv
    nperp, npar = bin_indices(n, L, n_bin)
    assert int(nperp.max()) < n_bin and int(npar.max()) < n_bin  # S2: the tool's bound test never fires
    ktot = np.sqrt((k2[:, None, None] + k2[None, :, None]) + k2[None, None, :nh])
    ii = npar[None, None, :] + np.uint64(n_bin) * nperp[:, :, None]
    hw = np.broadcast_to(hermitian_weight(n)[None, None, :], ii.shape)
    P = S.real * S.real + S.imag * S.imag
    nmode, (ksum, psum) = _bin_sums(ii, hw, (ktot, P), n_bin * n_bin)
    kmode, power = _normalise(ksum, psum, nmode, n, L)
    return kmode, nmode, power


def spec2d(signal, n, L, n_bin):
    """measure_spec2D (plane-parallel), vectorised on the Hermitian-weighted half grid; the transform is
    ``numpy.fft.rfftn`` in float64."""
    S = np.fft.rfftn(np.asarray(signal, dtype=np.float64).reshape(n, n, n))
    return spec2d_of_transform(S, n, L, n_bin)
