"""numpy restatement of the reference's correlation-function tools: ``measure_corr_grid`` (tools/corr_fct.cc:20-80)
and ``measure_corr2D`` (tools/2D_corr_fct.cc:23-124, plane-parallel), each as the literal triple loop (small grids) and
in vectorised form.  The transforms are ``numpy.fft`` on the full complex grid, like FFT3dR2C / FFT3dC2R
(fftwrapper.cc: the inverse is normalised by 1/N).

Two properties of the tools are carried as switches:

* ``guard`` (C1): ``measure_corr_grid`` does not bound its bin index (the test is commented out, corr_fct.cc:60-67) and
  writes element ``N_bin`` of its arrays for the corner cell.  ``guard=True`` (what the engine does) drops such a cell.
  ``guard=False`` is upstream with the memory it writes made visible: the arrays get ``N_bin + 1`` elements, and an
  index beyond that raises.  Either way the cells with an index >= N_bin are listed.
* ``odd_term`` (C2): ``absolute_squared_array(Signal, Signal, N)`` (2D_corr_fct.cc:43) sets the real part only, so the
  inverse transform sees |S|^2 + i Im S and A(r) carries (delta(r) - delta(-r)) / 2 as well.  ``odd_term=True`` is that
  form, ``False`` the plain autocorrelation.

The per-bin sums of the vectorised form run in ``numpy.longdouble``, so that the restatement's own summation error
(a plain double loop over up to N cells loses about sqrt(N) ulp) stays far inside the bounds it is compared at.
"""
import math

import numpy as np


def rmax_dr(L, n_bin):
    """2D_corr_fct.cc:35-39, in this order."""
    rmax = L / 2 * math.sqrt(3)
    return rmax, rmax / float(n_bin)


def auto_nbin(n, L):
    """The tools' "N_bin = 0" rule (2D_corr_fct.cc:277-286)."""
    rmax = L / 2 * math.sqrt(3)
    return int(math.ceil(rmax / (L / float(n))))


def pacman_center_on_origin(ix, n, d):
    """pacman.cpp:66-71"""
    return d * ix if ix <= n // 2 else -d * (n - ix)


def corr_field(signal, n, odd_term=False):
    """A(r) = FFT3dC2R[ absolute_squared(FFT3dR2C signal) ] as an (n, n, n) array [i, j, k]."""
    S = np.fft.fftn(np.asarray(signal, dtype=np.float64).reshape(n, n, n))
    P = (S.real * S.real + S.imag * S.imag).astype(np.complex128)
    if odd_term:
        P = P + 1j * S.imag
    return np.fft.ifftn(P).real


def _normalise(rsum, asum, nmode, N):
    rmode = np.zeros(nmode.shape)
    corr = np.zeros(nmode.shape)
    pop = nmode > 0
    rmode[pop] = np.asarray(rsum[pop] / nmode[pop], dtype=np.float64)
    corr[pop] = np.asarray(asum[pop], dtype=np.float64) / (nmode[pop].astype(np.float64) * float(N))
    return rmode, corr


# ---- literal loops --------------------------------------------------------------------------------------------
def corr_grid_loops(signal, n, L, n_bin, guard=True, odd_term=False):
    """corr_fct.cc:48-79 statement for statement.  Returns (rmode, nmode, corr, out_of_range) with out_of_range the list
    of (i, j, k, nbin) upstream would write past its arrays."""
    assert n <= 16, "the literal loop is for small grids"
    d = L / float(n)
    N = n ** 3
    _, dr = rmax_dr(L, n_bin)
    A = corr_field(signal, n, odd_term)
    size = n_bin if guard else n_bin + 1
    rmode, corr, nmode = np.zeros(size), np.zeros(size), np.zeros(size, dtype=np.uint64)
    out = []
    for i in range(n):
        for j in range(n):
            for k in range(n):
                x, y, z = (pacman_center_on_origin(t, n, d) for t in (i, j, k))
                rtot = math.sqrt(x * x + y * y + z * z)
                nbin = int(rtot / dr)
                if nbin >= n_bin:
                    out.append((i, j, k, nbin))
                    if guard:
                        continue
                rmode[nbin] += rtot  # guard off: IndexError beyond the one extra element
                corr[nbin] += A[i, j, k]
                nmode[nbin] += 1
    for l in range(size):
        if nmode[l] > 0:
            rmode[l] /= float(nmode[l])
            corr[l] /= float(nmode[l]) * float(N)
    return rmode, nmode, corr, out


def corr2d_loops(signal, n, L, n_bin, odd_term=False):
    """2D_corr_fct.cc:57-123 statement for statement; arrays of n_bin^2, element par + n_bin * perp."""
    assert n <= 16, "the literal loop is for small grids"
    d = L / float(n)
    N = n ** 3
    _, dr = rmax_dr(L, n_bin)
    A = corr_field(signal, n, odd_term)
    sq = n_bin * n_bin
    rmode, corr, nmode = np.zeros(sq), np.zeros(sq), np.zeros(sq, dtype=np.uint64)
    for i in range(n):
        for j in range(n):
            for k in range(n):
                x, y, z = (pacman_center_on_origin(t, n, d) for t in (i, j, k))
                rtot = math.sqrt(x * x + y * y + z * z)
                rpar = math.sqrt(z * z)
                rperp = math.sqrt(x * x + y * y)
                nbin_perp, nbin_par = int(rperp / dr), int(rpar / dr)
                if nbin_perp < n_bin and nbin_par < n_bin:
                    ii = nbin_par + n_bin * nbin_perp
                    rmode[ii] += rtot
                    corr[ii] += A[i, j, k]
                    nmode[ii] += 1
    for l in range(sq):
        if nmode[l] > 0:
            rmode[l] /= float(nmode[l])
            corr[l] /= float(nmode[l]) * float(N)
    return rmode, nmode, corr


# ---- vectorised -------------------------------------------------------------------------------------------------
def _positions(n, L):
    d = L / float(n)
    ix = np.arange(n)
    return np.where(ix <= n // 2, d * ix, -d * (n - ix))


def _bin_sums(bins, keep, values, n_bins):
    """Per-bin count and longdouble sums of every array in ``values`` over the cells with ``keep``."""
    idx = np.flatnonzero(keep.ravel())
    b = bins.ravel()[idx]
    order = np.argsort(b, kind="stable")
    bs = b[order]
    starts = np.flatnonzero(np.r_[True, bs[1:] != bs[:-1]])
    ub = bs[starts].astype(np.int64)
    nmode = np.zeros(n_bins, dtype=np.uint64)
    nmode[ub] = np.diff(np.r_[starts, bs.size]).astype(np.uint64)
    sums = []
    for v in values:
        full = np.zeros(n_bins, dtype=np.longdouble)
        full[ub] = np.add.reduceat(v.ravel()[idx][order].astype(np.longdouble), starts)
        sums.append(full)
    return nmode, sums


def corr_grid(signal, n, L, n_bin, guard=True, odd_term=False):
    """measure_corr_grid, vectorised.  Returns (rmode, nmode, corr, out_of_range) like ``corr_grid_loops``."""
    pos = _positions(n, L)
    _, dr = rmax_dr(L, n_bin)
    p2 = pos * pos
    rtot = np.sqrt((p2[:, None, None] + p2[None, :, None]) + p2[None, None, :])
    nbin = (rtot / dr).astype(np.uint64)
    out = [tuple(int(t) for t in c) + (int(nbin[tuple(c)]),) for c in np.argwhere(nbin >= n_bin)]
    size = n_bin if guard else n_bin + 1
    if not guard and out and max(o[3] for o in out) >= size:
        raise IndexError("bin index %d beyond the one extra element" % max(o[3] for o in out))
    nmode, (rsum, asum) = _bin_sums(nbin, nbin < size, (rtot, corr_field(signal, n, odd_term)), size)
    rmode, corr = _normalise(rsum, asum, nmode, n ** 3)
    return rmode, nmode, corr, out


def corr2d(signal, n, L, n_bin, odd_term=False):
    """measure_corr2D (plane-parallel), vectorised; flat arrays of n_bin^2, element par + n_bin * perp."""
    pos = _positions(n, L)
    _, dr = rmax_dr(L, n_bin)
    p2 = pos * pos
    r2p = p2[:, None] + p2[None, :]
    rtot = np.sqrt(r2p[:, :, None] + p2[None, None, :])
    nperp = (np.sqrt(r2p) / dr).astype(np.uint64)
    npar = (np.sqrt(p2) / dr).astype(np.uint64)
    keep = (nperp < n_bin)[:, :, None] & (npar < n_bin)[None, None, :]
    ii = npar[None, None, :] + np.uint64(n_bin) * nperp[:, :, None]
    nmode, (rsum, asum) = _bin_sums(ii, keep, (rtot, corr_field(signal, n, odd_term)), n_bin * n_bin)
    rmode, corr = _normalise(rsum, asum, nmode, n ** 3)
    return rmode, nmode, corr
