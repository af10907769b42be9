"""numpy restatement of the reference's up-resolving tools: ``interp_field`` (tools/interp_upres.cc:59-86, the whole of
that tool) and the two modes of tools/2D_corr_fct_interp.cc -- mode 0, ``interp_field`` followed by that file's
``measure_corr2D`` with its ``L_max`` cut (:66-174), and mode 1, ``measure_corr2D_FFTzeropad`` (:177-312) -- each as the
literal loops (small grids) and in vectorised form.  The shared pieces (positions, bin sums, normalisation, the
correlation field of a grid) are those of ``corr_restatement``.

Three properties of mode 1 are carried as switches or kept as they are:

* ``u1`` (U1): the tool's index map sends row ``i = n / 2`` to frequency ``-n / 2`` only, so for ``n_out > n`` the
  ``K = 0`` plane of the array it hands to its complex-to-real transform is not Hermitian.  ``u1="literal"`` gives that
  array to ``numpy.fft.irfftn`` as it is (which, like FFTW's c2r, returns the transform of the Hermitian part);
  ``u1="hermitian"`` (what the engine does) takes the Hermitian part of the self-conjugate planes explicitly, completes
  the full complex grid by conjugate symmetry and runs a complex inverse transform, whose imaginary part must vanish.
* ``odd_term`` (U2): as in ``corr_restatement``, upstream's ``absolute_squared_array`` leaves ``i Im S`` in the array.
* U3: mode 1 is normalised by ``N_out`` twice, so its ``corr`` is ``(N / N_out)^2`` times the correlation function.  Kept.
"""
import math

import numpy as np

from tests import corr_restatement as cr


# ---- interp_field -------------------------------------------------------------------------------------------------
def cic_cell(m, n, n_out, L):
    """getCICcells / getCICweights (interpolate_grid.cpp:27-79) of the centre of fine cell ``m`` along one axis, in the
    reference's expressions and order (Python floats: IEEE double, no contraction).  Returns (i0, i1, dx)."""
    d = L / float(n)
    d_out = L / float(n_out)
    pos = d_out * (0.5 + float(m))
    xpos = pos - 0.5 * d
    if xpos < 0.:  # pacman_coordinate, pacman.cpp:20-28
        xpos = math.fmod(xpos, L)
        xpos += L
    if xpos >= L:
        xpos = math.fmod(xpos, L)
    c = int(xpos / d)
    c = (c + n) % n
    return c, (c + 1) % n, xpos / d - float(c)


def cic_table(n, n_out, L):
    """(i0, i1, dx) of every fine index: the grid is a cube, so one table serves the three axes."""
    t = [cic_cell(m, n, n_out, L) for m in range(n_out)]
    return (np.array([c[0] for c in t], dtype=np.int64), np.array([c[1] for c in t], dtype=np.int64),
            np.array([c[2] for c in t], dtype=np.float64))


def interp_field_loops(signal, n, L, n_out):
    """interp_upres.cc:72-85 with interpolate_CIC (interpolate_grid.cpp:82-103) statement for statement."""
    assert n_out <= 16, "the literal loop is for small grids"
    f = np.asarray(signal, dtype=np.float64).reshape(n, n, n)
    out = np.empty((n_out, n_out, n_out))
    for i in range(n_out):
        i0, i1, dx0 = cic_cell(i, n, n_out, L)
        tx0 = 1. - dx0
        for j in range(n_out):
            j0, j1, dx1 = cic_cell(j, n, n_out, L)
            tx1 = 1. - dx1
            for k in range(n_out):
                k0, k1, dx2 = cic_cell(k, n, n_out, L)
                tx2 = 1. - dx2
                F = lambda a, b, c: float(f[a, b, c])  # noqa: E731
                out[i, j, k] = (F(i0, j0, k0) * tx0 * tx1 * tx2 +
                                F(i1, j0, k0) * dx0 * tx1 * tx2 +
                                F(i0, j1, k0) * tx0 * dx1 * tx2 +
                                F(i0, j0, k1) * tx0 * tx1 * dx2 +
                                F(i1, j1, k0) * dx0 * dx1 * tx2 +
                                F(i1, j0, k1) * dx0 * tx1 * dx2 +
                                F(i0, j1, k1) * tx0 * dx1 * dx2 +
                                F(i1, j1, k1) * dx0 * dx1 * dx2)
    return out.reshape(-1)


def interp_field(signal, n, L, n_out):
    """interp_field, vectorised: the same eight terms, products and sum in the same order (every numpy operation is one
    IEEE double operation per element, so this is the loop's result bit for bit)."""
    f = np.asarray(signal, dtype=np.float64).reshape(n, n, n)
    i0, i1, dx = cic_table(n, n_out, L)
    tx = 1. - dx
    a0, a1 = (i0[:, None, None], i1[:, None, None])
    b0, b1 = (i0[None, :, None], i1[None, :, None])
    c0, c1 = (i0[None, None, :], i1[None, None, :])
    dx0, dx1, dx2 = dx[:, None, None], dx[None, :, None], dx[None, None, :]
    tx0, tx1, tx2 = tx[:, None, None], tx[None, :, None], tx[None, None, :]
    out = ((f[a0, b0, c0] * tx0) * tx1) * tx2
    out = out + ((f[a1, b0, c0] * dx0) * tx1) * tx2
    out = out + ((f[a0, b1, c0] * tx0) * dx1) * tx2
    out = out + ((f[a0, b0, c1] * tx0) * tx1) * dx2
    out = out + ((f[a1, b1, c0] * dx0) * dx1) * tx2
    out = out + ((f[a1, b0, c1] * dx0) * tx1) * dx2
    out = out + ((f[a0, b1, c1] * tx0) * dx1) * dx2
    out = out + ((f[a1, b1, c1] * dx0) * dx1) * dx2
    return out.reshape(-1)


# ---- the 2-D bins of a correlation field on the fine grid, with the cut ---------------------------------------------
def bins2d_loops(A, n, L, n_bin, l_max=None):
    """2D_corr_fct_interp.cc:104-173 (``l_max`` given: the cut of :123, both comparisons strict) or :244-311 (None)."""
    assert n <= 16, "the literal loop is for small grids"
    d = L / float(n)
    N = n ** 3
    _, dr = cr.rmax_dr(L, n_bin)
    sq = n_bin * n_bin
    rmode, corr, nmode = np.zeros(sq), np.zeros(sq), np.zeros(sq, dtype=np.uint64)
    for i in range(n):
        for j in range(n):
            for k in range(n):
                x, y, z = (cr.pacman_center_on_origin(t, n, d) for t in (i, j, k))
                rpar = math.sqrt(z * z)
                rperp = math.sqrt(x * x + y * y)
                if l_max is not None and not (rpar < l_max and rperp < l_max):
                    continue
                nbin_perp, nbin_par = int(rperp / dr), int(rpar / dr)
                if nbin_perp < n_bin and nbin_par < n_bin:
                    ii = nbin_par + n_bin * nbin_perp
                    rmode[ii] += math.sqrt(x * x + y * y + z * z)
                    corr[ii] += A[i, j, k]
                    nmode[ii] += 1
    for l in range(sq):
        if nmode[l] > 0:
            rmode[l] /= float(nmode[l])
            corr[l] /= float(nmode[l]) * float(N)
    return rmode, nmode, corr


def bins2d(A, n, L, n_bin, l_max=None):
    """``bins2d_loops``, vectorised (``corr_restatement.corr2d``'s sums with the cut added to the mask)."""
    pos = cr._positions(n, L)
    _, dr = cr.rmax_dr(L, n_bin)
    p2 = pos * pos
    r2p = p2[:, None] + p2[None, :]
    rtot = np.sqrt(r2p[:, :, None] + p2[None, None, :])
    rperp, rpar = np.sqrt(r2p), np.sqrt(p2)
    nperp = (rperp / dr).astype(np.uint64)
    npar = (rpar / dr).astype(np.uint64)
    ok_perp, ok_par = nperp < n_bin, npar < n_bin
    if l_max is not None:
        ok_perp, ok_par = ok_perp & (rperp < l_max), ok_par & (rpar < l_max)
    keep = ok_perp[:, :, None] & ok_par[None, None, :]
    ii = npar[None, None, :] + np.uint64(n_bin) * nperp[:, :, None]
    nmode, (rsum, asum) = cr._bin_sums(ii, keep, (rtot, np.asarray(A).reshape(n, n, n)), n_bin * n_bin)
    rmode, corr = cr._normalise(rsum, asum, nmode, n ** 3)
    return rmode, nmode, corr


# ---- mode 0: CIC interpolation ----------------------------------------------------------------------------------------
def corr2d_interp_cic_loops(signal, n, L, n_out, n_bin, l_max, odd_term=False):
    fine = interp_field_loops(signal, n, L, n_out)
    return bins2d_loops(cr.corr_field(fine, n_out, odd_term), n_out, L, n_bin, l_max)


def corr2d_interp_cic(signal, n, L, n_out, n_bin, l_max, odd_term=False):
    fine = interp_field(signal, n, L, n_out)
    return bins2d(cr.corr_field(fine, n_out, odd_term), n_out, L, n_bin, l_max)


# ---- mode 1: zero padding of the power spectrum ---------------------------------------------------------------------------
def zeropad_index(n, n_out):
    """2D_corr_fct_interp.cc:205-214: where coarse index i goes (integer n / 2, for odd n too)."""
    i = np.arange(n)
    return np.where(i < n // 2, i, n_out - (n - i))


def _power_half(signal, n, odd_term):
    S = np.fft.rfftn(np.asarray(signal, dtype=np.float64).reshape(n, n, n))  # (n, n, n / 2 + 1), like fftR2C
    P = (S.real * S.real + S.imag * S.imag).astype(np.complex128)
    return P + 1j * S.imag if odd_term else P


def zeropad_power_loops(signal, n, n_out, odd_term=False):
    """The literal array of :203-222: (n_out, n_out, n_out / 2 + 1), zero but for the copied modes."""
    assert n <= 16 and n_out >= n
    P = _power_half(signal, n, odd_term)
    out = np.zeros((n_out, n_out, n_out // 2 + 1), dtype=np.complex128)
    for i in range(n):
        I = i if i < n // 2 else n_out - (n - i)
        for j in range(n):
            J = j if j < n // 2 else n_out - (n - j)
            for k in range(n // 2 + 1):
                out[I, J, k] = P[i, j, k]
    return out


def zeropad_power(signal, n, n_out, odd_term=False):
    assert n_out >= n
    out = np.zeros((n_out, n_out, n_out // 2 + 1), dtype=np.complex128)
    I = zeropad_index(n, n_out)
    out[np.ix_(I, I, np.arange(n // 2 + 1))] = _power_half(signal, n, odd_term)
    return out


def _neg(n):
    return (-np.arange(n)) % n


def hermitian_full(P, n_out):
    """The full complex (n_out, n_out, n_out) grid of the Hermitian part of the half-complex array P: the planes that
    are their own partner (K = 0, and K = n_out / 2 at even n_out) become (P(I, J, K) + conj P(-I, -J, K)) / 2, the
    planes K > n_out / 2 are the conjugates of their partners."""
    m = _neg(n_out)
    F = np.zeros((n_out, n_out, n_out), dtype=np.complex128)
    nh = n_out // 2 + 1
    F[:, :, :nh] = P
    own = [0] + ([n_out // 2] if n_out % 2 == 0 else [])
    for K in own:
        F[:, :, K] = 0.5 * (P[:, :, K] + np.conj(P[:, :, K][np.ix_(m, m)]))
    for K in range(nh, n_out):
        F[:, :, K] = np.conj(F[:, :, n_out - K][np.ix_(m, m)])
    return F


def zeropad_corr_field(P, n_out, u1="literal"):
    """The tool's fftC2R (normalised by 1 / N_out) of the zero-padded array."""
    if u1 == "literal":
        return np.fft.irfftn(P, s=(n_out,) * 3, axes=(0, 1, 2))
    assert u1 == "hermitian"
    A = np.fft.ifftn(hermitian_full(P, n_out))
    assert np.max(np.abs(A.imag)) <= 1e-13 * max(np.max(np.abs(A.real)), 1e-300)
    return A.real


def corr2d_zeropad_loops(signal, n, L, n_out, n_bin, u1="literal", odd_term=False):
    A = zeropad_corr_field(zeropad_power_loops(signal, n, n_out, odd_term), n_out, u1)
    return bins2d_loops(A, n_out, L, n_bin)


def corr2d_zeropad(signal, n, L, n_out, n_bin, u1="hermitian", odd_term=False):
    A = zeropad_corr_field(zeropad_power(signal, n, n_out, odd_term), n_out, u1)
    return bins2d(A, n_out, L, n_bin)
