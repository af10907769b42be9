"""The Legendre multipoles P_l(k) and xi_l(s), l = 0, 2, 4, about the line of sight z, stated twice.

* The definition (``power_def``, ``corr_def``): a plain enumeration of every mode of the full complex grid of
  ``numpy.fft.fftn``, and of every cell of A(r) for xi_l.  Bin indices are float64 expressions in the reference's operand
  order (measure_spectrum, field_statistics.cpp:20-90; measure_corr_grid, corr_fct.cc:48-79); weights and sums are
  ``numpy.longdouble``.
* The restatement (``power``, ``corr``): vectorised float64 on ``numpy.fft.rfftn`` with the Hermitian weight hw(k) -- 1
  for k = 0 and for k = n / 2 of an even n, 2 otherwise.  A mode and its conjugate partner share |k| and mu^2, so the
  weighted half-grid sum is the full-grid sum bin by bin.  Per-bin sums run in longdouble, as in the sister restatements,
  so that the summation error of the restatement stays far inside the bounds it is compared at.

With mu^2 = z^2 / (x^2 + y^2 + z^2):  L_0 = 1,  L_2 = 1.5 mu^2 - 0.5,  L_4 = (35 mu^4 - 30 mu^2 + 3) / 8, in exactly this
operand order.  The element at the origin (k = 0, r = 0) has no mu: it counts in l = 0, in the count and in the mean
|k| or r, and contributes 0 to l = 2, 4 and to leg.

    P_l[b]  = (2 l + 1) NORM sum |x^|^2 L_l / nmode[b],  NORM = L^3 / N^2
    xi_l[b] = (2 l + 1) sum A L_l / (nmode[b] N)
    leg[b]  = the mean of L_2 and of L_4 over the bin's elements

Every function returns a dict: ``t`` (mean |k| or r), ``nmode`` (uint64), ``leg`` (2, n_bin), ``m`` (3, n_bin).
``mutant`` in {None, "los_x", "l4_35", "no_hw", "no_2l1"} makes the restatement wrong on purpose (tests only).
"""
import math

import numpy as np

ELLS = (0, 2, 4)
MUTANTS = ("los_x", "l4_35", "no_hw", "no_2l1")


def kfac_of(L):
    return 2. * math.pi / L


def spectrum_dk(n, L, n_bin):
    """field_statistics.cpp:37-39: |k|_max / N_bin"""
    knyq = kfac_of(L) * float(n // 2)
    kmax = math.sqrt(knyq * knyq + knyq * knyq + knyq * knyq)
    return kmax / float(n_bin)


def corr_dr(L, n_bin):
    """corr_fct.cc / 2D_corr_fct.cc:35-39, in this order"""
    rmax = L / 2 * math.sqrt(3)
    return rmax / float(n_bin)


def coord(ix, n, u):
    """calc_ki (u = 2 pi / L) and pacman_center_on_origin (u = L / n)"""
    return u * float(ix) if ix <= n // 2 else -u * float(n - ix)


def legendre(mu2, mutant=None):
    l2 = 1.5 * mu2 - 0.5
    l4 = (35. * mu2 * mu2 - (35. if mutant == "l4_35" else 30.) * mu2 + 3.) / 8.
    return l2, l4


def corr_field(signal, n):
    """A(r) = C2R[|R2C signal|^2] / N: sum_x delta(x) delta(x + r), as an (n, n, n) array"""
    S = np.fft.fftn(np.asarray(signal, dtype=np.float64).reshape(n, n, n))
    return np.fft.ifftn((S.real * S.real + S.imag * S.imag).astype(np.complex128)).real


# ---- the definition ---------------------------------------------------------------------------------------------
def _enumerate(values, n, u, dt, n_bin, norm):
    """values[i, j, k] (real) summed over every element of the full grid with the weights L_l of its coordinates."""
    assert n <= 16, "the enumeration is for small grids"
    ld = np.longdouble
    tsum, cnt = [ld(0)] * n_bin, [0] * n_bin
    lsum = [[ld(0)] * n_bin for _ in range(2)]
    msum = [[ld(0)] * n_bin for _ in range(3)]
    for i in range(n):
        for j in range(n):
            for k in range(n):
                x, y, z = coord(i, n, u), coord(j, n, u), coord(k, n, u)
                t2 = x * x + y * y + z * z
                t = math.sqrt(t2)
                b = int(t / dt)
                if b >= n_bin:
                    continue
                l2, l4 = legendre((z * z) / t2) if t2 > 0. else (0., 0.)
                v = ld(values[i, j, k])
                cnt[b] += 1
                tsum[b] += ld(t)
                lsum[0][b] += ld(l2)
                lsum[1][b] += ld(l4)
                msum[0][b] += v
                msum[1][b] += v * ld(l2)
                msum[2][b] += v * ld(l4)
    out = dict(t=np.zeros(n_bin), nmode=np.array(cnt, dtype=np.uint64), leg=np.zeros((2, n_bin)), m=np.zeros((3, n_bin)))
    for b in range(n_bin):
        if cnt[b]:
            out["t"][b] = float(tsum[b] / cnt[b])
            for a in range(2):
                out["leg"][a, b] = float(lsum[a][b] / cnt[b])
            for a, ell in enumerate(ELLS):
                out["m"][a, b] = float(ld(2 * ell + 1) * ld(norm) * msum[a][b] / cnt[b])
    return out


def power_def(signal, n, L, n_bin):
    S = np.fft.fftn(np.asarray(signal, dtype=np.float64).reshape(n, n, n))
    N = float(n ** 3)
    return _enumerate(S.real * S.real + S.imag * S.imag, n, kfac_of(L), spectrum_dk(n, L, n_bin), n_bin, L * L * L / N / N)


def corr_def(signal, n, L, n_bin):
    return _enumerate(corr_field(signal, n), n, L / float(n), corr_dr(L, n_bin), n_bin, 1. / float(n ** 3))


# ---- the restatement --------------------------------------------------------------------------------------------
def coords(n, u):
    ix = np.arange(n)
    return np.where(ix <= n // 2, u * ix, -u * (n - ix))


def hermitian_weight(n):
    hw = np.full(n // 2 + 1, 2., dtype=np.float64)
    hw[0] = 1.
    if n % 2 == 0:
        hw[n // 2] = 1.
    return hw


def geometry(n, u, dt, nz, mutant=None):
    """(t, bin, L_2, L_4) of the elements [n, n, nz] of a grid with coordinates ``coords(n, u)``"""
    c = coords(n, u)
    c2 = c * c
    t2 = (c2[:, None, None] + c2[None, :, None]) + c2[None, None, :nz]
    t = np.sqrt(t2)
    b = (t / dt).astype(np.uint64)
    los2 = np.broadcast_to(c2[:, None, None] if mutant == "los_x" else c2[None, None, :nz], t2.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu2 = los2 / t2
    l2, l4 = legendre(mu2, mutant)
    origin = t2 == 0.
    return t, b, np.where(origin, 0., l2), np.where(origin, 0., l4)


def _bin_sums(bins, keep, weights, values, n_bins):
    """Per-bin sum of the weights (integers, exact) and longdouble sums of weights * values over the elements with keep"""
    idx = np.flatnonzero(keep.ravel())
    b = bins.ravel()[idx]
    order = np.argsort(b, kind="stable")
    bs = b[order]
    starts = np.flatnonzero(np.r_[True, bs[1:] != bs[:-1]]) if bs.size else np.zeros(0, dtype=np.int64)
    ub = bs[starts].astype(np.int64)
    w = np.broadcast_to(weights, bins.shape).ravel()[idx][order]
    nmode = np.zeros(n_bins, dtype=np.uint64)
    sums = [np.zeros(n_bins, dtype=np.longdouble) for _ in values]
    if bs.size:
        nmode[ub] = np.rint(np.add.reduceat(w.astype(np.longdouble), starts)).astype(np.uint64)
        for s, v in zip(sums, values):
            s[ub] = np.add.reduceat(v.ravel()[idx][order].astype(np.longdouble) * w.astype(np.longdouble), starts)
    return nmode, sums


def multipoles_of(values, n, u, dt, n_bin, norm, weights, mutant=None):
    """The restatement on values [n, n, nz] with per-column weights [nz]: one or several value arrays at once.
    Returns (t, nmode, leg, [m per value array])."""
    nz = values[0].shape[2]
    t, b, l2, l4 = geometry(n, u, dt, nz, mutant)
    w = weights[None, None, :]
    prods = [t, l2, l4]
    for v in values:
        prods += [v, v * l2, v * l4]
    nmode, sums = _bin_sums(b, b < n_bin, w, prods, n_bin)
    pop = nmode > 0
    cnt = nmode[pop].astype(np.longdouble)
    tmode, leg = np.zeros(n_bin), np.zeros((2, n_bin))
    tmode[pop] = (sums[0][pop] / cnt).astype(np.float64)
    leg[0, pop] = (sums[1][pop] / cnt).astype(np.float64)
    leg[1, pop] = (sums[2][pop] / cnt).astype(np.float64)
    ms = []
    for q in range(len(values)):
        m = np.zeros((3, n_bin))
        for a, ell in enumerate(ELLS):
            fac = 1. if mutant == "no_2l1" else float(2 * ell + 1)
            m[a, pop] = (np.longdouble(fac) * np.longdouble(norm) * sums[3 + 3 * q + a][pop] / cnt).astype(np.float64)
        ms.append(m)
    return tmode, nmode, leg, ms


def power_of_transforms(Sa, Sb, n, L, n_bin, mutant=None):
    """Sa, Sb: half-complex transforms [n, n, n / 2 + 1] (unnormalised).  Returns the dict with ``m`` = P^AA and, Sb not
    None, ``mbb`` and ``mab`` (summand re_a re_b + im_a im_b)."""
    N = float(n ** 3)
    vals = [Sa.real * Sa.real + Sa.imag * Sa.imag]
    if Sb is not None:
        vals += [Sb.real * Sb.real + Sb.imag * Sb.imag, Sa.real * Sb.real + Sa.imag * Sb.imag]
    hw = np.ones(n // 2 + 1) if mutant == "no_hw" else hermitian_weight(n)
    t, nmode, leg, ms = multipoles_of(vals, n, kfac_of(L), spectrum_dk(n, L, n_bin), n_bin, L * L * L / N / N, hw, mutant)
    out = dict(t=t, nmode=nmode, leg=leg, m=ms[0])
    if Sb is not None:
        out.update(mbb=ms[1], mab=ms[2])
    return out


def power(signal, n, L, n_bin, other=None, mutant=None):
    rf = lambda s: np.fft.rfftn(np.asarray(s, dtype=np.float64).reshape(n, n, n))  # noqa: E731
    return power_of_transforms(rf(signal), None if other is None else rf(other), n, L, n_bin, mutant)


def corr(signal, n, L, n_bin, mutant=None):
    """xi_l on the full real grid A(r) (every cell weighs 1; "no_hw" has no meaning here and changes nothing)"""
    A = corr_field(signal, n)
    t, nmode, leg, ms = multipoles_of([A], n, L / float(n), corr_dr(L, n_bin), n_bin, 1. / float(n ** 3), np.ones(n), mutant)
    return dict(t=t, nmode=nmode, leg=leg, m=ms[0])


# ---- fields with known answers --------------------------------------------------------------------------------------
def plane_wave(n, L, m):
    """cos(2 pi (m . x) / L) on the grid, m = (mx, my, mz) integers: all its power sits in the modes +-m"""
    ix = np.arange(n, dtype=np.float64)
    ph = (m[0] * ix[:, None, None] + m[1] * ix[None, :, None] + m[2] * ix[None, None, :]) * (2. * math.pi / n)
    return np.cos(ph).reshape(-1)


def kaiser_field(n, L, beta, seed):
    """A real field whose transform is (1 + beta mu^2) e^{i phi} with seeded Hermitian phases and unit modulus, DC = 0.
    Returns (field, transform as rfftn returns it)."""
    rng = np.random.RandomState(seed)
    white = np.fft.rfftn(rng.standard_normal((n, n, n)))
    mod = np.abs(white)
    phase = np.where(mod > 0, white / np.where(mod > 0, mod, 1.), 1.)  # Hermitian, |.| = 1; self-conjugate modes are +-1
    c = coords(n, kfac_of(L))
    c2 = c * c
    t2 = (c2[:, None, None] + c2[None, :, None]) + c2[None, None, :n // 2 + 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        mu2 = np.where(t2 > 0, c2[None, None, :n // 2 + 1] / t2, 0.)
    S = (1. + beta * mu2) * phase
    S[0, 0, 0] = 0.
    field = np.fft.irfftn(S, s=(n, n, n), axes=(0, 1, 2))
    return field.reshape(-1), np.fft.rfftn(field)


def kaiser_expected(n, L, n_bin, beta):
    """(2 l + 1) NORM mean[(1 + beta mu^2)^2 L_l] per bin from the geometry alone (DC contributes 0 power)"""
    nh = n // 2 + 1
    c = coords(n, kfac_of(L))
    c2 = c * c
    t2 = (c2[:, None, None] + c2[None, :, None]) + c2[None, None, :nh]
    with np.errstate(invalid="ignore", divide="ignore"):
        mu2 = np.where(t2 > 0, c2[None, None, :nh] / t2, 0.)
    amp = (1. + beta * mu2) ** 2
    amp[0, 0, 0] = 0.
    N = float(n ** 3)
    _, nmode, _, ms = multipoles_of([amp], n, kfac_of(L), spectrum_dk(n, L, n_bin), n_bin, L * L * L / N / N,
                                    hermitian_weight(n))
    return nmode, ms[0]
