"""The bispectrum of include/bchmc.h (bchmc_bispectrum, B1-B6) in numpy, stated twice and independently:

* ``enumerate_direct``: the definition.  Over all ordered pairs (k1, k2) of modes of the full grid that lie in a shell,
  k3 = -(k1 + k2) mod n per axis; where k3 lies in a shell too, the product x^1 x^2 x^3 (longdouble direct DFT, real part)
  and a 1 go into a table indexed by the three shells.  No filtered transform anywhere.  Affordable up to n = 16.
* ``restatement``: B2-B3 as the device computes them -- per shell D_s = N ifftn(x^ 1_s), I_s = N ifftn(1_s), sums over
  cells -- in float64, for the sizes the enumeration cannot reach, with the switches of the variants the tests show to
  be wrong.

    shell of a mode: s = (ULONG)((|k| - k_min) / dk) for |k| >= k_min and s < n_shell, none for k = 0
    ntri_t = #{(k1, k2, k3) in s1 x s2 x s3 : k1 + k2 + k3 = 0 mod n},   t = (s1 <= s2 <= s3) in lexicographic order
    B_t = L^6 / N^3 * (sum over those triples of x^1 x^2 x^3) / ntri_t
    nmode, kmean, power = L^3 / N^2 * sum |x^|^2 / nmode per shell;   Q_t = B_t / (P1 P2 + P2 P3 + P3 P1)

Arrays are indexed [i, j, k] = (x, y, z).  The tests give shells in units of the fundamental k_f = 2 pi / L (``edges``);
the functions here take h/Mpc like the C ABI.
"""
import numpy as np

from tests import tweb_reference as tr

box_of = tr.box_of
field = tr.field


def edges(n, k_min_kf, dk_kf):
    """(k_min, dk) in h/Mpc of shells given in fundamentals, formed as Engine.bispectrum(units="kf") forms them."""
    kf = 2.0 * np.pi / float(box_of(n))
    return float(k_min_kf) * kf, float(dk_kf) * kf


def mode_lengths(n, L):
    """|k| on the full grid as the kernels form it: sqrt(kx kx + ky ky + kz kz), no contraction."""
    kv = tr.kval(n, L)
    k2 = (kv * kv)[:, None, None] + (kv * kv)[None, :, None]
    return np.sqrt(k2 + (kv * kv)[None, None, :])


def shells(n, L, k_min, dk, n_shell, lower_edge_strict=False, admit_zero_mode=False):
    """The shell of every mode of the full grid, (n, n, n) int64, -1 for none (B1).  The two switches are mutants."""
    k = mode_lengths(n, L)
    inside = (k > k_min) if lower_edge_strict else (k >= k_min)
    s = np.floor((k - k_min) / dk)
    s = np.where(inside & (s < n_shell), s, -1).astype(np.int64)
    if not admit_zero_mode:
        s[0, 0, 0] = -1
    return s


def triplets(n_shell):
    n = int(n_shell)
    return np.array([(a, b, c) for a in range(n) for b in range(a, n) for c in range(b, n)], dtype=np.int32).reshape(-1, 3)


def rule_active(n, L, k_min, dk, n_shell):
    """B4's condition: every shell below 2/3 k_Nyquist, k_Nyquist = pi n / L, in the doubles of bchmc_bispectrum."""
    kfac = 2.0 * np.pi / float(L)
    return k_min + float(n_shell) * dk <= (2.0 / 3.0) * (kfac * (0.5 * float(n)))


def computed(n, L, k_min, dk, n_shell):
    """Which triplets bchmc_bispectrum computes (B4): boolean (T,)."""
    trip = triplets(n_shell)
    if not rule_active(n, L, k_min, dk, n_shell):
        return np.ones(len(trip), dtype=bool)
    s1, s2, s3 = (trip[:, c].astype(np.float64) for c in range(3))
    return ~(k_min + s3 * dk >= (k_min + (s1 + 1.0) * dk) + (k_min + (s2 + 1.0) * dk))


def dft_longdouble(x):
    """The unnormalised forward transform of x on the full grid by a direct DFT in longdouble."""
    x = np.asarray(x).astype(np.longdouble)
    return tr._dft3(x.astype(np.clongdouble), tr.dft_matrix(x.shape[0], -1))


def enumerate_direct(n, L, k_min, dk, n_shell, x=None, chunk=96):
    """(count, total): tables (n_shell, n_shell, n_shell) over ALL ordered shell triples of the number of closed mode
    triples (int64) and of the sum of Re x^1 x^2 x^3 over them (longdouble).  x None: counts only, total is None."""
    ns = int(n_shell)
    sh = shells(n, L, k_min, dk, ns).ravel()
    sel = np.flatnonzero(sh >= 0)
    ii, jj, kk = np.unravel_index(sel, (n, n, n))
    s_sel = sh[sel]
    xk = None if x is None else dft_longdouble(x).ravel()
    count = np.zeros(ns ** 3, dtype=np.int64)
    total = None if x is None else np.zeros(ns ** 3, dtype=np.longdouble)
    for c0 in range(0, sel.size, chunk):
        a = slice(c0, c0 + chunk)
        f3 = (((-(ii[a, None] + ii[None, :])) % n) * n + (-(jj[a, None] + jj[None, :])) % n) * n + (-(kk[a, None] + kk[None, :])) % n
        s3 = sh[f3]
        ok = s3 >= 0
        code = ((s_sel[a, None] * ns + s_sel[None, :]) * ns + s3)[ok]
        count += np.bincount(code, minlength=ns ** 3)
        if xk is not None:
            prod = ((xk[sel[a], None] * xk[sel][None, :]) * xk[f3]).real
            np.add.at(total, code, prod[ok])
    shape = (ns, ns, ns)
    return count.reshape(shape), None if total is None else total.reshape(shape)


def sorted_table(table):
    """The entries s1 <= s2 <= s3 of an (n_shell,) * 3 table in the order of ``triplets``."""
    t = triplets(table.shape[0])
    return table[t[:, 0], t[:, 1], t[:, 2]]


def shell_stats_exact(n, L, k_min, dk, n_shell, x=None):
    """(nmode int64, kmean, power) per shell over the full grid; power in longdouble from the direct DFT (x None: None)."""
    sh = shells(n, L, k_min, dk, n_shell).ravel()
    k = mode_lengths(n, L).ravel()
    nmode = np.bincount(sh[sh >= 0], minlength=n_shell).astype(np.int64)
    ksum = np.bincount(sh[sh >= 0], weights=k[sh >= 0], minlength=n_shell)
    kmean = np.where(nmode > 0, ksum / np.where(nmode > 0, nmode, 1), 0.0)
    power = None
    if x is not None:
        p2 = np.abs(dft_longdouble(x).ravel()) ** 2
        psum = np.array([np.sum(p2[sh == s]) for s in range(n_shell)], dtype=np.longdouble)
        N = np.longdouble(n) ** 3
        power = np.where(nmode > 0, psum / np.where(nmode > 0, nmode, 1) * (np.longdouble(L) ** 3 / N / N), 0)
    return nmode, kmean, power


def definition(x, L, k_min, dk, n_shell):
    """B, ntri (exact integers) and the per-shell statistics of field x by the enumeration: a dict like ``restatement``'s,
    B and power in longdouble; B is 0 where ntri is 0 or the triplet is not computed."""
    n = x.shape[0]
    count, total = enumerate_direct(n, L, k_min, dk, n_shell, x)
    ntri, tot = sorted_table(count), sorted_table(total)
    comp = computed(n, L, k_min, dk, n_shell)
    N = np.longdouble(n) ** 3
    norm = np.longdouble(L) ** 6 / N ** 3
    filled = comp & (ntri > 0)
    b = np.where(filled, norm * tot / np.where(ntri > 0, ntri, 1), 0)
    nmode, kmean, power = shell_stats_exact(n, L, k_min, dk, n_shell, x)
    return dict(triplets=triplets(n_shell), b=b, ntri=np.where(comp, ntri, 0), count_all=count, computed=comp,
                nmode=nmode, kmean=kmean, power=power, q=reduced(b, power, filled))


def reduced(b, power, filled):
    """B6: Q = B / (P1 P2 + P2 P3 + P3 P1), 0 where the denominator is 0 or the triplet is empty."""
    t = triplets(len(power))
    p1, p2, p3 = (np.asarray(power)[t[:, c]] for c in range(3))
    den = p1 * p2 + p2 * p3 + p3 * p1
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(~np.asarray(filled) | (den == 0), 0, np.asarray(b) / np.where(den == 0, 1, den))


def shell_fields(x, L, k_min, dk, n_shell, **mutant):
    """(D (n_shell, n, n, n), I (n_shell, n, n, n)) of B2 in float64 through numpy's transforms."""
    n = x.shape[0]
    N = float(n) ** 3
    xk = np.fft.fftn(np.asarray(x, dtype=np.float64))
    sh = shells(n, L, k_min, dk, n_shell, **mutant)
    D = np.stack([np.fft.ifftn(np.where(sh == s, xk, 0)).real * N for s in range(n_shell)])
    I = np.stack([np.fft.ifftn((sh == s).astype(np.complex128)).real * N for s in range(n_shell)])
    return D, I


def restatement(x, L, k_min, dk, n_shell, lower_edge_strict=False, admit_zero_mode=False, hermitian_weight=True,
                n_power=3):
    """B1-B6 as bchmc_bispectrum computes them, in float64: the shell fields through numpy's transforms, the sums over
    cells, the per-shell statistics from the half-complex modes with their Hermitian weights.  The switches are the
    mutants of tests/test_bispec_bounds.py; n_power is the power of N in B3's normalisation."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    N = float(n) ** 3
    mutant = dict(lower_edge_strict=lower_edge_strict, admit_zero_mode=admit_zero_mode)
    D, I = shell_fields(x, L, k_min, dk, n_shell, **mutant)
    trip = triplets(n_shell)
    comp = computed(n, L, k_min, dk, n_shell)
    S = np.array([np.sum(D[a] * D[b] * D[c]) if ok else 0.0 for (a, b, c), ok in zip(trip, comp)])
    ntri = np.array([np.sum(I[a] * I[b] * I[c]) / N if ok else 0.0 for (a, b, c), ok in zip(trip, comp)])
    filled = comp & ~(ntri < 0.5)
    with np.errstate(invalid="ignore", divide="ignore"):
        b = np.where(filled, float(L) ** 6 / N ** n_power * (S / (N * np.where(filled, ntri, 1.0))), 0.0)
    # per shell, from the stored half of the modes
    nh = n // 2 + 1
    sh = shells(n, L, k_min, dk, n_shell, **mutant)[:, :, :nh]
    hw = np.full((n, n, nh), 2.0)
    hw[:, :, 0] = 1.0
    if n % 2 == 0:
        hw[:, :, n // 2] = 1.0
    if not hermitian_weight:
        hw[:] = 1.0
    k = mode_lengths(n, L)[:, :, :nh]
    p2 = np.abs(np.fft.rfftn(x)) ** 2
    m = sh >= 0
    cnt = np.bincount(sh[m], weights=hw[m], minlength=n_shell)
    ksum = np.bincount(sh[m], weights=(hw * k)[m], minlength=n_shell)
    psum = np.bincount(sh[m], weights=(hw * p2)[m], minlength=n_shell)
    safe = np.where(cnt > 0, cnt, 1.0)
    kmean = np.where(cnt > 0, ksum / safe, 0.0)
    power = np.where(cnt > 0, psum / safe * (float(L) ** 3 / N / N), 0.0)
    return dict(triplets=trip, b=b, ntri=ntri, s=S, computed=comp, nmode=cnt.astype(np.uint64), kmean=kmean, power=power,
                q=reduced(b, power, filled), D=D, I=I)


def cosines(n, waves):
    """sum of a cos(2 pi (m . r) / n) over waves = [(a, (mx, my, mz)), ...]."""
    idx = np.indices((n, n, n))
    return sum(a * np.cos(2.0 * np.pi * (m[0] * idx[0] + m[1] * idx[1] + m[2] * idx[2]) / n) for a, m in waves)
