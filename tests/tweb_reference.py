"""The T-web of include/bchmc.h (bchmc_tweb_*) in numpy: the definition the HIP kernels are held to, a float64
restatement of their eigenvalue solver, and the solvers and rules the tests show to be wrong.

    laplace(phi) = x,  T_ab = d_a d_b phi:   T^_ab = (k_a k_b / k^2) W(k) x^,  0 at k = 0,  W = exp(-k^2 R^2 / 2)
    even n: an off-diagonal T^_ab is 0 where the index of axis a or of axis b is n / 2
    lambda_1 >= lambda_2 >= lambda_3 per cell;  type = #{lambda_i > lambda_th}: 0 void, 1 sheet, 2 filament, 3 knot

The transforms are FULL complex ones (numpy.fft.fftn, or a direct DFT in longdouble), so that the imaginary part of the
inverse transform shows whether an array is the transform of a real field.  Arrays are indexed [i, j, k] = (x, y, z);
the six components come in the order xx, xy, xz, yy, yz, zz.
"""
import numpy as np

COMPONENTS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
EPS64 = 2.0 ** -52
SWEEPS = 4  # kTwebSweeps of barcode_amd/csrc/tweb.hpp


def kval(n, L):
    """calc_ki as the kernels evaluate it, in double."""
    kfac = 2.0 * np.pi / float(L)
    i = np.arange(n)
    return np.where(i <= n // 2, kfac * i.astype(np.float64), -kfac * (n - i).astype(np.float64))


def multipliers(n, L, R, wdt=np.float64, nyquist_rule=True):
    """The six real multipliers (k_a k_b / k^2) W on the full n^3 grid, in `wdt`."""
    kv = kval(n, L).astype(wdt)
    k3 = (kv[:, None, None], kv[None, :, None], kv[None, None, :])
    k2 = k3[0] ** 2 + k3[1] ** 2 + k3[2] ** 2
    safe = np.where(k2 > 0, k2, 1)
    W = np.exp(-k2 * (wdt(R) * wdt(R) / 2))
    idx = np.arange(n)
    at_nyq = [(idx == n // 2).reshape([n if a == ax else 1 for ax in range(3)]) for a in range(3)]
    out = []
    for a, b in COMPONENTS:
        f = np.where(k2 > 0, k3[a] * k3[b] / safe * W, 0) + np.zeros((n, n, n), dtype=wdt)
        if nyquist_rule and n % 2 == 0 and a != b:
            f = np.where(at_nyq[a] | at_nyq[b], 0, f)
        out.append(f)
    return out, W


def tensor(x, L, R, nyquist_rule=True):
    """(T[6], x_s, worst |imaginary part| of the six inverse transforms) of field x (n, n, n), float64 through fftn."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    xk = np.fft.fftn(x)
    f6, W = multipliers(n, L, R, nyquist_rule=nyquist_rule)
    full = [np.fft.ifftn(f * xk) for f in f6]
    imag = max(float(np.max(np.abs(t.imag))) for t in full)
    return np.stack([t.real for t in full]), np.fft.ifftn(W * xk).real, imag


def dft_matrix(n, sign, wdt=np.longdouble):
    """exp(sign 2 pi i r s / n) in `wdt`, the angle reduced mod n in integers first."""
    rs = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    ang = 2 * wdt(np.pi if wdt is np.float64 else np.arccos(wdt(-1))) * rs.astype(wdt) / wdt(n)
    return np.cos(ang) + (1j * sign) * np.sin(ang)


def _dft3(a, m):
    for ax in range(3):
        a = np.moveaxis(np.tensordot(m, a, axes=([1], [ax])), 0, ax)
    return a


def tensor_longdouble(x, L, R):
    """T[6] (longdouble, real parts) of field x by direct DFTs in longdouble; x is taken as it is (no rounding)."""
    wdt = np.longdouble
    x = np.asarray(x).astype(wdt)
    n = x.shape[0]
    xk = _dft3(x.astype(np.clongdouble), dft_matrix(n, -1))
    f6, _ = multipliers(n, L, R, wdt=wdt)
    inv = dft_matrix(n, +1)
    return np.stack([(_dft3(f * xk, inv) / wdt(n) ** 3).real for f in f6])


def as_matrices(t6):
    """(6, ...) components -> (..., 3, 3) symmetric matrices."""
    t6 = np.asarray(t6)
    m = np.empty(t6.shape[1:] + (3, 3), dtype=t6.dtype)
    for c, (a, b) in enumerate(COMPONENTS):
        m[..., a, b] = t6[c]
        m[..., b, a] = t6[c]
    return m


def from_matrices(m):
    return np.stack([m[..., a, b] for a, b in COMPONENTS])


def eigenvalues(t6):
    """(3, ...) eigenvalues, descending, by numpy.linalg.eigvalsh in float64."""
    lam = np.linalg.eigvalsh(as_matrices(np.asarray(t6, dtype=np.float64)))
    return np.moveaxis(lam[..., ::-1], -1, 0)


def web_type(lam, lambda_th):
    return np.sum(np.asarray(lam) > lambda_th, axis=0).astype(np.uint8)


def stats(types, x):
    """(n_type[4], mass_type[4]) with the mass 1 + x of the unsmoothed source."""
    t = np.asarray(types).ravel()
    w = 1.0 + np.asarray(x, dtype=np.float64).ravel()
    return (np.array([np.count_nonzero(t == ty) for ty in range(4)], dtype=np.uint64),
            np.array([np.sum(w[t == ty]) for ty in range(4)]))


# ---- the solver of k_tweb_eigen, line by line in float64 over arrays of tensors --------------------------------------
def _rotate(act, app, aqq, apq, arp, arq):
    on = act & (apq != 0)
    d = np.where(on, apq, 1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        theta = (aqq - app) / (2.0 * d)
        t = np.copysign(1.0, theta) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    return (np.where(on, app - t * apq, app), np.where(on, aqq + t * apq, aqq), np.where(on, 0.0, apq),
            np.where(on, c * arp - s * arq, arp), np.where(on, s * arp + c * arq, arq))


def jacobi_eigenvalues(t6, sweeps=SWEEPS):
    """Cyclic Jacobi as tweb_eigenvalues (tweb.hpp) does it: power-of-two scaling, `sweeps` sweeps over (0,1), (0,2),
    (1,2), a sweep starting only while off(T) > eps |T|_F.  (3, ...) eigenvalues, descending."""
    a00, a01, a02, a11, a12, a22 = (np.array(c, dtype=np.float64) for c in t6)
    m = np.max(np.abs(np.stack([a00, a01, a02, a11, a12, a22])), axis=0)
    e = np.where(m > 0, np.frexp(m)[1], 0)
    a00, a01, a02, a11, a12, a22 = (np.ldexp(c, -e) for c in (a00, a01, a02, a11, a12, a22))
    act = np.ones(a00.shape, dtype=bool)
    for _ in range(sweeps):
        off2 = a01 * a01 + a02 * a02 + a12 * a12
        all2 = a00 * a00 + a11 * a11 + a22 * a22 + 2.0 * off2
        act = act & ~(off2 <= EPS64 ** 2 * all2)
        a00, a11, a01, a02, a12 = _rotate(act, a00, a11, a01, a02, a12)
        a00, a22, a02, a01, a12 = _rotate(act, a00, a22, a02, a01, a12)
        a11, a22, a12, a01, a02 = _rotate(act, a11, a22, a12, a01, a02)
    lam = np.sort(np.stack([a00, a11, a22]), axis=0)[::-1]
    return np.ldexp(lam, e)


def acos_eigenvalues(t6):
    """The closed form through acos (Smith 1961), in float64: what k_tweb_eigen does NOT use.  (3, ...), descending."""
    a00, a01, a02, a11, a12, a22 = (np.asarray(c, dtype=np.float64) for c in t6)
    q = (a00 + a11 + a22) / 3.0
    p1 = a01 * a01 + a02 * a02 + a12 * a12
    p2 = (a00 - q) ** 2 + (a11 - q) ** 2 + (a22 - q) ** 2 + 2.0 * p1
    p = np.sqrt(p2 / 6.0)
    ps = np.where(p > 0, p, 1.0)
    b00, b11, b22, b01, b02, b12 = (a00 - q) / ps, (a11 - q) / ps, (a22 - q) / ps, a01 / ps, a02 / ps, a12 / ps
    det = b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02)
    phi = np.arccos(np.clip(det / 2.0, -1.0, 1.0)) / 3.0
    l1 = q + 2.0 * p * np.cos(phi)
    l3 = q + 2.0 * p * np.cos(phi + 2.0 * np.pi / 3.0)
    return np.stack([l1, 3.0 * q - l1 - l3, l3])


# ---- chosen tensors ---------------------------------------------------------------------------------------------------
def random_rotations(rng, count):
    """`count` proper rotations (count, 3, 3) from QR of Gaussian matrices."""
    q, r = np.linalg.qr(rng.standard_normal((count, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def rotated(diag, rot):
    """rot diag(d) rot^T for each (d, rot): (count, 3) and (count, 3, 3) -> six components (6, count)."""
    m = np.einsum("cij,cj,ckj->cik", rot, np.asarray(diag, dtype=np.float64), rot)
    m = 0.5 * (m + np.swapaxes(m, 1, 2))
    return from_matrices(m)


def degenerate_set(rng, per_kind=64):
    """Tensors with known eigenvalues: (tensors (6, M), eigenvalues (3, M) descending).  (lambda, 0, 0) in general
    position, (lambda, lambda, 0) likewise, lambda I, diagonal tensors, and all of them scaled by 1e+-100."""
    lam = rng.uniform(0.5, 2.0, per_kind) * rng.choice([-1.0, 1.0], per_kind)
    zero = np.zeros(per_kind)
    kinds = [np.stack([lam, zero, zero], 1), np.stack([lam, lam, zero], 1), np.stack([lam, lam, lam], 1)]
    ts, ds = [], []
    for d in kinds:
        ts.append(rotated(d, random_rotations(rng, per_kind)))
        ds.append(d)
    d = rng.standard_normal((per_kind, 3))
    ts.append(from_matrices(np.einsum("cj,jk->cjk", d, np.eye(3))))
    ds.append(d)
    t = np.concatenate(ts, axis=1)
    d = np.concatenate(ds, axis=0)
    t = np.concatenate([t, t * 1e100, t * 1e-100], axis=1)
    d = np.concatenate([d, d * 1e100, d * 1e-100], axis=0)
    return t, np.sort(d, axis=1)[:, ::-1].T.copy()


# ---- the seeded fields of the tests ------------------------------------------------------------------------------------
def box_of(n):
    """L = 50 Mpc/h at n = 16, the same cell size at every n."""
    return 50.0 * n / 16.0


def field(n, seed=7):
    """Standard normals from Philox(seed), (n, n, n)."""
    return np.random.Generator(np.random.Philox(seed)).standard_normal((n, n, n))


def plane_wave(n, axes, m, A=1.0):
    """A cos(2 pi m (sum of the indices of `axes`) / n)."""
    idx = np.indices((n, n, n))
    return A * np.cos(2.0 * np.pi * m * sum(idx[a] for a in axes) / n)


def smooth_field(n, seed=8, cells=2.0):
    """field(n, seed) smoothed with a Gaussian of `cells` cells and scaled to unit standard deviation: a field whose
    norm is not dominated by modes the tensor's own smoothing removes."""
    L = box_of(n)
    xs = tensor(field(n, seed), L, cells * L / n)[1]
    return xs / np.std(xs)


def host_field(n, cells):
    """The host field of the random-field tests: white for R = 0, smooth for R = `cells` cells > 0."""
    return field(n) if cells == 0.0 else smooth_field(n, cells=cells)
