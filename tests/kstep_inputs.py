"""Input sets for the k-space step kernels (tests/test_kstep_bounds.py, tests/test_gpu_kstep.py), all built in k-space.

An input is a dict: n, L, nhp, Ck (3, n, n, nhp), q, p, g_in (n, n, nhp) in the storage type, wS, wM (n, n, nhp) double,
the scalars a, b, half_eps, eps, c_za.  Arrays are indexed [i, j, k].  For the planes kernels Ck is handed over in
planes space (x, ky, kz): the inverse x-DFT (float64, rounded once to T) of the k-space array built here.

- white(): white complex Gaussian data in every array; wS and wM with a dynamic range of 1e12 (10^U(-6, 6)) and zeros at
  DC and in a band of non-DC modes (a spectrum with holes); NaN in every row-padding column k in [nh, nhp) of every array.
- impulse_sets(): everything zero but unit impulses (1 - 0.5 i), one per x-column and so one at a time for kernels that
  treat columns independently: DC, the three Nyquist planes, their edges and the corner, the self-conjugate lines of
  the planes k = 0 and k = n / 2, (1,0,0), (0,1,0), (0,0,1), (n/2 -+ 1, ., .), k = nh - 2, the first and the last lane
  of the first and the last k-group.  Positions that share a column go to different layers; within a layer position t
  carries its impulse in field (t + rot) mod 5 of V^_x, V^_y, V^_z, q^, p^, so the five rotations of a layer put every
  field at every position.  Smooth positive wS, wM.
- variants(): the white set with a = 0 (no prior), b = 0, wM absent, eps < 0 (the reversed trajectory).
- corr_grid(): for k_prepare_mult, a full n^3 grid that depends on i, j and k separately, with zeros and negative entries.

The box length is 1.25 n, so that kfac is not 2 pi / n.
"""
import numpy as np

from tests.kstep_reference import BX_FIRST, BX_INTERIOR, BX_LAST, kval

FIELDS = ("Vx", "Vy", "Vz", "q", "p")
IMPULSE = 1.0 - 0.5j


def types(prec):
    return {"fp64": (np.float64, np.complex128), "fp32": (np.float32, np.complex64)}[prec]


def pass_kb(rdt):
    return 128 // (2 * np.dtype(rdt).itemsize)


def row_stride(n, rdt, pad=None):
    """fft_row_stride: n / 2 + 1, padded to whole 128-byte lines for n >= 128 (or when forced)."""
    nh, per = n // 2 + 1, pass_kb(rdt)
    if pad is None:
        pad = n >= 128
    return (nh + per - 1) // per * per if pad else nh


def box(n):
    return 1.25 * n


def ksq_grid(n, nhp, L):
    kv = kval(n, L, max(n, nhp))
    return kv[:n, None, None] ** 2 + kv[None, :n, None] ** 2 + kv[None, None, :nhp] ** 2


def to_planes(vk, cdt):
    """k-space (.., n, n, nhp) -> planes space: inverse x-DFT, normalised so that the kernel's forward pass returns vk."""
    with np.errstate(invalid="ignore"):
        return np.fft.ifft(vk.astype(np.complex128), axis=-3).astype(cdt)


def scalars(n):
    return dict(a=0.7, b=1.3, half_eps=0.05, eps=0.1, c_za=-0.83 / float(n) ** 3)


def empty(n, prec, pad=None):
    rdt, cdt = types(prec)
    nhp = row_stride(n, rdt, pad)
    L = box(n)
    z = lambda *s: np.zeros(s + (n, n, nhp), cdt)  # noqa: E731
    smooth = 1.0 / (1.0 + ksq_grid(n, nhp, L))
    d = dict(n=n, L=L, nhp=nhp, prec=prec, Ck=z(3), q=z(), p=z(), g_in=z(), wS=smooth.copy(), wM=0.5 * smooth + 0.1)
    d.update(scalars(n))
    return d


def white(n, prec, seed=1, pad=None, planes=True):
    rdt, cdt = types(prec)
    d = empty(n, prec, pad)
    nhp, nh = d["nhp"], n // 2 + 1
    rng = np.random.default_rng(seed + 1000 * n)

    def w(*s):
        return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(cdt)

    d["Ck"], d["q"], d["p"], d["g_in"] = w(3, n, n, nhp), w(n, n, nhp), w(n, n, nhp), w(n, n, nhp)
    ks = ksq_grid(n, nhp, d["L"])
    kmax = ks[:, :, :nh].max()
    for name in ("wS", "wM"):
        wt = 10.0 ** rng.uniform(-6, 6, (n, n, nhp))
        wt[(ks > 0.09 * kmax) & (ks < 0.16 * kmax)] = 0.0
        wt[0, 0, 0] = 0.0
        d[name] = wt
    if planes:
        d["Ck"] = to_planes(d["Ck"], cdt)
    for name in ("Ck", "q", "p", "g_in", "wS", "wM"):
        d[name][..., nh:] = np.nan
    return d


def positions(n, nhp, rdt):
    h, nh, kb = n // 2, n // 2 + 1, pass_kb(rdt)
    kl0 = (nhp // kb - 1) * kb if nhp % kb == 0 and nhp >= kb else 0
    kl0 = min(kl0, nh - 1)
    pos = [(0, 0, 0),
           (h, 1, 2), (1, h, 2), (1, 2, h), (h, h, 1), (h, 1, h), (1, h, h), (h, h, h),
           (h, 0, 0), (0, h, 0), (0, 0, h), (h, h, 0), (h, 0, h), (0, h, h), (3, n - 3, 0), (3, n - 3, h),
           (1, 0, 0), (0, 1, 0), (0, 0, 1),
           (h - 1, 2, 3), (h + 1, 3, 2), (2, h - 1, 3), (2, h + 1, 1), (2, 3, h - 1),
           (1, 1, nh - 2),
           (3, 5, 0), (3, 5, min(kb - 1, nh - 1)), (n - 1, 5, kl0), (3, n - 1, nh - 1)]
    seen, out = set(), []
    for p_ in pos:
        p_ = tuple(int(x) % n for x in p_[:2]) + (int(p_[2]),)
        if p_ not in seen and p_[2] < nh:
            seen.add(p_)
            out.append(p_)
    return out


def layers(n, nhp, rdt):
    """The positions dealt into layers with no x-column (j, k) used twice."""
    ls = []
    for p_ in positions(n, nhp, rdt):
        for layer in ls:
            if all((p_[1], p_[2]) != (o[1], o[2]) for o in layer):
                layer.append(p_)
                break
        else:
            ls.append([p_])
    return ls


def impulse_sets(n, prec, pad=None, planes=True, max_layers=None, rots=range(5)):
    """Yields (name, input)."""
    rdt, cdt = types(prec)
    nhp = row_stride(n, rdt, pad)
    for li, layer in enumerate(layers(n, nhp, rdt)[:max_layers]):
        for rot in rots:
            d = empty(n, prec, pad)
            for t, (i, j, k) in enumerate(layer):
                f = FIELDS[(t + rot) % 5]
                if f[0] == "V":
                    d["Ck"]["xyz".index(f[1]), i, j, k] = IMPULSE
                else:
                    d[f][i, j, k] = IMPULSE
            if planes:
                d["Ck"] = to_planes(d["Ck"], cdt)
            yield "impulses layer %d rot %d" % (li, rot), d


def variants(n, prec, pad=None, planes=True):
    """Yields (name, input): the white set with one thing changed."""
    for name, ch in (("a=0", dict(a=0.0)), ("b=0", dict(b=0.0)), ("no wM", dict(wM=None)),
                     ("eps<0", dict(eps=-0.1, half_eps=-0.05))):
        d = white(n, prec, seed=2, pad=pad, planes=planes)
        d.update(ch)
        yield name, d


def corr_grid(n, seed=5):
    """Full (n, n, n) grid for k_prepare_mult: a different dependence on each index, zeros and negative entries."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)[:, None, None]
    j = np.arange(n)[None, :, None]
    k = np.arange(n)[None, None, :]
    c = (1.0 + i) * (3.0 + 2.0 * j) ** 2 / (0.5 + k) + rng.uniform(0, 1e-3, (n, n, n))
    c[rng.uniform(size=c.shape) < 0.1] = 0.0
    c[rng.uniform(size=c.shape) < 0.1] *= -1.0
    c[0, 0, 0] = 0.0
    return c


def mode_name(at):
    return "(" + ",".join(str(x) for x in at) + ")"


# ---- what the CPU and the GPU test share ---------------------------------------------------------------------------------

def with_(inp, ch):
    d = dict(inp)
    d.update(ch)
    return d


# the uses of k_step_boundary_x the engine has: name -> (MODE, ALPT, what the use leaves out)
MODES = {"interior": (BX_INTERIOR, False, {}), "interior_alpt": (BX_INTERIOR, True, {}),
         "first": (BX_FIRST, False, {}), "first_za_only": (BX_FIRST, False, dict(g_in=None, p=None)),
         "first_alpt": (BX_FIRST, True, {}), "last": (BX_LAST, False, {}), "last_g_only": (BX_LAST, False, dict(p=None))}


def planes_sets(n, prec, layers=None, rots=5, with_variants=True):
    """Yields (name, input) for the planes kernels (rows padded): white, `layers` layers of impulses (None: all) in
    `rots` rotations of the fields, the variants."""
    yield "white", white(n, prec, pad=True)
    yield from impulse_sets(n, prec, pad=True, max_layers=layers, rots=range(rots))
    if with_variants:
        yield from variants(n, prec, pad=True)


def twin_sets(n, prec, pad=None, layers=None):
    """Yields (name, input) for the 3-D twins (everything in k-space)."""
    yield "white", white(n, prec, pad=pad, planes=False)
    yield from impulse_sets(n, prec, pad=pad, planes=False, max_layers=layers)
    yield from variants(n, prec, pad=pad, planes=False)


def alpt_inputs(inp):
    """The scalars of the ALPT mix on top of an input."""
    n = inp["n"]
    return with_(inp, dict(smol=1.7 * box(n) / n, inv_wtot=1.0 / 0.93, inv_n=1.0 / float(n) ** 3))
