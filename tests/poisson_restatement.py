"""numpy float64 restatement of the Poisson sampler of include/bchmc.h (properties P1-P5 of bchmc_poisson_draw): the
Philox4x32-10 uniforms, the rate, inversion by sequential search below lambda = 10, Hoermann's PTRS from there on, the
scan and the particle positions -- line for line the header's operand order, so that the device's counts are these
except where a decision is closer than the last bits of exp / log / lgamma (the `margin` every count comes with).
"""
import numpy as np
from scipy.special import gammaln

M32 = np.uint64(0xFFFFFFFF)
INV_CAP, PTRS_CAP, LAMBDA_MAX = 256, 64, 2.0 ** 30
TIGHT = 1e-9          # a decision margin below this makes a cell "tight": excluded from a comparison of counts
TIGHT_FRACTION = 1e-4  # at most this share of the cells may be tight


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Salmon et al. 2011, Random123 constants; counters and keys as uint64 arrays holding 32-bit words."""
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & M32, p1 >> s32, p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return c0, c1, c2, c3


def u53(hi, lo):
    """k_white_noise's uniform from two words."""
    return ((((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def uniforms(cells, j, stream, seed):
    cells = np.asarray(cells, dtype=np.uint64)
    seed = int(seed)
    r = philox4x32_10(cells & M32, cells >> np.uint64(32), np.uint64(j), np.uint64(2 * int(stream)),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return u53(r[0], r[1]), u53(r[2], r[3])


def rate(x, scale, rate_mode=0):
    x = np.asarray(x, dtype=np.float64)
    return scale * (1.0 + x) if rate_mode == 0 else scale * x


def _frac_margin(a):
    f = a - np.floor(a)
    return np.minimum(f, 1.0 - f)


def counts(lam, seed, stream=0, window=None):
    """Counts of the cells 0 .. lam.size - 1 at rates `lam` (flattened in cell order).  Returns a dict: counts (int64),
    margin (float64, the smallest decision margin met; inf where nothing was drawn), capped (bool), iters (int, the
    largest number of PTRS iterations any cell took), bad (first index of a refused lambda, or -1)."""
    lam = np.asarray(lam, dtype=np.float64).ravel()
    n = lam.size
    live = np.ones(n, dtype=bool) if window is None else (np.asarray(window).ravel() > 0)
    refused = live & ~(lam <= LAMBDA_MAX)  # NaN, +inf, above 2^30
    bad = int(np.flatnonzero(refused)[0]) if refused.any() else -1
    draw = live & ~refused & (lam > 0)
    out = np.zeros(n, dtype=np.int64)
    margin = np.full(n, np.inf)
    capped = np.zeros(n, dtype=bool)
    iters = 0
    with np.errstate(all="ignore"):
        # ---- inversion by sequential search
        idx = np.flatnonzero(draw & (lam < 10.0))
        if idx.size:
            l = lam[idx]
            u, _ = uniforms(idx, 0, stream, seed)
            p = np.exp(-l)
            s = p.copy()
            k = np.zeros(idx.size, dtype=np.int64)
            mg = np.abs(u - s)
            go = (u > s) & (k < INV_CAP)
            while go.any():
                k[go] += 1
                p[go] = p[go] * l[go] / k[go].astype(np.float64)
                s[go] = s[go] + p[go]
                mg[go] = np.minimum(mg[go], np.abs(u[go] - s[go]))
                go = go & (u > s) & (k < INV_CAP)
            out[idx], margin[idx], capped[idx] = k, mg, k >= INV_CAP
        # ---- PTRS
        idx = np.flatnonzero(draw & (lam >= 10.0))
        if idx.size:
            l = lam[idx]
            b = 0.931 + 2.53 * np.sqrt(l)
            a = -0.059 + 0.02483 * b
            inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
            vr = 0.9277 - 3.6224 / (b - 2.0)
            loglam = np.log(l)
            res = np.zeros(idx.size, dtype=np.int64)
            mg = np.full(idx.size, np.inf)
            act = np.ones(idx.size, dtype=bool)
            for j in range(PTRS_CAP):
                if not act.any():
                    break
                iters = j + 1
                t = np.flatnonzero(act)
                u, v = uniforms(idx[t], j, stream, seed)
                U = u - 0.5
                us = 0.5 - np.abs(U)
                arg = (2.0 * a[t] / us + b[t]) * U + l[t] + 0.43
                kf = np.floor(arg)
                m = np.minimum(_frac_margin(arg), np.abs(us - 0.07))
                fast = (us >= 0.07) & (v <= vr[t])
                m = np.where(us >= 0.07, np.minimum(m, np.abs(v - vr[t])), m)
                slow = ~fast
                m = np.where(slow, np.minimum(m, np.abs(us - 0.013)), m)
                m = np.where(slow & (us < 0.013), np.minimum(m, np.abs(v - us)), m)
                retry = slow & ((kf < 0) | ((us < 0.013) & (v > us)))
                test = slow & ~retry
                lhs = np.log(v) + np.log(inv_alpha[t]) - np.log(a[t] / (us * us) + b[t])
                rhs = -l[t] + kf * loglam[t] - gammaln(kf + 1.0)
                m = np.where(test, np.minimum(m, np.abs(lhs - rhs)), m)
                acc = fast | (test & (lhs <= rhs))
                mg[t] = np.minimum(mg[t], m)
                res[t] = np.where(kf > 0, kf, 0).astype(np.int64)  # the last candidate: what a capped cell returns
                act[t[acc]] = False
            out[idx], margin[idx], capped[idx] = res, mg, act
    return dict(counts=out, margin=margin, capped=capped, iters=iters, bad=bad)


def tight(r):
    """Cells excluded from a comparison of counts, and the assertion that they are few."""
    t = r["margin"] < TIGHT
    assert t.sum() <= TIGHT_FRACTION * t.size, "%d tight cells of %d" % (t.sum(), t.size)
    return t


def offsets(cnt):
    off = np.zeros(cnt.size + 1, dtype=np.uint64)
    np.cumsum(cnt.astype(np.uint64), out=off[1:])
    return off


def positions(cnt, seed, stream, n_in, L, first=0, m=None):
    """Particles first .. first + m - 1 of the sample with counts `cnt` (cell order k + n (j + n i)), upstream's order:
    x = d i + (w.x 2^-32) d and so on, w = philox((c_lo, c_hi, kk, 2 stream + 1), seed)."""
    cnt = np.asarray(cnt, dtype=np.int64).ravel()
    off = offsets(cnt)
    total = int(off[-1])
    m = total - first if m is None else m
    p = np.arange(first, first + m, dtype=np.uint64)
    c = np.searchsorted(off, p, side="right").astype(np.int64) - 1
    kk = p - off[c]
    seed = int(seed)
    cu = c.astype(np.uint64)
    w = philox4x32_10(cu & M32, cu >> np.uint64(32), kk, np.uint64(2 * int(stream) + 1), seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)
    d = L / float(n_in)
    k, ij = c % n_in, c // n_in
    j, i = ij % n_in, ij // n_in
    r32 = 2.0 ** -32
    return tuple(d * idx.astype(np.float64) + (wa.astype(np.float64) * r32) * d for idx, wa in ((i, w[0]), (j, w[1]), (k, w[2])))
