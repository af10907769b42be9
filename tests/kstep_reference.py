"""High-precision reference of the k-space step kernels (tests/test_kstep_bounds.py and tests/test_gpu_kstep.py judge the
numpy restatement and the HIP kernels against it, at the bound of tests/kstep_bound.py).

Written from the upstream formulas the kernel headers quote, not from the kernels:

    g^ = a wS q^ + b h^,  h^ = sum_j (k_j / k^2) (Im V^_j, -Re V^_j), 0 at k = 0 and where the Nyquist rule hits
                                                                        (gradient.cpp:167-210, HMC.cc:170-173, 205)
    p_end = p - (eps/2) g^;  guard = sum_k hw_k Re p_end;  p' = p_end - (eps/2) g^;  q' = q + eps wM p'   (HMC.cc:290-352)
    Psi^_j = (k_j / k^2) (Im phi^, -Re phi^), phi^ = c_za q^', 0 for k^2 <= 1e-14 and where the Nyquist rule hits
                                                                        (EqSolvers.cc:208-268)
    delta(1)^ = c q^,  Phi^ = -delta(1)^ / k^2 (0 at k = 0, no Nyquist rule)               (EqSolvers.cc:29-64)
    Psi^_j = P (k_j / (N k^2)) (Im M, -Re M),  M = K A^ + B^ - K B^,  K = exp(-k^2 kth^2 / 2) / wtot
                                                                        (EqSolvers.cc:280-368, convolution.cpp:327-377)
    P = (1 + exp(-2 pi i (i + j + k) / n)) / 2, the cell-boundary average of massFunctions.cc:588-658 by the shift theorem.

(Im z, -Re z) is -i z.  Every function starts from the inputs as they are stored in the kernel's type T and works in the
type `wdt` (np.longdouble; np.float64 for the whole-array pass at n = 256), with no rounding to T anywhere: the
roundings the kernels make on purpose (W = ky V_y + kz V_z, p_end, g^, the stored q') are u_T terms of the bound.  The
wave numbers are the kernels' own doubles (calc_ki: kfac i for i <= n / 2, -kfac (n - i) above, kfac = 2 pi / L), taken
as inputs.

The planes kernels are the composition  x-DFT -> element-wise map -> inverse x-DFT  with np.fft along axis 0.  Arrays
are indexed [i, j, k]; a function looks at the columns k < nh only, or at the columns `cols` it is given (pairs (j, k)),
and returns, beside the outputs, the intermediates the bound is built from.
"""
import numpy as np

BX_INTERIOR, BX_FIRST, BX_LAST = 0, 1, 2


def cdt_of(wdt):
    return np.clongdouble if np.dtype(wdt) == np.dtype(np.longdouble) else np.complex128


def kval(n, L, count=None):
    """calc_ki as the kernels evaluate it, in double, for indices 0 .. count - 1."""
    kfac = 2.0 * np.pi / float(L)
    i = np.arange(n if count is None else count)
    return np.where(i <= n // 2, kfac * i.astype(np.float64), -kfac * (n - i).astype(np.float64))


def nyq_keep(n, nk):
    """The weight of the Nyquist rule on (i, j, k < nk): 0 where i, j or k is n / 2 (integer division); at odd n, in the
    plane k = 0, the mean of that and the same for the conjugate partner (common.hpp, nyq_keep)."""
    h = n // 2
    i = np.arange(n)[:, None, None]
    j = np.arange(n)[None, :, None]
    k = np.arange(nk)[None, None, :]
    own = np.where((i == h) | (j == h) | (k == h), 0.0, 1.0)
    if n % 2 == 0:
        return own
    ic, jc = (n - i) % n, (n - j) % n
    partner = np.where((ic == h) | (jc == h), 0.0, 1.0) + 0 * k
    return np.where(k == 0, 0.5 * (own + partner), own)


def half_weight(n, nk):
    k = np.arange(nk)
    return np.where((k == 0) | ((n % 2 == 0) & (k == n // 2)), 1.0, 2.0)


class Geom:
    """Wave numbers of the columns looked at.  cols: None = every (j, k < nh), arrays come back as (n, n, nh); or a list
    of (j, k) pairs, arrays come back as (n, len(cols))."""

    def __init__(self, n, L, wdt, cols=None):
        self.n, self.L, self.wdt, self.cols = n, L, wdt, cols
        self.nh = n // 2 + 1
        kv = kval(n, L, max(n, 2 * n))  # k beyond n / 2 + 1 (row padding) is evaluated by the same rule
        if cols is None:
            self.kx = kv[:n, None, None].astype(wdt)
            self.ky = kv[None, :n, None].astype(wdt)
            self.kz = kv[None, None, :self.nh].astype(wdt)
            i = np.arange(n)[:, None, None]
            j = np.arange(n)[None, :, None]
            k = np.arange(self.nh)[None, None, :]
        else:
            jj = np.array([c[0] for c in cols])
            kk = np.array([c[1] for c in cols])
            self.kx = kv[:n, None].astype(wdt)
            self.ky = kv[jj][None, :].astype(wdt)
            self.kz = kv[kk][None, :].astype(wdt)
            i = np.arange(n)[:, None]
            j, k = jj[None, :], kk[None, :]
        self.i, self.j, self.k = i, j, k
        self.ksq = self.kx * self.kx + self.ky * self.ky + self.kz * self.kz
        self.nyq = (i == n // 2) | (j == n // 2) | (k == n // 2)
        self.hw = np.where((k == 0) | ((n % 2 == 0) & (k == n // 2)), 1.0, 2.0).astype(wdt)
        self.counted = k < self.nh  # columns that enter a reduction

    def take(self, a, cplx=True):
        """The columns looked at of a stored array (n, n, nhp), in the working type."""
        if a is None:
            return None
        t = cdt_of(self.wdt) if cplx else self.wdt
        if self.cols is None:
            return a[:, :, :self.nh].astype(t)
        jj = [c[0] for c in self.cols]
        kk = [c[1] for c in self.cols]
        return a[:, jj, kk].astype(t)


def safe_inv(x, mask):
    """1 / x where mask, 0 elsewhere."""
    return np.where(mask, 1 / np.where(mask, x, 1), 0)


def fwd(a):
    return np.fft.fft(a, axis=0)


def inv(a):
    return np.fft.ifft(a, axis=0, norm="forward")  # unnormalised, as the kernels' inverse pass


def planes_step(inp, mode, alpt, wdt=np.longdouble, cols=None):
    """k_step_boundary_x<MODE, ALPT> and k_step_boundary_x2.  inp: n, L, Ck (3, n, n, nhp), q, p, g_in, wS, wM (arrays or
    None), a, b, half_eps, eps, c_za.  Returns a dict of the reference outputs (Ck0 .. Ck2, q_out, p_out, g_out, guard;
    only those the mode writes) and of intermediates (names with a leading underscore)."""
    n = inp["n"]
    G = Geom(n, inp["L"], wdt, cols)
    a, b, he, eps, cza = (wdt(inp[s]) for s in ("a", "b", "half_eps", "eps", "c_za"))
    q = G.take(inp["q"])
    r = {"_G": G, "_q": q}
    kicked = False
    if mode != BX_FIRST:
        vx, vy, vz = (G.take(inp["Ck"][c]) for c in range(3))
        W = G.ky * vy + G.kz * vz
        vxh, wh = fwd(vx), fwd(W)
        hk = -1j * (G.kx * vxh + wh)
        f = b * safe_inv(G.ksq, (G.ksq > 0) & ~G.nyq)
        gg = f * hk
        prior = 0 * gg
        if inp["a"] != 0.0:
            prior = a * G.take(inp["wS"], False) * q
            gg = gg + prior
        r.update(_Wabs=np.abs(G.ky) * np.abs(vy) + np.abs(G.kz) * np.abs(vz), _vxh=vxh, _wh=wh, _f=f, _prior=prior, _gg=gg)
        r["g_out" if mode == BX_LAST else "_gs"] = gg
        if mode == BX_LAST and inp["p"] is None:
            return r
        p = G.take(inp["p"])
        pe = p - he * gg
        r.update(_p=p, _pe=pe, guard=np.sum(np.where(G.counted, G.hw * pe.real, 0)))
        if mode == BX_LAST:
            r["p_out"] = pe
            return r
        pp = pe - he * gg
        kicked = True
    elif inp["g_in"] is not None:
        p, g0 = G.take(inp["p"]), G.take(inp["g_in"])
        pp = p - he * g0
        r.update(_p=p, _g0=g0)
        kicked = True
    qq = q
    if kicked:
        r["p_out"] = pp
        if inp["wM"] is not None:
            ew = eps * G.take(inp["wM"], False)
            drift = ew * pp
            qq = q + drift
            r.update(_drift=drift, _ew=ew)
        r["q_out"] = qq
    r["_kicked"] = kicked
    if alpt:
        m1 = cza + 0 * G.ksq
        m2 = -cza * safe_inv(G.ksq, G.ksq > 0)
    else:
        ok = (G.ksq > 1e-14) & ~G.nyq
        m2 = -1j * cza * safe_inv(G.ksq, ok)
        m1 = m2 * G.kx
    o1, o2 = m1 * qq, m2 * qq
    X, B = inv(o1), inv(o2)
    r.update(_m1=m1, _m2=m2, _o1=o1, _o2=o2, _B=B, Ck0=X)
    if alpt:
        r["Ck1"] = B
    else:
        r["Ck1"], r["Ck2"] = G.ky * B, G.kz * B
    return r


def cell_phase(G, n, wdt):
    """P = (1 + exp(-2 pi i r / n)) / 2, r = (i + j + k) mod n, with the angle reduced exactly."""
    rr = (G.i + G.j + G.k) % n
    t = 2 * rr.astype(wdt) / wdt(n)
    pi = np.arctan(wdt(1)) * 4
    return 0.5 * (1 + np.cos(pi * t) - 1j * np.sin(pi * t))


def alpt_mix(inp, planes, wdt=np.longdouble, cols=None):
    """k_alpt_mix_x (planes: Ck in planes space, the plain Nyquist rule) and k_alpt_mix (Ck in k-space, nyq_keep).
    inp: n, L, Ck (3, n, n, nhp; components 0 and 1 read), smol, inv_wtot, inv_n."""
    n = inp["n"]
    G = Geom(n, inp["L"], wdt, cols)
    A, Bc = G.take(inp["Ck"][0]), G.take(inp["Ck"][1])
    if planes:
        A, Bc = fwd(A), fwd(Bc)
        keep = np.where(G.nyq, 0.0, 1.0).astype(wdt)
    else:
        assert cols is None
        keep = nyq_keep(n, G.nh).astype(wdt)
    ok = (G.ksq > 1e-14) & (keep != 0)
    arg = -G.ksq * wdt(inp["smol"]) * wdt(inp["smol"]) / 2
    K = np.exp(arg) * wdt(inp["inv_wtot"])
    M = K * A + Bc - K * Bc
    fac = keep * wdt(inp["inv_n"]) * safe_inv(G.ksq, ok)
    P = cell_phase(G, n, wdt)
    E = fac * (-1j * M) * P
    r = {"_G": G, "_A": A, "_B": Bc, "_K": K, "_arg": arg, "_M": M, "_fac": fac, "_E": E, "_ok": ok}
    if planes:
        Ei = inv(E)
        r.update(_Ei=Ei, Ck0=inv(G.kx * E), Ck1=G.ky * Ei, Ck2=G.kz * Ei)
    else:
        r.update(Ck0=G.kx * E, Ck1=G.ky * E, Ck2=G.kz * E)
    return r


# ---- the 3-D twins: everything in k-space, element-wise ---------------------------------------------------------------

def za_displacement(G, n, qq, cza, wdt):
    keep = nyq_keep(n, G.nh).astype(wdt)
    ok = (G.ksq > 1e-14) & (keep != 0)
    mz = -1j * cza * keep * safe_inv(G.ksq, ok)
    B = mz * qq
    return G.kx * B, G.ky * B, G.kz * B, mz


def kick_drift_za(inp, drift, wdt=np.longdouble):
    """k_kick_drift_za<DRIFT>: inp n, L, q, p, g_in, wM, extra, half_eps, eps, c_za."""
    n = inp["n"]
    G = Geom(n, inp["L"], wdt)
    q = G.take(inp["q"])
    r = {"_G": G, "_q": q}
    qq = q
    if drift:
        p, g0 = G.take(inp["p"]), G.take(inp["g_in"])
        pp = p - wdt(inp["half_eps"]) * g0
        v = 0 * pp
        terms = []
        if inp["wM"] is not None:
            terms.append(G.take(inp["wM"], False) * pp)
        if inp.get("extra") is not None:
            terms.append(G.take(inp["extra"]))
        for t in terms:
            v = v + t
        qq = q + wdt(inp["eps"]) * v
        r.update(_p=p, _g0=g0, _vabs=sum((np.abs(t) for t in terms), 0 * np.abs(pp)), p_out=pp, q_out=qq)
    r["Ck0"], r["Ck1"], r["Ck2"], r["_mz"] = za_displacement(G, n, qq, wdt(inp["c_za"]), wdt)
    return r


def assemble_g(inp, G, q, like_mode, wdt):
    n = inp["n"]
    a, b = wdt(inp["a"]), wdt(inp["b"])
    habs = 0
    if like_mode == 0:
        keep = nyq_keep(n, G.nh).astype(wdt)
        f = keep * safe_inv(G.ksq, (G.ksq > 0) & (keep != 0))
        vx, vy, vz = (G.take(inp["Ck"][c]) for c in range(3))
        hk = -1j * f * (G.kx * vx + G.ky * vy + G.kz * vz)
        habs = np.abs(f) * (np.abs(G.kx * vx) + np.abs(G.ky * vy) + np.abs(G.kz * vz))
    elif like_mode == 1:
        hk = G.take(inp["Ck"][0])
        habs = np.abs(hk)
    else:
        hk = 0 * q
    gg = b * hk
    gabs = np.abs(b) * habs
    if inp["a"] != 0.0:
        prior = a * G.take(inp["wS"], False) * q
        gg = gg + prior
        gabs = gabs + np.abs(prior)
    return gg, gabs


def assemble(inp, kick, like_mode, wdt=np.longdouble):
    """k_assemble<KICK>: g^ and, with KICK, p -= c_kick g^ and the guard sum of the new p."""
    G = Geom(inp["n"], inp["L"], wdt)
    q = G.take(inp["q"]) if inp["a"] != 0.0 else 0 * G.take(inp["Ck"][0])
    gg, gabs = assemble_g(inp, G, q, like_mode, wdt)
    r = {"_G": G, "g_out": gg, "_gabs": gabs}
    if kick:
        p = G.take(inp["p"])
        pe = p - wdt(inp["c_kick"]) * gg
        r.update(_p=p, p_out=pe, guard=np.sum(G.hw * pe.real))
    return r


def step_boundary(inp, last, like_mode, wdt=np.longdouble):
    """k_step_boundary<LAST>."""
    n = inp["n"]
    G = Geom(n, inp["L"], wdt)
    he, eps = wdt(inp["half_eps"]), wdt(inp["eps"])
    q, p = G.take(inp["q"]), G.take(inp["p"])
    gg, gabs = assemble_g(inp, G, q, like_mode, wdt)
    pe = p - he * gg
    r = {"_G": G, "_q": q, "_p": p, "_gg": gg, "_gabs": gabs, "_pe": pe, "guard": np.sum(G.hw * pe.real)}
    if last:
        r.update(p_out=pe, g_out=gg)
        return r
    pp = pe - he * gg
    qq = q
    if inp["wM"] is not None:
        r["_ew"] = eps * G.take(inp["wM"], False)
        r["_drift"] = r["_ew"] * pp
        qq = q + r["_drift"]
    r.update(p_out=pp, q_out=qq)
    r["Ck0"], r["Ck1"], r["Ck2"], r["_mz"] = za_displacement(G, n, qq, wdt(inp["c_za"]), wdt)
    return r


def alpt_poisson(inp, wdt=np.longdouble):
    """k_alpt_poisson: inp n, L, q, scale."""
    G = Geom(inp["n"], inp["L"], wdt)
    d1 = wdt(inp["scale"]) * G.take(inp["q"])
    return {"_G": G, "d1": d1, "phi": -safe_inv(G.ksq, G.ksq > 0) * d1}


def prepare_mult(corr, n, normFS, wdt=np.longdouble):
    """k_prepare_mult: corr a full (n, n, n) grid read at (i, j, k <= n / 2); normFS / corr where corr > 0, else 0."""
    c = corr[:, :, :n // 2 + 1].astype(wdt)
    return np.where(c > 0, wdt(normFS) / np.where(c > 0, c, 1), 0)


def parseval(x, w, n, wdt=np.longdouble):
    """k_parseval: sum over k < nh of hw w |x|^2; returns the sum and the sum of the absolute terms."""
    nh = n // 2 + 1
    xs = x[:, :, :nh].astype(cdt_of(wdt))
    t = half_weight(n, nh).astype(wdt) * w[:, :, :nh].astype(wdt) * (xs.real ** 2 + xs.imag ** 2)
    return np.sum(t), np.sum(np.abs(t))


def rollback(s, q0, p0, q1, p1, wdt=np.longdouble):
    """k_rollback with the guard tripped at step s >= 1: boundary s - 1 read pair (s - 1) % 2 and wrote the other;
    the state is (q_read, (p_read + p_written) / 2)."""
    c = cdt_of(wdt)
    qr, pr, pw = (q0, p0, p1) if (s - 1) % 2 == 0 else (q1, p1, p0)
    return qr.astype(c), (pr.astype(c) + pw.astype(c)) / 2
