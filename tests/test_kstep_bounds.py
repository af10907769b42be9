"""The bound of tests/kstep_bound.py on the CPU: achievable, measured, and able to fail.

Every k-space step kernel is restated here in numpy, operation by operation: arrays stored in float32 / float64, the
element-wise arithmetic in float64, the x passes through the radix-4 xfft_inplace restatement of
tests/test_fft_pass_bounds.py in the storage type, every rounding where the kernel has one, the row padding processed
like data (NaN in, whatever comes out).  No fused multiply-adds and sums in index order: that difference to the GPU is
what the margin of 4 in the constants is for.

(a) The restatements meet the bound at C = 1 against the longdouble reference on every input set; the worst fraction
    per kernel family, type and output is the figure kstep_bound.MEASURED records, asserted here.
(b) The same checker rejects each mutant of MUTANTS by more than 1e3 on at least one set.
(c) The control path of the restatement is the one the GPU test asserts: NaN in guard_prev does not trip the guard.
"""
import numpy as np
import pytest

from tests import kstep_bound as kb
from tests import kstep_inputs as ki
from tests import kstep_reference as ref
from tests.kstep_reference import BX_FIRST, BX_INTERIOR, BX_LAST
from tests.test_fft_pass_bounds import twiddles, xfft

F8 = np.float64


def split(z):
    return z.real.astype(F8), z.imag.astype(F8)


def join(re, im, cdt):
    out = np.empty(re.shape, cdt)
    out.real, out.imag = re, im
    return out


def fft_cols(z, inverse, rdt):
    """xfft_inplace over every x-column of a stored array (n, n, nhp)."""
    n = z.shape[0]
    re, im = xfft(z.real.reshape(n, -1), z.imag.reshape(n, -1), inverse, rdt)
    return join(re.reshape(z.shape), im.reshape(z.shape), z.dtype)


def geo(inp):
    n, nhp = inp["n"], inp["nhp"]
    kv = ref.kval(n, inp["L"], max(n, nhp))
    kx, ky, kz = kv[:n, None, None], kv[None, :n, None], kv[None, None, :nhp]
    i, j, k = np.arange(n)[:, None, None], np.arange(n)[None, :, None], np.arange(nhp)[None, None, :]
    nyq = (i == n // 2) | (j == n // 2) | (k == n // 2)
    return kx, ky, kz, kx * kx + ky * ky + kz * kz, nyq, (i, j, k)


def guard_sum(pe_re, n, nhp, mut):
    k = np.arange(nhp)
    hw = np.where((k == 0) | ((n % 2 == 0) & (k == n // 2)), 1.0, 2.0)
    if mut == "hw2_at_nyquist":
        hw = np.where(k == 0, 1.0, 2.0)
    upto = nhp if mut == "padding_counted" else n // 2 + 1
    return float(np.sum((hw * pe_re.astype(F8))[:, :, :upto]))


def restate_planes(inp, mode, alpt, mut=None):
    """k_step_boundary_x<T, NT, PER, MODE, ALPT> (k_step_boundary_x2: the same arithmetic).  Returns the outputs by name."""
    rdt, cdt = ki.types(inp["prec"])
    n, nhp = inp["n"], inp["nhp"]
    a, b, he, eps, cza = (inp[s] for s in ("a", "b", "half_eps", "eps", "c_za"))
    kx, ky, kz, ksq, nyq, (i, j, k) = geo(inp)
    out = {}
    qx, qy = split(inp["q"])
    kicked = False
    with np.errstate(all="ignore"):
        if mode != BX_FIRST:
            vx, vy, vz = inp["Ck"]
            vyx, vyy = split(vy)
            vzx, vzy = split(vz)
            if mut == "kz_term_dropped":
                W = join((ky * vyx + 0 * vzx).astype(rdt), (ky * vyy + 0 * vzy).astype(rdt), cdt)
            else:
                W = join((ky * vyx + kz * vzx).astype(rdt), (ky * vyy + kz * vzy).astype(rdt), cdt)
            vxh, wh = fft_cols(vx, False, rdt), fft_cols(W, False, rdt)
            vr, vi = split(vxh)
            wr, wi = split(wh)
            hx = kx * vi + wi
            hy = -(kx * vr) - wr
            if mut == "rotation_sign":
                hx, hy = -hx, -hy
            live = (ksq > 0) & ~nyq
            f = b * (1 / np.where(ksq > 0, ksq, 1))
            gx, gy = np.where(live, f * hx, 0.0), np.where(live, f * hy, 0.0)
            if a != 0.0:
                ws = inp["wS"]
                if mut == "wS_index_nh":
                    nh = n // 2 + 1
                    flat = np.concatenate([ws.reshape(-1), np.zeros(n * n * nhp)])
                    ws = flat[(k + nh * (j + n * i)).reshape(-1)].reshape(n, n, nhp)
                w = a * ws
                if mut == "prior_dropped_on_nyquist":
                    w = np.where(nyq, 0.0, w)
                gx, gy = gx + w * qx, gy + w * qy
            gsx, gsy = gx.astype(rdt), gy.astype(rdt)
            if mode == BX_LAST:
                out["g_out"] = join(gsx, gsy, cdt)
                if inp["p"] is None:
                    return out
            px, py = split(inp["p"])
            pex, pey = (px - he * gx).astype(rdt), (py - he * gy).astype(rdt)
            out["guard"] = guard_sum(pex, n, nhp, mut)
            if mode == BX_LAST:
                out["p_out"] = join(pex, pey, cdt)
                return out
            ppx, ppy = pex.astype(F8) - he * gsx.astype(F8), pey.astype(F8) - he * gsy.astype(F8)
            kicked = True
            dpx, dpy = (pex.astype(F8), pey.astype(F8)) if mut == "drift_before_second_kick" else (ppx, ppy)
        elif inp["g_in"] is not None:
            px, py = split(inp["p"])
            g0x, g0y = split(inp["g_in"])
            ppx, ppy = px - he * g0x, py - he * g0y
            dpx, dpy = ppx, ppy
            kicked = True
        if kicked:
            out["p_out"] = join(ppx.astype(rdt), ppy.astype(rdt), cdt)
            if inp["wM"] is not None:
                qx, qy = qx + eps * (inp["wM"] * dpx), qy + eps * (inp["wM"] * dpy)
            out["q_out"] = join(qx.astype(rdt), qy.astype(rdt), cdt)
        qsx, qsy = qx.astype(rdt).astype(F8), qy.astype(rdt).astype(F8)
        inv_ksq = 1.0 / np.where(ksq > 0, ksq, 1)
        if alpt:
            o1 = join((cza * qx).astype(rdt), (cza * qy).astype(rdt), cdt)
            f2 = np.where(ksq > 0, -inv_ksq, 0.0)
            o2 = join((f2 * (cza * qsx)).astype(rdt), (f2 * (cza * qsy)).astype(rdt), cdt)
        else:
            ok = (ksq > 1e-14) if mut == "psi_kept_on_nyquist" else (ksq > 1e-14) & ~nyq
            f1 = inv_ksq * kx
            o1 = join(np.where(ok, f1 * (cza * qy), 0.0).astype(rdt), np.where(ok, f1 * -(cza * qx), 0.0).astype(rdt), cdt)
            o2 = join(np.where(ok, inv_ksq * (cza * qsy), 0.0).astype(rdt),
                      np.where(ok, inv_ksq * -(cza * qsx), 0.0).astype(rdt), cdt)
        out["Ck0"] = fft_cols(o1, True, rdt)
        B = fft_cols(o2, True, rdt)
        if alpt:
            out["Ck1"] = B
        else:
            bx, by = split(B)
            k1, k2 = (kz, ky) if mut == "ky_kz_swapped" else (ky, kz)
            out["Ck1"] = join((k1 * bx).astype(rdt), (k1 * by).astype(rdt), cdt)
            out["Ck2"] = join((k2 * bx).astype(rdt), (k2 * by).astype(rdt), cdt)
    return out


def restate_alpt_mix(inp, planes, mut=None):
    """k_alpt_mix_x (planes) and k_alpt_mix."""
    rdt, cdt = ki.types(inp["prec"])
    n, nhp = inp["n"], inp["nhp"]
    kx, ky, kz, ksq, nyq, (i, j, k) = geo(inp)
    with np.errstate(all="ignore"):
        A, Bc = inp["Ck"][0], inp["Ck"][1]
        if planes:
            A, Bc = fft_cols(A, False, rdt), fft_cols(Bc, False, rdt)
            keep = np.where(nyq, 0.0, 1.0)
        else:
            keep = np.zeros((n, n, nhp))
            nh = n // 2 + 1
            keep[:, :, :nh] = ref.nyq_keep(n, nh)
            if mut == "plain_mask_at_odd_n":
                keep = np.where(nyq, 0.0, 1.0)
        ax, ay = split(A)
        bx, by = split(Bc)
        ok = (ksq > 1e-14) & (keep != 0)
        K = np.exp(-ksq * inp["smol"] * inp["smol"] / 2.0) * inp["inv_wtot"]
        if mut == "KB_not_subtracted":
            mr, mi = K * ax + bx, K * ay + by
        else:
            mr, mi = (K * ax + bx) - K * bx, (K * ay + by) - K * by
        fac = keep * inp["inv_n"] / np.where(ksq > 0, ksq, 1)
        ex, ey = fac * mi, fac * -mr
        r = (i + j + k) % n
        if planes:
            twr, twi = twiddles(n, rdt)
            sg = np.where(r >= n // 2, -1.0, 1.0)
            if mut == "phase_sign_flip_missing":
                sg = 1.0
            idx = r & (n // 2 - 1)
            pr, pi = 0.5 * (1.0 + sg * twr[idx].astype(F8)), 0.5 * (sg * twi[idx].astype(F8))
        else:
            ang = -2.0 * np.pi * ((i + j + k) % n) / n
            pr, pi = 0.5 * (1.0 + np.cos(ang)), 0.5 * np.sin(ang)
        er, ei = np.where(ok, ex * pr - ey * pi, 0.0), np.where(ok, ex * pi + ey * pr, 0.0)
        if not planes:
            return {"Ck%d" % c: join((kk * er).astype(rdt), (kk * ei).astype(rdt), cdt) for c, kk in enumerate((kx, ky, kz))}
        o1 = join((kx * er).astype(rdt), (kx * ei).astype(rdt), cdt)
        o2 = join(er.astype(rdt), ei.astype(rdt), cdt)
        X, E = fft_cols(o1, True, rdt), fft_cols(o2, True, rdt)
        vx, vy = split(E)
        return {"Ck0": X, "Ck1": join((ky * vx).astype(rdt), (ky * vy).astype(rdt), cdt),
                "Ck2": join((kz * vx).astype(rdt), (kz * vy).astype(rdt), cdt)}


def keep_grid(inp, mut=None):
    n, nhp = inp["n"], inp["nhp"]
    nyq = geo(inp)[4]
    if mut == "plain_mask_at_odd_n":
        return np.where(nyq, 0.0, 1.0)
    keep = np.zeros((n, n, nhp))
    keep[:, :, :n // 2 + 1] = ref.nyq_keep(n, n // 2 + 1)
    return keep


def za_out(inp, qx, qy, out, mut=None):
    rdt, cdt = ki.types(inp["prec"])
    kx, ky, kz, ksq, nyq, _ = geo(inp)
    keep = keep_grid(inp, mut)
    ok = (ksq > 1e-14) & (keep != 0)
    fac = keep / np.where(ksq > 0, ksq, 1)
    pr, pi = inp["c_za"] * qx, inp["c_za"] * qy
    for c, kk in enumerate((kx, ky, kz)):
        f = fac * kk
        out["Ck%d" % c] = join(np.where(ok, f * pi, 0.0).astype(rdt), np.where(ok, f * -pr, 0.0).astype(rdt), cdt)


def restate_kick_drift_za(inp, drift, mut=None):
    rdt, cdt = ki.types(inp["prec"])
    out = {}
    with np.errstate(all="ignore"):
        qx, qy = split(inp["q"])
        if drift:
            px, py = split(inp["p"])
            gx, gy = split(inp["g_in"])
            px, py = px - inp["half_eps"] * gx, py - inp["half_eps"] * gy
            out["p_out"] = join(px.astype(rdt), py.astype(rdt), cdt)
            vx, vy = 0 * px, 0 * py
            if inp["wM"] is not None:
                vx, vy = inp["wM"] * px, inp["wM"] * py
            if inp.get("extra") is not None:
                ex, ey = split(inp["extra"])
                vx, vy = vx + ex, vy + ey
            qx, qy = qx + inp["eps"] * vx, qy + inp["eps"] * vy
            out["q_out"] = join(qx.astype(rdt), qy.astype(rdt), cdt)
        za_out(inp, qx, qy, out, mut)
    return out


def assemble_g(inp, like_mode, qx, qy, mut=None):
    kx, ky, kz, ksq, nyq, _ = geo(inp)
    hx, hy = 0 * qx, 0 * qy
    if like_mode == 0:
        keep = keep_grid(inp, mut)
        live = (ksq > 0) & (keep != 0)
        f = keep / np.where(ksq > 0, ksq, 1)
        (vxx, vxy), (vyx, vyy), (vzx, vzy) = (split(inp["Ck"][c]) for c in range(3))
        fx, fy, fz = kx * f, ky * f, kz * f
        hx = np.where(live, fx * vxy + fy * vyy + fz * vzy, 0.0)
        hy = np.where(live, -(fx * vxx) - fy * vyx - fz * vzx, 0.0)
        if mut == "rotation_sign":
            hx, hy = -hx, -hy
    elif like_mode == 1:
        hx, hy = split(inp["Ck"][0])
    gx, gy = inp["b"] * hx, inp["b"] * hy
    if inp["a"] != 0.0:
        w = inp["a"] * inp["wS"]
        gx, gy = gx + w * qx, gy + w * qy
    return gx, gy


def restate_assemble(inp, kick, like_mode, mut=None):
    rdt, cdt = ki.types(inp["prec"])
    with np.errstate(all="ignore"):
        qx, qy = split(inp["q"]) if inp["a"] != 0.0 else (np.zeros(inp["q"].shape), np.zeros(inp["q"].shape))
        gx, gy = assemble_g(inp, like_mode, qx, qy, mut)
        out = {"g_out": join(gx.astype(rdt), gy.astype(rdt), cdt)}
        if kick:
            px, py = split(inp["p"])
            px, py = px - inp["c_kick"] * gx, py - inp["c_kick"] * gy
            out["p_out"] = join(px.astype(rdt), py.astype(rdt), cdt)
            k = np.arange(inp["nhp"])
            n = inp["n"]
            hw = np.where((k == 0) | ((n % 2 == 0) & (k == n // 2)), 1.0, 2.0)
            out["guard"] = float(np.sum((hw * px)[:, :, :n // 2 + 1]))  # the unrounded p, as k_assemble adds it
    return out


def restate_step_boundary(inp, last, like_mode, mut=None):
    rdt, cdt = ki.types(inp["prec"])
    he, eps = inp["half_eps"], inp["eps"]
    with np.errstate(all="ignore"):
        qx, qy = split(inp["q"])
        gx, gy = assemble_g(inp, like_mode, qx, qy, mut)
        px, py = split(inp["p"])
        pex, pey = (px - he * gx).astype(rdt), (py - he * gy).astype(rdt)
        gsx, gsy = gx.astype(rdt), gy.astype(rdt)
        out = {"guard": guard_sum(pex, inp["n"], inp["nhp"], mut)}
        if last:
            out.update(p_out=join(pex, pey, cdt), g_out=join(gsx, gsy, cdt))
            return out
        ppx, ppy = pex.astype(F8) - he * gsx.astype(F8), pey.astype(F8) - he * gsy.astype(F8)
        out["p_out"] = join(ppx.astype(rdt), ppy.astype(rdt), cdt)
        dpx, dpy = (pex.astype(F8), pey.astype(F8)) if mut == "drift_before_second_kick" else (ppx, ppy)
        if inp["wM"] is not None:
            qx, qy = qx + eps * (inp["wM"] * dpx), qy + eps * (inp["wM"] * dpy)
        out["q_out"] = join(qx.astype(rdt), qy.astype(rdt), cdt)
        za_out(inp, qx, qy, out, mut)
    return out


def restate_alpt_poisson(inp):
    rdt, cdt = ki.types(inp["prec"])
    ksq = geo(inp)[3]
    qx, qy = split(inp["q"])
    with np.errstate(all="ignore"):
        f = np.where(ksq > 0, -1.0 / np.where(ksq > 0, ksq, 1), 0.0)
        s = inp["scale"]
        return {"d1": join((s * qx).astype(rdt), (s * qy).astype(rdt), cdt),
                "phi": join((f * (s * qx)).astype(rdt), (f * (s * qy)).astype(rdt), cdt)}


def restate_prepare_mult(corr, n, nhp, normFS, mult, mut=None):
    """mult goes in and comes back with the columns k < nh written."""
    nh = n // 2 + 1
    ij = np.arange(n * n)[:, None]
    k = np.arange(nh)[None, :]
    flat = corr.reshape(-1)
    c = flat[k + (nh if mut == "corr_index_nh" else n) * ij]
    with np.errstate(all="ignore"):
        mult.reshape(n * n, nhp)[:, :nh] = np.where(c > 0, normFS / np.where(c > 0, c, 1), 0.0)
    return mult


def restate_parseval(x, w, n, nhp, mut=None):
    k = np.arange(nhp)
    hw = np.where((k == 0) | ((n % 2 == 0) & (k == n // 2)), 1.0, 2.0)
    if mut == "hw2_at_nyquist":
        hw = np.where(k == 0, 1.0, 2.0)
    xr, xi = split(x)
    upto = nhp if mut == "padding_counted" else n // 2 + 1
    with np.errstate(all="ignore"):
        return float(np.sum((hw * w * (xr * xr + xi * xi))[:, :, :upto]))


# ---- judging -----------------------------------------------------------------------------------------------------------

judge = kb.judge


def consts_of(family, inp, on):
    return kb.C[family][np.dtype(ki.types(inp["prec"])[0]).name] if on else None


def planes_fraction(inp, mode, alpt, mut=None, per=None, scaled=False):
    rdt, _ = ki.types(inp["prec"])
    r = ref.planes_step(inp, mode, alpt)
    nblocks = inp["n"] * (inp["nhp"] // ki.pass_kb(rdt))
    b = kb.planes_step_bound(r, inp, mode, alpt, rdt, nblocks=nblocks)
    return judge(restate_planes(inp, mode, alpt, mut), r, b, inp["n"] // 2 + 1, consts_of("planes_step", inp, scaled), per)


MODES = [(name,) + ki.MODES[name] for name in sorted(ki.MODES)]
with_, alpt_inputs, twin_sets = ki.with_, ki.alpt_inputs, ki.twin_sets


def planes_sets(n, prec, light=False):
    return ki.planes_sets(n, prec, 1, 1, False) if light else ki.planes_sets(n, prec)


def twin_fractions(inp, mut=None, per=None, scaled=False):
    """Every 3-D twin on one input: {kernel: (fraction, output, index)}."""
    rdt, _ = ki.types(inp["prec"])
    nh = inp["n"] // 2 + 1
    res = {}
    cs = consts_of("twins", inp, scaled)
    for drift in (False, True):
        for extra in ((False, True) if drift else (False,)):
            d = with_(inp, dict(extra=inp["Ck"][2] if extra else None))
            r = ref.kick_drift_za(d, drift)
            res["k_kick_drift_za<%d>%s" % (drift, " extra" if extra else "")] = judge(
                restate_kick_drift_za(d, drift, mut), r, kb.kick_drift_za_bound(r, d, drift, rdt), nh, cs, per)
    for like_mode in (0, 1, 2):
        for kick in (False, True):
            d = with_(inp, dict(c_kick=inp["half_eps"]))
            r = ref.assemble(d, kick, like_mode)
            res["k_assemble<%d> like_mode %d" % (kick, like_mode)] = judge(
                restate_assemble(d, kick, like_mode, mut), r, kb.assemble_bound(r, d, kick, rdt, nblocks=2048), nh, cs, per)
    for last in (False, True):
        for like_mode in (0, 1, 2):
            r = ref.step_boundary(inp, last, like_mode)
            res["k_step_boundary<%d> like_mode %d" % (last, like_mode)] = judge(
                restate_step_boundary(inp, last, like_mode, mut), r, kb.step_boundary_bound(r, inp, last, rdt, nblocks=2048), nh, cs, per)
    d = with_(inp, dict(scale=0.77 / float(inp["n"]) ** 3))
    r = ref.alpt_poisson(d)
    res["k_alpt_poisson"] = judge(restate_alpt_poisson(d), r, kb.alpt_poisson_bound(r, rdt), nh, cs, per)
    d = alpt_inputs(inp)
    r = ref.alpt_mix(d, False)
    res["k_alpt_mix"] = judge(restate_alpt_mix(d, False, mut), r, kb.alpt_mix_bound(r, d, False, rdt), nh, cs, per)
    return res


PLANES_NS = [32, 64]
TWIN_NS = [8, 9, 15, 16]
PRECS = ["fp32", "fp64"]
_measured = {}


def alpt_x_fraction(inp, mut=None, per=None, scaled=False):
    rdt = ki.types(inp["prec"])[0]
    d = alpt_inputs(inp)
    r = ref.alpt_mix(d, True)
    return judge(restate_alpt_mix(d, True, mut), r, kb.alpt_mix_bound(r, d, True, rdt), inp["n"] // 2 + 1,
                 consts_of("alpt_mix_x", inp, scaled), per)


def measure(family, prec):
    """Worst fraction of the bound at C = 1 of every output over every set (computed once per family and type).
    n = 32 sees every set; n = 64 the white set and the first layer of impulses; the planes step kernel also white data
    at 128, the first row of the launch table with the big block and rows that are padded by default."""
    key = (family, prec)
    if key in _measured:
        return _measured[key]
    per = {}
    if family == "twins":
        for n in TWIN_NS:
            for pad in (None, True):
                for sname, inp in twin_sets(n, prec, pad):
                    twin_fractions(inp, per=per)
    else:
        for n in PLANES_NS:
            for sname, inp in planes_sets(n, prec, light=n > 32):
                if family == "alpt_mix_x":
                    alpt_x_fraction(inp, per=per)
                    continue
                for mname, mode, alpt, ch in MODES:
                    planes_fraction(with_(inp, ch), mode, alpt, per=per)
        if family == "planes_step":
            planes_fraction(ki.white(128, prec), BX_INTERIOR, False, per=per)
    _measured[key] = per
    return per


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("family", ["planes_step", "alpt_mix_x", "twins"])
def test_measured_constants(family, prec):
    """(a) the restatement meets the bound at C = 1 everywhere, and the worst fraction of each output is the recorded
    figure (rounded up to two digits).  Cost: about 15 s for either type of the planes step kernel (140 longdouble
    references with their restatements at 32, 42 at 64 and one at 128), 5 s for the twins, 2 s for the ALPT mix."""
    per = measure(family, prec)
    name = np.dtype(ki.types(prec)[0]).name
    print("KSTEP-CPU %s %s: worst fraction of the bound at C = 1: %s" % (
        family, name, " ".join("%s %.3f" % kv for kv in sorted(per.items()))))
    rec = kb.MEASURED[family][name]
    assert sorted(rec) == sorted(per)
    for out, worst in per.items():
        assert worst <= 1.0, out
        assert 0.8 * rec[out] <= worst <= rec[out], out
        assert kb.C[family][name][out] == (1.0 if out == "guard" else kb.MARGIN * rec[out])
    assert kb.MARGIN == 4.0


# ---- (b) mutants -------------------------------------------------------------------------------------------------------

def planes_mutant_factor(mut, prec, n=32, modes=None):
    worst = 0.0
    for sname, inp in planes_sets(n, prec):
        for mname, mode, alpt, ch in MODES:
            if modes and mname not in modes:
                continue
            worst = max(worst, planes_fraction(with_(inp, ch), mode, alpt, mut, scaled=True)[0])
    return worst


def twin_mutant_factor(mut, prec, n, kernels, pad=None):
    worst = 0.0
    for sname, inp in twin_sets(n, prec, pad):
        for kname, (fr, _, _) in twin_fractions(inp, mut, scaled=True).items():
            if any(kname.startswith(s) for s in kernels):
                worst = max(worst, fr)
    return worst


def alpt_x_mutant_factor(mut, prec, n=32):
    return max(alpt_x_fraction(inp, mut, scaled=True)[0] for sname, inp in planes_sets(n, prec))


def prepare_mult_factor(mut, n=9):
    corr = ki.corr_grid(n)
    nhp = n // 2 + 1 + 3
    mult = restate_prepare_mult(corr, n, nhp, 0.37, np.full((n, n, nhp), -7.0), mut)
    want = ref.prepare_mult(corr, n, 0.37)
    fr, _ = kb.fraction(mult[:, :, :n // 2 + 1], want, 2 * kb.UD * np.abs(want))
    assert np.all(mult[:, :, n // 2 + 1:] == -7.0)
    return fr


def parseval_factor(mut, prec, n=16):
    inp = ki.white(n, prec, pad=True, planes=False)
    got = restate_parseval(inp["q"], inp["wS"], n, inp["nhp"], mut)
    want, sabs = ref.parseval(inp["q"], inp["wS"], n)
    return kb.scalar_fraction(got, want, (4 + n * n * (n // 2 + 1)) * kb.UD * float(sabs))


MUTANTS = {
    "rotation_sign": lambda p: max(planes_mutant_factor("rotation_sign", p, modes=("interior", "last")),
                                   twin_mutant_factor("rotation_sign", p, 8, ("k_assemble", "k_step_boundary"))),
    "kz_term_dropped": lambda p: planes_mutant_factor("kz_term_dropped", p, modes=("interior", "last_g_only")),
    "ky_kz_swapped": lambda p: planes_mutant_factor("ky_kz_swapped", p, modes=("interior", "first_za_only")),
    "prior_dropped_on_nyquist": lambda p: planes_mutant_factor("prior_dropped_on_nyquist", p, modes=("interior", "last")),
    "psi_kept_on_nyquist": lambda p: planes_mutant_factor("psi_kept_on_nyquist", p, modes=("interior", "first")),
    "hw2_at_nyquist": lambda p: max(planes_mutant_factor("hw2_at_nyquist", p, modes=("interior", "last")),
                                    parseval_factor("hw2_at_nyquist", p)),
    "padding_counted": lambda p: min(planes_mutant_factor("padding_counted", p, modes=("interior",)),
                                     parseval_factor("padding_counted", p)),
    "drift_before_second_kick": lambda p: min(planes_mutant_factor("drift_before_second_kick", p, modes=("interior",)),
                                              twin_mutant_factor("drift_before_second_kick", p, 8, ("k_step_boundary<0>",))),
    "wS_index_nh": lambda p: planes_mutant_factor("wS_index_nh", p, modes=("interior", "last")),
    "corr_index_nh": lambda p: prepare_mult_factor("corr_index_nh"),
    "plain_mask_at_odd_n": lambda p: min(twin_mutant_factor("plain_mask_at_odd_n", p, 9, ("k_kick_drift_za",)),
                                         twin_mutant_factor("plain_mask_at_odd_n", p, 9, ("k_assemble<0> like_mode 0",)),
                                         twin_mutant_factor("plain_mask_at_odd_n", p, 15, ("k_alpt_mix",))),
    "phase_sign_flip_missing": lambda p: alpt_x_mutant_factor("phase_sign_flip_missing", p),
    "KB_not_subtracted": lambda p: min(alpt_x_mutant_factor("KB_not_subtracted", p),
                                       twin_mutant_factor("KB_not_subtracted", p, 8, ("k_alpt_mix",))),
}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_bound_rejects_mutant(mut, prec):
    """(b) each mutant misses the bound, constants included, by more than 1e3 on at least one input set."""
    f = MUTANTS[mut](prec)
    print("KSTEP-CPU mutant %s %s: misses the bound by a factor of %.3g" % (mut, prec, f))
    assert f > 1e3


def test_unmutated_restatements_agree_with_the_mutant_harness():
    """The harness that rejects the mutants accepts the restatement itself (mutation None) on the same sets."""
    assert planes_mutant_factor(None, "fp32") <= 1.0
    assert alpt_x_mutant_factor(None, "fp32") <= 1.0
    assert prepare_mult_factor(None) <= 1.0
    assert parseval_factor(None, "fp64") <= 1.0


# ---- (c) control -------------------------------------------------------------------------------------------------------

def guard_trips(guard_prev, limit):
    """The kernels' test, fabs(*guard_prev) > limit, as upstream's comparison: false for NaN."""
    with np.errstate(invalid="ignore"):
        return bool(np.abs(np.float64(guard_prev)) > np.float64(limit))


def test_guard_comparison():
    lim = 1e50 * 32 ** 3
    assert not guard_trips(np.nextafter(lim, 0), lim) and not guard_trips(lim, lim)
    assert guard_trips(np.nextafter(lim, np.inf), lim) and guard_trips(-np.nextafter(lim, np.inf), lim)
    assert guard_trips(np.inf, lim) and guard_trips(-np.inf, lim)
    assert not guard_trips(np.nan, lim)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_rollback_reference_picks_the_pair_boundary_s_minus_1_read(s):
    q0, p0, q1, p1 = (np.full(4, v + 0j) for v in (1.0, 2.0, 3.0, 4.0))
    q, p = ref.rollback(s, q0, p0, q1, p1)
    assert np.all(q == (1.0 if s % 2 == 1 else 3.0)) and np.all(p == 3.0)


def test_checker_fails_closed_on_nan():
    """NaN in what the kernel returned, in the reference or in a bound is a failure, not a fraction of 0."""
    one = np.ones((2, 1, 1))
    nan = np.array([1.0, np.nan]).reshape(2, 1, 1)
    assert kb.fraction(nan, one, one)[0] == np.inf and kb.fraction(one, nan, one)[0] == np.inf
    assert kb.fraction(one, one, nan)[0] == np.inf and kb.fraction(one, one, one, col=nan[1:])[0] == np.inf
    assert kb.scalar_fraction(np.nan, 1.0, 1.0) == kb.scalar_fraction(1.0, np.nan, 1.0) == kb.scalar_fraction(1.0, 1.0, np.nan) == np.inf
    got, bounds = {"a": one, "b": one}, {"a": (one, None), "b": (one, None)}
    assert kb.judge(got, {"a": one, "b": nan}, bounds, 1)[0] == np.inf
