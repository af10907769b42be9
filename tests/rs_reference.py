"""High-precision reference of the real-space ALPT kernels and of the calc_h 0 / 3 force variants
(tests/test_rs_bounds.py and tests/test_gpu_rs.py judge the numpy restatement and the HIP kernels against it, at the bound
of tests/rs_bound.py).

Written in numpy longdouble from the upstream definitions the kernels cite, not from the kernels:

    gradfindif (gradient.cpp:81-154):  out[c] = -fac ((4/3)(in[c-1] - in[c+1]) - (1/6)(in[c-2] - in[c+2])), fac = N1 / (2 L1),
        the four neighbours wrapped periodically along the one axis `dim`.
    calc_m2v_mem (EqSolvers.cc:403-421):  g_c = gradfindif(Phi, c);  xx, xy, xz = gradfindif(g_x, x / y / z),
        yy, yz = gradfindif(g_y, y / z), zz = gradfindif(g_z, z);  m2v = xx yy - xy^2 + xx zz - xz^2 + yy zz - yz^2.
    Lag2Eul_non_zeldovich (Lag2Eul.cc:199-226):  A = D1 delta(1) - D2 m2v;  psi_lin = -D1 delta(1);
        psi_sc = 3 (sqrt(1 + 2/3 psi_lin) - 1) if 1 + 2/3 psi_lin > 0 else -3;  B = -psi_sc.
    kernelcomp (convolution.cpp:224-324, filtertype 1):  K = exp(-k^2 smol^2 / 2) on the half-complex grid.
    likelihood_calc_h (HMC_models_testing.cpp:25-50):  V_c = part_like * d f / d x_c, the derivative spectral (gradfft,
        gradient.cpp:22-78: i k_c f^, zero where the Nyquist rule hits) or by gradfindif of f(delta_x);
        f = log(rho_c (1 + max(delta_x, delta_min))) for the log-normal likelihood (lognormal_independent.cpp:57-64).
    likelihood_calc_V_SPH_fourier_TSC (HMC_models_testing.cpp:117-130):  conv^_c = (h k_c (-Im pl^) F, h k_c (Re pl^) F).
    interpolate_TSC (interpolate_grid.cpp:134-202):  cell = (unsigned)(x / d), dx = x / d - (cell + 1/2),
        w[1] = 3/4 - dx^2, w[0] = (3/2 - |dx + 1|)^2 / 2, w[2] = (3/2 - |dz - 1|)^2 / 2 FOR ALL THREE AXES (lines 166-168
        take dz for x and y as well: kept on purpose), 27 cells wrapped periodically;  with RSD out_z += f1 out_z
        (HMC_models_testing.cpp:172-185).

Every function starts from the inputs as they are stored in the kernel's type T (exact) and works in longdouble with no
rounding to T anywhere.  Taken as inputs, like tests/kstep_reference.py does: the wave numbers (calc_ki in double) and the
Nyquist weight (tests/kstep_reference.py: nyq_keep); for the TSC the particle positions in T (particle_pos, bitwise:
tests/pm_reference.py: positions) and x / d in double, one correctly rounded division that fixes the home cell.

Beside each output come the sums tests/rs_bound.py needs (names with a leading underscore).  Arrays are indexed [i, j, k].
"""
import numpy as np

from tests import pm_reference as pm
from tests.kstep_reference import kval, nyq_keep

LD = np.longdouble
CLD = np.clongdouble
OFFSETS = (-1, 1, -2, 2)  # l, r, ll, rr


def arm(a, off, axis):
    """a[c + off] along `axis`, wrapped periodically."""
    return np.roll(a, -off, axis=axis)


def gradfindif(a, axis, n, L):
    """-> (derivative, S): S = fac ((4/3)(|l| + |r|) + (1/6)(|ll| + |rr|)), the moduli that enter it."""
    a = np.asarray(a, LD)
    fac = LD(n) / (2 * LD(L))
    l, r, ll, rr = (arm(a, o, axis) for o in OFFSETS)
    with np.errstate(invalid="ignore", over="ignore"):
        out = -(fac * ((LD(4) / 3) * (l - r) - (LD(1) / 6) * (ll - rr)))
        S = fac * ((LD(4) / 3) * (np.abs(l) + np.abs(r)) + (LD(1) / 6) * (np.abs(ll) + np.abs(rr)))
    return out, S


def stencil_reach(mask, axis):
    """Cells whose gradfindif stencil along `axis` reads a cell of `mask`."""
    out = np.zeros_like(mask)
    for o in OFFSETS:
        out |= arm(mask, o, axis)
    return out


def alpt_grad(phi, n, L):
    g, S = zip(*(gradfindif(phi, c, n, L) for c in range(3)))
    return {"g3": np.array(g), "_S": np.array(S)}


def grad_support(n, at):
    """Per component, the cells an impulse at `at` reaches: 4 per axis, 3 at n = 4 where ll and rr are one cell."""
    m = np.zeros((n, n, n), bool)
    m[at] = True
    return np.array([stencil_reach(m, c) for c in range(3)])


PAIRS = (("xx", 0, 0), ("xy", 0, 1), ("xz", 0, 2), ("yy", 1, 1), ("yz", 1, 2), ("zz", 2, 2))
PRODUCTS = (("xx", "yy", 1), ("xy", "xy", -1), ("xx", "zz", 1), ("xz", "xz", -1), ("yy", "zz", 1), ("yz", "yz", -1))


def m2v_support(n, at):
    """Cells where m2v of an impulse of Phi at `at` can differ from 0: one of the six products has both factors reached."""
    g = grad_support(n, at)
    s = {name: stencil_reach(g[c], ax) for name, c, ax in PAIRS}
    out = np.zeros((n, n, n), bool)
    for p, q, _ in PRODUCTS:
        out |= s[p] & s[q]
    return out


def alpt_sources(g3, d1, n, L, D1, D2):
    """-> a, b and _m2v, _P = sum |products|, _X = sum over the products of |p| S_q + |q| S_p, _t = 2/3 psi_lin,
    _arg = 1 + _t."""
    g3 = np.asarray(g3, LD)
    d1 = np.asarray(d1, LD)
    v, S = {}, {}
    for name, c, ax in PAIRS:
        v[name], S[name] = gradfindif(g3[c], ax, n, L)
    m2v, P, X = LD(0), LD(0), LD(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for p, q, sign in PRODUCTS:
            m2v = m2v + sign * (v[p] * v[q])
            P = P + np.abs(v[p] * v[q])
            X = X + np.abs(v[p]) * S[q] + np.abs(v[q]) * S[p]
        a = LD(D1) * d1 - LD(D2) * m2v
        psilin = -LD(D1) * d1
        t = (LD(2) / 3) * psilin
        arg = 1 + t
        psisc = np.where(arg > 0, 3 * (np.sqrt(np.where(arg > 0, arg, 0)) - 1), LD(-3))
    return {"a": a, "b": -psisc, "_m2v": m2v, "_P": P, "_X": X, "_t": t, "_arg": arg,
            "_aabs": np.abs(LD(D1) * d1) + np.abs(LD(D2) * m2v)}


def kgrid(n, nh, L):
    kv = kval(n, L, max(n, nh)).astype(LD)
    return kv[:n, None, None], kv[None, :n, None], kv[None, None, :nh]


def kernel_table(n, nhp, L, smol):
    """-> tab (n, n, nhp) complex: K for k < nh, 0 in the row padding; _arg the exponent."""
    nh = n // 2 + 1
    kx, ky, kz = kgrid(n, nh, L)
    arg = -(kx * kx + ky * ky + kz * kz) * LD(smol) * LD(smol) / 2
    tab = np.zeros((n, n, nhp), CLD)
    tab[:, :, :nh] = np.exp(arg)
    full = np.zeros((n, n, nhp), LD)
    full[:, :, :nh] = arg
    return {"tab": tab, "_arg": full}


def rot(v):
    """(-Im, Re) of a complex array: multiplication by i."""
    return -v.imag + 1j * v.real


def gradfft_mult(fk, n, L, inv_n):
    """fk: (n, n, >= nh) stored -> Ck (3, n, n, nh) = i k_c f^ keep / N and _keep."""
    nh = n // 2 + 1
    f = np.asarray(fk)[:, :, :nh].astype(CLD)
    keep = nyq_keep(n, nh).astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.array([np.where(keep != 0, rot(f) * (k * (keep * LD(inv_n))), 0) for k in kgrid(n, nh, L)])
    return {"Ck": out, "_keep": keep}


def conv_kernel(pl, F, n, L, hh, inv_n):
    nh = n // 2 + 1
    f = np.asarray(pl)[:, :, :nh].astype(CLD)
    Fl = np.asarray(F)[:, :, :nh].astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.array([rot(f) * (LD(hh) * k * Fl * LD(inv_n)) for k in kgrid(n, nh, L)])
    return {"Ck": out}


def mul3(a, b3):
    with np.errstate(invalid="ignore", over="ignore"):
        return {"out3": np.asarray(a, LD)[None] * np.asarray(b3, LD)}


def f_delta_x(dX, likelihood, rho_c, delta_min):
    """f(delta_x) and the absolute error a double evaluation of it makes per unit of u_d (0 for the identity)."""
    v = np.asarray(dX, LD)
    if likelihood != 2:
        return v, 0 * np.abs(np.where(np.isfinite(v), v, 0))
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.log(LD(rho_c) * (1 + np.where(v < LD(delta_min), LD(delta_min), v)))
    return f, 3 + 2 * np.abs(f)


def findif_mul(dX, plike, n, L, likelihood, rho_c=1.0, delta_min=-0.99):
    """-> V (3, n, n, n), _S the moduli of the difference, _E the arms' own errors through it (per unit of u_d)."""
    f, ef = f_delta_x(dX, likelihood, rho_c, delta_min)
    pl = np.asarray(plike, LD)
    fac = LD(n) / (2 * LD(L))
    V, S, E = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            d, s = gradfindif(f, c, n, L)
            l, r, ll, rr = (arm(ef, o, c) for o in OFFSETS)
            V.append(pl * d)
            S.append(np.abs(pl) * s)
            E.append(np.abs(pl) * fac * ((LD(4) / 3) * (l + r) + (LD(1) / 6) * (ll + rr)))
    return {"V": np.array(V), "_S": np.array(S), "_E": np.array(E)}


def tsc_positions(psi, geo, rsd, dtype, cpecvel, v_norm):
    """particle_pos in the storage type (bitwise) and pos_ok."""
    pos = pm.positions(psi, geo, rsd, dtype, cpecvel, v_norm)
    T = np.dtype(dtype).type
    ok = np.ones(geo.N, bool)
    with np.errstate(invalid="ignore"):
        for x in pos:
            ok &= (x >= T(0)) & (x <= T(geo.L))
    return pos, ok


def tsc_weights(xk, dz_for_upper=None):
    """One axis: cell (unsigned)(xk), the three weights; the upper one from `dz_for_upper` if given (the upstream bug)."""
    cell = np.trunc(xk).astype(np.int64)
    dx = xk.astype(LD) - (cell.astype(LD) + LD(0.5))
    du = dx if dz_for_upper is None else dz_for_upper
    w = [LD(0.5) * (LD(1.5) - np.abs(dx + 1)) ** 2, LD(0.75) - dx * dx, LD(0.5) * (LD(1.5) - np.abs(du - 1)) ** 2]
    return cell, dx, w


def interp_tsc(psi, conv, geo, dtype, rsd, f1, cpecvel=0.0, v_norm=0.0, fix_dz_bug=False):
    """psi (3, N) in T, conv (3, n, n, n) in T -> V (3, N); _W = sum |w conv| and _D = sum (wy wz + wx wz + wx wy) |conv|
    per component; _ok.  A particle that fails pos_ok gets 0 with both sums 0."""
    n, N = geo.n, geo.N
    pos, ok = tsc_positions(psi, geo, rsd, dtype, cpecvel, v_norm)
    xk = [np.where(ok, x.astype(np.float64), 0.5) / np.float64(geo.d) for x in pos]  # the kernel's double division
    cz, dz, wz = tsc_weights(xk[2])
    cx, _, wx = tsc_weights(xk[0], None if fix_dz_bug else dz)
    cy, _, wy = tsc_weights(xk[1], None if fix_dz_bug else dz)
    conv = np.asarray(conv).reshape(3, n, n, n)
    V, W, D = np.zeros((3, N), LD), np.zeros((3, N), LD), np.zeros((3, N), LD)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                ia, ib, ic = (cx + a - 1) % n, (cy + b - 1) % n, (cz + c - 1) % n
                w = wx[a] * wy[b] * wz[c]
                dw = np.abs(wy[b] * wz[c]) + np.abs(wx[a] * wz[c]) + np.abs(wx[a] * wy[b])
                for comp in range(3):
                    f = conv[comp][ia, ib, ic].astype(LD)
                    V[comp] += w * f
                    W[comp] += np.abs(w * f)
                    D[comp] += dw * np.abs(f)
    pre = V[2].copy()
    if rsd:
        V[2] = V[2] + LD(f1) * V[2]
    for arr in (V, W, D):
        arr[:, ~ok] = 0
    return {"V": V, "_W": W, "_D": D, "_ok": ok, "_o2": np.where(ok, np.abs(pre), 0), "_pos": pos}
