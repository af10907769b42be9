"""The error bound the k-space step kernels are held to (tests/test_kstep_bounds.py measures its constants on a numpy
restatement and shows that it can fail; tests/test_gpu_kstep.py applies it to the HIP kernels).  Reference:
tests/kstep_reference.py.  Laid out after tests/fft_bound.py and tests/like_bound.py.

Notation.  u_T is the unit round-off of the storage type T (FFT arithmetic and every stored array), u_d = 2^-53 that of
the doubles the element-wise arithmetic runs in.  |z| of a complex number is its modulus: rounding its two parts to T
moves it by at most u_T |z|.  For a column y along x (length n), ||y|| is its 2-norm.  All bounds are to first order in u.

Transforms.  One pass of xfft_inplace over a column with exact input returns y^ with ||y^ - y|| <= log2(n) u_T ||y|| and
hence max |y^ - y| <= log2(n) u_T ||y|| (the single-pass term of fft_bound at C = 1).  If the input column itself is
off by d (element-wise bounds d_i), the transform carries that to sqrt(n) ||d|| in the 2-norm (the DFT matrix has norm
sqrt(n)) and so also in the maximum.  The transform term of a column is therefore

    E(y; d) = log2(n) u_T ||y|| + sqrt(n) ||d||.

Element-wise maps.  After a forward pass, element i of the column is used with a multiplier (kx_i for V^_x, 1 for W^, then
f_i = b / k_i^2, half_eps, eps wM_i, the inverse-pass multipliers c_za kx_i / k_i^2 and c_za / k_i^2, ...): its error is
the transform term times the modulus of the product of these multipliers -- per element, which is never more than the
column's largest multiplier.  Every operation in double adds u_d and every rounding to T adds u_T, each times the sum of
the moduli of the terms the value is made of (so cancellation is paid for).  The counted numbers of double operations
are the integers in the code below.

The roundings the kernels make on purpose are carried by the bound, not by the reference: W = ky V_y + kz V_z rounded to
T before its transform (u_T + 3 u_d times |ky V_y| + |kz V_z| per element, through the transform as d); p_end and g^
rounded to T between the two half kicks (u_T |p_end|, u_T |g^|, carried into p' with half_eps); the first inverse pass
takes q' as computed (its error without the u_T |q'| of the store) and the second q' as stored (with it).

k_step_boundary_x, per column (j, k) and element i (MODE selects which lines exist):

    e_h   = |kx_i| E(V^_x; 0) + E(W^; (u_T + 3 u_d)(|ky V_y| + |kz V_z|))
    S_g   = |f_i| (|kx_i V^_x,i| + |W^_i|) + |a wS_i q_i|
    e_g   = |f_i| e_h + 6 u_d S_g                                  g_out:  e_g + u_T |g|
    e_pe  = |half_eps| e_g + u_T |p_end| + 2 u_d (|p| + |half_eps| S_g)          (p_out of BX_LAST)
    e_p'  = e_pe + |half_eps| (e_g + u_T |g|) + 2 u_d (|p_end| + |half_eps| S_g) p_out:  e_p' + u_T |p'|
          (BX_FIRST with g_in: e_p' = 2 u_d (|p| + |half_eps g_in|))
    e_q'  = |eps wM_i| e_p' + 3 u_d (|q| + |eps wM_i p'|)                        q_out:  e_q' + u_T |q'|
          (no wM, or no kick at all: q' = q exactly, both bounds 0)
    d1_i  = |m1_i| e_q' + (u_T + 4 u_d) |m1_i q'_i|,   d2_i = |m2_i| (e_q' + u_T |q'|) + (u_T + 4 u_d) |m2_i q'_i|
    Ck[0] = X:        E(X; d1)              in the 2-norm of the column and per element
    Ck[1] = ky B:     |ky| E(B; d2) + (u_T + u_d) |ky B_i|   per element; the same with ||B|| for the column; Ck[2] with kz
          (ALPT: Ck[1] = B itself, E(B; d2); Ck[2] is not written)

with m1 = -i c_za kx / k^2, m2 = -i c_za / k^2, both 0 for k^2 <= 1e-14 and on the Nyquist planes (ALPT: m1 = c_za
everywhere, m2 = -c_za / k^2, 0 at k = 0 only).  An element or a column whose bound is 0 must be exact: the planes of
Psi^ the rule zeroes, DC, q_out without a mass, everything a mode does not touch.

The guard sum: the kernels add hw Re p_end (rounded to T) in double, PER terms per thread, 6 + log2(NT / 64) levels of
shuffles and one atomic per workgroup in any order, at most  G = 18 + (number of workgroups)  additions on any path:

    |guard^ - guard|  <=  sum_k hw_k e_pe  +  G u_d sum_k hw_k |Re p_end|.

k_alpt_mix_x:  e_M = K E(A^; 0) + (1 + K) E(B^; 0) + u_d (3 |arg| + 8)(|K A^| + |B^| + |K B^|)  with arg = -k^2 kth^2 / 2
(the exponential's argument is off by 3 u_d |arg| and moves K by that much relatively);  P from the twiddle table in T is
off by (u_T + 2 u_d) / 2;  e_E = fac (|P| e_M + (u_T + 2 u_d) |M| / 2 + 8 u_d |M|),  fac = 1 / (N k^2);  d1 = |kx| e_E +
(u_T + u_d) |kx E|,  d2 = e_E + u_T |E|;  the outputs as above.  k_alpt_mix (3-D) is the per-element part with sincospi in
double (u_T -> 0 in P) and one rounding to T at the store.

The 3-D twins have no transform: every output is bounded by (counted u_d + u_T of the store) times the sum of the moduli
of its terms, with e_g, e_pe, e_p', e_q' as above at e_h = 0 and S_g from the three V^ terms.

Constants.  The bound of each output is multiplied by one constant C per kernel family, type and output.  tests/test_kstep_bounds.py runs
the numpy restatement of each kernel (float32 / float64 storage, the radix-4 xfft_inplace restatement of
tests/test_fft_pass_bounds.py inside) on the input sets of tests/kstep_inputs.py and finds the worst fraction of the
bound at C = 1: MEASURED below, asserted there.  C = 4 x that figure, the margin every constant of this suite has (the
GPU contracts multiply-adds and sums in another order).  Without fused multiply-adds a single rounding can use its
u_T |z| up, so the figures are of order one where an output is a stored copy of one rounded sum.  The guard sum is the
exception: its bound is counted as above and used as it stands (C = 1); the restatement's fraction of it is recorded
all the same (the per-element errors add up like a random walk, far below their sum).
"""
import numpy as np

from tests.fft_bound import unit_roundoff
from tests.kstep_reference import BX_FIRST, BX_LAST

UD = 2.0 ** -53
MARGIN = 4.0
# worst fraction of the bound at C = 1 that the numpy restatement reaches, per kernel family, storage type and output
# (rounded up to two digits)
MEASURED = {
    "planes_step": {
        "float32": {"Ck0": 0.42, "Ck1": 0.37, "Ck2": 0.34, "g_out": 0.99, "guard": 0.65, "p_out": 1.0, "q_out": 1.0},
        "float64": {"Ck0": 0.33, "Ck1": 0.28, "Ck2": 0.27, "g_out": 0.36, "guard": 0.0085, "p_out": 0.42, "q_out": 0.48},
    },
    "alpt_mix_x": {
        "float32": {"Ck0": 0.095, "Ck1": 0.087, "Ck2": 0.087},
        "float64": {"Ck0": 0.096, "Ck1": 0.14, "Ck2": 0.14},
    },
    "twins": {
        "float32": {"Ck0": 1.0, "Ck1": 0.99, "Ck2": 0.98, "d1": 0.99, "g_out": 1.0, "guard": 0.56, "p_out": 1.0, "phi": 0.98, "q_out": 1.0},
        "float64": {"Ck0": 0.52, "Ck1": 0.52, "Ck2": 0.52, "d1": 0.49, "g_out": 0.37, "guard": 0.0011, "p_out": 0.38, "phi": 0.46, "q_out": 0.46},
    },
}
# the guard sum keeps its counted bound (C = 1): its constant is counted, not measured
C = {fam: {t: {o: (1.0 if o == "guard" else MARGIN * f) for o, f in d.items()} for t, d in per.items()}
     for fam, per in MEASURED.items()}


def col2(a):
    """2-norm of every column along x (axis 0), kept broadcastable."""
    return np.sqrt(np.sum(np.abs(a) ** 2, axis=0, keepdims=True))


def transform_term(y, d, n, uT):
    return np.log2(n) * uT * col2(y) + np.sqrt(n) * col2(d)


def planes_step_bound(r, inp, mode, alpt, dtype, c=1.0, nblocks=0):
    """Bounds of planes_step's outputs: {name: (per-element bound, column bound or None)}, 'guard': scalar."""
    uT, n = unit_roundoff(dtype), inp["n"]
    G = r["_G"]
    A = np.abs
    he = abs(inp["half_eps"])
    out = {}
    e_ppu = None
    if mode != BX_FIRST:
        e_h = A(G.kx) * transform_term(r["_vxh"], 0 * r["_Wabs"], n, uT) + transform_term(r["_wh"], (uT + 3 * UD) * r["_Wabs"], n, uT)
        S_g = A(r["_f"]) * (A(G.kx * r["_vxh"]) + A(r["_wh"])) + A(r["_prior"])
        e_g = A(r["_f"]) * e_h + 6 * UD * S_g
        e_gs = e_g + uT * A(r["_gg"])
        if mode == BX_LAST:
            out["g_out"] = (c * e_gs, None)
            if inp["p"] is None:
                return out
        e_pe = he * e_g + uT * A(r["_pe"]) + 2 * UD * (A(r["_p"]) + he * S_g)
        cnt = np.where(G.counted, 1.0, 0.0)
        out["guard"] = c * float(np.sum(cnt * G.hw * e_pe) + (18 + nblocks) * UD * np.sum(cnt * G.hw * A(r["_pe"].real)))
        if mode == BX_LAST:
            out["p_out"] = (c * e_pe, None)
            return out
        e_ppu = e_pe + he * e_gs + 2 * UD * (A(r["_pe"]) + he * S_g)
    elif r["_kicked"]:
        e_ppu = 2 * UD * (A(r["_p"]) + he * A(r["_g0"]))
    zero = 0 * A(r["_q"])
    e_qu = e_qs = zero
    if r["_kicked"]:
        out["p_out"] = (c * (e_ppu + uT * A(r["p_out"])), None)
        if inp["wM"] is not None:
            e_qu = A(r["_ew"]) * e_ppu + 3 * UD * (A(r["_q"]) + A(r["_drift"]))
            e_qs = e_qu + uT * A(r["q_out"])
        out["q_out"] = (c * e_qs, None)
    d1 = A(r["_m1"]) * e_qu + (uT + 4 * UD) * A(r["_o1"])
    d2 = A(r["_m2"]) * e_qs + (uT + 4 * UD) * A(r["_o2"])
    E_X = transform_term(r["Ck0"], d1, n, uT)
    E_B = transform_term(r["_B"], d2, n, uT)
    out["Ck0"] = (c * (E_X + zero), c * E_X)
    if alpt:
        out["Ck1"] = (c * (E_B + zero), c * E_B)
    else:
        for name, kk in (("Ck1", G.ky), ("Ck2", G.kz)):
            out[name] = (c * (A(kk) * E_B + (uT + UD) * A(kk * r["_B"])), c * A(kk) * (E_B + (uT + UD) * col2(r["_B"])))
    return out


def alpt_mix_bound(r, inp, planes, dtype, c=1.0):
    uT, n = unit_roundoff(dtype), inp["n"]
    G = r["_G"]
    A = np.abs
    K = A(r["_K"])
    S_M = K * A(r["_A"]) + A(r["_B"]) + K * A(r["_B"])
    e_M = UD * (3 * A(r["_arg"]) + 8) * S_M
    uP = 2 * UD
    if planes:
        zero = 0 * S_M
        e_M = e_M + K * transform_term(r["_A"], zero, n, uT) + (1 + K) * transform_term(r["_B"], zero, n, uT)
        uP = uT + 2 * UD
    Pabs = A(r["_E"]) / np.where(r["_ok"] & (A(r["_M"]) > 0), r["_fac"] * A(r["_M"]), 1)  # |P| where it is used
    Pabs = np.where(r["_ok"] & (A(r["_M"]) > 0), Pabs, 1.0)
    e_E = r["_fac"] * (Pabs * e_M + 0.5 * uP * A(r["_M"]) + 8 * UD * A(r["_M"]))
    out = {}
    if not planes:
        for name, kk in (("Ck0", G.kx), ("Ck1", G.ky), ("Ck2", G.kz)):
            out[name] = (c * (A(kk) * e_E + (uT + UD) * A(r[name])), None)
        return out
    d1 = A(G.kx) * e_E + (uT + UD) * A(G.kx * r["_E"])
    d2 = e_E + uT * A(r["_E"])
    E_X = transform_term(r["Ck0"], d1, n, uT)
    E_B = transform_term(r["_Ei"], d2, n, uT)
    out["Ck0"] = (c * (E_X + 0 * S_M), c * E_X)
    for name, kk in (("Ck1", G.ky), ("Ck2", G.kz)):
        out[name] = (c * (A(kk) * E_B + (uT + UD) * A(kk * r["_Ei"])), c * A(kk) * (E_B + (uT + UD) * col2(r["_Ei"])))
    return out


def za_bound(r, uT, e_q, c):
    """Psi^_j = k_j (keep / k^2) (-i c_za q'): the error of q' through the multiplier, 6 double operations and the store."""
    G = r["_G"]
    return {name: (c * (np.abs(kk * r["_mz"]) * e_q + (uT + 6 * UD) * np.abs(r[name])), None)
            for name, kk in (("Ck0", G.kx), ("Ck1", G.ky), ("Ck2", G.kz))}


def kick_drift_za_bound(r, inp, drift, dtype, c=1.0):
    uT = unit_roundoff(dtype)
    A = np.abs
    out = {}
    e_q = 0 * A(r["_q"])
    if drift:
        e_pp = 2 * UD * (A(r["_p"]) + abs(inp["half_eps"]) * A(r["_g0"]))
        out["p_out"] = (c * (e_pp + uT * A(r["p_out"])), None)
        wabs = np.abs(inp["wM"][:, :, :r["_G"].nh]) if inp["wM"] is not None else 0
        e_q = abs(inp["eps"]) * wabs * e_pp + 4 * UD * (A(r["_q"]) + abs(inp["eps"]) * r["_vabs"])
        out["q_out"] = (c * (e_q + uT * A(r["q_out"])), None)
    out.update(za_bound(r, uT, e_q, c))
    return out


def assemble_bound(r, inp, kick, dtype, c=1.0, nblocks=0):
    uT = unit_roundoff(dtype)
    A = np.abs
    G = r["_G"]
    e_g = 8 * UD * r["_gabs"]
    out = {"g_out": (c * (e_g + uT * A(r["g_out"])), None)}
    if kick:
        ck = abs(inp["c_kick"])
        e_p = ck * e_g + 2 * UD * (A(r["_p"]) + ck * r["_gabs"]) + uT * A(r["p_out"])
        out["p_out"] = (c * e_p, None)
        out["guard"] = c * float(np.sum(G.hw * e_p) + (18 + nblocks) * UD * np.sum(G.hw * A(r["p_out"].real)))
    return out


def step_boundary_bound(r, inp, last, dtype, c=1.0, nblocks=0):
    uT = unit_roundoff(dtype)
    A = np.abs
    G = r["_G"]
    he = abs(inp["half_eps"])
    e_g = 8 * UD * r["_gabs"]
    e_gs = e_g + uT * A(r["_gg"])
    e_pe = he * e_g + uT * A(r["_pe"]) + 2 * UD * (A(r["_p"]) + he * r["_gabs"])
    out = {"guard": c * float(np.sum(G.hw * e_pe) + (18 + nblocks) * UD * np.sum(G.hw * A(r["_pe"].real)))}
    if last:
        out["g_out"] = (c * e_gs, None)
        out["p_out"] = (c * e_pe, None)
        return out
    e_ppu = e_pe + he * e_gs + 2 * UD * (A(r["_pe"]) + he * r["_gabs"])
    out["p_out"] = (c * (e_ppu + uT * A(r["p_out"])), None)
    e_q = 0 * A(r["_q"])
    e_qs = e_q
    if inp["wM"] is not None:
        e_q = A(r["_ew"]) * e_ppu + 3 * UD * (A(r["_q"]) + A(r["_drift"]))
        e_qs = e_q + uT * A(r["q_out"])
    out["q_out"] = (c * e_qs, None)
    out.update(za_bound(r, uT, e_q, c))
    return out


def alpt_poisson_bound(r, dtype, c=1.0):
    uT = unit_roundoff(dtype)
    return {"d1": (c * (uT + UD) * np.abs(r["d1"]), None), "phi": (c * (uT + 6 * UD) * np.abs(r["phi"]), None)}


def fraction(got, ref, elem, col=None):
    """Worst |got - ref| / bound over the elements (and ||got - ref|| / bound over the columns along axis 0 if `col` is
    given), with the index of the worst element.  A zero bound demands equality; NaN or inf in `got` gives inf."""
    got = np.asarray(got)
    if not np.isfinite(got).all():
        bad = np.argwhere(~np.isfinite(got))[0]
        return np.inf, tuple(int(x) for x in bad)
    d = np.abs(got.astype(ref.dtype) - ref)
    elem = np.broadcast_to(elem, d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        fr = np.where(elem > 0, d / np.where(elem > 0, elem, 1), np.where(d > 0, np.inf, 0))
    fr = np.where(np.isfinite(d) & ~np.isnan(elem), fr, np.inf)  # NaN in the reference or the bound: fail closed
    at = np.unravel_index(int(np.argmax(fr)), fr.shape)
    worst = float(fr[at])
    if col is not None:
        e2 = np.sqrt(np.sum(d ** 2, axis=0, keepdims=True))
        col = np.broadcast_to(col, e2.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            f2 = np.where(col > 0, e2 / np.where(col > 0, col, 1), np.where(e2 > 0, np.inf, 0))
        f2 = np.where(np.isfinite(e2) & ~np.isnan(col), f2, np.inf)
        if float(np.max(f2)) > worst:
            at = np.unravel_index(int(np.argmax(f2)), f2.shape)
            worst = float(f2[at])
    return worst, tuple(int(x) for x in at)


def judge(got, r, bounds, nh, consts=None, per=None, slicer=None):
    """Worst fraction over the outputs the bounds name -> (fraction, output, index).  got: the outputs as stored
    (n, n, nhp), cut to k < nh or by `slicer`; consts: the constant of each output (None: the bound at C = 1); per: a
    dict that collects the worst fraction of each output.  A fraction that is not finite (NaN from a reference or a bound
    included) counts as inf: the checker fails closed."""
    worst = (0.0, None, ())
    for name, bd in bounds.items():
        c = 1.0 if consts is None else consts[name]
        if name == "guard":
            fr, at = scalar_fraction(got["guard"], r["guard"], c * bd), ()
        else:
            g = got[name][:, :, :nh] if slicer is None else slicer(got[name])
            fr, at = fraction(g, r[name], c * bd[0], None if bd[1] is None else c * bd[1])
        if not np.isfinite(fr):
            fr = np.inf
        if per is not None:
            per[name] = max(per.get(name, 0.0), fr)
        if worst[1] is None or fr > worst[0]:
            worst = (fr, name, at)
    return worst


def scalar_fraction(got, ref, bound):
    if not np.isfinite(got):
        return np.inf
    d = abs(np.longdouble(got) - np.longdouble(ref))
    if not (np.isfinite(d) and np.isfinite(bound)):
        return np.inf  # NaN in the reference or the bound: fail closed
    return float(d / bound) if bound > 0 else (np.inf if d > 0 else 0.0)
