"""The error bound the real-space ALPT kernels and the calc_h 0 / 3 kernels are held to, per cell
(tests/test_rs_bounds.py measures its constants on a numpy restatement and shows that it can fail; tests/test_gpu_rs.py
applies it to the HIP kernels).  Reference: tests/rs_reference.py.  Laid out after tests/kstep_bound.py and tests/pm_bound.py.

Notation.  u_T is the unit round-off of the storage type T, u_d = 2^-53 that of the doubles all arithmetic of these kernels
runs in.  Inputs are exact in T.  Every double operation adds u_d times the moduli that enter it (so cancellation is paid
for), the final rounding adds u_T |out|.  All bounds are to first order in u.  The counted numbers of operations are the
integers in the code below.

Finite difference.  D(a)[c] = -fac ((4/3)(a_l - a_r) - (1/6)(a_ll - a_rr)) with S = fac ((4/3)(|a_l| + |a_r|) + (1/6)(|a_ll| +
|a_rr|)):  two differences, the rounded constants 4/3 and 1/6 and their products, the outer difference, fac = n / (2 L) and
its product: at most 6 roundings on any term,

    e_D = 6 u_d S.                                       k_alpt_grad:  e_D + u_T |g|.

delta(2).  Each of xx .. zz is a D of a stored first derivative: e_p = 6 u_d S_p.  A product p q is off by |p| e_q + |q| e_p
+ u_d |p q|, and the five additions add at most 5 u_d sum |products|:

    e_m2v = 6 u_d X + 6 u_d P,   X = sum over the six products of (|p| S_q + |q| S_p),   P = sum |p q|.

    a = D1 dl - D2 m2v:   |D2| e_m2v + 3 u_d (|D1 dl| + |D2 m2v|) + u_T |a|.

The spherical-collapse source.  b = 3 (1 - sqrt(max(arg, 0))), arg = 1 + t, t = -(2/3) D1 dl: both branches of the
upstream `if` in one expression, continuous at arg = 0.  The computed argument: psi_lin (1 rounding), the rounded constant
2/3 and its product (2), the sum (u_d |arg| <= u_d (1 + |t|)): off by at most 4 u_d (1 + |t|).  A perturbation of the
argument by +-x moves sqrt(max(arg, 0)) by at most sqrt(max(arg, 0) + 3 x) - sqrt(max(arg, 0)) in either direction (upwards
by concavity with x itself; downwards, for arg = s x: s >= 1 needs 3 (sqrt(s) + sqrt(s - 1)) >= sqrt(s + 3) + sqrt(s), true at
s = 1 with equality and beyond; s < 1 falls into the other branch and moves by sqrt(arg) <= sqrt(arg + 3 x) - sqrt(arg)).  So with

    eta = 12 u_d (1 + |t|):    |b^ - b| <= 3 (sqrt(max(arg, 0) + eta) - sqrt(max(arg, 0))) + 3 u_d (sqrt(max(arg, 0)) + 1 + |b|) + u_T |b|

(the square root, the difference with 1 and the product with 3 are the three counted roundings), about 3 sqrt(eta) at the
edge and 1.5 eta / sqrt(arg) away from it, valid across the edge: no cell is left out.  Where dl is NaN or +inf the `else`
branch returns the constant 3 (t is not finite: eta = 0) and the bound is the u_T term alone.

k_alpt_kernel_table.  K = exp(arg), arg = -(kx^2 + ky^2 + kz^2) smol^2 / 2 from the kernel's own wave numbers: 3 squares and
2 sums, smol^2, two more products: <= 7 roundings of arg, which move K by 7 u_d |arg| K; the exponential itself 2 u_d K:

    u_d (7 |arg| + 2) K + u_T K;     0 for the imaginary part and for the row padding (bound 0: exact).

k_gradfft_mult.  Ck_c = i k_c f^ keep / N: keep / N and two products, (3 u_d + u_T) |Ck_c|; keep = 0 -> bound 0.
k_conv_kernel.  Ck_c = i h k_c pl^ F / N: four products, (4 u_d + u_T) |Ck_c|; F = 0 -> bound 0.
k_mul3.  One product in T: u_T |out|.

k_findif_mul.  V_c = pl D_c(f(delta_x)):  (6 u_d |pl| S + u_d |V|) + u_T |V| for f the identity.  The log-normal arm
f = log(rho_c (1 + max(v, delta_min))): the clamp compares exact values; 1 + v and the product with rho_c are each rounded
relative to their result, however close 1 + v is to 0, so the argument x of the logarithm is off by 2 u_d x, which its
derivative 1 / x turns into an ABSOLUTE 2 u_d -- the conditioning term: it does not shrink with |f| -- and the logarithm
itself adds u_d (1 + 2 |f|) (2 ulp allowed for the device function):  e_f = u_d (3 + 2 |f|) per neighbour, through the
difference as E = |pl| fac ((4/3)(e_l + e_r) + (1/6)(e_ll + e_rr)).

k_interp_tsc.  Positions and the home cells are compared bitwise (inputs).  dx = xk - (cell + 1/2) is exact or off by u_d / 2;
every one-dimensional weight (values in [0, 3/4], intermediates below 5/2) is off by at most 8 u_d absolutely.  A product
w = wx wy wz is off by 8 u_d (wy wz + wx wz + wx wy) + 2 u_d w; each term w conv adds u_d and the 27 additions 27 u_d:

    e_o = 8 u_d D + 30 u_d W,   D = sum (wy wz + wx wz + wx wy) |conv|,   W = sum |w conv|;   out:  e_o + u_T |V|
    with RSD, z component:  (1 + |f1|) e_o + 2 u_d (1 + |f1|) |o2| + u_T |V|.

A particle that fails pos_ok has D = W = 0: bound 0, the output is exactly 0.

A cell whose bound is 0 must be exact.  A reference value that is not finite must come back as the same class (NaN, +inf,
-inf); a finite one must come back finite.

Constants.  Each bound is multiplied by one constant C per kernel, type and output: 4 x the worst fraction of the bound at
C = 1 that the numpy restatement of tests/test_rs_bounds.py reaches on the input sets of tests/rs_inputs.py (MEASURED
below, asserted there), the margin every constant of this suite has (the GPU contracts multiply-adds and its libm differs).
"""
import numpy as np

from tests.fft_bound import unit_roundoff

UD = 2.0 ** -53
MARGIN = 4.0
LD = np.longdouble
# worst fraction of the bound at C = 1 that the numpy restatement reaches, per kernel, storage type and output (rounded
# up to two digits)
MEASURED = {
    "alpt_grad": {"float32": {"g3": 1.0}, "float64": {"g3": 0.44}},
    "alpt_sources": {"float32": {"a": 1.0, "b": 1.0}, "float64": {"a": 0.49, "b": 0.19}},
    "kernel_table": {"float32": {"tab": 1.0}, "float64": {"tab": 0.51}},
    "gradfft_mult": {"float32": {"Ck": 1.0}, "float64": {"Ck": 0.47}},
    "conv_kernel": {"float32": {"Ck": 1.0}, "float64": {"Ck": 0.64}},
    "mul3": {"float32": {"out3": 1.0}, "float64": {"out3": 1.0}},
    "findif_mul": {"float32": {"V": 1.0}, "float64": {"V": 0.47}},
    "interp_tsc": {"float32": {"V": 1.0}, "float64": {"V": 0.093}},
}
C = {k: {t: {o: MARGIN * f for o, f in d.items()} for t, d in per.items()} for k, per in MEASURED.items()}


def consts(kernel, dtype):
    return C[kernel][np.dtype(np.empty(0, dtype).real.dtype).name]


def _fin(x):
    """x where finite, 0 elsewhere (a term of a bound at a cell whose reference is not finite is never used)."""
    return np.where(np.isfinite(x), x, 0)


def alpt_grad_bound(r, dtype):
    return {"g3": 6 * UD * r["_S"] + unit_roundoff(dtype) * np.abs(r["g3"])}


def alpt_sources_bound(r, dtype, D2):
    uT = unit_roundoff(dtype)
    e_m2v = 6 * UD * (r["_X"] + r["_P"])
    a = abs(D2) * e_m2v + 3 * UD * r["_aabs"] + uT * np.abs(r["a"])
    t = r["_t"]
    eta = np.where(np.isfinite(t), 12 * UD * (1 + np.abs(_fin(t))), 0)
    m = np.where(r["_arg"] > 0, _fin(r["_arg"]), 0)
    rt = np.sqrt(m)
    b = 3 * (np.sqrt(m + eta) - rt) + 3 * UD * (rt + 1 + np.abs(_fin(r["b"]))) + uT * np.abs(r["b"])
    return {"a": a, "b": b}


def kernel_table_bound(r, dtype):
    K = np.abs(r["tab"])
    return {"tab": (UD * (7 * np.abs(r["_arg"]) + 2) + unit_roundoff(dtype)) * K}


def gradfft_mult_bound(r, dtype):
    return {"Ck": (3 * UD + unit_roundoff(dtype)) * np.abs(r["Ck"])}


def conv_kernel_bound(r, dtype):
    return {"Ck": (4 * UD + unit_roundoff(dtype)) * np.abs(r["Ck"])}


def mul3_bound(r, dtype):
    return {"out3": unit_roundoff(dtype) * np.abs(r["out3"])}


def findif_mul_bound(r, dtype):
    return {"V": UD * (6 * r["_S"] + r["_E"] + np.abs(r["V"])) + unit_roundoff(dtype) * np.abs(r["V"])}


def interp_tsc_bound(r, dtype, rsd, f1):
    uT = unit_roundoff(dtype)
    e = 8 * UD * r["_D"] + 30 * UD * r["_W"]
    if rsd:
        e[2] = (1 + abs(f1)) * e[2] + 2 * UD * (1 + abs(f1)) * r["_o2"]
    return {"V": e + uT * np.abs(r["V"])}


def fraction(got, ref, bound):
    """Worst |got - ref| / bound over the elements with the index of the worst one.  A zero bound demands equality.  Where
    the reference is not finite `got` must be of the same class, and that is all; where it is finite `got` must be.  NaN in
    a bound that is used fails closed."""
    got = np.asarray(got)
    ref = np.asarray(ref)
    wide = np.clongdouble if np.iscomplexobj(ref) or np.iscomplexobj(got) else LD
    g = got.astype(wide)
    bound = np.broadcast_to(np.asarray(bound, LD), ref.shape)
    fin = np.isfinite(ref)

    def cls(x):
        parts = (x.real, x.imag) if np.iscomplexobj(x) else (x,)
        return [np.where(np.isnan(p), 2, np.where(np.isposinf(p), 1, np.where(np.isneginf(p), -1, 0))) for p in parts]

    same = np.ones(ref.shape, bool)
    for a, b in zip(cls(g), cls(ref.astype(wide))):
        same &= a == b
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.abs(np.where(fin, g, 0) - np.where(fin, ref, 0))
        fr = np.where(bound > 0, d / np.where(bound > 0, bound, 1), np.where(d > 0, np.inf, 0))
        fr = np.where(np.isnan(bound) | ~np.isfinite(d), np.inf, fr)
    fr = np.where(fin, np.where(np.isfinite(g), fr, np.inf), np.where(same, 0.0, np.inf))
    at = np.unravel_index(int(np.argmax(fr)), fr.shape)
    return float(fr[at]), tuple(int(x) for x in at)


def judge(got, r, bounds, consts=None, per=None):
    """Worst fraction over the outputs the bounds name -> (fraction, output, index).  consts: the constant of each output
    (None: the bound at C = 1); per collects the worst fraction of each output."""
    worst = (0.0, None, ())
    for name, bd in bounds.items():
        c = 1.0 if consts is None else consts[name]
        fr, at = fraction(got[name], r[name], c * bd)
        if per is not None:
            per[name] = max(per.get(name, 0.0), fr)
        if worst[1] is None or fr > worst[0]:
            worst = (fr, name, at)
    return worst
