"""The error bounds bchmc_bispectrum is held to (tests/test_bispec_bounds.py shows that they hold for the float64
restatement against the enumerated definition and that they can fail, tests/test_gpu_bispec.py applies them to the HIP
kernels).  Nothing here is chosen: every term is the unit round-off of a number format times a norm, with the constant
of tests/fft_bound.py (fft_bound.C, kept as it is) for a transform pass.

Shell fields.  D_s = C2R[x^ 1_s] with x^ = R2C[x] (every source has one R2C behind it: a host field and deltaX in the
call, the chain state in bchmc_chain_set_state).  As in tests/tweb_bound.py a 3-D transform is three passes, each bounded
by  C log2(n) u_T  times the 2-norm of its input, and the filter has |1_s| <= 1 and is a selection, not a multiplication.
With d_s = D_s / N the normalised shell field and u_T the unit round-off of the handle's storage type:

    rounding of x to T                          u_T ||x||_2
    R2C, its error filtered by |1_s| <= 1       3 C log2(n) u_T ||x||_2
    C2R and the rounding of its output          (3 C log2(n) + 1) u_T ||d_s||_2

    ||dD_s||_2  <=  N u_T (1 + 3 C log2(n)) (||x||_2 + ||d_s||_2)                                  (shell_field_bound)

I_s = C2R[1_s] has exact input (zeros and ones):  ||dI_s||_2 <= u_T (1 + 3 C log2(n)) ||I_s||_2,  ||I_s||_2 = sqrt(N nmode_s).

Sums.  S = sum over cells of D_1 D_2 D_3, products and sum in double.  The product of the three computed fields is
expanded in full -- not to first order: a shell that holds no power has D_s = 0 and the first-order terms of its triplets
vanish, while the device's D_s is round-off and its triplets are products of two or three errors:

    |dS|  <=  E + N u_64 (sum |D_1 D_2 D_3| + E),
    E  =    sum over the factors a of        ||dD_a||_2 ||D_b D_c||_2
          + sum over the pairs a < b of      ||dD_a||_2 ||dD_b||_2 ||D_c||_2
          +                                  ||dD_1||_2 ||dD_2||_2 ||dD_3||_2                              (sum_bound)

(Cauchy-Schwarz, with max |v| <= ||v||_2 for the third factor of the higher terms; N terms added in some fixed order,
Higham section 4.2; the two roundings of a product are inside the N >= 64 of that term.)  The same with I for the
triangle sum  SI = sum I_1 I_2 I_3 = N ntri.

Normalisation.  B = (L^6 / N^3) S / SI: the quotient of two numbers with the errors above and NORM_U64 roundings of its
own (L^3, its square, N^3, the division by N ntri, the product):

    |dB|  <=  (L^6 / N^3) ( dS / |SI| + |S| dSI / SI^2 )  +  NORM_U64 u_64 |B|                              (b_bound)

The bound of a reference computed in float64 (the restatement, where the enumeration is out of reach) is this bound
with T = float64; a comparison of the device with it adds the two.

ntri.  |d ntri| <= dSI / N; rint(ntri) is the exact count where that is below 1/2.

Power.  power = NORM sum hw |x^|^2 / nmode.  The computed x^ has a 2-norm error  e = (1 + 3 C log2(n)) u_T ||x^||_2
(full-grid norms; rounding of x and the R2C), and | |x^ + d|^2 - |x^|^2 | <= 2 |x^| |d| + |d|^2, again in full: a shell
without power has only the second term.  By Cauchy-Schwarz over the shell's modes the sum is within
2 ||x^ 1_s||_2 e + e^2, plus nmode u_64 times itself for the summation.                                  (power_bound)
"""
import numpy as np

from tests import fft_bound

NORM_U64 = 8.0


def _pass3(n):
    return 3.0 * fft_bound.C * np.log2(n)


def _norm(a):
    return float(np.sqrt(np.sum(np.asarray(a, dtype=np.float64) ** 2)))


def shell_field_bound(x, D, dtype):
    """||dD_s||_2 per shell: x the source (n, n, n), D the reference shell fields (n_shell, n, n, n), unnormalised."""
    n = x.shape[0]
    N = float(n) ** 3
    u = fft_bound.unit_roundoff(dtype)
    xn = _norm(x)
    return np.array([N * u * (1.0 + _pass3(n)) * (xn + _norm(d) / N) for d in D])


def indicator_field_bound(I, dtype):
    n = I.shape[1]
    u = fft_bound.unit_roundoff(dtype)
    return np.array([u * (1.0 + _pass3(n)) * _norm(i) for i in I])


def sum_bound(F, dF, trip):
    """|d sum F_1 F_2 F_3| per triplet: F the fields (n_shell, ...), dF their 2-norm error bounds."""
    u64 = fft_bound.unit_roundoff(np.float64)
    N = float(F[0].size)
    out = np.empty(len(trip))
    for t, (a, b, c) in enumerate(trip):
        fa, fb, fc = F[a], F[b], F[c]
        e = (dF[a] * _norm(fb * fc) + dF[b] * _norm(fa * fc) + dF[c] * _norm(fa * fb)
             + dF[a] * dF[b] * _norm(fc) + dF[a] * dF[c] * _norm(fb) + dF[b] * dF[c] * _norm(fa) + dF[a] * dF[b] * dF[c])
        out[t] = e + N * u64 * (float(np.sum(np.abs(fa * fb * fc))) + e)
    return out


def bounds(x, L, ref, dtype):
    """The allowed errors of one call on field x against the exact values: dict of ``b`` (T,), ``ntri`` (T,), ``power``
    (n_shell,).  ref: tests/bispec_reference.restatement(x, ...) -- its fields D, I, its sums and counts serve as the
    norms (the bounds are first-order, so a float64 stand-in for the exact fields changes them by u_64)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    N = float(n) ** 3
    u = fft_bound.unit_roundoff(dtype)
    u64 = fft_bound.unit_roundoff(np.float64)
    trip = ref["triplets"]
    D, I = ref["D"], ref["I"]
    dS = sum_bound(D, shell_field_bound(x, D, dtype), trip)
    dSI = sum_bound(I, indicator_field_bound(I, dtype), trip)
    SI = N * np.asarray(ref["ntri"], dtype=np.float64)
    S = np.asarray(ref["s"], dtype=np.float64)
    filled = ref["computed"] & (SI >= 0.5 * N)
    safe = np.where(filled, SI, 1.0)
    norm = float(L) ** 6 / N ** 3
    db = np.where(filled, norm * (dS / safe + np.abs(S) * dSI / safe ** 2) + NORM_U64 * u64 * np.abs(ref["b"]), 0.0)
    # power: full-grid norms of x^ and of its part in the shell; ||x^||_2 = sqrt(N) ||x||_2, ||x^ 1_s||_2 = ||D_s||_2 / sqrt(N)
    pn = float(L) ** 3 / N / N
    nm = np.asarray(ref["nmode"], dtype=np.float64)
    e = (1.0 + _pass3(n)) * u * np.sqrt(N) * _norm(x)
    dpow = np.array([pn / max(m, 1.0) * (2.0 * _norm(d) / np.sqrt(N) * e + e * e) for d, m in zip(D, nm)])
    dpow = dpow + (nm + NORM_U64) * u64 * np.abs(ref["power"])
    # kmean = sum hw |k| / nmode: two sums of at most nmode terms in double (the device's and the reference's), a
    # division and the rounding of |k| itself on each side
    dkm = (2.0 * nm + 4.0) * u64 * np.asarray(ref["kmean"], dtype=np.float64)
    return dict(b=db, ntri=np.where(ref["computed"], dSI / N, 0.0), power=dpow, kmean=dkm, s=dS)


def fraction(err, bound):
    """max err / bound; where the bound is 0 the error must be 0."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r))
