"""The error bound the particle-mesh kernels are held to, per cell of the density and per particle of the adjoint
gather (tests/test_pm_bounds.py shows that restatements of the kernels' arithmetic meet it and that wrong ones do not,
tests/test_gpu_particle_mesh.py applies it to the kernels; tests/pm_reference.py supplies the exact sums).

Density.  Cell c receives W(q_pc) w_norm from each of its cnt_c particles, S_c being the exact sum.  A storage-type
evaluation (unit round-off u_T) differs from it by

  * the arithmetic of one weight: a few u_T relative.  Where W itself cancels (t = 2 - q -> 0) the error is that of q,
    covered by the next item;
  * the coordinates.  cc + i d and x - (...) are numbers of the size of the box, each rounded once: <= u_T L = u_T n d
    absolute per operation, a shift of q by about u_T n d / h, and |dW/dq| <= w_norm (its maximum, at q = 2/3, is
    exactly w_norm);
  * the additions that land on the cell.  The order of atomic adds is not the kernel's to choose, so the bound takes
    the worst serial order: every one of the cnt_c additions may lose u_T of the running sum, which never exceeds S_c
    (all terms are >= 0).  a_c = 4 + cnt_c: four roundings for the weight (W_4 has three or four operations after q), one
    per addition.  (The other candidate, 1 + log2(1 + cnt_c), is what a pairwise tree guarantees, and no kernel here
    sums in a tree; at cnt_c = 1 .. 30, where almost every cell of every set lives, the two differ by less than the
    coordinate term.)

      |rho^_c - rho_c|  <=  C u_T ( a_c S_c + (n d / h) w_norm cnt_c )                                            (1)

  NGP / CIC / TSC: the same with w_norm -> 1 and h -> d (the weights are polynomials of x / d with |slope| <= 1).
  cnt_c counts the particles with q <= 2 + q_slack: one within the coordinate shift of the cut-off may land on either
  side of it.  A cell with cnt_c = 0 must be exactly 0.
  fp32 handles accumulate in double in LDS and flush floats: fewer float additions than a_c allows; the double
  accumulation adds cnt_c 2^-53 S_c.  Deterministic handles round every contribution to a multiple of 2^-46 w_norm
  (common.hpp: llrint(v 2^46 / w_norm)) before exact integer adds: + cnt_c 2^-46 w_norm, not multiplied by C (it is an
  exact statement about llrint), and then convert once.

Gather.  V_p,e = F sum_c pl_c g(q) x_e with F = rho_c d^3 (and 1 + f1 on z under RSD), g = dW/dq / q / (pi h^4) in h
units.  |g| + q |dg/dq| = 3 / (pi h^4) for q <= 1 and 3 (2 - q) / q / (pi h^4) <= that beyond, so a shift of the
coordinates by u_T n d / h changes one term by at most 3 / (pi h^4) |pl_c| u_T n d / h.  The terms have both signs: the
in-thread sum of the m_p stencil cells loses at most u_T of sum |term| per addition.

      |V^_p,e - V_p,e|  <=  C u_T ( (4 + m_p) A_p,e + (n d / h) 3 / (pi h^4) P_p )                                 (2)

  A_p,e = F sum_c |pl_c g x_e|, P_p = F sum |pl_c| over the cells with q <= 2 + q_slack, m_p their number.  A particle
  with no such cell, or with a non-finite position, must get exactly 0.

C is measured, not chosen: tests/test_pm_bounds.py evaluates numpy restatements of the generic tile kernels and of the
unrolled 81-cell kernels (float32 and float64, every operation rounded, no fused multiply-add) on every position set at
n = 16 and 32 and finds the worst fraction of (1) and of (2) with C = 1, recorded in MEASURED below: 0.048 of (1)
(float64, the generic kernel on the mixed set at 16^3; float32 0.026) and 0.50 of (2) (float64, one impulse of
part_like seen from uniform positions at h = 1.0599 d: V is then a single term, nothing averages, and x / h of a particle
far from the origin carries half an ulp of a number of size n; float32 0.43; white part_like stays below 0.18);
NGP / CIC / TSC as k_scatter_tile_low evaluates them reach 0.54 of (1) in
float64 (CIC, 32^3: x / d is a number of size n rounded once, and the weights have slope 1) and 0.027 in float32
(the arithmetic stays in double there).  Every C is its own figure times 4.
The margin of 4 covers what the restatement does not do: the GPU's fused multiply-adds, the hardware rsq seed (results
within 2 ulp of the correctly rounded 1 / sqrt; that figure is the comment in common.hpp next to fast_rsqrt / sqrt_rsq,
scripts/rsq_accuracy.hip measures it and has not been re-run for this file) and the order of the atomics -- the same
margin for the same reason as tests/fft_bound.py.
"""
import numpy as np

# worst fraction of (1) / (2) at C = 1 reached by the restatements (tests/test_pm_bounds.py asserts that these are not
# exceeded and that every C is four times its figure).  One constant per inequality, kernel class and storage type:
# "low" is (1) for NGP / CIC / TSC, whose float32 handles do their arithmetic in double and round once per weight.
MEASURED = {"scatter": {"float32": 0.026, "float64": 0.048}, "gather": {"float32": 0.43, "float64": 0.50},
            "low": {"float32": 0.027, "float64": 0.54}}
MARGIN = 4.0
C = {kind: {t: MARGIN * f for t, f in per_type.items()} for kind, per_type in MEASURED.items()}


def constant(kind, dtype):
    return C[kind][np.dtype(dtype).name]


Q_SLACK_ULPS = 8.0  # q_slack = 8 u_T n d / h: three coordinate roundings per axis, and the sqrt

UNIT_ROUNDOFF = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
LD = np.longdouble


def unit_roundoff(dtype):
    return UNIT_ROUNDOFF[np.dtype(dtype)]


def q_slack(dtype, n, d_over_h):
    return Q_SLACK_ULPS * unit_roundoff(dtype) * n * d_over_h


def density_bound(S, cnt, dtype, n, d_over_h, w_norm, deterministic=False, c=None, kind="scatter"):
    """Right-hand side of (1) per cell (longdouble).  For NGP / CIC / TSC pass d_over_h = 1, w_norm = 1, kind="low"."""
    c = constant(kind, dtype) if c is None else c
    u = LD(unit_roundoff(dtype))
    S = np.asarray(S, dtype=LD)
    cnt = np.asarray(cnt).astype(LD)
    b = c * u * ((4 + cnt) * S + LD(n) * LD(d_over_h) * LD(w_norm) * cnt)
    if np.dtype(dtype) == np.dtype(np.float32):
        b = b + cnt * LD(2.0 ** -53) * S
    if deterministic:
        b = b + cnt * LD(2.0 ** -46) * LD(w_norm)
    return b


def gather_bound(A, P, ncell, dtype, n, d_over_h, norm, zfac=1.0, c=None):
    """Right-hand side of (2), shape (3, N).  norm = 1 / (pi h^4); zfac = 1 + f1 under RSD (P carries rho_c d^3 only)."""
    c = constant("gather", dtype) if c is None else c
    u = LD(unit_roundoff(dtype))
    A = np.asarray(A, dtype=LD)
    coord = LD(n) * LD(d_over_h) * 3 * LD(norm) * np.asarray(P, dtype=LD)
    b = c * u * ((4 + np.asarray(ncell).astype(LD))[None, :] * A + coord[None, :] * np.array([1, 1, zfac], dtype=LD)[:, None])
    return b


def worst_fraction(got, ref, bound):
    """max |got - ref| / bound, with 0 / 0 = 0 and anything / 0 = inf (a term that must be exactly zero); NaN or inf in
    `got` gives inf.  Returns (fraction, flat index of the worst element)."""
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        bad = np.flatnonzero(~np.isfinite(got.ravel()))
        return np.inf, int(bad[0])
    err = np.abs(got.astype(LD) - np.asarray(ref, dtype=LD)).ravel()
    bound = np.asarray(bound, dtype=LD).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    i = int(np.argmax(f))
    return float(f[i]), i
