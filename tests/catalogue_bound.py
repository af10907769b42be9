"""The error bound bchmc_density_particles is held to, per cell: inequality (1) of tests/pm_bound.py with weights.

Cell c receives w_p W_pc from each of its cnt_c particles (tests/catalogue_reference.py: S_c the signed sum, A_c the sum
of |w_p W_pc|, M_c the sum of |w_p|).  The three error sources of pm_bound's derivation carry over term by term:

  * the arithmetic of one contribution, a few u_T relative to |w_p W_pc|, and one rounding per addition that lands on the
    cell.  The terms have both signs now, so the running sum is bounded by A_c, not by S_c: (4 + cnt_c) A_c;
  * the coordinates: a shift of q by about u_T n d / h, |dW/dq| <= w_norm, times the particle's |w_p|:
    (n d / h) w_norm M_c (w_norm -> 1, h -> d for NGP / CIC / TSC);
  * nothing else.

      |rho^_c - S_c|  <=  C u_T ( (4 + cnt_c) A_c + (n d / h) w_norm M_c )                                         (1w)

  + cnt_c 2^-53 A_c on fp32 handles (the accumulation in double);
  + cnt_c 2^-46 w_norm max|w| on deterministic handles: every contribution is rounded to a multiple of
    2^-46 max|w| w_norm (an exact statement about llrint, not multiplied by C) before exact integer adds.
A cell with cnt_c = 0 must be exactly 0.  With unit weights A_c = S_c and M_c = cnt_c: the bound IS
pm_bound.density_bound at the same C, bit for bit (tests/test_catalogue_bounds.py asserts it).

C is measured the way pm_bound's is: tests/test_catalogue_bounds.py evaluates numpy restatements of cat_deposit
(barcode_amd/csrc/catalogue.hpp; SPH at h = d as the 81-cell hull form with the folded spline, other h as the cube)
-- the storage type's positions, double arithmetic with every operation rounded and no
fused multiply-add, the CIC / TSC products rounded to the storage type, serial double accumulation -- on every catalogue
of tests/catalogue_reference.catalogue_sets at n = 16, and records the worst fraction of (1w) at C = 1 in MEASURED below.
Where a figure does not exceed pm_bound.MEASURED of the same class, that class's constant is REUSED (C = 4 x pm_bound's
figure); where it does, C is 4 x the figure measured here.  The margin and its reason are pm_bound's: FMA contraction and
the order of the atomics (the catalogue kernels take IEEE sqrt and divide, no rsq seed).
  low     float64 0.39 (TSC, the faces set) <= 0.54: reused.  float32 0.12 > 0.027: own.  The faces set has a particle at
          x == min + L, which upstream's TSC keeps in cell 0 at distance n - 1/2 from its centre: a weight of -240 per
          axis, rounded to float once -- half an ulp of a term that IS A_c, where pm_bound's lattice sets have weights
          below 1 beside a coordinate term of size n.
  scatter float32 below 1e-4 (the SPH arithmetic stays in double on fp32 handles) <= 0.026: reused.  float64 0.16 (h =
          1.3 d, the sparse set: a cell reached by one particle) > 0.048: own.
"""
import numpy as np

from tests import pm_bound

LD = np.longdouble

# worst fraction of (1w) at C = 1 reached by the restatements of tests/test_catalogue_bounds.py, per kernel class of
# pm_bound ("scatter": SPH, "low": NGP / CIC / TSC) and storage type.  The test asserts that none is exceeded and that
# every C is pm_bound's where the figure allows it and four times the figure where not.
MEASURED = {"scatter": {"float32": 1e-4, "float64": 0.16}, "low": {"float32": 0.12, "float64": 0.39}}
C = {kind: {t: pm_bound.MARGIN * f if f > pm_bound.MEASURED[kind][t]
            else pm_bound.C[kind][t] for t, f in per_type.items()} for kind, per_type in MEASURED.items()}


def kind_of(mk):
    return "scatter" if mk == 3 else "low"


def constant(mk, dtype):
    return C[kind_of(mk)][np.dtype(dtype).name]


def density_bound(ref, mk, dtype, n, d_over_h=1.0, w_norm=1.0, max_w=1.0, deterministic=False, c=None):
    """Right-hand side of (1w) per cell (longdouble).  ref: a catalogue_reference.Density.  For NGP / CIC / TSC leave
    d_over_h = w_norm = 1."""
    c = constant(mk, dtype) if c is None else c
    u = LD(pm_bound.unit_roundoff(dtype))
    A = np.asarray(ref.A, dtype=LD)
    M = np.asarray(ref.M, dtype=LD)
    cnt = np.asarray(ref.cnt).astype(LD)
    b = c * u * ((4 + cnt) * A + LD(n) * LD(d_over_h) * LD(w_norm) * M)
    if np.dtype(dtype) == np.dtype(np.float32):
        b = b + cnt * LD(2.0 ** -53) * A
    if deterministic:
        b = b + cnt * LD(2.0 ** -46) * LD(w_norm) * LD(max_w)
    return b


worst_fraction = pm_bound.worst_fraction
q_slack = pm_bound.q_slack
