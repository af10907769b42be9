"""The error bounds bchmc_tweb_classify is held to (tests/test_tweb_bounds.py shows that they hold for the float64
restatement and that they can fail, tests/test_gpu_tweb.py applies them to the HIP kernels).

Tensor stage.  A component is  C2R[ f x^ ],  f = (k_a k_b / k^2) W / N with |N f| <= 1,  x^ = R2C[x]  (every source has
one R2C behind it: a host field and deltaX in the call, the chain state in bchmc_chain_set_state).  tests/fft_bound.py
bounds one pass over columns of length n by  C log2(n) u_T ||y||_2  per column, so a pass over the whole array by the
same multiple of the array's 2-norm, and a 3-D transform, three passes, by  3 C log2(n) u_T  times it (to first order;
the transforms are unitary up to the scalings folded into f).  With u_T the unit round-off of the handle's storage type:

    rounding of x to T                         u_T ||x||_2
    R2C, its error filtered by |N f| <= 1      3 C log2(n) u_T ||x||_2
    the multiply: f in double (k_a k_b / k^2, exp and 1 / N: a few u_64 each, MULT_U64 together) and one rounding of the
    product to T                               (1 + MULT_U64 u_64 / u_T) u_T ||T_ab||_2
    C2R and the rounding of its output         (3 C log2(n) + 1) u_T ||T_ab||_2

and  max |T_dev - T| <= ||T_dev - T||_2  <=  the sum.  tensor_bound returns it per component; it is applied to the largest
element error.  C is fft_bound.C, kept as it is.

Eigen stage.  k_tweb_eigen runs cyclic Jacobi: SWEEPS sweeps of 3 rotations.  A rotation replaces A by J^T A J with a
computed J; by the standard analysis of plane rotations (Higham, Accuracy and Stability of Numerical Algorithms, 2nd
ed., Lemma 19.8 and section 19.6: fl(J^T A J) = Q^T (A + E) Q with Q exactly orthogonal) the backward error of one
two-sided rotation is at most  2 * 6 sqrt(2) u ||A||_F < 16 eps ||A||_F  with eps = 2 u = 2^-52 -- generous by a factor of
two, which also covers the short forms a_pp - t a_pq, a_qq + t a_pq in place of the full products and setting a_pq to
zero.  Orthogonal similarities keep ||A||_F, so the errors add:  C_ROT * 3 * SWEEPS eps ||T||_F.  A sweep is not started
once off(A) <= eps ||A||_F: dropping the off-diagonal part then perturbs A by ||E||_F = sqrt(2) off(A) < C_EXIT eps ||A||_F.
The power-of-two scaling is exact.  After the last sweep the off-diagonal part still there is dropped unseen: Jacobi
converges quadratically, and over 1.2 10^7 tensors (Gaussian entries; small diagonals; small off-diagonals; nearly equal
diagonals; entries spread over six decades; the degenerate set) the restatement is within 10 eps ||T||_F after four
sweeps and off by up to 3.3 10^6 eps ||T||_F after three, which is why SWEEPS is 4 and what the test with one sweep
too few shows.  The reference, numpy.linalg.eigvalsh (LAPACK's tridiagonal reduction and QL / divide and conquer), is
backward stable too, with  p(3) eps ||T||_2  and a modest p: C_EIGVALSH = 32.  Eigenvalues of a symmetric matrix move by
at most ||E||_2 <= ||E||_F under a perturbation E (Weyl), so per cell

    |lambda_dev - lambda_ref|  <=  (C_ROT * 3 * SWEEPS + C_EXIT + C_EIGVALSH) eps ||T||_F  =  C_EIGEN eps ||T||_F.

A cell is UNDECIDED when some |lambda_i - lambda_th| is within the sum of the eigen bound and the shift a tensor error
at its bound can cause, ||dT||_F <= sqrt(b_xx^2 + b_yy^2 + b_zz^2 + 2 (b_xy^2 + b_xz^2 + b_yz^2)); types are compared on
decided cells only.

Masses.  The device sums 1 + x over a type's cells in double, M terms in some fixed order: within
M u_64 sum |1 + x| of the exact sum (Higham, section 4.2).  A host source is summed from the caller's doubles; the chain
state's x has an R2C and a C2R behind it, each bounded as above, and sum |dx| <= sqrt(N) ||dx||_2.  mass_bound applies the
round-trip term to every source but the host one.
"""
import numpy as np

from tests import fft_bound
from tests.tweb_reference import EPS64, SWEEPS

C_ROT = 16.0
C_EXIT = 2.0
C_EIGVALSH = 32.0
C_EIGEN = C_ROT * 3 * SWEEPS + C_EXIT + C_EIGVALSH
MULT_U64 = 16.0
UNDECIDED_CAP = 0.01


def frobenius(t6):
    """||T||_F per cell of six components (6, ...)."""
    t6 = np.asarray(t6, dtype=np.float64)
    with np.errstate(over="ignore"):
        m = np.max(np.abs(t6), axis=0)
        s = np.where(m > 0, m, 1.0)
        r = t6 / s
        return s * np.sqrt(r[0] ** 2 + r[3] ** 2 + r[5] ** 2 + 2.0 * (r[1] ** 2 + r[2] ** 2 + r[4] ** 2)) * (m > 0)


def eigen_bound(t6):
    return C_EIGEN * EPS64 * frobenius(t6)


def _pass3(n):
    return 3.0 * fft_bound.C * np.log2(n)


def tensor_bound(x, t_ref, dtype):
    """Largest allowed |T_dev - T| of each component: six numbers.  x: the source (n, n, n); t_ref: the reference
    tensor (6, n, n, n); dtype: the handle's storage type."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    u = fft_bound.unit_roundoff(dtype)
    u64 = fft_bound.unit_roundoff(np.float64)
    xn = float(np.sqrt(np.sum(x ** 2)))
    tn = np.sqrt(np.sum(np.asarray(t_ref, dtype=np.float64).reshape(6, -1) ** 2, axis=1))
    return u * ((1.0 + _pass3(n)) * xn + (2.0 + MULT_U64 * u64 / u + _pass3(n)) * tn)


def tensor_shift(b6):
    """The eigenvalue shift a tensor error at its bound b6 (six numbers) can cause."""
    b = np.asarray(b6, dtype=np.float64)
    return float(np.sqrt(b[0] ** 2 + b[3] ** 2 + b[5] ** 2 + 2.0 * (b[1] ** 2 + b[2] ** 2 + b[4] ** 2)))


def undecided(lam, lambda_th, margin):
    """Cells where some eigenvalue is within `margin` (a number or per cell) of the threshold."""
    return np.any(np.abs(np.asarray(lam) - lambda_th) <= margin, axis=0)


def mass_bound(x, cells, dtype, host_source):
    """Largest allowed error of a per-type mass: x the source, cells the boolean map of the type's cells."""
    x = np.asarray(x, dtype=np.float64).ravel()
    cells = np.asarray(cells).ravel()
    n = round(x.size ** (1.0 / 3.0))
    u64 = fft_bound.unit_roundoff(np.float64)
    b = np.count_nonzero(cells) * u64 * float(np.sum(np.abs(1.0 + x[cells])))
    if not host_source:
        u = fft_bound.unit_roundoff(dtype)
        b += np.sqrt(x.size) * u * (2.0 * _pass3(n) + 2.0) * float(np.sqrt(np.sum(x ** 2)))
    return b
