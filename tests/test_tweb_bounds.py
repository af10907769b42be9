"""The T-web's definition, bounds and bindings without a GPU: the numpy reference obeys the identities and the known
answers of include/bchmc.h (T1-T6), the bounds of tests/tweb_bound.py hold for the float64 restatement of k_tweb_eigen's
solver on random and on degenerate tensors, three wrong variants each miss a bound or a known answer, and the seeded
fields of tests/test_gpu_tweb.py leave at most 1 % of their cells undecided."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import tweb_bound as tb
from tests import tweb_reference as tr

GRIDS = (4, 5, 8, 9, 16)


def cells_of(n):
    return 2.0 * tr.box_of(n) / n


@pytest.mark.parametrize("n", GRIDS)
@pytest.mark.parametrize("cells", (0.0, 2.0))
def test_reference_is_real_and_obeys_the_trace_identity(n, cells):
    """With the Nyquist rule the six inverse FULL-complex transforms are real to round-off (T3), and the trace is the
    smoothed field minus its mean (T4); so is the sum of the eigenvalues."""
    x = tr.field(n)
    L = tr.box_of(n)
    t, xs, imag = tr.tensor(x, L, cells * L / n)
    scale = float(np.max(np.abs(x)))
    assert imag <= 1e-14 * scale
    want = xs - np.mean(xs)
    assert np.max(np.abs(t[0] + t[3] + t[5] - want)) <= 1e-13 * scale
    assert np.max(np.abs(np.sum(tr.eigenvalues(t), axis=0) - want)) <= 1e-13 * scale
    if cells == 0.0:
        assert np.max(np.abs(xs - x)) <= 1e-13 * scale


def test_dropping_the_nyquist_rule_leaves_a_complex_tensor():
    """Mutant: without the rule the off-diagonal components of an even grid are not transforms of real fields."""
    x = tr.field(16)
    t, _, imag = tr.tensor(x, tr.box_of(16), 0.0, nyquist_rule=False)
    assert imag > 1e-3 * float(np.max(np.abs(t)))
    assert tr.tensor(tr.field(9), tr.box_of(9), 0.0, nyquist_rule=False)[2] <= 1e-14 * 10  # odd n: nothing to drop


@pytest.mark.parametrize("n", (4, 5, 8, 9, 16))
def test_reference_known_answers_plane_waves(n):
    """x = A cos(2 pi m i / n) along one axis: T_aa = x, every other component 0, eigenvalues (x, 0, 0) sorted, types 0
    and 1 only at lambda_th = 0.25 A.  m = 1 and, at even n, the Nyquist wave m = n / 2."""
    A, L = 1.5, tr.box_of(n)
    for m in (1,) + ((n // 2,) if n % 2 == 0 else ()):
        for axis in range(3):
            x = tr.plane_wave(n, (axis,), m, A)
            t, _, _ = tr.tensor(x, L, 0.0)
            diag = (0, 3, 5)[axis]
            for c in range(6):
                assert np.max(np.abs(t[c] - (x if c == diag else 0.0))) <= 1e-13 * A
            lam = tr.eigenvalues(t)
            want = np.sort(np.stack([x, 0 * x, 0 * x]), axis=0)[::-1]
            assert np.max(np.abs(lam - want)) <= 1e-13 * A
            assert set(np.unique(tr.web_type(lam, 0.25 * A))) <= {0, 1}


def test_reference_known_answer_diagonal_wave_and_three_waves():
    """The wave along (1, 1, 0): T_xy = T_xx = T_yy = x / 2 (sign and indexing of an off-diagonal component).  Three
    waves along the three axes at n = 16: T is the diagonal of the three terms and all four types occur."""
    n, A, L = 16, 1.0, tr.box_of(16)
    x = tr.plane_wave(n, (0, 1), 1, A)
    t, _, _ = tr.tensor(x, L, 0.0)
    for c, want in enumerate((x / 2, x / 2, 0 * x, x / 2, 0 * x, 0 * x)):
        assert np.max(np.abs(t[c] - want)) <= 1e-13
    terms = [tr.plane_wave(n, (0,), 1, A), tr.plane_wave(n, (1,), 2, A), tr.plane_wave(n, (2,), 3, A)]
    t, _, _ = tr.tensor(sum(terms), L, 0.0)
    for c, want in zip((0, 3, 5), terms):
        assert np.max(np.abs(t[c] - want)) <= 1e-13
    types = tr.web_type(np.sort(np.stack(terms), axis=0)[::-1], 0.25 * A)
    assert set(np.unique(types)) == {0, 1, 2, 3}
    assert np.array_equal(tr.web_type(tr.eigenvalues(t), 0.25 * A), types)


@pytest.mark.parametrize("n", (8, 9))
def test_tensor_bound_holds_for_float64_transforms(n):
    x = tr.field(n)
    L = tr.box_of(n)
    for R in (0.0, cells_of(n)):
        ref = tr.tensor_longdouble(x, L, R)
        t, _, _ = tr.tensor(x, L, R)
        b = tb.tensor_bound(x, ref, np.float64)
        err = np.max(np.abs(t - ref).reshape(6, -1), axis=1).astype(np.float64)
        assert np.all(err <= b), (err, b)
        # and it bites: the transform of the field rounded to float32 misses the float64 bound
        t32, _, _ = tr.tensor(x.astype(np.float32), L, R)
        assert np.any(np.max(np.abs(t32 - ref).reshape(6, -1), axis=1) > b)


@functools.lru_cache(maxsize=None)
def tensor_sets():
    rng = np.random.Generator(np.random.Philox(11))
    rand = rng.standard_normal((6, 200000))
    deg, lam = tr.degenerate_set(rng)
    return rand, deg, lam


def ratio(lam, ref, t6):
    """max |lam - ref| / eigen bound; a zero tensor must give zeros."""
    b = tb.eigen_bound(t6)
    d = np.max(np.abs(lam - ref), axis=0)
    return float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1), np.where(d > 0, np.inf, 0))))


def test_eigen_bound_holds_for_the_restated_solver():
    rand, deg, lam_known = tensor_sets()
    assert ratio(tr.jacobi_eigenvalues(rand), tr.eigenvalues(rand), rand) <= 1.0
    assert ratio(tr.jacobi_eigenvalues(deg), tr.eigenvalues(deg), deg) <= 1.0
    # against the eigenvalues the set was built from (the rotation into general position rounds: a few eps |T|_F)
    assert ratio(tr.jacobi_eigenvalues(deg), lam_known, deg) <= 1.0 + 16.0 / tb.C_EIGEN
    zero = np.zeros((6, 3))
    assert np.array_equal(tr.jacobi_eigenvalues(zero), np.zeros((3, 3)))


def test_diagonal_tensors_come_back_exactly():
    rng = np.random.Generator(np.random.Philox(12))
    d = rng.standard_normal((3, 1000)) * 10.0 ** rng.uniform(-100, 100, (1, 1000))
    t = np.zeros((6, 1000))
    t[0], t[3], t[5] = d
    assert np.array_equal(tr.jacobi_eigenvalues(t), np.sort(d, axis=0)[::-1])


def test_acos_closed_form_misses_the_bound_on_degenerate_tensors():
    """Mutant: d phi ~ sqrt(eps) at r = +-1, half the digits."""
    _, deg, _ = tensor_sets()
    assert ratio(tr.acos_eigenvalues(deg), tr.eigenvalues(deg), deg) > 1e3


def test_one_sweep_too_few_misses_the_bound():
    """Mutant: three sweeps leave off-diagonal elements that the bound does not cover."""
    rand, _, _ = tensor_sets()
    assert ratio(tr.jacobi_eigenvalues(rand, sweeps=tr.SWEEPS - 1), tr.eigenvalues(rand), rand) > 10.0


@pytest.mark.parametrize("n", GRIDS + (32,))
@pytest.mark.parametrize("cells", (0.0, 2.0))
def test_seeded_fields_leave_few_cells_undecided(n, cells):
    """The fields of tests/test_gpu_tweb.py at the margin of an fp32 handle, the widest one: at most 1 % undecided."""
    x = tr.host_field(n, cells)
    L = tr.box_of(n)
    t, _, _ = tr.tensor(x, L, cells * L / n)
    lam = tr.eigenvalues(t)
    margin = tb.eigen_bound(t) + tb.tensor_shift(tb.tensor_bound(x, t, np.float32))
    und = tb.undecided(lam, 0.0, margin)
    assert np.count_nonzero(und) <= tb.UNDECIDED_CAP * und.size, np.count_nonzero(und)
    if n == 16:
        assert set(np.unique(tr.web_type(lam, 0.0))) == {0, 1, 2, 3}


@pytest.mark.parametrize("n", (9, 16))
def test_chain_and_deltax_sources_leave_few_cells_undecided(n):
    """The device sources of tests/test_gpu_tweb.py: the seeded case's initial state and the forward model of it."""
    from tests.util import Case
    c = Case(Nx=n, likelihood=1)
    L = c.p.L
    for x in (c.q0, c.oracle.Lag2Eul(c.q0)[0]):
        x = np.asarray(x).reshape((n,) * 3)
        for cells in (0.0, 2.0):
            t, _, _ = tr.tensor(x, L, cells * L / n)
            margin = tb.eigen_bound(t) + tb.tensor_shift(tb.tensor_bound(x, t, np.float32))
            und = tb.undecided(tr.eigenvalues(t), 0.0, margin)
            assert np.count_nonzero(und) <= tb.UNDECIDED_CAP * und.size, (cells, np.count_nonzero(und))


def test_library_exports_and_bindings():
    from barcode_amd import engine, hamil, io, shim
    names = ("bchmc_tweb_classify", "bchmc_tweb_tensor", "bchmc_tweb_samples", "bchmc_tweb_fetch", "bchmc_tweb_merge",
             "bchmc_tweb_reset", "bchmc_tweb_release")
    raw = C.CDLL(engine.LIB_PATH)
    for name in names:
        assert name in engine.EXPORTS and hasattr(raw, name)
    lib = engine.load()
    assert lib.bchmc_tweb_classify.argtypes and C.sizeof(engine.TwebOpts) == 24 and C.sizeof(engine.TwebStats) == 72
    # a NULL handle is refused without touching a device
    assert lib.bchmc_tweb_classify(None, 0, None, None, None, None, None) == 1
    assert lib.bchmc_tweb_tensor(None, 0, None) == 1 and lib.bchmc_tweb_release(None) == 1
    for fn in ("tweb_classify", "tweb_tensor", "tweb_samples", "tweb_fetch", "tweb_merge", "tweb_reset", "tweb_release"):
        assert callable(getattr(engine.Engine, fn))
    assert callable(hamil.tweb_classify) and callable(hamil.tweb_probability) and callable(io.dump_tweb)
    slib = shim.load()
    for name in ("bchmc_shim_tweb_classify", "bchmc_shim_tweb_probability"):
        assert name in shim.SHIM_EXPORTS and getattr(slib, name).argtypes
