"""The generic trajectory's real-space mass and GRF kernels cell by cell: k_div_mass_r, k_kin_rs, k_grf_grad, k_grf_loglike,
k_scale_c and k_add_r run alone through libbchmc_fft_probe.so (the engine's kernels on the engine's launch shapes:
barcode_amd/csrc/fft_probe.hip), each compared with the longdouble reference of tests/massrs_reference.py under the counted
bounds of tests/massrs_bound.py, on masses with zeros, negatives, NaN and infinities and on windows with holes; then the
entry points that reach these kernels against the oracle on such inputs.  tests/test_massrs_bounds.py shows on the CPU that
the checker rejects the plausible bugs (m >= 0, m != 0, fabs(m), no guard, the 0.5 dropped, 1 / m twice, w != 0, w as a factor,
sigma for sigma^2 and the reverse, a flipped sign, a sum without its second turn, idle blocks left unwritten).

Sizes: 1, 255, 256, 257 (the block edge), 729, 4096 (odd and even, several blocks), 2048 * 256 + 3 (past nblk_stride's cap of
2048 blocks: the grid-stride loop turns), and for the two sums 1024 * 256 + 3, where three threads of block 0 take a second
cell.  Below 1024 * 256 cells the sums leave blocks idle: their partials must come back exactly 0.

The momenta a draw leaves resident are fetched through a transform pair; after a draw for a real-space mass alone
bchmc_chain_get_momenta hands back exact zeros in the closed cells (k_zero_closed) for as long as the resident momenta are
that draw and mass_r is the array it was drawn with: test_philox_draw_on_a_mass_with_closed_cells and
test_fetched_zeros_belong_to_the_draw_alone.  Worst fractions per kernel: tests/massrs_bound.py::MEASURED.

Every cell is compared; nothing is excluded.  Output arrays go in filled with a pattern, the probe's canaries stand behind
every device array, and every check prints a line `MASSRS <kernel><type> <set>: worst fraction ... at element ...` before it
asserts <= 1.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import massrs_bound as mb
from tests import massrs_reference as ref
from tests.test_gpu_parity import TOL_F32_ENERGY, TOL_F32_FIELD, TOL_F32_TRAJ
from tests.util import TOL_ENERGY, TOL_FIELD, TOL_TRAJ_10, Case, rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "barcode_amd", "libbchmc_fft_probe.so")
PRECS = ["fp64", "fp32"]
FILL = mb.FILL


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the process-wide HIP runtime first, as barcode_amd.engine does)
    assert os.path.exists(PROBE), "%s not built (make -C barcode_amd/csrc)" % PROBE
    L = C.CDLL(PROBE)
    vp, i, ll, d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    L.fftp_div_mass_r.argtypes = [i, ll, vp, vp, vp]
    L.fftp_kin_rs.argtypes = [i, ll, vp, vp, vp]
    L.fftp_grf_grad.argtypes = [i, ll, vp, vp, vp, vp, vp]
    L.fftp_grf_loglike.argtypes = [i, ll, vp, vp, vp, vp, vp]
    L.fftp_scale_c.argtypes = [i, ll, vp, vp, d]
    L.fftp_add_r.argtypes = [i, ll, vp, vp, vp]
    assert L.fftp_parseval_blocks() == ref.RED_BLOCKS
    yield L
    oracle_run.cache_clear()
    mb.entry_case.cache_clear()


def ptr(a):
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


def check_status(st):
    if st == -2:   # nothing more runs on a device that has reported an error
        pytest.exit("HIP error in a probe call", returncode=3)
    assert st == 0, {-1: "arguments outside the probe's range"}.get(st, "canary after device array %d overwritten" % st)


def storage(prec):
    return np.dtype(np.float64 if prec == "fp64" else np.float32)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def report(kernel, prec, what, f, at):
    rec = mb.MEASURED[kernel][storage(prec).name]
    print("\nMASSRS %s<%s> %s: worst fraction %.4f at element %d (recorded over all sets: restatement %s, device %s)"
          % (kernel, prec, what, f, at, rec[0], rec[1]))
    assert f <= 1.0


# ---- per element through the probes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("count", mb.COUNTS)
def test_k_div_mass_r(lib, prec, count):
    """Out of place and in place (the engine's call, on iop): the same bits; closed cells (m <= 0, -0, NaN) exactly 0."""
    dt = storage(prec)
    p, m = mb.mass_inputs(count, dt)
    out = np.full(count, FILL, dt)
    check_status(lib.fftp_div_mass_r(PRECS.index(prec), count, ptr(p), ptr(m), ptr(out)))
    report("div_mass_r", prec, "count=%d" % count, *mb.check_div_mass_r(out, p, m, dt))
    assert np.all(out[~(m > 0)] == 0)
    buf = p.copy()
    check_status(lib.fftp_div_mass_r(PRECS.index(prec), count, ptr(buf), ptr(m), ptr(buf)))
    assert same_bits(buf, out), "in place differs from out of place"


def run_sum(lib, fn, prec, count, arrays):
    """Two calls into pattern-filled partials: bitwise equal (block sums without atomics), idle blocks exactly 0."""
    got = []
    for _ in range(2):
        part = np.full(ref.RED_BLOCKS, FILL)
        check_status(fn(PRECS.index(prec), count, *[ptr(a) for a in arrays], ptr(part)))
        got.append(part)
    assert same_bits(*got), "two calls differ"
    idle = ref.trips(count) == 0
    assert idle.any() == (count <= mb.FULL - ref.RED_THREADS) and np.all(got[0][idle] == 0)
    assert not same_bits(got[0][~idle], np.full(int((~idle).sum()), FILL)), "no block wrote"
    return got[0]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("count", mb.SUM_COUNTS)
def test_k_kin_rs(lib, prec, count):
    """Both sum sets: "confined" holds every edge and spoils one partial in four, "moderate" has finite terms only, so that
    its total is judged by value at every size."""
    for kind in mb.SUM_SETS:
        p, m = mb.mass_inputs(count, storage(prec), confined=kind)
        part = run_sum(lib, lib.fftp_kin_rs, prec, count, (p, m))
        report("kin_rs", prec, "%s count=%d (element 1024: the total)" % (kind, count), *mb.check_kin_rs(part, p, m))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("count", mb.SUM_COUNTS)
def test_k_grf_loglike(lib, prec, count):
    for kind in mb.SUM_SETS:
        a = mb.grf_inputs(count, storage(prec), confined=kind)
        part = run_sum(lib, lib.fftp_grf_loglike, prec, count, a)
        report("grf_loglike", prec, "%s count=%d (element 1024: the total)" % (kind, count), *mb.check_grf_loglike(part, *a))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("count", mb.COUNTS)
def test_k_grf_grad(lib, prec, count):
    dt = storage(prec)
    q, nobs, noise, w = mb.grf_inputs(count, dt)
    out = np.full(count, FILL, dt)
    check_status(lib.fftp_grf_grad(PRECS.index(prec), count, ptr(q), ptr(nobs), ptr(noise), ptr(w), ptr(out)))
    report("grf_grad", prec, "count=%d" % count, *mb.check_grf_grad(out, q, nobs, noise, w, dt))
    assert np.all(out[~(w > 0)] == 0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("count", mb.COUNTS)
def test_k_scale_c_and_k_add_r(lib, prec, count):
    dt = storage(prec)
    z, s = mb.scale_inputs(count, dt)
    out = np.full(count, FILL * (1 + 1j), z.dtype)
    check_status(lib.fftp_scale_c(PRECS.index(prec), count, ptr(z), ptr(out), s))
    report("scale_c", prec, "count=%d" % count, *mb.check_scale_c(out, z, s, dt))
    a, b = mb.add_inputs(count, dt)
    out = np.full(count, FILL, dt)
    check_status(lib.fftp_add_r(PRECS.index(prec), count, ptr(a), ptr(b), ptr(out)))
    report("add_r", prec, "count=%d" % count, *mb.check_add_r(out, a, b, dt))


# ---- the entry points against the oracle ------------------------------------------------------------------------------------
NEPS = 10


def tolerances(prec):
    """(trajectory, energy, field) of tests/test_gpu_parity.py for the handle's precision."""
    return (TOL_TRAJ_10, TOL_ENERGY, 10 * TOL_FIELD) if prec == "fp64" else (TOL_F32_TRAJ, TOL_F32_ENERGY, 10 * TOL_F32_FIELD)


@functools.lru_cache(maxsize=None)
def oracle_run(kind, n):
    """The oracle's side of a case, computed once for both precisions."""
    c = mb.entry_case(kind, n)
    q1, p1, done = c.oracle.Hamiltonian_EoM(c.q0, c.p0, c.eps, NEPS)
    dH, t = c.oracle.delta_Hamiltonian(c.q0, c.p0, q1, p1)
    assert done == NEPS and np.all(np.isfinite(q1)) and np.all(np.isfinite(p1)) and np.all(np.isfinite(t))
    return c, q1, p1, dH, t


def check_dh(prec, dH, t, dHo, to, factor=1.0):
    """The six energies within the precision's energy tolerance (times `factor`, 10 where the existing tests of that entry
    point have it), dH as tests/test_gpu_parity.py::test_delta_hamiltonian has it on fp64 handles.  On fp32 handles, where no
    test states a figure, dH is a signed sum of the six terms and may miss by the sum of what they may."""
    te = tolerances(prec)[1] * factor
    assert np.all(np.abs(t - to) <= te * np.abs(to)), (t, to)
    assert abs(dH - dHo) <= (1e-9 * max(np.abs(to).max(), 1.0) if prec == "fp64" else te * np.abs(to).sum()), (dH, dHo)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", mb.ENTRY_N)
@pytest.mark.parametrize("mass_type", [0, 5])
def test_real_space_mass_with_zero_negative_and_nan_cells(mass_type, n, prec):
    """kinetic_term, a 10-step leapfrog, delta_hamiltonian, leapfrog_dh and one resident attempt from chain_set_momenta on a
    mass_r with 20 % zeros, 5 % negatives and 2 % NaN: the m > 0 guard of k_div_mass_r and k_kin_rs at every step."""
    c, q1o, p1o, dHo, to = oracle_run("mass%d" % mass_type, n)
    tt, te, _ = tolerances(prec)
    e = c.engine(precision=PRECS.index(prec))
    try:
        K, Ko = e.kinetic_term(c.p0), c.oracle.kinetic_term(c.p0)
        assert np.isfinite(Ko) and abs(K - Ko) <= te * abs(Ko), (K, Ko)
        q1, p1, done = e.leapfrog(c.q0, c.p0, c.eps, NEPS)
        print("\nMASSRS leapfrog<%s> mass_type=%d n=%d: rel-L2 %.2e in q1, %.2e in p1" % (prec, mass_type, n, rel_l2(q1, q1o), rel_l2(p1, p1o)))
        assert done == NEPS and rel_l2(q1, q1o) < tt and rel_l2(p1, p1o) < tt
        check_dh(prec, *e.delta_hamiltonian(c.q0, c.p0, q1o, p1o), dHo, to)
        q1, p1, done, dH, t = e.leapfrog_dh(c.q0, c.p0, c.eps, NEPS)
        assert done == NEPS and rel_l2(q1, q1o) < tt and rel_l2(p1, p1o) < tt
        check_dh(prec, dH, t, dHo, to, factor=10.0)
        e.chain_set_state(c.q0)
        e.chain_set_momenta(c.p0)
        dH, t, done = e.chain_attempt(c.eps, NEPS)
        q1, p1 = e.chain_get_proposal()
        assert done == NEPS and rel_l2(q1, q1o) < tt and rel_l2(p1, p1o) < tt
        check_dh(prec, dH, t, dHo, to, factor=10.0)
    finally:
        e.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", mb.ENTRY_N)
@pytest.mark.parametrize("mass_type", [0, 5])
def test_philox_draw_on_a_mass_with_closed_cells(mass_type, n, prec):
    """One resident attempt after chain_draw_momenta: with a real-space mass alone the drawn momenta are exactly 0 wherever
    mass_r is not positive (zeros, negatives, NaN), and dH is the oracle's delta_Hamiltonian of the fetched state."""
    c = mb.entry_case("mass%d" % mass_type, n)
    tt, _, _ = tolerances(prec)
    e = c.engine(precision=PRECS.index(prec))
    try:
        e.chain_set_state(c.q0)
        e.chain_draw_momenta(0x5EED0000000000A1, 3)
        p = e.chain_get_momenta()
        closed = ~(c.mass_r.ravel() > 0)
        assert np.all(np.isfinite(p)) and np.any(p != 0)
        if mass_type == 0:
            assert np.all(p.ravel()[closed] == 0) and np.all(p.ravel()[~closed] != 0)
        dH, t, done = e.chain_attempt(c.eps, NEPS)
        q1, p1 = e.chain_get_proposal()
    finally:
        e.close()
    q1o, p1o, done_o = c.oracle.Hamiltonian_EoM(c.q0, p, c.eps, NEPS)
    dHo, to = c.oracle.delta_Hamiltonian(c.q0, p, q1o, p1o)
    assert done == done_o == NEPS and rel_l2(q1, q1o) < tt and rel_l2(p1, p1o) < tt
    check_dh(prec, dH, t, dHo, to, factor=10.0)


@pytest.mark.parametrize("prec", PRECS)
def test_fetched_zeros_belong_to_the_draw_alone(prec):
    """bchmc_chain_get_momenta puts exact zeros into the closed cells only while the resident momenta are a draw for the
    real-space mass that is still uploaded: the MT19937 draw has them too; momenta set by the caller come back as they were
    set, closed cells included; after another mass_r is uploaded the fetched draw is the plain transform pair again."""
    from barcode_amd.gsl_mt19937 import GslMT19937
    c = mb.entry_case("mass0", 8)
    closed = ~(c.mass_r.ravel() > 0)
    e = c.engine(precision=PRECS.index(prec))
    try:
        e.chain_draw_momenta_mt19937(GslMT19937(77))
        p = e.chain_get_momenta().ravel()
        assert np.all(p[closed] == 0) and np.all(p[~closed] != 0)
        e.chain_set_momenta(c.p0)
        back = e.chain_get_momenta().ravel()
        assert np.all(c.p0.ravel()[closed] != 0) and rel_l2(back[closed], c.p0.ravel()[closed]) < (1e-14 if prec == "fp64" else 1e-6)
        e.chain_draw_momenta(0x5EED0000000000A1, 3)
        p = e.chain_get_momenta().ravel()
        assert np.all(p[closed] == 0)
        e.upload(mass_r=np.where(closed, 1.0, c.mass_r.ravel()))
        again = e.chain_get_momenta().ravel()
        assert np.any(again[closed] != 0) and np.abs(again[closed]).max() < 1e-5 * np.abs(p).max()
        assert rel_l2(again[~closed], p[~closed]) < (1e-14 if prec == "fp64" else 1e-6)
    finally:
        e.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", mb.ENTRY_N)
def test_grf_likelihood_with_holes(n, prec):
    """likelihood 3 with 30 % of the window zero: gradient (with grad_like fetched), psi, a 10-step leapfrog and
    delta_hamiltonian: the w > 0 mask of k_grf_grad and k_grf_loglike."""
    c, q1o, p1o, dHo, to = oracle_run("grf", n)
    tt, te, tf = tolerances(prec)
    hole = c.window.ravel() == 0
    assert 0.2 < hole.mean() < 0.4
    e = c.engine(precision=PRECS.index(prec))
    try:
        g, gp, gl = c.oracle.gradient_psi(c.q0)
        gg = e.gradient(c.q0)
        got_gl = e.fetch("grad_like")
        assert np.all(gl.ravel()[hole] == 0)   # the fetched copy went through k-space: zero to round-off, judged in rel-L2
        assert rel_l2(got_gl, gl) < tf and rel_l2(gg, g) < tf
        E, Eo = e.psi(c.q0), c.oracle.psi(c.q0)
        assert np.all(np.abs(E - Eo) <= te * np.abs(Eo)), (E, Eo)
        q1, p1, done = e.leapfrog(c.q0, c.p0, c.eps, NEPS)
        print("\nMASSRS leapfrog<%s> grf with holes n=%d: rel-L2 %.2e in q1, %.2e in p1" % (prec, n, rel_l2(q1, q1o), rel_l2(p1, p1o)))
        assert done == NEPS and rel_l2(q1, q1o) < tt and rel_l2(p1, p1o) < tt
        check_dh(prec, *e.delta_hamiltonian(c.q0, c.p0, q1o, p1o), dHo, to)
    finally:
        e.close()


@pytest.mark.parametrize("prec", PRECS)
def test_jasche_mass_with_a_mask(prec):
    """mass_type 6 at 8^3 with 30 % of the window zero: the mass built on the device is exactly 0 where the window is, positive
    elsewhere; the oracle takes the fetched mass, and a 10-step leapfrog and delta_hamiltonian agree -- every masked cell
    drifts and takes its kinetic energy through the m > 0 guard."""
    c = Case(Nx=8, likelihood=1, mass_type=6, window_zero_fraction=0.3, eps_scale=mb.JASCHE_EPS_SCALE)
    tt, _, _ = tolerances(prec)
    hole = c.window.ravel() == 0
    e = c.engine(precision=PRECS.index(prec))
    try:
        mf, mass_r = e.hamiltonian_mass(c.q0)
        assert mf is None and np.all(mass_r[hole] == 0) and not np.any(np.signbit(mass_r[hole])) and np.all(mass_r[~hole] > 0)
        assert 0.2 < hole.mean() < 0.4
        c.oracle.set(mass_r=mass_r)
        q1o, p1o, done_o = c.oracle.Hamiltonian_EoM(c.q0, c.p0, c.eps, NEPS)
        dHo, to = c.oracle.delta_Hamiltonian(c.q0, c.p0, q1o, p1o)
        q1, p1, done = e.leapfrog(c.q0, c.p0, c.eps, NEPS)
        print("\nMASSRS leapfrog<%s> jasche mass with a mask n=8: rel-L2 %.2e in q1, %.2e in p1" % (prec, rel_l2(q1, q1o), rel_l2(p1, p1o)))
        assert done == done_o == NEPS and rel_l2(q1, q1o) < tt and rel_l2(p1, p1o) < tt
        check_dh(prec, *e.delta_hamiltonian(c.q0, c.p0, q1o, p1o), dHo, to)
    finally:
        e.close()
