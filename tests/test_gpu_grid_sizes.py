"""The hot path on the odd and the smallest grids bchmc_create accepts, against the CPU oracle ("Grid sizes").

    n = 4            the tiled path with one 4 x 4 x 4 tile whose halo (R = 2) wraps onto the tile itself: the image is
                     (2 n)^3 and holds every cell 8 times; with BCHMC_NO_TILES=1 the direct kernels, whose stencil
                     offsets -2 and +2 are one cell; the ALPT 4th-order stencil has ll == rr
    n = 5, 6, 7      no tile shape divides them: the direct kernels; at 5 the stencil is as wide as the box
    n = 5, 7, 9, 11, 15   odd: nh = (n + 1) / 2, rows of n + 1 reals, radix-3 / 5 / 7 / 11 real transforms, and the
                     reference's "Nyquist" rule i == n / 2 (integer division) zeroes an ordinary mode and leaves its
                     conjugate partner alone (tests/test_known_answers.py, K2o), in every kernel that copies it

The prime above 8 is 11: rocFFT has radix-11 and radix-13 butterflies, so neither 11 nor 13 needs a Bluestein plan and
either would do.  Tolerances are those of tests/util.py and, for fp32 handles, of test_gpu_parity.test_fp32_field_mode.
Step sizes: Case's defaults but where the probe of DESIGN.md 7 asks for a smaller one (EPS_AT).  Every check prints its
figure ("GRID n=.. <config>: <what> <rel-L2>") before it asserts.
"""
import numpy as np
import pytest

from tests.util import TOL_ENERGY, TOL_FIELD, TOL_TRAJ_10, Case, rel_l2

pytestmark = pytest.mark.gpu

TOL_F32_FIELD = 2e-5   # test_gpu_parity.test_fp32_field_mode
TOL_F32_TRAJ = 1e-4
TOL_F32_ENERGY = 1e-5

SIZES = (4, 5, 6, 7, 9, 11, 15)
EVERY_SIZE = {
    "gauss_rsd": dict(likelihood=1, rsd_model=1),
    "alpt": dict(likelihood=1, rsd_model=0, sfmodel=2),    # stencil_row's (n & 7) != 0 branch; aliased stencil at 4
}
AT_5_AND_9 = {
    "poisson": dict(likelihood=0, rsd_model=0),
    "lognormal": dict(likelihood=2, rsd_model=0),
    "grf": dict(likelihood=3, rsd_model=0),
    "calc_h0": dict(likelihood=1, rsd_model=0, calc_h=0),
    "calc_h1": dict(likelihood=1, rsd_model=0, calc_h=1),
    "calc_h3": dict(likelihood=1, rsd_model=0, calc_h=3),
    "ngp": dict(likelihood=0, rsd_model=0, calc_h=1, mk=0),
    "cic": dict(likelihood=1, rsd_model=0, calc_h=1, mk=1),
    "tsc": dict(likelihood=1, rsd_model=1, calc_h=1, mk=2),
    "holes": dict(likelihood=0, window_zero_fraction=0.4),
    "offset": dict(likelihood=1, rsd_model=0, min1=1.0, min2=2.0, min3=0.5),
}
# probed with the oracle over the 5 steps taken here (a 1e-13 perturbation of q0 must grow by < 100): amplification 205 at
# the default 0.1 and 0.45 at 0.03; 512 at the default 0.03 and 0.93 at 0.01
EPS_AT = {(5, "calc_h3"): 0.03, (9, "poisson"): 0.01}
NEPS = 5

MATRIX = [(n, name) for n in SIZES for name in EVERY_SIZE] + [(n, name) for n in (5, 9) for name in AT_5_AND_9]
KW = dict(EVERY_SIZE, **AT_5_AND_9)


def make_case(n, name, **more):
    kw = dict(KW[name], **more)
    if (n, name) in EPS_AT:
        kw["eps_scale"] = EPS_AT[n, name]
    c = Case(Nx=n, **kw)
    c.label = "GRID n=%d %s" % (n, name)
    return c


def say(c, what, value):
    print("%s: %s %.3g" % (c.label, what, value))
    return value


def expected_path(n):
    return "tiled" if n == 4 else "direct"


def assert_path(e, n, want=None):
    """Which particle-mesh kernels the handle dispatches to: the tile kernels at 4 (4 x 4 x 4 tiles divide it), the direct
    ones at every other size of this file (no tile shape divides them)."""
    info = e.tile_info()
    assert ("tiled" if info["tiled"] else "direct") == (want or expected_path(n)), info


# ---- the oracle's side of a case, computed once and shared ---------------------------------------------------------------
class Ref:
    def __init__(self, c):
        o, p = c.oracle, c.p
        self.fwd = None
        if p.likelihood != 3:
            rsd = p.rsd_model
            dX, px, py, pz = o.Lag2Eul(c.truth, rsd=rsd)
            psi = o.alpt_displacement(c.truth) if (p.sfmodel != 1 and not rsd) else o.theta2vel(-p.D1 * c.truth.ravel())
            self.fwd = dict(psi=psi, pos=(px, py, pz), rho=o.getDensity(p.mk, px, py, pz), dX=dX)
        self.g, self.gp, self.gl = o.gradient_psi(c.q0)
        self.force = None
        if p.likelihood != 3:
            dX = o.get("deltaX")
            pl = o.partial_f_delta_x_log_like(dX)
            V = None
            if p.calc_h in (2, 3):
                pos = [o.get(k) for k in ("posx", "posy", "posz")]
                V = (o.likelihood_calc_V_SPH if p.calc_h == 2 else o.likelihood_calc_V_SPH_fourier_TSC)(pl, *pos)
            self.force = dict(dX=dX, pl=pl, V=V)
        self.q1, self.p1, self.done = o.Hamiltonian_EoM(c.q0, c.p0, c.eps, NEPS)
        self.dH, self.terms = o.delta_Hamiltonian(c.q0, c.p0, self.q1, self.p1)


def check_intermediates(c, e, r, tol_field):
    """One forward model and one force evaluation, the lists of test_gpu_parity.test_forward_model_intermediates and
    test_gradient_psi_and_its_pieces: psi, positions, rho, deltaX | grad_prior, grad_like, gradient, deltaX, part_like, V."""
    if r.fwd is not None:
        e.forward(c.truth, c.p.rsd_model)
        for name, ref in zip(("psix", "psiy", "psiz"), r.fwd["psi"]):
            assert say(c, name, rel_l2(e.fetch(name), ref)) < tol_field
        for name, ref in zip(("posx", "posy", "posz"), r.fwd["pos"]):
            assert say(c, name, rel_l2(e.fetch(name), ref)) < tol_field
        assert say(c, "rho", rel_l2(e.fetch("rho"), r.fwd["rho"])) < tol_field
        assert say(c, "deltaX", rel_l2(e.fetch("deltaX"), r.fwd["dX"])) < tol_field
    gg = e.gradient(c.q0)
    assert say(c, "grad_prior", rel_l2(e.fetch("grad_prior"), r.gp)) < tol_field
    assert say(c, "grad_like", rel_l2(e.fetch("grad_like"), r.gl)) < 10 * tol_field
    assert say(c, "gradient", rel_l2(gg, r.g)) < 10 * tol_field
    if r.force is not None:
        assert say(c, "deltaX(q0)", rel_l2(e.fetch("deltaX"), r.force["dX"])) < tol_field
        assert say(c, "part_like", rel_l2(e.fetch("part_like"), r.force["pl"])) < 10 * tol_field
        if r.force["V"] is not None:
            for name, ref in zip(("Vx", "Vy", "Vz"), r.force["V"]):
                assert say(c, name, rel_l2(e.fetch(name), ref)) < 10 * tol_field


def check_trajectory(c, e, r, tol_traj):
    q1, p1, done = e.leapfrog(c.q0, c.p0, c.eps, NEPS)
    assert done == r.done == NEPS
    assert say(c, "q1", rel_l2(q1, r.q1)) < tol_traj
    assert say(c, "p1", rel_l2(p1, r.p1)) < tol_traj
    return q1, p1


def worst_term(t, to):
    return float(np.max(np.abs(np.asarray(t) - to) / np.abs(to)))


def check_energies(c, e, r, tol_traj, tol_energy, chain=True):
    """The six terms of delta_Hamiltonian three ways: bchmc_leapfrog + bchmc_delta_hamiltonian, bchmc_leapfrog_dh, and
    one attempt of the resident chain, each against the oracle's."""
    to, scale = r.terms, np.abs(r.terms).max()
    q1, p1, _ = e.leapfrog(c.q0, c.p0, c.eps, NEPS)
    dH, t = e.delta_hamiltonian(c.q0, c.p0, q1, p1)
    assert say(c, "terms leapfrog + delta_hamiltonian", worst_term(t, to)) <= tol_energy
    assert abs(dH - r.dH) <= 1e-9 * max(scale, 1.0)
    q1, p1, done, dH, t = e.leapfrog_dh(c.q0, c.p0, c.eps, NEPS)
    assert done == NEPS and rel_l2(q1, r.q1) < tol_traj and rel_l2(p1, r.p1) < tol_traj
    assert say(c, "terms leapfrog_dh", worst_term(t, to)) <= tol_energy
    assert abs(dH - r.dH) <= 1e-9 * max(scale, 1.0)
    if chain:
        e.chain_set_state(c.q0)
        e.chain_set_momenta(c.p0)
        dH, t, done = e.chain_attempt(c.eps, NEPS)
        q1, p1 = e.chain_get_proposal()
        assert done == NEPS and rel_l2(q1, r.q1) < tol_traj and rel_l2(p1, r.p1) < tol_traj
        assert say(c, "terms chain_attempt", worst_term(t, to)) <= tol_energy
        assert abs(dH - r.dH) <= 1e-9 * max(scale, 1.0)
        e.chain_accept(True)
        assert rel_l2(e.chain_get_state(), r.q1) < tol_traj


# ---- every size x configuration, fp64 ------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=MATRIX, ids=["n%d-%s" % m for m in MATRIX])
def case(request):
    n, name = request.param
    c = make_case(n, name)
    c.n, c.ref = n, Ref(c)
    c.e = c.engine()
    yield c
    c.e.close()


def test_dispatch(case):
    assert_path(case.e, case.n)


def test_intermediates_of_one_force_evaluation(case):
    check_intermediates(case, case.e, case.ref, TOL_FIELD)


def test_five_step_trajectory(case):
    check_trajectory(case, case.e, case.ref, TOL_TRAJ_10)


def test_energy_terms_three_ways(case):
    check_energies(case, case.e, case.ref, TOL_TRAJ_10, TOL_ENERGY)


# ---- fp32 handles at 4, 5 and 9 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EVERY_SIZE))
@pytest.mark.parametrize("n", (4, 5, 9))
def test_fp32_handles(n, name):
    c = make_case(n, name)
    c.label += " fp32"
    r = Ref(c)
    e = c.engine(precision=1)
    assert_path(e, n)
    g = e.gradient(c.q0)
    assert say(c, "grad_prior", rel_l2(e.fetch("grad_prior"), r.gp)) < TOL_F32_FIELD
    assert say(c, "gradient", rel_l2(g, r.g)) < 10 * TOL_F32_FIELD
    assert say(c, "deltaX(q0)", rel_l2(e.fetch("deltaX"), r.force["dX"])) < 10 * TOL_F32_FIELD
    check_trajectory(c, e, r, TOL_F32_TRAJ)
    dH, t = e.delta_hamiltonian(c.q0, c.p0, r.q1, r.p1)
    assert say(c, "terms delta_hamiltonian", worst_term(t, r.terms)) <= TOL_F32_ENERGY
    e.close()


# ---- deterministic mode at 4 and 9 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EVERY_SIZE))
@pytest.mark.parametrize("n", (4, 9))
def test_deterministic_handles_repeat_bitwise(n, name):
    from barcode_amd.engine import Engine
    c = make_case(n, name)
    c.label += " deterministic"
    r = Ref(c)
    runs = []
    for _ in range(2):
        e = Engine(c.p, deterministic=1)     # a fresh handle each time: nothing carried over
        e.upload(**c.arrays())
        assert_path(e, n)
        e.forward(c.q0)
        rho = e.fetch("rho")
        g = e.gradient(c.q0)
        q1, p1, done = e.leapfrog(c.q0, c.p0, c.eps, NEPS)
        dH, terms = e.delta_hamiltonian(c.q0, c.p0, q1, p1)
        runs.append((rho, g, q1, p1, terms))
        if len(runs) == 2:
            check_intermediates(c, e, r, TOL_FIELD)
        e.close()
    for what, a, b in zip(("rho", "gradient", "q1", "p1", "terms"), *runs):
        assert np.array_equal(a, b), what
    assert say(c, "q1", rel_l2(runs[0][2], r.q1)) < TOL_TRAJ_10 and say(c, "p1", rel_l2(runs[0][3], r.p1)) < TOL_TRAJ_10
    assert say(c, "terms", worst_term(runs[0][4], r.terms)) <= TOL_ENERGY


# ---- an odd logical row inside a padded one; the direct kernels at 4 -----------------------------------------------------
@pytest.mark.parametrize("name", list(EVERY_SIZE) + ["calc_h3", "grf"])
def test_padded_half_complex_rows_at_9(monkeypatch, name):
    """BCHMC_FFT_PAD=1 as test_gpu_parity.test_padded_half_complex_rows sets it: nh = 5 complex elements in a row of 8."""
    monkeypatch.setenv("BCHMC_FFT_PAD", "1")
    c = make_case(9, name)
    c.label += " padded"
    r = Ref(c)
    e = c.engine()
    assert_path(e, 9)
    check_intermediates(c, e, r, TOL_FIELD)
    check_trajectory(c, e, r, TOL_TRAJ_10)
    check_energies(c, e, r, TOL_TRAJ_10, TOL_ENERGY)
    e.close()


@pytest.mark.parametrize("name", list(EVERY_SIZE))
def test_direct_kernels_at_4(monkeypatch, name):
    """BCHMC_NO_TILES=1 at n = 4: the stencil offsets -2 and +2 of k_scatter_sph / k_gather_sph land on the same cell, which
    must receive (and give) both contributions."""
    monkeypatch.setenv("BCHMC_NO_TILES", "1")
    c = make_case(4, name)
    c.label += " no tiles"
    r = Ref(c)
    e = c.engine()
    assert_path(e, 4, "direct")
    check_intermediates(c, e, r, TOL_FIELD)
    check_trajectory(c, e, r, TOL_TRAJ_10)
    check_energies(c, e, r, TOL_TRAJ_10, TOL_ENERGY)
    e.close()


# ---- the runaway guard at an odd size ------------------------------------------------------------------------------------
def test_runaway_guard_at_9():
    """As test_gpu_parity.test_runaway_guard_matches_reference_semantics (HMC.cc:360-364).  p[0] is the sum of p^ over the
    half-complex array with Hermitian weights; at odd n no column has the Nyquist weight 1."""
    c = Case(Nx=9)
    e = c.engine()
    p0 = c.p0.copy().ravel()
    p0[0] = 1e60
    q1o, p1o, done_o = c.oracle.Hamiltonian_EoM(c.q0, p0, 1e-6, 5)
    q1, p1, done = e.leapfrog(c.q0, p0, 1e-6, 5)
    assert done == done_o == 1
    assert rel_l2(p1, p1o) < 1e-10
    # and a normal trajectory afterwards is unaffected by the tripped flag
    q2o, p2o, _ = c.oracle.Hamiltonian_EoM(c.q0, c.p0, c.eps, 3)
    q2, p2, done2 = e.leapfrog(c.q0, c.p0, c.eps, 3)
    assert done2 == 3 and rel_l2(q2, q2o) < TOL_TRAJ_10 and rel_l2(p2, p2o) < TOL_TRAJ_10
    # the resident chain stops and rolls back in the same way
    e.chain_set_state(c.q0)
    e.chain_set_momenta(p0)
    _, _, donec = e.chain_attempt(1e-6, 5)
    assert donec == 1
    assert rel_l2(e.chain_get_proposal()[1], p1o) < 1e-10
    e.close()
