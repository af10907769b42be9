"""Hamiltonian_mass on the device (bchmc_hamiltonian_mass; HMC_mass.cc:315-368) against the numpy restatement in
tests/mass_restatement.py, and its use by the resident chain and by hamil.HamiltonianMC's massnum schedule."""
import dataclasses

import numpy as np
import pytest

from barcode_amd import hamil, inputs
from barcode_amd.engine import BchmcError, Engine
from tests import mass_restatement as mr
from tests.util import Case, rel_l2

pytestmark = pytest.mark.gpu


def _max_rel(a, b):
    """Largest elementwise relative error; where b is 0, a must be 0 too."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    err = np.where(b == 0.0, np.abs(a), np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b)))
    return float(err.max())


def _restated(c, p, **kw):
    return mr.hamiltonian_mass(p, c.oracle, c.q0, c.signal_PS, c.window, c.noise, **kw)


@pytest.mark.parametrize("t", [0, 1, 4])
def test_elementwise_types_are_bitwise_numpy(t):
    c = Case(Nx=16, likelihood=1, mass_type=t)
    e = c.engine()  # uploads a random mass_r and 1/P as mass_f: the build must replace them
    mf, mrr = e.hamiltonian_mass(mass_factor=1.7)
    if t == 0:
        assert mf is None and np.array_equal(mrr, np.ones(c.p.N))
        assert np.array_equal(e.fetch("mass_r"), mrr)
    else:
        P = c.signal_PS.ravel()
        want = 1.7 * (inputs.inverse_power_mass(P) if t == 1 else P)
        assert mrr is None and np.array_equal(mf, want)
        assert np.array_equal(e.fetch("mass_f"), mf)
    e.close()


FORCE_CASES = [dict(likelihood=1), dict(likelihood=0), dict(likelihood=2), dict(likelihood=1, rsd_model=1),
               dict(likelihood=1, calc_h=1), dict(likelihood=1, calc_h=3), dict(likelihood=2, deltaQ_factor=0.7)]


@pytest.mark.parametrize("kw", FORCE_CASES, ids=["gauss", "poisson", "lognormal", "gauss_rsd", "calc_h1", "calc_h3",
                                                 "lognormal_dq07"])
def test_force_masses_match_the_restatement(kw):
    """Types 2 and 3 at 16^3, N_bin 200 and 7: the force spectrum, its bins (corner rule included) and F-bar."""
    c = Case(Nx=16, **kw)
    for t in (2, 3):
        p = dataclasses.replace(c.p, mass_type=t)
        e = Engine(p)
        e.upload(**c.arrays())
        for n_bin in (200, 7):
            mf, mrr = e.hamiltonian_mass(c.q0, n_bin=n_bin, mass_factor=1.3)
            want, _ = _restated(c, p, n_bin=n_bin, mass_factor=1.3)
            assert mrr is None
            # rel-L2 1e-12 as the force itself (TOL_FIELD); per element 1e-11 -- a mode in a wrong bin is off by far more
            assert rel_l2(mf, want) <= 1e-12 and _max_rel(mf, want) <= 1e-11, (t, n_bin, _max_rel(mf, want))
        e.close()


def test_force_mass_at_32_cubed_from_the_resident_state():
    c = Case(Nx=32, likelihood=1, mass_type=2)
    e = c.engine()
    e.chain_set_state(c.q0)
    mf, _ = e.hamiltonian_mass(None, n_bin=200)
    want, _ = _restated(c, c.p, n_bin=200)
    assert rel_l2(mf, want) <= 1e-12 and _max_rel(mf, want) <= 1e-11
    e.close()


def test_grf_likelihood_is_unsupported_for_force_masses():
    c = Case(Nx=8, likelihood=3, mass_type=3)
    e = c.engine()
    with pytest.raises(BchmcError) as ei:
        e.hamiltonian_mass(c.q0)
    assert ei.value.code == 5  # BCHMC_ERR_UNSUPPORTED
    e.close()


JASCHE_CASES = [(8, dict(likelihood=1), 6), (8, dict(likelihood=1, rsd_model=1), 6),
                (8, dict(likelihood=1, sfmodel=2), 6),
                (8, dict(likelihood=2, deltaQ_factor=0.8, particle_kernel_h_rel=1.5), 5),
                (16, dict(likelihood=0), 6)]


@pytest.mark.parametrize("n,kw,t", JASCHE_CASES, ids=["za_8", "rsd_8", "alpt_8", "type5_dq_h15_8", "poisson_16"])
def test_jasche_masses_match_the_literal_restatement(n, kw, t):
    """Types 5 / 6 with 30 % of the window zero: the literal per-cell FFT form upstream runs; two builds bitwise equal;
    deltaX / pos* afterwards are bchmc_forward's (Lag2Eul(signal), no deltaQ_factor)."""
    c = Case(Nx=n, window_zero_fraction=0.3, mass_type=t, **kw)
    e = c.engine()
    mf, mrr = e.hamiltonian_mass(c.q0, mass_factor=0.9)
    pos = [e.fetch(k) for k in ("posx", "posy", "posz")]
    dX = e.fetch("deltaX")
    mf2, mrr2 = e.hamiltonian_mass(c.q0, mass_factor=0.9)
    assert np.array_equal(mrr, mrr2) and (mf is None or np.array_equal(mf, mf2))
    want_f, want_r = _restated(c, c.p, mass_factor=0.9)
    assert _max_rel(mrr, want_r) <= 1e-11, _max_rel(mrr, want_r)
    if t == 5:
        assert np.array_equal(mf, want_f)
    e.forward(c.q0)
    for a, k in zip(pos, ("posx", "posy", "posz")):
        assert np.array_equal(a, e.fetch(k))
    assert rel_l2(dX, e.fetch("deltaX")) < 1e-13
    e.close()


def test_type_60_switches_at_s_eps_total():
    c = Case(Nx=8, likelihood=1, mass_type=60, window_zero_fraction=0.3)
    e = c.engine()
    mf, before = e.hamiltonian_mass(c.q0, iGibbs=3, s_eps_total=5)
    assert mf is None and np.array_equal(before, np.ones(c.p.N))
    _, after = e.hamiltonian_mass(c.q0, iGibbs=5, s_eps_total=5)
    _, want = _restated(c, c.p, iGibbs=5, s_eps_total=5)
    assert _max_rel(after, want) <= 1e-11
    e.close()


@pytest.mark.parametrize("t", [2, 6])
def test_built_mass_equals_an_upload_of_its_host_copy(t, monkeypatch):
    """Resident chain, deterministic handles: build from the resident state, then 3 attempts == a handle that uploaded
    the returned arrays, bit for bit; the carried gradient survives the build (same samples as without the carry)."""
    c = Case(Nx=16, likelihood=1, mass_type=t)
    moms = [np.roll(c.p0, 37 * k) for k in range(4)]

    def run(masses):
        e = Engine(c.p, deterministic=1)
        e.upload(**c.arrays())
        e.chain_set_state(c.q0)
        e.chain_set_momenta(moms[0])
        e.chain_attempt(c.eps, 3)
        e.chain_accept(True)  # the chain now carries the gradient at its state
        if masses is None:
            masses = e.hamiltonian_mass(None)
        else:
            e.upload(**{k: v for k, v in zip(("mass_f", "mass_r"), masses) if v is not None})
        dH = []
        for k in range(1, 4):
            e.chain_set_momenta(moms[k])
            dH.append(e.chain_attempt(c.eps, 3)[0])
            e.chain_accept(True)
        q = e.chain_get_state()
        e.close()
        return masses, dH, q

    masses, dH_a, q_a = run(None)
    _, dH_b, q_b = run(masses)
    assert dH_a == dH_b and np.array_equal(q_a, q_b)
    monkeypatch.setenv("BCHMC_NO_FORCE_CARRY", "1")
    _, dH_c, q_c = run(None)
    assert np.allclose(dH_a, dH_c, rtol=1e-9, atol=1e-9) and rel_l2(q_a, q_c) < 1e-11


@pytest.mark.parametrize("t", [2, 6])
def test_fp32_handle_against_the_fp64_restatement(t):
    c = Case(Nx=16, likelihood=1, mass_type=t, window_zero_fraction=0.3 if t == 6 else 0.0)
    e = c.engine(precision=1)
    mf, mrr = e.hamiltonian_mass(c.q0)
    want_f, want_r = _restated(c, c.p)
    got, want = (mf, want_f) if t == 2 else (mrr, want_r)
    assert rel_l2(got, want) <= 1e-4
    e.close()


def _mc_run(c, arrays, samples, explicit=False, **mc):
    rng = np.random.default_rng(7)
    u = lambda: float(rng.random())  # noqa: E731
    hd = hamil.HamilData(c.p, N_eps_fac=3.0, eps_fac=4 * c.eps, **arrays)
    hd.engine.chain_set_state(c.q0)
    logs = []
    for s in range(1, samples + 1):
        hd.numerical.iGibbs = s
        if explicit:
            hamil.Hamiltonian_mass(hd)
        logs += hamil.HamiltonianMC(hd, u, seed=11, itmax=20, **mc)
    x = hd.engine.chain_get_state()
    mass_f = hd.engine.fetch("mass_f")
    hd.engine.close()
    return logs, x, mass_f


def _same_samples(la, lb, xa, xb):
    assert len(la) == len(lb) >= 3
    for a, b in zip(la, lb):
        assert a["accepted"] == b["accepted"] and a["Neps"] == b["Neps"]
        scale = max(abs(b[k]) for k in ("H_kin_i", "psi_prior_i", "psi_likeli_i", "H_kin_f", "psi_prior_f", "psi_likeli_f"))
        assert abs(a["dH"] - b["dH"]) <= 1e-9 * scale
    assert rel_l2(xa, xb) < 1e-11


def test_hamiltonian_mc_rebuilds_the_mass_on_its_schedule():
    """massnum_init = 1 (iGibbs <= massnum_burn): the mass is rebuilt at the top of every sample, from the resident
    state -- the same samples as building it explicitly before each sample."""
    c = Case(Nx=16, likelihood=1, mass_type=2)
    la, xa, mfa = _mc_run(c, c.arrays(), 3, massnum_init=1, massnum_burn=10)
    lb, xb, mfb = _mc_run(c, c.arrays(), 3, explicit=True)
    _same_samples(la, lb, xa, xb)
    assert _max_rel(mfa, mfb) <= 1e-12


def _shim_run(c, arrays, samples, massnum_init, massnum_burn):
    from barcode_amd.shim import ShimHamil
    rng = np.random.default_rng(7)
    u = lambda: float(rng.random())  # noqa: E731
    hd = ShimHamil(c.p, N_eps_fac=3.0, eps_fac=4 * c.eps, **arrays)
    hd.numerical.massnum_init, hd.numerical.massnum_burn = massnum_init, massnum_burn
    hd.chain_set_state(c.q0)
    logs = []
    for s in range(1, samples + 1):
        hd.numerical.iGibbs = s
        logs += hd.HamiltonianMC(u, seed=11, itmax=20)
    x = hd.chain_get_state()
    hd.close()
    return logs, x


@pytest.mark.parametrize("massnum", [1, 0])
def test_cpp_hamiltonian_mc_schedule_matches_the_python_mirror(massnum):
    """bchmc_shim::HamiltonianMC with massnum_init = 1 rebuilds the mass every sample like hamil.HamiltonianMC (and the
    caller-owned mass_f receives it); with 0 nothing is built and the scaled uploaded mass_f stays."""
    c = Case(Nx=16, likelihood=1, mass_type=2)
    arrays = c.arrays()
    arrays["mass_f"] = 1.5 * arrays["mass_f"]
    scaled = arrays["mass_f"].copy()
    lc, xc = _shim_run(c, arrays, 3, massnum, 10)
    lp, xp, mfp = _mc_run(c, {k: v.copy() for k, v in arrays.items()}, 3, massnum_init=massnum, massnum_burn=10)
    _same_samples(lc, lp, xc, xp)
    if massnum:
        assert _max_rel(arrays["mass_f"], mfp) <= 1e-12  # the C++ loop wrote the built mass where hd->mass_f points
    else:
        assert np.array_equal(arrays["mass_f"], scaled) and np.array_equal(mfp, scaled.ravel())


def test_massnum_zero_never_builds():
    """massnum 0 (data/input.par:104-105): nothing is built, a deliberately scaled uploaded mass_f stays in use and the
    samples are those of the plain loop."""
    c = Case(Nx=16, likelihood=1, mass_type=1)
    arrays = c.arrays()
    arrays["mass_f"] = 1.5 * arrays["mass_f"]
    la, xa, mfa = _mc_run(c, arrays, 3, massnum_init=0, massnum_burn=0)
    lb, xb, _ = _mc_run(c, arrays, 3)
    assert np.array_equal(mfa, arrays["mass_f"].ravel())
    _same_samples(la, lb, xa, xb)
