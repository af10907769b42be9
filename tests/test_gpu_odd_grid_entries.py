"""The entry points beside the hot path on odd grids ("Grid sizes"): spectrum, correlation functions,
chain_forward, Hamiltonian_mass, the Philox momentum draw -- each against the reference its own test file uses, with
that file's tolerances -- and the refusals of the entries that need an even Nx (create_GARFIELD's walk), which must leave
the generator, the chain and the uploaded inputs exactly as they were.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from barcode_amd import inputs
from barcode_amd.engine import BchmcError, Engine, MockOpts
from barcode_amd.gsl_mt19937 import GslMT19937
from barcode_amd.params import HamilParams
from tests import corr_restatement as cr
from tests import mass_restatement as mr
from tests import mock_restatement as mock
from tests.test_gpu_corr import both, check_field, tol_of
from tests.test_gpu_mass import _max_rel
from tests.test_gpu_mt19937_draw import check_state, close, restate_draw
from tests.util import TOL_ENERGY, TOL_FIELD, Case, rel_l2

pytestmark = pytest.mark.gpu

UNSUPPORTED = 5


# ---- bchmc_measure_spectrum -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("n", (5, 9))
def test_measure_spectrum_host_field_and_resident_state(n, precision):
    """As test_gpu_chain.test_measure_spectrum_host_field_and_resident_state: the Hermitian weight of the half-complex sum
    has no Nyquist column at odd n."""
    c = Case(Nx=n)
    e = c.engine(precision=precision)
    tol = 1e-12 if precision == 0 else 2e-5
    for nb in (20, 200):
        kmo, pwo = c.oracle.measure_spectrum(c.q0, nb)
        km, pw = e.measure_spectrum(c.q0, nb)
        atol = tol * pwo.max()  # the k = 0 bin of a zero-mean field is round-off on both sides
        assert np.allclose(km, kmo, rtol=1e-13, atol=0) and np.allclose(pw, pwo, rtol=tol, atol=atol)
        e.chain_set_state(c.q0)
        km2, pw2 = e.measure_spectrum(None, nb)
        assert np.allclose(km2, kmo, rtol=1e-13, atol=0) and np.allclose(pw2, pwo, rtol=tol, atol=atol)
    e.close()


# ---- bchmc_measure_corr / bchmc_measure_corr2d / bchmc_chain_forward ----------------------------------------------------
@pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
@pytest.mark.parametrize("n", (5, 9))
def test_corr_of_all_three_sources(n, precision):
    """Host field, resident state and deltaX (after chain_forward with and without RSD) against tests/corr_restatement.py,
    exactly as tests/test_gpu_corr.py holds them: nmode equal, rmode to 1e-14, corr to TOL_FIELD of its maximum.  At odd n
    corr.hpp's fold of k and n - k has no self-paired plane but k = 0."""
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    L, tol = c.p.L, tol_of(precision)
    e = c.engine(precision=precision)
    e.chain_set_state(c.q0)
    for nb in (n, cr.auto_nbin(n, L), 200):
        tag = "%d^3 %s n_bin %d" % (n, "fp32" if precision else "fp64", nb)
        check_field(tag + " host", e, c.truth, n, L, nb, tol)
        check_field(tag + " chain", e, c.q0, n, L, nb, tol, "chain", send=False)
    for rsd in (1, 0):
        e.chain_forward(rsd)
        dX = e.fetch("deltaX")
        for nb in (n, cr.auto_nbin(n, L)):
            check_field("%d^3 deltaX rsd %d n_bin %d" % (n, rsd, nb), e, dX, n, L, nb, tol, "deltaX", send=False)
        assert np.array_equal(e.fetch("deltaX"), dX)  # the measurement left it alone
    e.close()


@pytest.mark.parametrize("n", (5, 9))
def test_corr_repeats_bitwise_on_two_handles(n):
    """As test_gpu_corr.test_repeatable: two calls on each of two fresh handles, 1-D and 2-D, chain and host source."""
    p = HamilParams(Nx=n, L=200.0 * n / 64.0)
    f = inputs.make_fields(p)
    runs = []
    for _ in range(2):
        e = Engine(p)
        e.chain_set_state(f["q0"])
        for _ in range(2):
            runs.append([both(e, None, nb, "chain") + both(e, f["truth"], nb) for nb in (n, 5, 2048)])
        e.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            for r1, r2 in zip(a, b):
                assert all(np.array_equal(x, y) for x, y in zip(r1, r2))


@pytest.mark.parametrize("rsd", (0, 1), ids=("real", "rsd"))
@pytest.mark.parametrize("n", (5, 9))
def test_chain_forward_against_the_oracle(n, rsd):
    c = Case(Nx=n, likelihood=1, rsd_model=rsd)
    e = c.engine()
    e.chain_set_state(c.truth)
    e.chain_forward(rsd)
    dX, px, py, pz = c.oracle.Lag2Eul(c.truth, rsd=rsd)
    for k, want in zip(("deltaX", "posx", "posy", "posz"), (dX, px, py, pz)):
        lvl = rel_l2(e.fetch(k), want)
        print("GRID n=%d chain_forward(%d): %s %.3g" % (n, rsd, k, lvl))
        assert lvl < TOL_FIELD
    assert rel_l2(e.chain_get_state(), c.truth) < 1e-14
    e.close()


# ---- bchmc_hamiltonian_mass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (5, 7))
def test_force_mass_type_2(n):
    """As test_gpu_mass.test_force_masses_match_the_restatement: the force spectrum, its bins and F-bar."""
    c = Case(Nx=n, likelihood=1)
    p = dataclasses.replace(c.p, mass_type=2)
    e = Engine(p)
    e.upload(**c.arrays())
    for n_bin in (200, 7):
        mf, mrr = e.hamiltonian_mass(c.q0, n_bin=n_bin, mass_factor=1.3)
        want, _ = mr.hamiltonian_mass(p, c.oracle, c.q0, c.signal_PS, c.window, c.noise, n_bin=n_bin, mass_factor=1.3)
        assert mrr is None
        print("GRID n=%d mass_type 2 n_bin %d: rel-L2 %.3g, max rel %.3g" % (n, n_bin, rel_l2(mf, want), _max_rel(mf, want)))
        assert rel_l2(mf, want) <= 1e-12 and _max_rel(mf, want) <= 1e-11
    e.close()


@pytest.mark.parametrize("n", (5, 7))
def test_jasche_mass_type_6(n):
    """As test_gpu_mass.test_jasche_masses_match_the_literal_restatement, 30 % of the window zero."""
    c = Case(Nx=n, window_zero_fraction=0.3, mass_type=6, likelihood=1)
    e = c.engine()
    mf, mrr = e.hamiltonian_mass(c.q0, mass_factor=0.9)
    mf2, mrr2 = e.hamiltonian_mass(c.q0, mass_factor=0.9)
    assert mf is None and np.array_equal(mrr, mrr2)
    _, want_r = mr.hamiltonian_mass(c.p, c.oracle, c.q0, c.signal_PS, c.window, c.noise, mass_factor=0.9)
    print("GRID n=%d mass_type 6: max rel %.3g" % (n, _max_rel(mrr, want_r)))
    assert _max_rel(mrr, want_r) <= 1e-11
    e.close()


# ---- bchmc_chain_draw_momenta (Philox) ----------------------------------------------------------------------------------
DRAWS = 16


def test_philox_draw_at_9_is_a_real_field_with_the_right_statistics():
    """The statistics of test_gpu_chain.test_device_momentum_draw_statistics_and_reproducibility at n = 9, and the
    self-conjugate set: at odd n only k = 0 is its own partner, every other mode of the plane k_z = 0 has one at (n - i, n -
    j).  A draw that pairs them wrongly is not the transform of a real field: its kinetic term, summed over the resident
    half-complex array, then differs from the one of the field get_momenta returns.

    Bounds for this shape: K = 1/2 p^T M^-1 p is chi^2 / 2 with N - 1 = 728 degrees of freedom, mean 364 and variance 364,
    held to 5 sigma per draw as there.  The mean of |p^|^2 / expectation over the (N - 1) / 2 = 364 independent complex modes
    of one draw (each exponential, mean 1, variance 1) has sigma 1 / sqrt(364); over DRAWS = 16 draws sigma = 0.0131, held
    to 5 sigma = 0.066 (the 0.02 used at 32^3 is 2.5 of that shape's sigma and would be 1.5 sigma here)."""
    n = 9
    c = Case(Nx=n)
    e = c.engine()
    e.chain_set_state(c.q0)
    e.chain_draw_momenta(1234, 0)
    pa = e.chain_get_momenta()
    e.chain_draw_momenta(1234, 0)
    assert np.array_equal(pa, e.chain_get_momenta())
    n_modes = c.p.N - 1  # mass_f(k = 0) = 0: that mode carries no momentum
    expect = c.p.N ** 2 * c.mass_f[:, :, : n // 2 + 1] / c.p.L ** 3
    sel = expect > 0
    ratios, draws = [], []
    for attempt in range(DRAWS):
        e.chain_draw_momenta(1234, attempt)
        p = e.chain_get_momenta()
        draws.append(p)
        # the resident p^ -> H_kin_i of an attempt; the fetched real field -> kinetic_term; back in -> the same again
        _, terms, _ = e.chain_attempt(c.eps, 1)
        e.chain_accept(False)
        K_host = e.kinetic_term(p)
        assert abs(terms[0] - K_host) <= TOL_ENERGY * abs(K_host), (attempt, terms[0], K_host)
        assert abs(K_host - c.oracle.kinetic_term(p)) <= TOL_ENERGY * abs(K_host)
        e.chain_set_momenta(p)
        assert rel_l2(e.chain_get_momenta(), p) < 1e-13
        _, terms2, _ = e.chain_attempt(c.eps, 1)
        e.chain_accept(False)
        assert abs(terms2[0] - terms[0]) <= TOL_ENERGY * abs(terms[0])
        assert abs(K_host - n_modes / 2) < 5 * np.sqrt(n_modes / 2), K_host
        assert abs(p.mean()) < 1e-10 * np.abs(p).max() + 1e-12  # no k = 0 power
        pk = np.abs(np.fft.rfftn(p.reshape(n, n, n))) ** 2
        ratios.append((pk[sel] / expect[sel]).mean())
    print("GRID n=9 Philox draw: mean |p^|^2 / expectation over %d draws %.4f" % (DRAWS, np.mean(ratios)))
    assert abs(np.mean(ratios) - 1) < 5 / np.sqrt(DRAWS * n_modes / 2)
    e.chain_draw_momenta(1235, 0)
    pc = e.chain_get_momenta()
    # correlation of two independent fields of N = 729 cells: sigma = 1 / sqrt(N) = 0.037, 5 sigma
    assert abs(np.corrcoef(draws[0], draws[1])[0, 1]) < 5 / np.sqrt(c.p.N)
    assert abs(np.corrcoef(draws[0], pc)[0, 1]) < 5 / np.sqrt(c.p.N)
    e.close()


# ---- the entries that need an even Nx ----------------------------------------------------------------------------------
def snapshot(e, c):
    return dict(state=e.chain_get_state(), mom=e.chain_get_momenta(),
                **{k: e.fetch(k) for k in ("signal_PS", "mass_f", "window", "noise", "nobs")})


def refused_untouched(e, c, call, what):
    """`call(mt, mti, used)` must return BCHMC_ERR_UNSUPPORTED with last_error naming the size, leave mt / mti bit for bit,
    the chain and the inputs as they were, and the handle fit for a gradient that matches the oracle."""
    rng = GslMT19937(4711)
    rng.raw(211)  # a mid-block state
    mt0, mti0 = rng.get_state()
    mt = np.ascontiguousarray(mt0, dtype=np.uint32).copy()
    mti, used = C.c_int32(int(mti0)), C.c_uint64(12345)
    before = snapshot(e, c)
    rc = call(mt.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(mti), C.byref(used))
    assert rc == UNSUPPORTED, (what, rc)
    text = e.lib.bchmc_last_error(e.h).decode()
    assert "even Nx" in text and "(%d)" % c.p.Nx in text, text
    assert np.array_equal(mt, np.asarray(mt0, dtype=np.uint32)) and mti.value == int(mti0), what
    after = snapshot(e, c)
    for k in before:
        assert np.array_equal(before[k], after[k]), (what, k)
    g, _, _ = c.oracle.gradient_psi(c.q0)
    assert rel_l2(e.gradient(c.q0), g) < 10 * TOL_FIELD, what


def test_entries_that_need_an_even_nx_refuse_5_and_touch_nothing():
    n = 5
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    e = c.engine()
    e.chain_set_state(c.q0)
    e.chain_set_momenta(c.p0)
    lib, h = e.lib, e.h
    refused_untouched(e, c, lambda mt, mti, used: lib.bchmc_chain_draw_momenta_mt19937(h, mt, mti, used),
                      "chain_draw_momenta_mt19937")
    o = MockOpts(1, 0, 0, 0, 1.0, 0.0)
    refused_untouched(e, c, lambda mt, mti, used: lib.bchmc_setup_random_test(h, C.byref(o), mt, mti, used, None, None),
                      "setup_random_test")
    for guess in (2, 3):
        refused_untouched(e, c, lambda mt, mti, used: lib.bchmc_make_initial_guess(h, guess, None, 1, 3 * c.p.d, mt, mti, used),
                          "make_initial_guess %d" % guess)
    # the Python layer raises the same code and leaves its generator alone
    rng = GslMT19937(3)
    ref = rng.copy()
    for fn in (lambda: e.chain_draw_momenta_mt19937(rng), lambda: e.setup_random_test(rng), lambda: e.make_initial_guess(rng, 2)):
        with pytest.raises(BchmcError) as err:
            fn()
        assert err.value.code == UNSUPPORTED
    check_state(ref, 0, rng)
    e.close()


def test_initial_guesses_0_1_and_4_work_at_5():
    """As test_gpu_mock.test_all_five_guesses for the guesses that do not go through create_GARFIELD."""
    from oracle.oracle import Oracle
    n, seed = 5, 7
    p = mock.params(n)
    P = mock.power(p)
    e = Engine(p)
    e.upload(signal_PS=P, mass_f=inputs.inverse_power_mass(P))
    ff = np.sin(np.arange(p.N, dtype=np.float64))
    orc = Oracle(p)
    for guess in (0, 1, 4):
        rng, ref = GslMT19937(seed), GslMT19937(seed)
        rng.raw(211), ref.raw(211)
        before = rng.copy()
        used = e.make_initial_guess(rng, guess, file_field=ff, smoothing_type=1, smoothing_scale=3 * p.d)
        used_r, sig = mock.make_initial_guess(p, P, ref, guess, file_field=ff, smoothing_scale=3 * p.d, oracle=orc)
        assert used == used_r and (used > 0) == (guess == 4)
        check_state(before, used, rng)
        q = e.chain_get_state()
        if guess == 0:
            assert not q.any()
        else:
            close(q, sig)
    e.close()


def test_mt19937_draw_with_a_real_space_mass_works_at_5():
    """mass_type 0 has no Fourier-space part and so no walk: p = sqrt(mass_r) g, one Gaussian of the stream per cell, against
    test_gpu_mt19937_draw.restate_draw (the oracle's draw_momenta takes even sizes only)."""
    c = Case(Nx=5, mass_type=0)
    e = c.engine()
    rng = GslMT19937(1005)
    before = rng.copy()
    used = e.chain_draw_momenta_mt19937(rng)
    used_r, want = restate_draw(c, before.copy())
    close(e.chain_get_momenta(), want)
    assert used == used_r
    check_state(before, used, rng)
    e.close()
