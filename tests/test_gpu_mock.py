"""setup_random_test and make_initial_guess on the device (bchmc_setup_random_test, bchmc_make_initial_guess) against
the numpy restatement of barcoderunner.cc:42-247 (tests/mock_restatement.py): fields by the project's tolerances, the
window, the set of clamped cells, the words consumed and the generator state exactly.  tests/test_mock_restatement.py
asserts, on the restatement alone, that no cell of these cases lies within 1e-9 of a threshold; the margins are asserted
here again before the engine is looked at."""
import numpy as np
import pytest

from barcode_amd import inputs
from barcode_amd.engine import BchmcError, Engine
from barcode_amd.gsl_mt19937 import GslMT19937
from barcode_amd.params import HamilParams
from tests import mock_restatement as mr
from tests.test_gpu_mt19937_draw import check_state, close
from tests.test_gpu_parity import TOL_F32_FIELD
from tests.util import TOL_FIELD, rel_l2

pytestmark = pytest.mark.gpu


def engine_for(p, P, **kw):
    e = Engine(p, **kw)
    e.upload(signal_PS=P, mass_f=inputs.inverse_power_mass(P))
    return e


def run(e, rng, o, **kw):
    return e.setup_random_test(rng, window_type=o.window_type, data_model=o.data_model, negative_obs=o.negative_obs,
                               random_test_rsd=o.random_test_rsd, sigma_min=o.sigma_min, sigma_fac=o.sigma_fac, **kw)


def clamps(p, o):
    return o.data_model == 0 and p.likelihood == 1 and not o.negative_obs


def check(e, p, o, r, before, rng, used, dl, de, tol=TOL_FIELD, lag=close):
    lag(dl, r["delta_lag"])
    print("rel-L2: delta_eul %.3g" % rel_l2(de, r["delta_eul"]))
    assert rel_l2(de, r["delta_eul"]) < tol
    assert rel_l2(e.fetch("deltaX"), r["delta_eul"]) < tol   # deltaX / pos* of the handle are the truth's
    w, nobs, noise = e.fetch("window"), e.fetch("nobs"), e.fetch("noise")
    assert np.array_equal(w, r["window"])                     # exact, no cell left out
    print("rel-L2: nobs %.3g noise %.3g" % (rel_l2(nobs, r["nobs"]), rel_l2(noise, r["noise"])))
    assert rel_l2(nobs, r["nobs"]) < tol
    assert np.array_equal(noise == 0, r["noise"] == 0) and rel_l2(noise, r["noise"]) < tol
    if clamps(p, o):
        assert np.array_equal((nobs == 0) & (w > 0), r["clamped"])
    else:
        assert not r["clamped"].any()
    assert used == r["words"]
    check_state(before, used, rng)


@pytest.mark.parametrize("case", mr.GRID + mr.VARIANTS, ids=mr.case_id)
def test_mock_data_equal_the_restatement(case):
    p, P, o, r, _ = mr.restate_case(case)
    mr.assert_margins(r)
    e = engine_for(p, P)
    rng = GslMT19937(case[1])
    before = rng.copy()
    used, dl, de = run(e, rng, o)
    check(e, p, o, r, before, rng, used, dl, de)
    e.close()


def test_all_five_guesses():
    from oracle.oracle import Oracle
    n, seed = 16, 7
    p = mr.params(n)
    P = mr.power(p)
    e = engine_for(p, P)
    ff = np.sin(np.arange(p.N, dtype=np.float64))
    orc = Oracle(p)
    for guess in (0, 1, 2, 3, 4):
        rng, ref = GslMT19937(seed), GslMT19937(seed)
        rng.raw(211), ref.raw(211)
        before = rng.copy()
        used = e.make_initial_guess(rng, guess, file_field=ff, smoothing_type=1, smoothing_scale=3 * p.d)
        used_r, sig = mr.make_initial_guess(p, P, ref, guess, file_field=ff, smoothing_scale=3 * p.d, oracle=orc)
        assert used == used_r and (used > 0) == (guess >= 2)
        check_state(before, used, rng)
        q = e.chain_get_state()
        if guess == 0:
            assert not q.any()
        else:
            close(q, sig)
    assert e.make_initial_guess(None, 0) == 0
    with pytest.raises(BchmcError) as ei:
        e.make_initial_guess(GslMT19937(1), 3, smoothing_type=2, smoothing_scale=1.0)
    assert ei.value.code == 1
    with pytest.raises(BchmcError) as ei:
        e.make_initial_guess(GslMT19937(1), 5)
    assert ei.value.code == 1
    e.close()


def test_a_run_from_its_seed():
    """Mock data, initial guess and three samples of HamiltonianMC(momenta="mt19937") from ONE seeded generator ==
    the same loop on an engine that was uploaded the restatement's arrays and state: same Neps, epsilon, accept
    sequence and final generator state."""
    from barcode_amd import hamil
    case = mr.GRID[0]
    p, P, o, r, after = mr.restate_case(case)
    mass_f = inputs.inverse_power_mass(P)
    eps = 0.1 * p.eps_heuristic()
    ref = after.copy()
    _, guess = mr.make_initial_guess(p, P, ref, 4)
    logs = []
    for built in (True, False):
        if built:
            hd = hamil.HamilData(p, N_eps_fac=4.0, eps_fac=4 * eps, signal_PS=P, mass_f=mass_f)
            rng = GslMT19937(case[1])
            run(hd.engine, rng, o, deltas=False)
            hd.engine.make_initial_guess(rng, 4)
        else:
            hd = hamil.HamilData(p, N_eps_fac=4.0, eps_fac=4 * eps, signal_PS=P, mass_f=mass_f, window=r["window"],
                                 nobs=r["nobs"], noise=r["noise"])
            hd.engine.chain_set_state(guess)
            rng = ref.copy()
        log = []
        for _ in range(3):
            log += hamil.HamiltonianMC(hd, rng, itmax=50, momenta="mt19937")
        logs.append((log, rng.get_state()))
        hd.engine.close()
    (a, sa), (b, sb) = logs
    assert len(a) == len(b) and sum(x["accepted"] for x in a) == 3
    for ra, rb in zip(a, b):
        assert ra["Neps"] == rb["Neps"] and ra["epsilon"] == rb["epsilon"] and ra["accepted"] == rb["accepted"]
    assert sa[1] == sb[1] and np.array_equal(sa[0], sb[0])


def test_built_arrays_act_like_uploaded_ones_and_repeat_bitwise():
    """Deterministic handles: two calls from the same state give bit-identical arrays, and a handle uploaded with the
    fetched window / nobs / noise gives the bit-identical bchmc_gradient."""
    case = mr.GRID[1]
    p, P, o, r, _ = mr.restate_case(case)
    e = engine_for(p, P, deterministic=1)
    out = []
    for _ in range(2):
        rng = GslMT19937(case[1])
        used, dl, de = run(e, rng, o)
        out.append((used, dl, de, e.fetch("window"), e.fetch("nobs"), e.fetch("noise"), rng.get_state()))
    for x, y in zip(out[0][:6], out[1][:6]):
        assert np.array_equal(x, y)
    assert out[0][6][1] == out[1][6][1] and np.array_equal(out[0][6][0], out[1][6][0])
    q = 0.5 * r["delta_lag"]
    g = e.gradient(q)
    e2 = engine_for(p, P, deterministic=1)
    e2.upload(window=out[0][3], nobs=out[0][4], noise=out[0][5])
    assert np.array_equal(e2.gradient(q), g)
    e.close(), e2.close()


def test_segment_boundaries_and_continuation_are_invisible(monkeypatch):
    case = (32, 2, dict(), dict(window_type=23, random_test_rsd=True))
    p, P, o, r, _ = mr.restate_case(case)
    out = []
    for env in ({}, {"BCHMC_MT_SEGMENT_WORDS": "624"}, {"BCHMC_MT_CAPACITY": "40000"},
                {"BCHMC_MT_SEGMENT_WORDS": "1248", "BCHMC_MT_CAPACITY": "30000"}):
        for k in ("BCHMC_MT_SEGMENT_WORDS", "BCHMC_MT_CAPACITY"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = engine_for(p, P, deterministic=1)
        rng = GslMT19937(case[1])
        used, dl, de = run(e, rng, o)
        used_g = e.make_initial_guess(rng, 4)
        out.append((used, dl, de, e.fetch("window"), e.fetch("nobs"), e.fetch("noise"), used_g, e.chain_get_state(),
                    rng.get_state()))
        e.close()
    assert out[0][0] == r["words"]
    for o_ in out[1:]:
        for x, y in zip(o_[:8], out[0][:8]):
            assert np.array_equal(x, y)
        assert o_[8][1] == out[0][8][1] and np.array_equal(o_[8][0], out[0][8][0])


def test_fp32_handle_draws_the_same_stream():
    """No threshold in play (window of ones, negative_obs): words and state exact, fields to float accuracy --
    delta_lag to the exact momentum draw's fp32 figure, delta_eul / nobs to what test_fp32_field_mode holds deltaX to."""
    case = (32, 1, dict(), dict(negative_obs=True))
    p, P, o, r, _ = mr.restate_case(case)
    mr.assert_margins(r)
    e = engine_for(p, P, precision=1)
    rng = GslMT19937(case[1])
    before = rng.copy()
    used, dl, de = run(e, rng, o)

    def lag(a, b):
        assert rel_l2(a, b) < 1e-6

    check(e, p, o, r, before, rng, used, dl, de, tol=10 * TOL_F32_FIELD, lag=lag)
    e.close()


def test_error_paths():
    n = 16
    for like, ok, code, text in ((0, dict(), 5, "Poissonian"), (2, dict(data_model=0), 1, "linear data model was chosen"),
                                 (1, dict(data_model=2), 1, "data_model = 2"), (1, dict(window_type=2), 1, "window_type"),
                                 (1, dict(sigma_min=0., sigma_fac=0.), 9, "noise = 0 found! Index 0")):
        p = mr.params(n, likelihood=like)
        e = engine_for(p, mr.power(p))
        rng = GslMT19937(3)
        rng.raw(17)
        before = rng.get_state()
        with pytest.raises(BchmcError) as ei:
            run(e, rng, mr.MockOpts(**ok))
        assert ei.value.code == code and text in str(ei.value)
        after = rng.get_state()
        assert before[1] == after[1] and np.array_equal(before[0], after[0])   # the caller's generator is untouched
        e.close()
    p = mr.params(n)
    e = Engine(p)
    with pytest.raises(BchmcError) as ei:
        run(e, GslMT19937(3), mr.MockOpts())
    assert ei.value.code == 9 and "signal_PS" in str(ei.value)
    with pytest.raises(BchmcError) as ei:
        e.make_initial_guess(GslMT19937(3), 2)
    assert ei.value.code == 9
    e.close()


def test_256_mock_data_against_the_oracle():
    """256^3 set up like the big cases of tests/test_gpu_large.py, MockOpts defaults: the truth against
    orc.create_GARFIELD, its forward model against Oracle.Lag2Eul (OpenMP build), the noise against
    orc.ugaussian_stream; the first seed from 1 on whose restatement keeps every cell 1e-9 away from the clamp's edge."""
    from oracle import oracle as orc
    from oracle.oracle import Oracle
    p = HamilParams(Nx=256, L=200.0, likelihood=1, rsd_model=1, sfmodel=2)
    P = mr.power(p)
    o = mr.MockOpts()
    N = p.N
    orc_h = Oracle(p, omp=True)
    for seed in range(1, 6):
        dl_r = orc.create_GARFIELD(p.Nx, p.L, P, seed)
        de_r = orc_h.Lag2Eul(dl_r, rsd=0)[0]
        g = orc.ugaussian_stream(seed, 3 * N)[2 * N:]
        w = mr.window_of(o.window_type, de_r)
        nobs, noise, clamped, edges = mr.observe(p, o, dl_r, de_r, w, g, np.ones(N))   # sigma = 1: g = 1 * g * 1
        if all(v > mr.EDGE for v in edges.values()):
            break
    else:
        pytest.fail("no seed in 1..5 keeps the 256^3 case away from the thresholds")
    print("256^3: seed %d, edges %s" % (seed, edges))
    r = dict(delta_lag=dl_r, delta_eul=de_r, window=w, nobs=nobs, noise=noise, clamped=clamped,
             words=mr.words_for(GslMT19937(seed), 3 * N))
    e = engine_for(p, P)
    rng = GslMT19937(seed)
    before = rng.copy()
    used, dl, de = run(e, rng, o)
    check(e, p, o, r, before, rng, used, dl, de)
    e.close()


def test_cpp_shim_and_the_mock_module_follow_the_engine(tmp_path):
    """bchmc_shim::setup_random_test / make_initial_guess (the caller's arrays receive what was built) and
    barcode_amd.mock.load_initial_fields with its dumps give the engine's arrays, state and generator."""
    from barcode_amd import hamil, io, mock
    from barcode_amd.shim import ShimHamil
    case = mr.VARIANTS[4]   # sigma_fac = 0.3
    p, P, o, r, after = mr.restate_case(case)
    mass_f = inputs.inverse_power_mass(P)
    ref = after.copy()
    _, guess = mr.make_initial_guess(p, P, ref, 2)
    own = {k: np.full(p.N, -7.) for k in ("window", "nobs", "noise")}
    hs = ShimHamil(p, signal_PS=P, mass_f=mass_f, **own)
    rng = GslMT19937(case[1])
    dl, de = hs.setup_random_test(rng, sigma_min=o.sigma_min, sigma_fac=o.sigma_fac)
    close(dl, r["delta_lag"])
    assert rel_l2(de, r["delta_eul"]) < TOL_FIELD
    kept = hs._keep
    assert np.array_equal(kept["window"], r["window"]) and rel_l2(kept["nobs"], r["nobs"]) < TOL_FIELD
    assert rel_l2(kept["noise"], r["noise"]) < TOL_FIELD
    assert np.array_equal((kept["nobs"] == 0) & (kept["window"] > 0), r["clamped"])
    hs.make_initial_guess(rng, 2)
    close(hs.chain_get_state(), guess)
    assert rng.get_state()[1] == ref.get_state()[1] and np.array_equal(rng.get_state()[0], ref.get_state()[0])
    with pytest.raises(RuntimeError, match="window_type"):
        hs.setup_random_test(rng, window_type=5)
    hs.close()

    hd = hamil.HamilData(p, signal_PS=P, mass_f=mass_f)
    m = mock.MockParams(seed=case[1], sigma_fac=o.sigma_fac, initial_guess=2, dir=str(tmp_path), N_bin=20)
    rng = GslMT19937(m.seed)
    mock.load_initial_fields(hd, rng, m)
    assert rng.get_state()[1] == ref.get_state()[1] and np.array_equal(rng.get_state()[0], ref.get_state()[0])
    assert np.array_equal(io.read_array(str(tmp_path / "win"), p.N), r["window"])
    assert rel_l2(io.read_array(str(tmp_path / "nobs"), p.N), r["nobs"]) < TOL_FIELD
    assert rel_l2(io.read_array(str(tmp_path / "sigma"), p.N), r["noise"]) < TOL_FIELD
    close(io.read_array(str(tmp_path / "deltaLAGtest"), p.N), r["delta_lag"])
    close(io.read_array(str(tmp_path / "initial_guess"), p.N), guess)
    assert (tmp_path / "spec_initial_guess.dat").read_text().count("\n") > 5
    # the same arrays from files (random_test = false), the guess read back from its dump
    hd2 = hamil.HamilData(p, signal_PS=P, mass_f=mass_f)
    m2 = mock.MockParams(random_test=False, initial_guess=1, initial_guess_file="initial_guess", dir=str(tmp_path))
    mock.load_initial_fields(hd2, GslMT19937(1), m2)
    assert np.array_equal(hd2.engine.fetch("nobs"), hd.engine.fetch("nobs"))
    close(hd2.engine.chain_get_state(), guess)
    hd.engine.close(), hd2.engine.close()
