"""CPU side of the device mock data (no GPU): tests/mock_restatement.py is pinned to the oracle's C stream and checked
rule by rule on hand-sized inputs; the new input.par mapping; the library's new entry points and their ctypes
signatures; and, for exactly the cases tests/test_gpu_mock.py runs, the margins that let that file demand exact window
and clamp masks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from barcode_amd import engine
from barcode_amd.gsl_mt19937 import GslMT19937
from barcode_amd.params import HamilParams
from tests import mock_restatement as mr
from tests.test_gpu_mt19937_draw import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,seed", [(8, 5), (16, 1)])
def test_restatement_is_pinned_to_the_oracles_stream(n, seed):
    """Truth == orc.create_GARFIELD from the same seed; the Gaussians handed to the noise are numbers 2N .. 3N of
    orc.ugaussian_stream (window of ones, sigma = 1: gsl_ran_gaussian(1) is the unit Gaussian), by the momentum draw's
    criterion: numpy's log / sqrt and the C library's may differ in the last bit."""
    from oracle import oracle as orc
    p = mr.params(n)
    P = mr.power(p)
    rng = GslMT19937(seed)
    r = mr.setup_random_test(p, P, rng, mr.MockOpts(negative_obs=True))
    close(r["delta_lag"], orc.create_GARFIELD(n, p.L, P, seed))
    g = orc.ugaussian_stream(seed, 3 * p.N)[2 * p.N:]
    close(r["gaussians"], g)
    close(r["nobs"], p.rho_c * (1. + r["delta_eul"]) + g)
    assert np.array_equal(r["noise"], np.ones(p.N)) and np.array_equal(r["window"], np.ones(p.N))
    ref = GslMT19937(seed)
    ref.raw(r["words"])
    assert ref.get_state()[1] == rng.get_state()[1] and np.array_equal(ref.get_state()[0], rng.get_state()[0])


# eight cells: empty, below delta_min, at 0, just under / over the window's threshold, dense, two ordinary ones
DE = np.array([-1., -0.9995, 0., 2.9, 3.1, 5., -0.5, 1.])
DL = np.array([0.3, -0.2, 0.1, 1.5, -2., 0.7, 0., -1.])
Y = np.array([0.5, -0.9, 0.25, -0.75, 0.1, 0.6, -0.3, 0.8])
ROOT_ = np.array([1.5, 2.5, 0.7, 1.1, 3., 0.2, 1.9, 1.3])


def _serial(p, o, window):
    """barcoderunner.cc:117-188 as its loop, one cell at a time."""
    nobs, noise, clamped, k = [], [], [], 0
    for i in range(DE.size):
        sig, cl = 0., False
        if o.data_model == 0:
            Lam = p.rho_c * (1. + DE[i])
            v = 0.
            if window[i] > 0:
                if p.likelihood == 1:
                    sig = o.sigma_min + o.sigma_fac * Lam
                    v = Lam + sig * Y[k] * ROOT_[k]
                    if not o.negative_obs and v < 0:
                        v, cl = 0., True
                else:
                    sig = o.sigma_min + o.sigma_fac * (DL[i] * DL[i])
                    v = DL[i] + sig * Y[k] * ROOT_[k]
                k += 1
        else:
            Lam = math.log(p.rho_c * (1. + max(DE[i], p.delta_min)))
            if window[i] > 0:
                sig = o.sigma_fac
                v = Lam + sig * Y[k] * ROOT_[k]
                k += 1
            else:
                v = math.log((p.rho_c * (1 + p.delta_min)) ** 2)
        nobs.append(v), noise.append(sig), clamped.append(cl)
    return np.array(nobs), np.array(noise), np.array(clamped), k


@pytest.mark.parametrize("window_type,count", [(1, 8), (10, 4), (23, 2)])
@pytest.mark.parametrize("likelihood,data_model", [(1, 0), (3, 0), (2, 1)])
@pytest.mark.parametrize("negative_obs", [False, True])
def test_rules_on_hand_sized_inputs(window_type, count, likelihood, data_model, negative_obs):
    p = HamilParams(Nx=2, likelihood=likelihood, rho_c=1.5)
    o = mr.MockOpts(window_type=window_type, data_model=data_model, negative_obs=negative_obs, sigma_min=0.5,
                    sigma_fac=0.3)
    w = mr.window_of(window_type, DE)
    assert int(w.sum()) == count
    if window_type == 10:
        assert np.array_equal(w, [0, 0, 0, 0, 1, 1, 1, 1])
    if window_type == 23:
        assert np.array_equal(w, [0, 0, 0, 0, 1, 1, 0, 0])
    nobs, noise, clamped, edges = mr.observe(p, o, DL, DE, w, Y[:count], ROOT_[:count])
    nobs_s, noise_s, clamped_s, used = _serial(p, o, w)
    assert used == count
    assert np.array_equal(nobs, nobs_s) and np.array_equal(noise, noise_s) and np.array_equal(clamped, clamped_s)
    if likelihood == 1 and window_type == 1:
        assert clamped[1] == (not negative_obs)   # Lambda = 0.00075, g = -1.1 sigma: negative before the clamp
    if data_model == 1:
        assert nobs[0] == nobs_s[0] and (window_type != 1 or noise[0] == 0.3)
        assert abs(edges["delta_min"] - 0.0005) < 1e-12
    if window_type == 23:
        assert abs(edges["window"] - 0.1) < 1e-12


def test_error_cases():
    with pytest.raises(ValueError, match="linear data model was chosen"):
        mr.check_opts(HamilParams(Nx=4, likelihood=2), mr.MockOpts(data_model=0))
    with pytest.raises(ValueError, match="data_model = 2"):
        mr.check_opts(HamilParams(Nx=4), mr.MockOpts(data_model=2))
    with pytest.raises(ValueError, match="window_type = 3"):
        mr.check_opts(HamilParams(Nx=4), mr.MockOpts(window_type=3))
    with pytest.raises(NotImplementedError):
        mr.check_opts(HamilParams(Nx=4, likelihood=0), mr.MockOpts())
    o = mr.MockOpts(sigma_min=0., sigma_fac=0.)
    with pytest.raises(RuntimeError, match="noise = 0 found! Index 0"):
        mr.observe(HamilParams(Nx=2), o, DL, DE, np.ones(8), Y, ROOT_)
    with pytest.raises(RuntimeError, match="Index 4"):
        mr.observe(HamilParams(Nx=2), o, DL, DE, mr.window_of(10, DE), Y[:4], ROOT_[:4])


def test_all_five_guesses():
    from oracle import oracle as orc
    from oracle.oracle import Oracle
    n, seed = 8, 11
    p = mr.params(n)
    P = mr.power(p)
    ff = np.arange(p.N, dtype=np.float64)
    for guess in (0, 1):
        rng = GslMT19937(seed)
        used, sig = mr.make_initial_guess(p, P, rng, guess, file_field=ff)
        assert used == 0 and np.array_equal(sig, ff if guess else np.zeros(p.N))
        assert rng.get_state()[1] == GslMT19937(seed).get_state()[1]
    rng = GslMT19937(seed)
    used2, grf = mr.make_initial_guess(p, P, rng, 2)
    close(grf, orc.create_GARFIELD(n, p.L, P, seed))
    rng3 = GslMT19937(seed)
    used3, sm = mr.make_initial_guess(p, P, rng3, 3, smoothing_scale=2 * p.d)
    assert used3 == used2 and np.array_equal(sm, Oracle(p).convcomp(grf, 2 * p.d))
    assert np.var(sm) < 0.7 * np.var(grf)
    rng4 = GslMT19937(seed)
    used4, noise = mr.make_initial_guess(p, P, rng4, 4)
    g = orc.ugaussian_stream(seed, p.N)
    close(noise, 0.1 * g)
    y, root = mr.split_stream(GslMT19937(seed), p.N)[1:]
    assert np.array_equal(noise, 0.1 * y * root)   # GSL's product order
    with pytest.raises(ValueError, match=r"invalid choice of initial_guess \(5\)"):
        mr.make_initial_guess(p, P, rng, 5)


def test_input_par_mapping_of_the_reference_template():
    from barcode_amd import input_par
    from barcode_amd.mock import MockParams
    path = os.path.join(ROOT, "tests", "golden", "reference_template_input.par")
    kw = input_par.mock_params(path)
    assert kw["random_test"] is True and kw["random_test_rsd"] is False and kw["negative_obs"] is False
    assert (kw["window_type"], kw["data_model"], kw["likelihood"], kw["initial_guess"], kw["seed"]) == (1, 0, 1, 0, 1)
    assert (kw["sigma_min"], kw["sigma_fac"]) == (1.0, 0.0)
    assert kw["initial_guess_file"] == "deltaLAGtest" and kw["initial_guess_smoothing_type"] == 1
    assert kw["initial_guess_smoothing_scale"] == 20.0 and kw["N_bin"] == 200
    m = MockParams(**kw)
    assert m.seed == 1 and m.dir == ""
    for bad in (dict(data_model=1), dict(likelihood=2)):
        with pytest.raises(RuntimeError, match="incompatible data_model and likelihood"):
            input_par.mock_params(path, **bad)
    assert input_par.mock_params(path, data_model=1, likelihood=2)["data_model"] == 1


CTYPE = {"bchmc_handle *": C.c_void_p, "const bchmc_mock_opts *": C.POINTER(engine.MockOpts),
         "uint32_t [624]": C.POINTER(C.c_uint32), "int32_t *": C.POINTER(C.c_int32), "uint64_t *": C.POINTER(C.c_uint64),
         "double *": C.POINTER(C.c_double), "const double *": C.POINTER(C.c_double), "int32_t": C.c_int32,
         "double": C.c_double}


def _prototype(text, sym):
    args = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % sym, text, flags=re.S).group(1)
    out = []
    for a in args.split(","):
        m = re.match(r"\s*(.*?)\s*(\*?)\s*\b([A-Za-z_]\w*)\s*(\[\d+\])?\s*$", " ".join(a.split()))
        base, star, _, arr = m.groups()
        out.append(" ".join(x for x in (base, star, arr) if x))
    return out


def test_library_exports_the_mock_entry_points_with_the_headers_signatures():
    """The library loads without a GPU; the entry points are declared, exported and bound with the header's types."""
    text = open(os.path.join(ROOT, "include", "bchmc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(engine.LIB_PATH)
    lib = engine.load()
    for sym in ("bchmc_setup_random_test", "bchmc_make_initial_guess"):
        assert hasattr(raw, sym), sym
        assert sym in engine.EXPORTS
        assert getattr(lib, sym).argtypes == [CTYPE[t] for t in _prototype(text, sym)], sym
    fields = re.search(r"typedef struct bchmc_mock_opts \{(.*?)\}", text, flags=re.S).group(1)
    names = []
    for decl in fields.split(";"):
        decl = decl.strip()
        if decl:
            ctype = C.c_int32 if decl.startswith("int32_t") else C.c_double
            names += [(n.strip(), ctype) for n in decl.split(None, 1)[1].split(",")]
    assert names == list(engine.MockOpts._fields_)
    for name in ("setup_random_test", "make_initial_guess"):
        assert callable(getattr(engine.Engine, name))
    from barcode_amd import mock
    for name in ("setup_random_test", "make_initial_guess", "load_initial_fields"):
        assert callable(getattr(mock, name))


@pytest.mark.parametrize("case", mr.GRID + mr.VARIANTS, ids=mr.case_id)
def test_margins_of_the_gpu_cases(case):
    """No cell of a case of tests/test_gpu_mock.py lies within 1e-9 of a threshold, and the masks are real masks."""
    p, P, o, r, _ = mr.restate_case(case)
    mr.assert_margins(r)
    if o.window_type == 23:
        assert 0 < r["window"].sum() < p.N
    if o.data_model == 0 and p.likelihood == 1 and not o.negative_obs:
        assert "clamp" in r["edges"] and (r["clamped"].any() or o.window_type == 23)   # Lambda > 4 under window 23
    if o.window_type != 23 and case in mr.GRID:
        assert abs(r["delta_eul"] - 3).min() > mr.EDGE and abs(r["delta_eul"] - p.delta_min).min() > mr.EDGE
