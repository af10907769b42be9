"""bchmc_poisson_* without a GPU: the restatement's own sanity (Philox known answers, the distribution of its counts at
seven rates), and the declarations through every layer (header, library, engine.py, hamil.py, mock.py, io.py).

The distribution checks hold the numpy restatement of the header's sampler (tests/poisson_restatement.py) to the Poisson
law on 32^3 constant fields, seed 12345, stream 0; the GPU tests then hold the device to the restatement cell by cell.
Bounds: |mean - lambda| < 5 sqrt(lambda / N); variance / lambda within 5 sqrt((2 + 1 / lambda) / N) of 1 (the variance of
the sample variance of a Poisson law is lambda^2 (2 + 1 / lambda) / N to leading order); chi^2 against
scipy.stats.poisson over bins of expected count >= 5 with p > 1e-6; no cell at a cap.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
from scipy import stats

from tests import poisson_restatement as pr
from tests.test_catalogue_cpu import _fields, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = (0.05, 1.0, 9.99, 10.0, 37.5, 1000.0, 1e6)
SEED, NCELL = 12345, 32 ** 3


def header_args(name):
    """The parameter types of a prototype in bchmc.h, comments removed; an array parameter `T a[n]` reads `T *`."""
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    decl = re.search(r"\bint %s\(([^)]*)\);" % name, text).group(1)
    out = []
    for a in decl.split(","):
        a = " ".join(a.split())
        array = re.search(r"\[\d+\]$", a) is not None
        m = re.match(r"^(.*?)(\w+)$", re.sub(r"\[\d+\]$", "", a))
        out.append(m.group(1).strip() + (" *" if array else ""))
    return out


def test_restatement_philox_known_answers():
    """The three Random123 vectors of tests/test_gpu_chain.py."""
    f = 0xffffffff
    for ctr, key, want in (([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                           ([f, f, f, f], [f, f], [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
                            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        got = pr.philox4x32_10(*(np.array([c], dtype=np.uint64) for c in ctr), *key)
        assert [int(g[0]) for g in got] == want


def test_uniforms_lie_inside_the_unit_interval_and_depend_on_every_argument():
    c = np.arange(4096)
    u, v = pr.uniforms(c, 0, 0, SEED)
    assert u.min() > 0 and u.max() <= 1 and v.min() > 0 and v.max() <= 1
    for other in (pr.uniforms(c, 1, 0, SEED), pr.uniforms(c, 0, 1, SEED), pr.uniforms(c, 0, 0, SEED + 1),
                  pr.uniforms(c + 4096, 0, 0, SEED)):
        assert not np.array_equal(other[0], u)
    # the counter takes the cell's high word: cells 2^32 apart differ
    assert pr.uniforms([5], 0, 0, SEED)[0][0] != pr.uniforms([5 + 2 ** 32], 0, 0, SEED)[0][0]


@pytest.fixture(scope="module", params=LAMBDAS, ids=lambda l: "lambda%g" % l)
def sample(request):
    lam = request.param
    return lam, pr.counts(np.full(NCELL, lam), SEED, 0)


def test_restatement_mean_and_variance(sample):
    lam, r = sample
    k = r["counts"].astype(np.float64)
    sigma = abs(k.mean() - lam) / np.sqrt(lam / NCELL)
    ratio = k.var(ddof=1) / lam
    print("lambda %g: mean off by %.2f sigma, variance / lambda = %.4f, PTRS iterations <= %d" % (lam, sigma, ratio, r["iters"]))
    assert sigma < 5
    assert abs(ratio - 1) < 5 * np.sqrt((2 + 1 / lam) / NCELL)


def test_restatement_chi_square_and_caps(sample):
    lam, r = sample
    k = r["counts"]
    assert not r["capped"].any() and r["bad"] == -1
    lo = max(0, int(np.floor(lam - 12 * np.sqrt(lam) - 10)))
    hi = int(np.ceil(lam + 12 * np.sqrt(lam) + 20))
    ks = np.arange(lo, hi + 1)
    exp = NCELL * stats.poisson.pmf(ks, lam)
    exp[0] += NCELL * stats.poisson.cdf(lo - 1, lam)
    exp[-1] += NCELL * stats.poisson.sf(hi, lam)
    obs = np.bincount(np.clip(k, lo, hi) - lo, minlength=ks.size).astype(np.float64)
    # bins of expected count >= 5: consecutive k merged from the left, the remainder into the last bin
    e_bins, o_bins, e_acc, o_acc = [], [], 0.0, 0.0
    for e, o in zip(exp, obs):
        e_acc, o_acc = e_acc + e, o_acc + o
        if e_acc >= 5:
            e_bins.append(e_acc), o_bins.append(o_acc)
            e_acc = o_acc = 0.0
    e_bins[-1] += e_acc
    o_bins[-1] += o_acc
    e_bins, o_bins = np.array(e_bins), np.array(o_bins)
    assert len(e_bins) >= 2 and abs(e_bins.sum() - NCELL) < 1e-6 * NCELL and o_bins.sum() == NCELL
    chi2 = float(np.sum((o_bins - e_bins) ** 2 / e_bins))
    p = float(stats.chi2.sf(chi2, len(e_bins) - 1))
    print("lambda %g: chi^2 = %.1f over %d bins, p = %.3g" % (lam, chi2, len(e_bins), p))
    assert p > 1e-6


def test_restatement_edges():
    """lambda <= 0 and cells outside the window draw nothing; NaN, +inf and a rate above 2^30 are refused, the first
    such index named; -inf is lambda <= 0.  Constant inversion fields have no tight cell at 1e-9."""
    lam = np.array([0.0, -3.0, -np.inf, 5.0, 5.0, 2.0 ** 30])
    r = pr.counts(lam, 7, 3, window=[1, 1, 1, 0, 1, 1])
    assert r["bad"] == -1 and list(r["counts"][:4]) == [0, 0, 0, 0] and np.isinf(r["margin"][:4]).all()
    for badval in (np.nan, np.inf, 2.0 ** 30 + 1):
        lam2 = lam.copy()
        lam2[4] = badval
        assert pr.counts(lam2, 7, 3)["bad"] == 4
        lam2[1] = badval
        assert pr.counts(lam2, 7, 3)["bad"] == 1
        assert pr.counts(lam2, 7, 3, window=[1, 0, 1, 1, 0, 1])["bad"] == -1  # outside the window nothing is looked at
    for l in (0.05, 1.0, 9.99):
        assert not (pr.counts(np.full(NCELL, l), SEED, 0)["margin"] < pr.TIGHT).any()
    assert np.array_equal(pr.rate([0.5, -1.0], 4.0, 0), [6.0, 0.0]) and np.array_equal(pr.rate([0.5], 4.0, 1), [2.0])


def test_restatement_positions_follow_upstreams_order():
    cnt = np.array([0, 3, 0, 0, 2, 0, 0, 1] + [0] * 19)  # 27 cells, n_in = 3
    x, y, z = pr.positions(cnt, 9, 2, 3, 6.0)
    assert x.size == 6
    cells = [1, 1, 1, 4, 4, 7]
    for p, c in enumerate(cells):
        k, j, i = c % 3, (c // 3) % 3, c // 9
        for v, a in ((x[p], i), (y[p], j), (z[p], k)):
            assert 2.0 * a <= v < 2.0 * (a + 1)
    xs, ys, zs = pr.positions(cnt, 9, 2, 3, 6.0, first=2, m=3)  # a piece that cuts through two cells
    assert np.array_equal(xs, x[2:5]) and np.array_equal(ys, y[2:5]) and np.array_equal(zs, z[2:5])
    assert pr.positions(np.zeros(8, dtype=np.int64), 9, 2, 2, 1.0)[0].size == 0


# ---- the declarations through the layers ---------------------------------------------------------------------------------

def test_header_prototypes_match_the_engines_argtypes():
    from barcode_amd import engine
    text = header()
    assert "#define BCHMC_ABI_VERSION 4" in text
    ct = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double, "uint64_t": C.c_uint64}
    assert [(n, ct[t]) for n, t in _fields("bchmc_poisson_opts")] == list(engine.PoissonOpts._fields_)
    assert [(n, ct[t]) for n, t in _fields("bchmc_poisson_stats")] == list(engine.PoissonStats._fields_)
    assert C.sizeof(engine.PoissonOpts) == 32 and C.sizeof(engine.PoissonStats) == 40
    dp, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    ctype = {"bchmc_handle *": C.c_void_p, "bchmc_corr_source": C.c_int, "const double *": dp, "double *": dp,
             "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "uint64_t *": C.POINTER(C.c_uint64),
             "int32_t *": C.POINTER(C.c_int32), "uint32_t *": u32p,
             "const bchmc_poisson_opts *": C.POINTER(engine.PoissonOpts), "bchmc_poisson_stats *": C.POINTER(engine.PoissonStats),
             "const bchmc_density_opts *": C.POINTER(engine.DensityOpts), "bchmc_density_stats *": C.POINTER(engine.DensityStats),
             "const bchmc_mock_opts *": C.POINTER(engine.MockOpts)}
    lib = engine.load()
    raw = C.CDLL(engine.LIB_PATH)
    for name in ("bchmc_poisson_draw", "bchmc_poisson_positions", "bchmc_poisson_density", "bchmc_poisson_release",
                 "bchmc_setup_random_test_poisson"):
        want = [ctype[a] for a in header_args(name)]
        assert list(getattr(lib, name).argtypes) == want, name
        assert name in engine.EXPORTS and hasattr(raw, name)
    doc = text[text.index("Poisson samples of a density field"):text.index("typedef struct bchmc_poisson_opts")]
    for k in range(1, 9):
        assert re.search(r"\bP%d\b" % k, doc), "property P%d" % k
    assert text.count("Added within ABI version 4: no struct or existing entry point changed") >= 4
    # a null handle: BCHMC_ERR_ARG without touching a device
    o = engine.PoissonOpts(1, 0, 0, 1.0, 0, -1)
    x = np.zeros(1)
    p = x.ctypes.data_as(dp)
    assert lib.bchmc_poisson_draw(None, 0, p, 1, C.byref(o), p, None) == 1
    assert lib.bchmc_poisson_positions(None, 0, 0, p, p, p) == 1
    assert lib.bchmc_poisson_density(None, None, p, None) == 1
    assert lib.bchmc_poisson_release(None) == 1
    assert lib.bchmc_setup_random_test_poisson(None, None, None, None, None, 1, 0, None, None) == 1


def test_python_layers_bind_the_new_names(tmp_path, monkeypatch):
    from barcode_amd import engine, hamil, input_par, io, mock, shim
    lib = shim.load()
    for name in ("bchmc_shim_discrete_poisson_sample", "bchmc_shim_poisson_positions", "bchmc_shim_poisson_upres",
                 "bchmc_shim_setup_random_test_poisson"):
        assert name in shim.SHIM_EXPORTS and getattr(lib, name).argtypes
    text = open(os.path.join(ROOT, "include", "bchmc_shim.hpp")).read()
    assert "-> bchmc_shim::discrete_poisson_sample" in text[:text.index("#ifndef BCHMC_SHIM_HPP")]  # the opening name map
    assert re.search(r"discrete_poisson_sample\(HamilView \*hd, const real_prec \*lambda, unsigned N1", text)
    assert re.search(r"void poisson_upres\(HamilView \*hd, const real_prec \*delta, unsigned N1, real_prec Nbar", text)
    assert re.search(r"void setup_random_test\(HamilView \*hd.*?const uint64_t \*poisson_seed = nullptr", text, flags=re.S)
    for name in ("discrete_poisson_sample", "poisson_upres"):
        assert callable(getattr(shim.ShimHamil, name))
    assert "poisson_seed" in inspect.signature(shim.ShimHamil.setup_random_test).parameters
    for name in ("poisson_draw", "poisson_positions", "poisson_density", "poisson_release", "setup_random_test_poisson"):
        assert callable(getattr(engine.Engine, name)), name
    assert list(inspect.signature(hamil.discrete_poisson_sample).parameters)[:4] == ["hd", "field", "Nbar", "seed"]
    sig = inspect.signature(hamil.poisson_upres)
    assert list(sig.parameters)[:5] == ["hd", "field", "Nbar", "seed", "mk"] and sig.parameters["mk"].default == 1
    assert mock.MockParams().poisson_seed is None and "poisson_seed" in mock.__doc__
    assert "poisson_seed" not in inspect.getsource(input_par.mock_params)  # input.par has no such key: it stays None
    with pytest.raises(ValueError):
        engine.Engine.poisson_density(None, download=False)
    # the tool's default output name (tools/poisson_upres.cc:88) and its writer
    assert io.poisson_filename("deltaEUL_12", 256, 8) == "deltaEUL_12_poisCIC256_Nbar8"
    assert io.poisson_filename("in", "128", "0.50") == "in_poisCIC128_Nbar0.50"
    monkeypatch.chdir(tmp_path)
    rho = np.arange(8, dtype=np.float64)
    path = io.dump_poisson(rho, "field", 2, 8)
    assert path == "field_poisCIC2_Nbar8.dat" and np.array_equal(io.read_array("field_poisCIC2_Nbar8", 8), rho)
    assert io.dump_poisson(rho, "field", 2, 8, fname_out="other") == "other.dat"


def test_documents_name_the_feature():
    for doc, words in (("README.md", ("bchmc_poisson_draw",)),
                       ("DESIGN.md", ("9.10", "k_pois_counts", "k_pois_positions", "poisson_bench"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
