"""CPU checks around the ensemble accumulators and the cross-spectrum: the numpy restatement
(tests/ensemble_restatement.py) against a two-pass longdouble mean and variance, known answers of the cross-spectrum, the
host-side RunningBins, the declarations of the new entry points through every layer, and the file writer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from barcode_amd import io
from barcode_amd.ensemble import RunningBins
from tests import ensemble_restatement as er
from tests.test_corr_restatement import CTYPE, header_args, rel_max
from tests.util import TOL_FIELD, Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CELLS = 512
NEW_SYMBOLS = ("bchmc_measure_cross_spectrum", "bchmc_ensemble_add", "bchmc_ensemble_count", "bchmc_ensemble_fetch",
               "bchmc_ensemble_merge", "bchmc_ensemble_reset", "bchmc_ensemble_release")
CTYPE_NEW = dict(CTYPE, **{"int32_t": C.c_int32, "bchmc_ens_what": C.c_int})


def samples_of(count, offset, seed=11):
    rng = np.random.Generator(np.random.Philox(seed))
    return offset + rng.standard_normal((count, CELLS))


def box_of(n):
    return 200. * n / 64.


# ---- Welford and Chan against two passes in longdouble --------------------------------------------------------------
@pytest.mark.parametrize("offset", (0., 1e3), ids=("zero-mean", "offset-1e3"))
@pytest.mark.parametrize("count", (7, 33))
def test_welford_and_chan_against_two_pass_longdouble(count, offset):
    """Mean, ddof = 1 variance and standard deviation within TOL_FIELD of the largest reference value.  The worst case
    of the arithmetic itself on these samples is 8.6e-14 (offset 1e3, 33 samples, the variance: the one-pass sums lose
    the digits the offset takes), an 11-fold margin; at zero mean it is 4e-16."""
    s = samples_of(count, offset)
    mean0, var0 = er.two_pass(s)
    seq = er.Welford(CELLS)
    for x in s:
        seq.add(x)
    cut = count // 2
    a, b = er.Welford(CELLS), er.Welford(CELLS)
    for x in s[:cut]:
        a.add(x)
    for x in s[cut:]:
        b.add(x)
    a.merge(*b.export())
    assert seq.count == a.count == count
    for tag, w in (("welford", seq), ("chan", a)):
        lm = float(np.max(np.abs(w.mean - mean0)) / np.max(np.abs(mean0)))
        lv = float(np.max(np.abs(w.variance() - var0)) / np.max(np.abs(var0)))
        ls = float(np.max(np.abs(w.std() - np.sqrt(var0))) / np.max(np.sqrt(var0)))
        print("%s, %d samples, offset %g: mean %.2e, variance %.2e, std %.2e of max" % (tag, count, offset, lm, lv, ls))
        assert lm <= TOL_FIELD and lv <= TOL_FIELD and ls <= TOL_FIELD


def test_merge_edge_cases_and_non_finite_cells():
    s = samples_of(5, 0.5)
    w = er.Welford(CELLS)
    for x in s:
        w.add(x)
    before = w.export()
    w.merge(0, None, None)  # count 0: a no-op
    assert w.count == 5 and np.array_equal(w.mean, before[1]) and np.array_equal(w.m2, before[2])
    empty = er.Welford(CELLS).merge(*before)  # into an empty accumulator: a copy
    assert empty.count == 5 and np.array_equal(empty.mean, before[1]) and np.array_equal(empty.m2, before[2])
    for bad in (np.nan, np.inf, -np.inf):
        v = er.Welford(CELLS)
        for i, x in enumerate(s):
            x = x.copy()
            if i == 2:
                x[17] = bad
            v.add(x)
        nan = np.isnan(v.mean)
        assert nan[17] and nan.sum() == 1 and np.array_equal(np.isnan(v.variance()), nan)
        keep = ~nan
        assert np.array_equal(v.mean[keep], w.mean[keep]) and np.array_equal(v.m2[keep], w.m2[keep])


def test_running_bins_is_the_same_arithmetic():
    s = samples_of(9, 3.0)[:, :40].reshape(9, 5, 8)
    rb, w = RunningBins(), er.Welford(40)
    for x in s:
        rb.add(x)
        w.add(x)
    assert rb.count == 9 and rb.mean.shape == (5, 8)
    assert np.array_equal(rb.mean.ravel(), w.mean) and np.array_equal(rb.variance.ravel(), w.variance())
    assert np.array_equal(rb.std.ravel(), w.std())
    a, b = RunningBins(), RunningBins((5, 8))
    for x in s[:4]:
        a.add(x)
    for x in s[4:]:
        b.add(x)
    wa, wb = er.Welford(40), er.Welford(40)
    for x in s[:4]:
        wa.add(x)
    for x in s[4:]:
        wb.add(x)
    a.merge(b)
    wa.merge(*wb.export())
    assert a.count == 9 and np.array_equal(a.mean.ravel(), wa.mean) and np.array_equal(a.m2.ravel(), wa.m2)
    assert RunningBins().merge(a).count == 9 and a.merge(RunningBins()).count == 9
    with pytest.raises(ValueError):
        RunningBins().add(s[0]).variance
    with pytest.raises(ValueError):
        a.add(np.zeros(3))


# ---- known answers of the cross-spectrum, shared with tests/test_gpu_cross_spectrum.py ---------------------------------
KNOWN_N, KNOWN_NBIN, KNOWN_M = 16, 16, (2, 1, 3)


def plane_waves(n, m):
    """cos(k.x) and sin(k.x) of the mode m = (mx, my, mz) on the grid [i, j, k]."""
    i = np.arange(n)
    phase = 2 * np.pi * (m[0] * i[:, None, None] + m[1] * i[None, :, None] + m[2] * i[None, None, :]) / n
    return np.cos(phase).ravel(), np.sin(phase).ravel()


def wave_bin(n, L, n_bin, m):
    kv = er.sr.kvals(n, L)
    ktot = np.sqrt((kv[m[0]] * kv[m[0]] + kv[m[1]] * kv[m[1]]) + kv[m[2]] * kv[m[2]])
    return int(ktot / er.spectrum_dk(n, L, n_bin))


def check_known_answers(measure, field, n, L, n_bin, m, tol=TOL_FIELD):
    """`measure(a, b)` -> (kmode, nmode, power_a, power_b, cross, coeff) of n_bin each.  The field is lifted off zero
    mean, so that the bin of the k = 0 mode carries power like every other populated bin."""
    field = np.asarray(field) + 0.25
    res = measure(field, field)
    pop = np.asarray(res[1]) > 0
    assert pop.any() and np.max(np.abs(res[5][pop] - 1.)) <= tol and np.all(res[5][~pop] == 0)
    assert rel_max(res[2], res[3]) <= tol and rel_max(res[4], res[2]) <= tol
    res = measure(field, -field)
    assert np.max(np.abs(res[5][pop] + 1.)) <= tol and np.all(res[5][~pop] == 0)
    cos, sin = plane_waves(n, m)
    res = measure(cos, sin)
    b = wave_bin(n, L, n_bin, m)
    assert 0 < b < n_bin and res[1][b] > 0 and res[2][b] > 0 and res[3][b] > 0
    assert abs(res[5][b]) <= tol, res[5][b]
    assert abs(res[2][b] - res[3][b]) <= tol * res[2][b]  # both waves carry the same power


def test_known_answers_of_the_restatement():
    n, L = KNOWN_N, box_of(KNOWN_N)
    c = Case(Nx=n)
    check_known_answers(lambda a, b: er.cross_spectrum(a, b, n, L, KNOWN_NBIN), c.truth, n, L, KNOWN_NBIN, KNOWN_M)


@pytest.mark.parametrize("n", (8, 9, 16))
def test_power_a_is_measure_spectrum(n):
    """power_a and kmode of the cross-spectrum restatement are measure_spectrum's: against the oracle's C restatement
    of field_statistics.cpp:20-90 and against the literal full-grid sum, nmode against the latter's counts."""
    c = Case(Nx=n)
    L = c.p.L
    for n_bin in (1, 2, n, 20, 200):
        km, nm, pa, pb, cross, coeff = er.cross_spectrum(c.q0, c.truth, n, L, n_bin)
        km0, pw0 = c.oracle.measure_spectrum(c.q0, n_bin)
        km1, pw1, cnt1 = er.spectrum_full_grid(c.q0, n, L, n_bin)
        assert nm.dtype == np.uint64 and np.array_equal(nm, cnt1) and int(nm.sum()) <= n ** 3
        assert rel_max(pa, pw0) <= 1e-13 and rel_max(pa, pw1) <= 1e-13
        assert rel_max(km, km0) <= 1e-14 and rel_max(km, km1) <= 1e-14
        assert rel_max(pb, c.oracle.measure_spectrum(c.truth, n_bin)[1]) <= 1e-13
        pop = nm > 0
        assert np.all(np.abs(coeff[pop]) <= 1. + 1e-12) and np.all(coeff[~pop] == 0) and np.all(cross[~pop] == 0)
        assert np.array_equal(coeff, er.coeff_of(pa, pb, cross))


# ---- declarations ---------------------------------------------------------------------------------------------------
def test_header_declares_and_documents_the_entry_points():
    text = open(os.path.join(ROOT, "include", "bchmc.h")).read()
    assert header_args("bchmc_ensemble_add") == ["bchmc_handle *", "int32_t", "bchmc_corr_source", "const double *"]
    assert header_args("bchmc_ensemble_fetch") == ["bchmc_handle *", "int32_t", "bchmc_ens_what", "double *"]
    assert header_args("bchmc_ensemble_merge") == ["bchmc_handle *", "int32_t", "uint64_t", "const double *", "const double *"]
    assert header_args("bchmc_measure_cross_spectrum") == [
        "bchmc_handle *", "bchmc_corr_source", "const double *", "bchmc_corr_source", "const double *", "uint64_t",
        "double *", "uint64_t *", "double *", "double *", "double *", "double *"]
    assert re.search(r"^#define BCHMC_ABI_VERSION 4\s*$", text, flags=re.M)
    assert re.search(r"BCHMC_ENS_SLOTS\s*=\s*4\b", text)
    assert re.search(r"BCHMC_ENS_MEAN = 0, BCHMC_ENS_VARIANCE = 1, BCHMC_ENS_STD = 2, BCHMC_ENS_M2 = 3", text)
    def flat(s):  # one line, single blanks: a comment may wrap anywhere
        return " ".join(s.replace("\n *", " ").split())

    doc = flat(text[:text.index("int bchmc_ensemble_add(")].rsplit("/* ----", 1)[1])
    for tag in ("E1", "E8", "d = x - mean; mean = mean + d / c; m2 = m2 + d * (x - mean);",
                "d = mean_b - mean; mean = mean + d * w; m2 = (m2 + m2_b) + (d * d) * c", "Chan, Golub & LeVeque",
                "a pending proposal", "bchmc_live_resources"):
        assert tag in doc, tag
    doc = flat(text[:text.index("int bchmc_measure_cross_spectrum(")].rsplit("/* ----", 1)[1])
    for tag in ("NOT bitwise repeatable", "bchmc_measure_spectrum_src", "sqrt(power_a power_b)"):
        assert tag in doc, tag


def test_engine_binds_the_entry_points_like_the_header():
    """Declared, exported, bound with the header's types; the library loads without a GPU and refuses a null handle or
    a null output with BCHMC_ERR_ARG before it touches a device."""
    from barcode_amd import engine
    lib = engine.load()
    for name in NEW_SYMBOLS:
        assert name in engine.EXPORTS and hasattr(C.CDLL(engine.LIB_PATH), name)
        assert list(getattr(lib, name).argtypes) == [CTYPE_NEW[t] for t in header_args(name)], name
    assert engine.ENS_SLOTS == 4 and engine.ENS_WHAT == dict(mean=0, variance=1, std=2, m2=3)
    for method in ("ensemble_add", "ensemble_count", "ensemble_fetch", "ensemble_export", "ensemble_merge",
                   "ensemble_reset", "ensemble_release", "measure_cross_spectrum"):
        assert callable(getattr(engine.Engine, method))
    ARG = 1
    x = np.zeros(1)
    dp = x.ctypes.data_as(C.POINTER(C.c_double))
    n = C.c_uint64()
    assert lib.bchmc_ensemble_add(None, 0, 0, dp) == ARG
    assert lib.bchmc_ensemble_count(None, 0, C.byref(n)) == ARG
    assert lib.bchmc_ensemble_fetch(None, 0, 0, dp) == ARG
    assert lib.bchmc_ensemble_merge(None, 0, 1, dp, dp) == ARG
    assert lib.bchmc_ensemble_reset(None, 0) == ARG and lib.bchmc_ensemble_release(None) == ARG
    assert lib.bchmc_measure_cross_spectrum(None, 0, dp, 0, dp, 1, dp, None, dp, dp, dp, dp) == ARG


def test_hamil_and_io_bind_the_new_names(tmp_path, monkeypatch):
    from barcode_amd import hamil
    monkeypatch.chdir(tmp_path)
    os.mkdir("run")
    for name in ("ensemble_add", "ensemble_fetch", "measure_cross_spectrum"):
        assert callable(getattr(hamil, name))

    class FakeEngine:
        def ensemble_fetch(self, slot, what):
            assert slot == 2
            return np.arange(8.) + dict(mean=0., std=100.)[what]

    d = "run"
    assert io.ensemble_filenames(d, "deltaLAG") == (os.path.join(d, "deltaLAG_mean"), os.path.join(d, "deltaLAG_std"))
    paths = io.dump_ensemble(FakeEngine(), d, 2, "deltaLAG")
    assert paths == (os.path.join(d, "deltaLAG_mean.dat"), os.path.join(d, "deltaLAG_std.dat"))
    assert np.array_equal(io.read_array(os.path.join(d, "deltaLAG_mean"), 8), np.arange(8.))
    assert np.array_equal(io.read_array(os.path.join(d, "deltaLAG_std"), 8), np.arange(8.) + 100.)
