"""CPU checks around the correlation-function measurement: the numpy restatement of the reference's tools
(tests/corr_restatement.py) against itself and against closed forms, the two findings about the tools (C1, C2), the
bin-count helper, the ctypes bindings of the new entry points against the header, and the file writers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from barcode_amd import inputs, io
from barcode_amd.params import HamilParams
from tests import corr_restatement as cr
from tests.util import TOL_FIELD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, L, n_bin) of the C1 / C2 checks
SIX = ((16, 200., 16), (16, 200., 200), (32, 1000., 32), (32, 200., 28), (64, 1250., 64), (64, 200., 200))


def field(n, L, which="truth"):
    return inputs.make_fields(HamilParams(Nx=n, L=L))[which]


def rel_bins(a, b, nmode):
    """Largest relative difference over the populated bins (a bin whose reference value is 0 counts absolutely)."""
    pop = np.asarray(nmode).ravel() > 0
    a, b = np.asarray(a).ravel()[pop], np.asarray(b).ravel()[pop]
    return float(np.max(np.abs(a - b) / np.where(b != 0, np.abs(b), 1.)))


def rel_max(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.mark.parametrize("n", (8, 16))
@pytest.mark.parametrize("nb", ("n", "auto", 200))
def test_vectorised_equals_literal_loops(n, nb):
    """nmode equal, rmode relative per populated bin (a bin that holds r = 0 alone absolutely) and corr relative to
    max |corr| to 1e-14."""
    L = 200. * n / 64.
    n_bin = n if nb == "n" else cr.auto_nbin(n, L) if nb == "auto" else nb
    sig = field(n, L)
    r1, n1, c1, o1 = cr.corr_grid_loops(sig, n, L, n_bin)
    r2, n2, c2, o2 = cr.corr_grid(sig, n, L, n_bin)
    assert np.array_equal(n1, n2) and o1 == o2
    assert rel_bins(r1, r2, n2) <= 1e-14 and rel_max(c1, c2) <= 1e-14
    r1, n1, c1 = cr.corr2d_loops(sig, n, L, n_bin)
    r2, n2, c2 = cr.corr2d(sig, n, L, n_bin)
    assert np.array_equal(n1, n2)
    assert rel_bins(r1, r2, n2) <= 1e-14 and rel_max(c1, c2) <= 1e-14
    assert int(n1.sum()) <= n ** 3 and int(n2.sum()) > 0


@pytest.mark.parametrize("n,L,n_bin", SIX)
def test_c1_only_the_corner_cell_leaves_the_arrays(n, L, n_bin):
    """C1: measure_corr_grid has no bound on its bin index.  With the guard off the restatement shows what upstream
    writes: exactly one cell, (n/2, n/2, n/2), at index n_bin exactly -- one element past rmode, corr and nmode."""
    sig = field(n, L)
    r, nm, c, out = cr.corr_grid(sig, n, L, n_bin, guard=False)
    assert out == [(n // 2, n // 2, n // 2, n_bin)]
    assert nm.size == n_bin + 1 and nm[n_bin] == 1
    rg, nmg, cg, outg = cr.corr_grid(sig, n, L, n_bin, guard=True)
    assert outg == out and np.array_equal(nmg, nm[:n_bin]) and int(nmg.sum()) == n ** 3 - 1
    assert np.array_equal(rg, r[:n_bin]) and np.array_equal(cg, c[:n_bin])
    if n <= 16:
        assert cr.corr_grid_loops(sig, n, L, n_bin, guard=False)[3] == out
    # the 2-D function has the bound and drops the same kind of cell
    assert int(cr.corr2d(sig, n, L, n_bin)[1].sum()) <= n ** 3


@pytest.mark.parametrize("n,L,n_bin", SIX)
def test_c2_the_odd_term_cancels_in_every_bin(n, L, n_bin):
    """C2: upstream's inverse transform sees |S|^2 + i Im S; the extra (delta(r) - delta(-r)) / 2 cancels inside every
    bin because each bin is symmetric under r -> -r.  Both forms to 1e-14 of max |corr|."""
    sig = field(n, L)
    a = cr.corr_grid(sig, n, L, n_bin, odd_term=False)
    b = cr.corr_grid(sig, n, L, n_bin, odd_term=True)
    assert np.array_equal(a[1], b[1]) and rel_max(b[2], a[2]) <= 1e-14
    a2 = cr.corr2d(sig, n, L, n_bin, odd_term=False)
    b2 = cr.corr2d(sig, n, L, n_bin, odd_term=True)
    assert np.array_equal(a2[1], b2[1]) and rel_max(b2[2], a2[2]) <= 1e-14
    # the term itself is not small: the fields differ cell by cell
    assert np.max(np.abs(cr.corr_field(sig, n, True) - cr.corr_field(sig, n, False))) > 1e-3 * np.max(np.abs(sig))


def known_constant(n, c):
    return np.full(n ** 3, c)


def known_spike(n, a):
    s = np.zeros(n ** 3)
    s[(3 * n * n + 5 * n + 7) % n ** 3] = a
    return s


def known_cosine(n, a, m):
    return np.broadcast_to(a * np.cos(2 * np.pi * m * np.arange(n) / n), (n, n, n)).reshape(-1).copy()


def check_constant(res1, res2, c):
    for rm, nm, co in (res1, res2):
        pop = nm.ravel() > 0
        assert np.max(np.abs(co.ravel()[pop] - c * c)) <= TOL_FIELD * c * c
        assert np.all(co.ravel()[~pop] == 0)


def check_spike(res1, res2, a, N):
    for rm, nm, co in (res1, res2):
        nm, co = nm.ravel(), co.ravel()
        c0 = a * a / (float(nm[0]) * N)
        assert abs(co[0] - c0) <= TOL_FIELD * c0
        assert np.max(np.abs(co[1:])) <= TOL_FIELD * c0


def check_cosine(res2, n, L, a, m):
    rm, nm, co = res2
    n_bin = int(round(math.sqrt(nm.size)))
    nm, co = nm.reshape(n_bin, n_bin), co.reshape(n_bin, n_bin)
    _, dr = cr.rmax_dr(L, n_bin)
    seen = 0
    for kk in range(n // 2 + 1):
        z = cr.pacman_center_on_origin(kk, n, L / float(n))
        par = int(math.sqrt(z * z) / dr)
        want = 0.5 * a * a * math.cos(2 * math.pi * m * kk / n)
        pop = nm[:, par] > 0
        assert pop.any()
        assert np.max(np.abs(co[pop, par] - want)) <= TOL_FIELD * 0.5 * a * a
        seen += int(pop.sum())
    assert seen == int((nm > 0).sum())  # every populated bin was one of those: one |z| per par bin


@pytest.mark.parametrize("n", (16, 32, 64))
def test_known_answers_of_the_restatement(n):
    """Closed forms, with A(r) = sum_x delta(x) delta(x + r) and corr = sum_bin A / (nmode N):

    * delta = c: A = c^2 N in every cell, so corr = c^2 in every populated bin of both functions.
    * delta = a at one cell, 0 elsewhere: A(0) = a^2 and A = 0 elsewhere.  Bin 0 holds r = 0, so
      corr[0] = a^2 / (nmode[0] N) and every other bin is 0.
    * delta = a cos(2 pi m k / n) along z: A(r) = a^2 sum_x cos(t_x) cos(t_x + 2 pi m z / n) = (a^2 N / 2)
      cos(2 pi m z / n) (0 < m < n/2), a function of |z| alone.  With the automatic bin count dr < d, so a par bin
      holds one |z| and corr[par + n_bin perp] = (a^2 / 2) cos(2 pi m z / n) whatever perp: this pins the line of sight
      to z and the element order."""
    L = 200. * n / 64.
    nb = cr.auto_nbin(n, L)
    N = float(n ** 3)
    check_constant(cr.corr_grid(known_constant(n, 1.7), n, L, nb)[:3], cr.corr2d(known_constant(n, 1.7), n, L, nb), 1.7)
    check_spike(cr.corr_grid(known_spike(n, 2.5), n, L, nb)[:3], cr.corr2d(known_spike(n, 2.5), n, L, nb), 2.5, N)
    check_cosine(cr.corr2d(known_cosine(n, 1.3, 3), n, L, nb), n, L, 1.3, 3)


def test_corr_auto_nbin():
    from barcode_amd.engine import corr_auto_nbin
    for L in (200., 1000., 1250.):
        for n in range(16, 513):
            want = int(math.ceil(L / 2 * math.sqrt(3) / (L / n)))
            assert corr_auto_nbin(n, L) == want == cr.auto_nbin(n, L)


CTYPE = {"bchmc_handle *": C.c_void_p, "bchmc_corr_source": C.c_int, "const double *": C.POINTER(C.c_double),
         "double *": C.POINTER(C.c_double), "uint64_t": C.c_uint64, "uint64_t *": C.POINTER(C.c_uint64), "int": C.c_int}


def header_args(name):
    text = open(os.path.join(ROOT, "include", "bchmc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/bchmc.h" % name
    # "const double *signal" -> "const double *": everything before the parameter's name
    return [" ".join(re.match(r"^(.*?)\w+$", a.strip(), flags=re.S).group(1).split()) for a in m.group(1).split(",")]


def test_engine_binds_the_new_entry_points_like_the_header():
    from barcode_amd import engine
    lib = engine.load()
    for name in ("bchmc_measure_corr", "bchmc_measure_corr2d", "bchmc_chain_forward"):
        want = [CTYPE[t] for t in header_args(name)]
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want, name
        assert name in engine.EXPORTS + engine.EXPORTS_CORR2D
    assert engine.CORR_SOURCES == dict(host=0, chain=1, deltaX=2)
    for meth in ("measure_corr", "measure_corr2d", "chain_forward"):
        assert callable(getattr(engine.Engine, meth))


def test_shim_and_hamil_bind_the_new_hooks():
    from barcode_amd import hamil, shim
    lib = shim.load()
    for name in ("bchmc_shim_measure_corr_grid", "bchmc_shim_measure_corr2D", "bchmc_shim_chain_forward"):
        assert name in shim.SHIM_EXPORTS and getattr(lib, name).argtypes
    text = open(os.path.join(ROOT, "include", "bchmc_shim.hpp")).read()
    for name in ("measure_corr_grid", "measure_corr2D", "chain_forward"):
        assert re.search(r"\bvoid %s\(HamilView \*hd" % name, text) and "bchmc_shim_" + name in text
    assert callable(hamil.measure_corr_grid) and callable(hamil.measure_corr2D)
    with pytest.raises(RuntimeError, match="non-plane-parallel option not yet implemented"):
        hamil.measure_corr2D(None, planepar=False)


def test_corr_writers(tmp_path, monkeypatch):
    """Names relative to the working directory, as the tools write them; write_array's extension rule
    (IOfunctionsGen.cc:185-191) looks for a '.' anywhere in the name, so a dotted directory keeps the bare name."""
    monkeypatch.chdir(tmp_path)
    os.mkdir("v1.2")
    rng = np.random.default_rng(5)
    for shape, auto in (((28,), True), ((28, 28), True), ((200,), False)):
        r, c = rng.random(shape), rng.standard_normal(shape)
        tail = "_Nbin28" if auto else ""
        for base, ext in (("corr_fct_2D", ".dat"), (os.path.join("v1.2", "corr_fct_2D"), "")):
            paths = io.dump_corr(base, r, c, auto_nbin=auto)
            assert paths == (base + tail + "_r" + ext, base + tail + "_eta" + ext)
            assert os.path.getsize(paths[0]) == 8 * r.size
            assert io.read_array(base + tail + "_r", r.size).tobytes() == r.tobytes()
            assert io.read_array(base + tail + "_eta", c.size).tobytes() == c.tobytes()
    assert io.corr_filenames("x", 28, True) == ("x_Nbin28_r", "x_Nbin28_eta")
    assert io.corr_filenames("x", 28) == ("x_r", "x_eta")


class FakeEngine:
    """What dump_deltas needs of an Engine: the fields are labelled by the forward model that made them."""

    def __init__(self, rsd_model):
        self.params = HamilParams(Nx=4, L=10., rsd_model=rsd_model, likelihood=1)
        self.calls, self.last = [], None

    def chain_get_state(self):
        return np.full(64, 1.0)

    def chain_forward(self, rsd=-1):
        self.calls.append(rsd)
        self.last = rsd

    def fetch(self, name):
        assert name == "deltaX" and self.last is not None
        return np.full(64, 10.0 + self.last)


def test_dump_deltas_names_and_order(tmp_path, monkeypatch):
    """IOfunctionsGen.cc:136-171: deltaLAG, then deltaEUL; with rsd_model deltaLAG, deltaRSS (the configured model),
    deltaEUL (a second Lag2Eul without RSD).  Written into a directory given relative to the working directory, so that
    write_array's extension rule sees no '.' and appends ".dat"."""
    monkeypatch.chdir(tmp_path)
    os.mkdir("out")
    e = FakeEngine(0)
    paths = io.dump_deltas(e, "out", "_7")
    assert paths == [os.path.join("out", x) for x in ("deltaLAG_7.dat", "deltaEUL_7.dat")] and e.calls == [0]
    assert io.read_array(paths[1], 64)[0] == 10.0
    e = FakeEngine(1)
    paths = io.dump_deltas(e, "out", "_8")
    assert paths == [os.path.join("out", x) for x in ("deltaLAG_8.dat", "deltaRSS_8.dat", "deltaEUL_8.dat")]
    assert e.calls == [1, 0]
    assert [io.read_array(p, 64)[0] for p in paths] == [1.0, 11.0, 10.0]
    assert io.dump_deltas(FakeEngine(0), "", "") == ["deltaLAG.dat", "deltaEUL.dat"]
