"""Two k-space arrays, not three, between the inverse x pass and the y pass (planes mode with the engine's own y pass).

The Zel'dovich step boundary (k_step_boundary_x<BX_FIRST | BX_INTERIOR>, k_step_boundary_x2) stores Psi^_x and
B = (1/k^2)(Im phi^, -Re phi^) only; k_ypass_pair reads the two, forms ky(j) B and kz B with the multiply the boundary
kernel makes on the three-array path (double, rounded to the storage type: the operands are the same numbers) and writes
the three y-transformed arrays k_zbin_direct reads.  BCHMC_NO_PAIR=1 restores the three arrays.

Only this inverse side is in the engine: the forward side (V^_x and W = ky V^_y + kz V^_z out of a forward y pass) and
the V records of the gather are not, so the Psi-dependent outputs of the two paths are EXACTLY equal in both precisions
and test 1 asserts array_equal on the positions and the state of a 1-step trajectory (first and last step at once: both
BX_FIRST launches, k_ypass_pair twice, k_zbin_direct storing Psi on the way) in the deterministic mode, where one path
repeats itself bit for bit.  Whole trajectories in the default mode are compared at the tolerance of
tests/test_gpu_large.py::test_256_z_pass_inside_the_binning, the scatter's summation noise: the density goes through
floating-point atomics whose order differs from run to run.

Grids: 128^3 (the smallest at which these kernels exist; BCHMC_ZBIN_128=1 as tests/test_gpu_large.py::
test_128_z_pass_inside_the_binning sets it) for everything but one 256^3 case (another NZ / PER instantiation)."""
import ctypes as C
import os

import numpy as np
import pytest

from barcode_amd import inputs
from barcode_amd.params import HamilParams
from tests.fft_bound import worst_ratio
from tests.util import Case, rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "barcode_amd", "libbchmc_fft_probe.so")
SWITCHES = ("BCHMC_NO_PAIR", "BCHMC_NO_PLANES", "BCHMC_NO_ZBIN", "BCHMC_SORT_CAP", "BCHMC_SORT_CAP_FIXED",
            "BCHMC_DETERMINISTIC")
# tests/test_gpu_large.py::test_256_z_pass_inside_the_binning: (q, p) per precision
NOISE = {0: (1e-13, 1e-12), 1: (1e-5, 1e-5)}


class Work:
    """A seeded workload: parameters, fields, mock data, step size."""

    def __init__(self, p, f, window, noise, nobs, eps):
        self.p, self.f, self.eps = p, f, eps
        self.arrays = dict(signal_PS=f["signal_PS"], mass_f=f["mass_f"], window=window, noise=noise, nobs=nobs)
        self.q0, self.p0 = f["q0"], f["p0"]

    def engine(self, precision=0):
        from barcode_amd.engine import Engine
        e = Engine(self.p, precision=precision)
        e.upload(**self.arrays)
        return e


@pytest.fixture(scope="module")
def case128():
    """128^3, Zel'dovich + plane-parallel RSD, Gaussian likelihood (mock data from the oracle's forward model)."""
    c = Case(Nx=128, L=200.0, likelihood=1, rsd_model=1)
    c.oracle.close()
    return c


@pytest.fixture(scope="module")
def work128(case128):
    c = case128
    return Work(c.p, dict(signal_PS=c.signal_PS, mass_f=c.mass_f, q0=c.q0, p0=c.p0), c.window, c.noise, c.nobs, c.eps)


@pytest.fixture(scope="module")
def work256():
    """BASELINE config 3: 256^3, Zel'dovich + plane-parallel RSD, Gaussian likelihood (mock data from the engine's own
    forward model, as the `big` fixture of tests/test_gpu_large.py makes them)."""
    from barcode_amd.engine import Engine
    p = HamilParams(Nx=256, L=200.0, likelihood=1, rsd_model=1, sfmodel=2)
    f = inputs.make_fields(p)
    e = Engine(p)
    e.upload(signal_PS=f["signal_PS"], mass_f=f["mass_f"], nobs=np.zeros(p.N), window=np.ones(p.N), noise=np.ones(p.N))
    e.forward(f["truth"], 1)
    dX = e.fetch("deltaX").reshape((p.Nx,) * 3)
    e.close()
    window, noise, nobs = inputs.mock_observations(p, dX)
    return Work(p, f, window, noise, nobs, 0.5 * p.eps_heuristic())


def set_env(monkeypatch, env, n):
    for k in SWITCHES + ("BCHMC_ZBIN_128",):
        monkeypatch.delenv(k, raising=False)
    if n == 128:
        monkeypatch.setenv("BCHMC_ZBIN_128", "1")  # 128^3 keeps rocFFT's C2R by default
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run(monkeypatch, w, env, precision, neps, q0=None, p0=None, eps=None, fetch=()):
    """A fresh handle under `env`: one trajectory, the state it returns and the fetched arrays."""
    set_env(monkeypatch, env, w.p.Nx)
    e = w.engine(precision)
    q1, p1, done = e.leapfrog(w.q0 if q0 is None else q0, w.p0 if p0 is None else p0, w.eps if eps is None else eps, neps)
    out = dict(q=q1, p=p1, done=done, info=e.tile_info())
    for name in fetch:
        out[name] = e.fetch(name)
    e.close()
    return out


# ---- 1. the new default against the three-array path and against the 3-D plans ------------------------------------------

@pytest.mark.parametrize("precision", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("grid", ["128x3", "256x2"])
def test_two_arrays_against_three_and_against_the_3d_plans(request, monkeypatch, grid, precision):
    n, neps = (int(v) for v in grid.split("x"))
    w = request.getfixturevalue("work%d" % n)
    new = run(monkeypatch, w, {}, precision, neps)
    old = run(monkeypatch, w, dict(BCHMC_NO_PAIR="1"), precision, neps)
    d3 = run(monkeypatch, w, dict(BCHMC_NO_PLANES="1"), precision, neps)
    assert new["done"] == old["done"] == d3["done"] == neps
    tq, tp = NOISE[precision]
    for name, other in (("three arrays", old), ("3-D plans", d3)):
        rq, rp = rel_l2(new["q"], other["q"]), rel_l2(new["p"], other["p"])
        print("\nTWOARRAY %s %s against %s: rel-L2 q %.3e (%.0e) p %.3e (%.0e)" % (grid, "fp32" if precision else "fp64",
                                                                                  name, rq, tq, rp, tp))
        assert rq < tq and rp < tp


@pytest.mark.parametrize("precision", [0, 1], ids=["fp64", "fp32"])
def test_positions_of_a_one_step_trajectory_are_bit_for_bit_the_three_array_ones(monkeypatch, work128, precision):
    """ky B and kz B are the same products of the same operands on either path, so the fetched positions are equal, not
    close.  fp32 too: the product is made in double from the stored fp32 B and rounded once on either path.
    In the deterministic mode (fixed-point mass assignment): the positions of the last step come from q after the drift,
    which holds the gradient of the force evaluation before the first step, and with the default floating-point atomics
    that gradient differs in the last bit from run to run on ONE path (measured here at 128^3 fp64: the same path twice
    differs in 146 / 116 / 65 positions by one ulp, 3610 elements of q, 1.4 million of p).  With the fixed-point scatter
    nothing is left to chance, and the returned state is asserted equal as well."""
    names = ("posx", "posy", "posz")
    det = dict(BCHMC_DETERMINISTIC="1")
    new = run(monkeypatch, work128, det, precision, 1, fetch=names)
    old = run(monkeypatch, work128, dict(det, BCHMC_NO_PAIR="1"), precision, 1, fetch=names)
    assert new["done"] == old["done"] == 1
    for name in names + ("q", "p"):
        assert np.all(np.isfinite(new[name]))
        assert np.array_equal(new[name], old[name]), name
    assert np.ptp(new["posz"]) > 0.5 * work128.p.L  # real positions, not a cleared array


# ---- 2. oracle parity ------------------------------------------------------------------------------------------------------

def test_three_steps_at_128_cubed_against_the_oracle(monkeypatch, case128, work128):
    """BX_FIRST twice, two interior boundaries, BX_LAST twice, all with two arrays, against the OpenMP oracle at the
    project's trajectory tolerance (1e-11 rel-L2, as bench.py's parity_at_size)."""
    from oracle.oracle import Oracle
    c = case128
    o = Oracle(c.p, omp=True)
    o.set(**c.arrays())
    q1o, p1o, done_o = o.Hamiltonian_EoM(c.q0, c.p0, c.eps, 3)
    o.close()
    new = run(monkeypatch, work128, {}, 0, 3)
    assert new["done"] == done_o == 3
    rq, rp = rel_l2(new["q"], q1o), rel_l2(new["p"], p1o)
    print("\nTWOARRAY oracle 128x3: rel-L2 q %.3e p %.3e (1e-11)" % (rq, rp))
    assert rq < 1e-11 and rp < 1e-11


# ---- 3. trajectory lengths and the runaway guard ---------------------------------------------------------------------------

@pytest.mark.parametrize("neps", [1, 2])
def test_first_and_last_boundary_meet(monkeypatch, work128, neps):
    """neps = 1: BX_FIRST opens, BX_LAST closes, no interior boundary; neps = 2: one interior boundary between them."""
    new = run(monkeypatch, work128, {}, 0, neps, fetch=("deltaX",))
    old = run(monkeypatch, work128, dict(BCHMC_NO_PAIR="1"), 0, neps, fetch=("deltaX",))
    assert new["done"] == old["done"] == neps
    tq, tp = NOISE[0]
    assert rel_l2(new["q"], old["q"]) < tq and rel_l2(new["p"], old["p"]) < tp
    assert rel_l2(new["deltaX"], old["deltaX"]) < 1e-11  # the same test's figure for the density contrast


def test_guard_stopped_trajectory_returns_the_three_array_state(monkeypatch, work128):
    """The runaway-guard recipe of tests/test_gpu_large.py::test_256_runaway_guard_with_the_fused_z_pass: a momentum of
    1e60 stops the trajectory after its first step; the boundary kernels already enqueued return at once and k_ypass_pair
    runs on whatever is in Ck.  k_rollback and the state returned must be what the three-array path returns, and a normal
    trajectory on the same handle afterwards is unaffected."""
    w = work128
    p_bad = w.p0.copy().ravel()
    p_bad[0] = 1e60
    outs = []
    for env in (dict(BCHMC_NO_PAIR="1"), {}):
        set_env(monkeypatch, env, 128)
        e = w.engine()
        qb, pb, doneb = e.leapfrog(w.q0, p_bad, 1e-6, 6)
        q1, p1, done = e.leapfrog(w.q0, w.p0, w.eps, 3)
        e.close()
        assert doneb == 1 and done == 3
        assert np.all(np.isfinite(qb)) and np.all(np.isfinite(q1))
        outs.append((qb, pb, q1, p1))
    for a, b in zip(outs[0], outs[1]):
        assert rel_l2(b, a) < 1e-12


# ---- 4. a forced overflow of the record segments ----------------------------------------------------------------------------

def test_forced_overflow_finds_the_three_y_transformed_arrays(monkeypatch, work128):
    """BCHMC_SORT_CAP=2048 pinned (test_128_z_pass_inside_the_binning's recipe): segments overflow inside interior steps
    and k_zbin_direct<PSI_ONLY> transforms Ck again for the fallback sort -- all three components, the two that
    k_ypass_pair made from B included."""
    cap = dict(BCHMC_SORT_CAP="2048", BCHMC_SORT_CAP_FIXED="1")
    ref = run(monkeypatch, work128, dict(BCHMC_NO_PAIR="1"), 0, 4)
    new = run(monkeypatch, work128, cap, 0, 4)
    old = run(monkeypatch, work128, dict(cap, BCHMC_NO_PAIR="1"), 0, 4)
    assert new["info"]["cap"] == old["info"]["cap"] == 2048 and new["info"]["one_pass"] == 1
    assert new["done"] == old["done"] == ref["done"] == 4
    tq, tp = NOISE[0]
    for other in (old, ref):
        assert rel_l2(new["q"], other["q"]) < tq and rel_l2(new["p"], other["p"]) < tp


# ---- 5. a chosen spectrum through k_ypass_pair -------------------------------------------------------------------------------

PREC = {"fp64": (0, np.float64, np.complex128), "fp32": (1, np.float32, np.complex64)}


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the process-wide HIP runtime first, as barcode_amd.engine does)
    assert os.path.exists(PROBE), "%s not built (make -C barcode_amd/csrc)" % PROBE
    L = C.CDLL(PROBE)
    vp, i = C.c_void_p, C.c_int
    L.fftp_row_stride.argtypes = [i, i]
    L.fftp_ypass.argtypes = [i, i, i, vp]
    L.fftp_ypass_pair.argtypes = [i, i, C.c_double, vp]
    return L


def kvals(n, m, box):
    """kval of common.hpp for indices 0 .. m - 1, in double like the kernels."""
    kfac = 2.0 * np.pi / box
    i = np.arange(m)
    return np.where(i <= n // 2, kfac * i.astype(np.float64), -kfac * (n - i).astype(np.float64))


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_k_ypass_pair_on_a_chosen_spectrum(lib, prec, n):
    """B with a single non-zero mode per plane at j in {0, 1, n/2, n-1} x k in {0, n/2} (planes 0 .. 7 and, mirrored,
    n-1 .. n-8), white data in the other planes and in Psi^_x, NaN in the row padding, a sentinel in component 2 (dead on
    this path: every element of it must be overwritten).  Components 1 and 2 must come out as the inverse y transforms of
    ky(j) B and kz B: (a) equal to what k_ypass makes of the three arrays multiplied out on the host in double and
    rounded to the storage type, bit for bit -- the three-array path; (b) on the chosen planes, the analytic transform
    of the single mode within the bound of tests/fft_bound.py.  A wrong kval index, a Nyquist row taken with the wrong
    sign, or the row padding read as data fails (a) and (b)."""
    p, rdt, cdt = PREC[prec]
    box = 200.0
    nhp, nh = lib.fftp_row_stride(n, p), n // 2 + 1
    rng = np.random.default_rng(900 + n + p)
    x = np.empty((3, n, n, nhp), cdt)
    for c in range(2):
        x[c, :, :, :nh] = (rng.standard_normal((n, n, nh)) + 1j * rng.standard_normal((n, n, nh))).astype(cdt)
    x[2] = 7.0 - 3.0j
    x[:2, :, :, nh:] = np.nan + 1j * np.nan
    modes = [(j, k) for j in (0, 1, n // 2, n - 1) for k in (0, n // 2)]
    amp = 1.25 - 0.5j
    chosen = []
    for m, (j, k) in enumerate(modes):
        for i in (m, n - 1 - m):
            x[1, i, :, :nh] = 0
            x[1, i, j, k] = amp
            chosen.append((i, j, k))
    ky, kz = kvals(n, n, box), kvals(n, nhp, box)

    def scaled(b, f):  # the boundary kernel's product: double, rounded to the storage type
        return ((f * b.real.astype(np.float64)).astype(rdt) + 1j * (f * b.imag.astype(np.float64)).astype(rdt)).astype(cdt)

    three = np.empty_like(x)
    three[0] = x[0]
    three[1] = scaled(x[1], ky[None, :, None])
    three[2] = scaled(x[1], kz[None, None, :])
    y = x.copy()
    st = lib.fftp_ypass_pair(p, n, box, y.ctypes.data_as(C.c_void_p))
    assert st == 0, st
    st = lib.fftp_ypass(p, n, 1, three.ctypes.data_as(C.c_void_p))
    assert st == 0, st
    assert not np.isnan(y[..., :nh]).any()
    assert np.isnan(y[..., nh:]).all()  # padding columns are transformed like data: NaN stays in them, the sentinel is gone
    for c in range(3):
        assert np.array_equal(y[c, :, :, :nh], three[c, :, :, :nh]), "component %d" % c
    # (b) the single modes: out[j'] = f amp exp(+2 pi i j j' / n) in column k, zero elsewhere
    jj = np.arange(n, dtype=np.longdouble)
    worst = 0.0
    for i, j, k in chosen:
        for c, f in ((1, ky[j]), (2, kz[k])):
            a = complex(rdt(f * amp.real), rdt(f * amp.imag))
            ref = np.zeros((n, nh), np.clongdouble)
            ref[:, k] = a * np.exp(2j * np.pi * ((j * jj) % n) / n)
            worst = max(worst, worst_ratio(y[c, i, :, :nh], ref, n, rdt, axis=0))
            if f == 0.0:
                assert not y[c, i, :, :nh].any()  # ky(0) = kz(0) = 0: exactly zero
    print("\nTWOARRAY k_ypass_pair<%s> n=%d single modes: worst fraction of the bound %.3f" % (prec, n, worst))
    assert worst <= 1.0
