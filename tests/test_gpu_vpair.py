"""V as records and two k-space arrays, not three, into the forward x pass (planes mode, the engine's own forward passes).

The forward side of a planes-space evaluation: k_gather_tile81<.., REC> stores V as one record {vx, vy, vz, 0} per
particle, k_zr2c<.., REC> makes the row pass from the records, k_ypass_fwd_pair the column pass, storing V^_x and
W = ky V^_y + kz V^_z only (bx_w_of, the function the boundary kernels form W with on the three-array path), and the
Zel'dovich k_step_boundary_x (interior, BX_LAST) / k_step_boundary_x2 read the two with `vpair`.  BCHMC_NO_VPAIR=1 restores
the three arrays of V, rocFFT's 2-D R2C and three arrays into the boundary; BCHMC_NO_VREC=1 keeps the new transforms and
feeds k_zr2c the three arrays of V.

Probe tests run the kernels alone through libbchmc_fft_probe.so, on the engine's launch code.  Engine tests compare
trajectories between the paths: in the deterministic mode records against arrays are EXACTLY equal (the same V, the same
transforms); the default against BCHMC_NO_VPAIR differs by another transform's round-off on top of the scatter's
summation noise, the figures tests/test_gpu_two_array_passes.py holds planes mode against the 3-D plans to.

Grids: 128^3 (the smallest at which these kernels exist; BCHMC_ZBIN_128=1) for everything but one 256^3 case per test
family (another NZ / PER instantiation)."""
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
SWITCHES = ("BCHMC_NO_VPAIR", "BCHMC_NO_VREC", "BCHMC_NO_PAIR", "BCHMC_NO_PLANES", "BCHMC_NO_ZBIN", "BCHMC_SORT_CAP",
            "BCHMC_SORT_CAP_FIXED", "BCHMC_DETERMINISTIC")
# tests/test_gpu_two_array_passes.py (from tests/test_gpu_large.py::test_256_z_pass_inside_the_binning): (q, p) per precision
NOISE = {0: (1e-13, 1e-12), 1: (1e-5, 1e-5)}
PREC = {"fp64": (0, np.float64, np.complex128), "fp32": (1, np.float32, np.complex64)}
BX_INTERIOR, BX_FIRST, BX_LAST = 0, 1, 2


# ---- the kernels alone ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the process-wide HIP runtime first, as barcode_amd.engine does)
    assert os.path.exists(PROBE), "%s not built (make -C barcode_amd/csrc)" % PROBE
    L = C.CDLL(PROBE)
    vp, i, d, ull = C.c_void_p, C.c_int, C.c_double, C.c_ulonglong
    L.fftp_row_stride.argtypes = [i, i]
    L.fftp_ypass.argtypes = [i, i, i, vp]
    L.fftp_ypass_fwd_pair.argtypes = [i, i, d, vp]
    L.fftp_zr2c.argtypes = [i, i, vp, vp]
    L.fftp_zr2c_rec.argtypes = [i, i, vp, vp]
    L.fftp_step_boundary_x.argtypes = [i, i, d, i, i, i] + [vp] * 7 + [vp, vp, vp, vp, vp, vp, vp, d, ull]
    L.fftp_step_boundary_x_vpair.argtypes = L.fftp_step_boundary_x.argtypes + [i]
    return L


def ptr(a):
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def kvals(n, m, box):
    """kval of common.hpp for indices 0 .. m - 1, in double like the kernels."""
    kfac = 2.0 * np.pi / box
    i = np.arange(m)
    return np.where(i <= n // 2, kfac * i.astype(np.float64), -kfac * (n - i).astype(np.float64))


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_k_zr2c_from_records_is_k_zr2c_from_arrays(lib, prec, n):
    """The same V as three arrays and as records with NaN in every record's fourth word, NaN in the row padding of ck:
    equal bit for bit on k <= n / 2, the padding back as it went in, no NaN anywhere else."""
    p, rdt, cdt = PREC[prec]
    nhp, nh = lib.fftp_row_stride(n, p), n // 2 + 1
    rng = np.random.default_rng(700 + n + p)
    V = rng.standard_normal((3, n, n, n)).astype(rdt)
    rec = np.empty((n, n, n, 4), rdt)
    rec[..., :3] = np.moveaxis(V, 0, -1)
    rec[..., 3] = np.nan
    ck0 = np.empty((3, n, n, nhp), cdt)
    ck0[..., :nh] = 5.0 - 2.0j
    ck0[..., nh:] = np.nan + 1j * np.nan
    a, b = ck0.copy(), ck0.copy()
    assert lib.fftp_zr2c(p, n, ptr(V), ptr(a)) == 0
    assert lib.fftp_zr2c_rec(p, n, ptr(rec), ptr(b)) == 0
    assert not np.isnan(b[..., :nh]).any()
    assert same_bits(a[..., :nh], b[..., :nh])
    assert same_bits(b[..., nh:], ck0[..., nh:]) and same_bits(a[..., nh:], ck0[..., nh:])
    assert np.ptp(b[..., :nh].real) > 1.0  # a transform, not the sentinel


def boundary(lib, p, n, box, mode, two_tile, ck, q, pin, wS, wM, scal, vpair):
    """One boundary launch on a copy of ck; returns every array it writes, by name."""
    ck = ck.copy()
    stop, done, guard = np.zeros(1, np.int32), np.zeros(1, np.uint64), np.zeros(1)
    qo = po = go = None
    if mode == BX_INTERIOR:
        qo, po = np.zeros_like(q), np.zeros_like(q)
    else:
        go = np.zeros_like(q)
    args = (p, n, box, mode, 0, int(two_tile), ptr(ck), ptr(q), ptr(pin) if mode == BX_INTERIOR else None, None, ptr(qo),
            ptr(po), ptr(go), ptr(wS), ptr(wM) if mode == BX_INTERIOR else None, ptr(scal),
            ptr(guard) if mode == BX_INTERIOR else None, ptr(stop), ptr(done), None, 0.0, 0)
    st = lib.fftp_step_boundary_x_vpair(*args, 1) if vpair else lib.fftp_step_boundary_x(*args)
    assert st == 0, st
    assert stop[0] == 0
    out = dict(guard=guard)
    if mode == BX_INTERIOR:
        out.update(q_out=qo, p_out=po, Ck0=ck[0], Ck1=ck[1], Ck2=ck[2])
    else:
        out.update(g_out=go)
    return out


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_k_ypass_fwd_pair_on_a_chosen_field(lib, prec, n):
    """Components 1 and 2 (z-transformed V_y, V_z) hold a single non-zero y row j0 in {0, 1, n/2, n-1} at k in {0, n/2} on
    the chosen planes (planes 0 .. 7 and, mirrored, n-1 .. n-8), white data elsewhere and in component 0, NaN in the row
    padding.  (a) Component 0 comes out as k_ypass<forward> makes it, bit for bit.  (b) On the chosen planes W is the
    analytic transform of the two impulses, (ky(j') a_y + kz(k) a_z) exp(-2 pi i j0 j' / n), within the bound of
    tests/fft_bound.py, and exactly zero where ky and kz are both zero and in every other column.  (c) With component 2
    overwritten by NaN, the boundary kernels with `vpair` on the two arrays return, bit for bit, what they return without
    it on the three arrays k_ypass<forward> makes of the same input -- BX_LAST (g only), interior one tile and two.  A
    wrong kval index, a Nyquist row with the wrong sign, another rounding of W or a read of component 2 fails (b) or (c)."""
    p, rdt, cdt = PREC[prec]
    box = 200.0
    nhp, nh = lib.fftp_row_stride(n, p), n // 2 + 1
    rng = np.random.default_rng(1300 + n + p)

    def white(shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdt)

    x = np.empty((3, n, n, nhp), cdt)
    x[..., :nh] = white((3, n, n, nh))
    x[..., nh:] = np.nan + 1j * np.nan
    modes = [(j, k) for j in (0, 1, n // 2, n - 1) for k in (0, n // 2)]
    ay, az = 1.25 - 0.5j, -0.75 + 2.0j
    chosen = []
    for m, (j, k) in enumerate(modes):
        for i in (m, n - 1 - m):
            x[1:, i, :, :nh] = 0
            x[1, i, j, k] = ay
            x[2, i, j, k] = az
            chosen.append((i, j, k))
    three = x.copy()
    assert lib.fftp_ypass(p, n, 0, ptr(three)) == 0
    y = x.copy()
    assert lib.fftp_ypass_fwd_pair(p, n, box, ptr(y)) == 0
    assert not np.isnan(y[:2, :, :, :nh]).any()
    assert same_bits(y[2], x[2])  # component 2 is read only
    # (a)
    assert same_bits(y[0, :, :, :nh], three[0, :, :, :nh])
    # the whole of W against the host's statement of bx_w_of on the three arrays: at most the last bit (the device may
    # contract ky vy + kz vz into a fused multiply-add); (c) below decides bit for bit against the device's own
    ky, kz = kvals(n, n, box), kvals(n, nhp, box)
    t1, t2 = three[1, :, :, :nh], three[2, :, :, :nh]
    w_host = (ky[None, :, None] * t1.real.astype(np.float64) + kz[None, None, :nh] * t2.real.astype(np.float64)) + 1j * (
        ky[None, :, None] * t1.imag.astype(np.float64) + kz[None, None, :nh] * t2.imag.astype(np.float64))
    err = np.abs(y[1, :, :, :nh] - w_host)
    mag = np.abs(ky)[None, :, None] * np.abs(t1) + np.abs(kz)[None, None, :nh] * np.abs(t2)
    assert np.all(err <= 4 * np.finfo(rdt).eps * mag)
    # (b)
    jj = np.arange(n, dtype=np.longdouble)
    worst = 0.0
    for i, j, k in chosen:
        ref = np.zeros((n, nh), np.clongdouble)
        ref[:, k] = (ky * ay + kz[k] * az) * np.exp(-2j * np.pi * ((j * jj) % n) / n)
        worst = max(worst, worst_ratio(y[1, i, :, :nh], ref, n, rdt, axis=0))
        if k == 0:
            assert y[1, i, 0, 0] == 0  # ky(0) = kz(0) = 0: exactly zero
    print("\nVPAIR k_ypass_fwd_pair<%s> n=%d impulses: worst fraction of the bound %.3f" % (prec, n, worst))
    assert worst <= 1.0
    # (c)
    two = y.copy()
    two[2] = np.nan + 1j * np.nan
    q, pin = np.zeros((n, n, nhp), cdt), np.zeros((n, n, nhp), cdt)
    q[..., :nh], pin[..., :nh] = white((n, n, nh)), white((n, n, nh))
    wS = np.zeros((n, n, nhp))
    wM = np.zeros((n, n, nhp))
    wS[..., :nh] = rng.uniform(0.5, 2.0, (n, n, nh))
    wM[..., :nh] = rng.uniform(0.5, 2.0, (n, n, nh))
    scal = np.array([0.7, -1.3, 0.05, 0.1, -0.4 / n ** 3])
    for mode, two_tile in ((BX_LAST, False), (BX_INTERIOR, False), (BX_INTERIOR, True)):
        new = boundary(lib, p, n, box, mode, two_tile, two, q, pin, wS, wM, scal, True)
        old = boundary(lib, p, n, box, mode, two_tile, three, q, pin, wS, wM, scal, False)
        # The guard slot is a sum over the workgroups by floating-point atomics in double, whose order differs from launch
        # to launch on ONE path: G workgroup partials, so two orders differ by at most (G - 1) 2^-53 sum |partial|, and
        # sum |partial| <= 2 sum |Re p| over the elements (weights 1 or 2) of the half-kicked momentum, which the stored
        # p_out bounds to a factor of two here (half_eps g is small against p).
        if mode == BX_INTERIOR:
            groups = n * nhp // (128 // np.dtype(cdt).itemsize)
            tol = groups * 2.0 ** -53 * 4.0 * np.abs(new["p_out"][..., :nh].real).sum()
            assert abs(new["guard"][0] - old["guard"][0]) <= tol and new["guard"][0] != 0
        for name in new:
            if name == "guard":
                continue
            a, b = new[name], old[name]
            if a.ndim == 3:
                a, b = a[..., :nh], b[..., :nh]
            assert np.all(np.isfinite(a)), (mode, two_tile, name)
            assert same_bits(a, b), (mode, two_tile, name)
        key = "g_out" if mode == BX_LAST else "p_out"
        assert np.ptp(new[key][..., :nh].real) > 0  # something was computed


# ---- the engine -------------------------------------------------------------------------------------------------------------

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
        monkeypatch.setenv("BCHMC_ZBIN_128", "1")  # 128^3 keeps rocFFT's transforms by default
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run(monkeypatch, w, env, precision, neps, fetch=()):
    """A fresh handle under `env`: one trajectory, the state it returns and the fetched arrays."""
    set_env(monkeypatch, env, w.p.Nx)
    e = w.engine(precision)
    q1, p1, done = e.leapfrog(w.q0, w.p0, w.eps, neps)
    out = dict(q=q1, p=p1, done=done, info=e.tile_info())
    for name in fetch:
        out[name] = e.fetch(name)
    e.close()
    return out


V3 = ("Vx", "Vy", "Vz")


@pytest.mark.parametrize("precision", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("grid", ["128x3", "256x2"])
def test_default_against_three_arrays_and_against_the_3d_plans(request, monkeypatch, grid, precision):
    n, neps = (int(v) for v in grid.split("x"))
    w = request.getfixturevalue("work%d" % n)
    new = run(monkeypatch, w, {}, precision, neps)
    old = run(monkeypatch, w, dict(BCHMC_NO_VPAIR="1"), precision, neps)
    d3 = run(monkeypatch, w, dict(BCHMC_NO_PLANES="1"), precision, neps)
    assert new["done"] == old["done"] == d3["done"] == neps
    tq, tp = NOISE[precision]
    for name, other in (("three arrays", old), ("3-D plans", d3)):
        rq, rp = rel_l2(new["q"], other["q"]), rel_l2(new["p"], other["p"])
        print("\nVPAIR %s %s against %s: rel-L2 q %.3e (%.0e) p %.3e (%.0e)" % (grid, "fp32" if precision else "fp64",
                                                                               name, rq, tq, rp, tp))
        assert rq < tq and rp < tp


@pytest.mark.parametrize("precision", [0, 1], ids=["fp64", "fp32"])
def test_records_against_arrays_bit_for_bit(monkeypatch, work128, precision):
    """Deterministic mode (fixed-point mass assignment: one path repeats itself bit for bit): V as records and V as three
    arrays are the same numbers through the same transforms, so q, p and the fetched V are equal after 1 and 2 steps; and
    after the gradient at q0 alone V is also what BCHMC_NO_VPAIR=1 gathers -- V is made before any transform."""
    det = dict(BCHMC_DETERMINISTIC="1")
    got = []
    for env in (det, dict(det, BCHMC_NO_VREC="1"), dict(det, BCHMC_NO_VPAIR="1")):
        set_env(monkeypatch, env, 128)
        w, out = work128, {}
        e = w.engine(precision)
        e.gradient(w.q0)
        out["gradient"] = [e.fetch(name) for name in V3]
        if "BCHMC_NO_VPAIR" not in env:
            for neps in (1, 2):
                q1, p1, done = e.leapfrog(w.q0, w.p0, w.eps, neps)
                assert done == neps
                out[neps] = [q1, p1] + [e.fetch(name) for name in V3]
        e.close()
        got.append(out)
    new, old, three = got
    for neps in (1, 2):
        for a, b, name in zip(new[neps], old[neps], ("q", "p") + V3):
            assert np.all(np.isfinite(a))
            assert np.array_equal(a, b), (neps, name)
        assert np.ptp(new[neps][4]) > 0  # a gathered V, not a cleared array
    for other in (old, three):
        for a, b, name in zip(new["gradient"], other["gradient"], V3):
            assert np.ptp(a) > 0
            assert np.array_equal(a, b), name


def test_three_steps_at_128_cubed_against_the_oracle(monkeypatch, case128, work128):
    """BX_FIRST twice, two interior boundaries, BX_LAST twice, every forward side from records through two arrays, against
    the OpenMP oracle at the project's trajectory tolerance (1e-11 rel-L2, as bench.py's parity_at_size)."""
    from oracle.oracle import Oracle
    c = case128
    o = Oracle(c.p, omp=True)
    o.set(**c.arrays())
    q1o, p1o, done_o = o.Hamiltonian_EoM(c.q0, c.p0, c.eps, 3)
    o.close()
    new = run(monkeypatch, work128, {}, 0, 3)
    assert new["done"] == done_o == 3
    rq, rp = rel_l2(new["q"], q1o), rel_l2(new["p"], p1o)
    print("\nVPAIR oracle 128x3: rel-L2 q %.3e p %.3e (1e-11)" % (rq, rp))
    assert rq < 1e-11 and rp < 1e-11


def test_guard_stopped_trajectory_returns_the_three_array_state(monkeypatch, work128):
    """The runaway-guard recipe of tests/test_gpu_two_array_passes.py: a momentum of 1e60 stops the trajectory after its
    first step; the boundary kernels already enqueued return at once and the gather, k_zr2c and k_ypass_fwd_pair run on
    whatever the stale Ck gives them.  The state returned must be what the three-array path returns, and a normal
    trajectory on the same handle afterwards is unaffected."""
    w = work128
    p_bad = w.p0.copy().ravel()
    p_bad[0] = 1e60
    outs = []
    for env in (dict(BCHMC_NO_VPAIR="1"), {}):
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


def test_forced_overflow_ends_in_the_record_gather(monkeypatch, work128):
    """BCHMC_SORT_CAP=2048 pinned: segments overflow inside interior steps and the two-pass fallback sort orders the
    records; it still ends in k_gather_tile81, so V goes out as records there too."""
    cap = dict(BCHMC_SORT_CAP="2048", BCHMC_SORT_CAP_FIXED="1")
    ref = run(monkeypatch, work128, dict(BCHMC_NO_VPAIR="1"), 0, 4)
    new = run(monkeypatch, work128, cap, 0, 4)
    plain = run(monkeypatch, work128, {}, 0, 4)
    old = run(monkeypatch, work128, dict(cap, BCHMC_NO_VPAIR="1"), 0, 4)
    assert new["info"]["cap"] == old["info"]["cap"] == 2048 and new["info"]["one_pass"] == 1
    assert new["done"] == old["done"] == ref["done"] == plain["done"] == 4
    tq, tp = NOISE[0]
    for got in (new, plain):
        for other in (old, ref):
            assert rel_l2(got["q"], other["q"]) < tq and rel_l2(got["p"], other["p"]) < tp


@pytest.mark.parametrize("neps", [1, 2])
def test_first_and_last_boundary_meet(monkeypatch, work128, neps):
    """neps = 1: BX_FIRST opens, BX_LAST closes (with `vpair`), no interior boundary; neps = 2: one interior boundary."""
    new = run(monkeypatch, work128, {}, 0, neps, fetch=("deltaX",))
    old = run(monkeypatch, work128, dict(BCHMC_NO_VPAIR="1"), 0, neps, fetch=("deltaX",))
    assert new["done"] == old["done"] == neps
    tq, tp = NOISE[0]
    assert rel_l2(new["q"], old["q"]) < tq and rel_l2(new["p"], old["p"]) < tp
    assert rel_l2(new["deltaX"], old["deltaX"]) < 1e-11  # tests/test_gpu_two_array_passes.py's figure for the density contrast
