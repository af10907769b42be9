"""The x-column tile layout of a fused trajectory's k-space state and weights (barcode_amd/csrc/xtile.hpp).

Between the opening and the closing boundary of trajectory_fused the ping-pong pairs (q^, p^) and the weight pair
{wS, wM} live in the layout the x pass owns them in: tile t = j (nhp / KB) + k0 / KB is one contiguous run of n KB
elements, element (i, j, k) at (t n + i) KB + k % KB.  Nothing but addresses changes, so everything here is compared
EXACTLY with the natural layout (BCHMC_NO_XTILE=1, or the natural instantiation of the same kernel):

- kernel level, through fftp_step_boundary_x_xtile of libbchmc_fft_probe.so: k_step_boundary_x<BX_FIRST> with g_in (q_in,
  p_in, g_in natural, q_out, p_out tiled), <BX_INTERIOR> (all four tiled), <BX_LAST> with p_out (q_in, p_in tiled, p_out,
  g_out natural) and k_step_boundary_x2, at n = 32 (padded rows), 64 and 128 in both precisions, on the input sets of
  tests/kstep_inputs.py with the tiled arrays prepared on the host by the permutation: every output array, un-permuted
  on the host, is array_equal to the natural kernel's, padding columns included.  Those sets carry NaN in the padding
  columns of every input, and which of two NaN operands an instruction hands on (sign and payload) is the compiler's
  choice per instantiation, so there the comparison is array_equal(equal_nan=True): NaN where the natural kernel has
  NaN, the same number everywhere else; a further white set with finite random data in the padding columns is compared
  with plain array_equal over the whole arrays.  The guard slot is a sum of per-workgroup
  sums added with floating-point atomics in any order, so it is judged as tests/test_gpu_kstep.py judges it: against the
  longdouble reference within the counted bound of tests/kstep_bound.py (constant 1).  The control path tiled: *stop set
  writes nothing, a tripped guard sets steps_done and stop and writes nothing else.
- k_xtile_weights: the pair is the permuted {wS, wM} bit for bit (NaN padding included), canaries intact.
- trajectories at 128^3 (BCHMC_ZBIN_128=1, as tests/test_gpu_two_array_passes.py sets it), default against
  BCHMC_NO_XTILE=1, in the deterministic mode (fixed-point mass assignment: one path repeats itself bit for bit), both
  precisions, 1, 2 and 3 steps (the opening meets the closing; one interior boundary; both pairs written tiled):
  array_equal on q1 and p1.  One case with the default floating-point atomics at that file's NOISE figures, which are
  tests/test_gpu_large.py::test_256_z_pass_inside_the_binning's: 1e-13 / 1e-12 rel-L2 on q / p at fp64.
- the runaway guard, detected by an odd boundary (the recipe of test_guard_stopped_trajectory_returns_the_three_array_state:
  p0[0] = 1e60 trips in step 0, boundary 1 sees it), by the last boundary (the same with 2 steps) and by an even one (a
  q0[0] whose prior force carries p(x = 0) over the limit in step 1: guard_s = N p_s(0), p_s(0) ~ -(s + 1) eps g(0), and
  eps is chosen so that eps |g(0)| is 0.7 of the limit): state and steps_done equal BCHMC_NO_XTILE=1's, and a normal
  3-step trajectory on the same handle afterwards too.
- stale weights: a trajectory, another mass_f and signal_PS, a trajectory again: equal to a fresh BCHMC_NO_XTILE=1 handle
  given the same uploads.
- the early q: Engine.leapfrog takes q before the last force evaluation (out of the tiles through the scaling pass) and,
  under BCHMC_NO_DOWNLOAD_OVERLAP=1, after the closing pass; both equal BCHMC_NO_XTILE=1's.
"""
import ctypes as C

import numpy as np
import pytest

from barcode_amd import inputs
from barcode_amd.params import HamilParams
from tests import kstep_bound as kb
from tests import kstep_inputs as ki
from tests import kstep_reference as ref
from tests import test_gpu_kstep as tk
from tests.kstep_reference import BX_FIRST, BX_INTERIOR, BX_LAST
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

PRECS = ["fp64", "fp32"]
SWITCHES = ("BCHMC_NO_XTILE", "BCHMC_NO_PAIR", "BCHMC_NO_VPAIR", "BCHMC_NO_VREC", "BCHMC_NO_PLANES", "BCHMC_NO_ZBIN",
            "BCHMC_BX_V1", "BCHMC_BX_V2", "BCHMC_DETERMINISTIC", "BCHMC_NO_DOWNLOAD_OVERLAP", "BCHMC_NO_UPLOAD_OVERLAP",
            "BCHMC_ZBIN_128")
# tests/test_gpu_two_array_passes.py NOISE = tests/test_gpu_large.py::test_256_z_pass_inside_the_binning: (q, p) rel-L2 of
# two paths that differ by the scatter's summation order only
NOISE = {0: (1e-13, 1e-12), 1: (1e-5, 1e-5)}


# ---- the permutation, on the host --------------------------------------------------------------------------------------

def tile(a, kbv):
    """(n, n, nhp[, m]) natural -> flat tiled: [j, k0 / KB, i, k % KB]."""
    n, nhp = a.shape[0], a.shape[2]
    rest = a.shape[3:]
    return np.ascontiguousarray(a.reshape((n, n, nhp // kbv, kbv) + rest).transpose((1, 2, 0, 3) + tuple(range(4, 4 + len(rest)))))


def untile(t, n, nhp, kbv):
    return np.ascontiguousarray(t.reshape(n, nhp // kbv, n, kbv).transpose(2, 0, 1, 3)).reshape(n, n, nhp)


def test_host_permutation_is_the_documented_index():
    """tile() above against (t n + i) KB + k % KB, t = j (nhp / KB) + k / KB, element by element at 32^3."""
    n, nhp, kbv = 32, 24, 8
    a = np.arange(n * n * nhp, dtype=np.int64).reshape(n, n, nhp)
    t = tile(a, kbv).ravel()
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(nhp), indexing="ij")
    e = ((j * (nhp // kbv) + k // kbv) * n + i) * kbv + k % kbv
    assert np.array_equal(t[e.ravel()], a.ravel())
    assert np.array_equal(untile(t, n, nhp, kbv), a)


# ---- kernel level -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the process-wide HIP runtime first, as barcode_amd.engine does)
    import os
    assert os.path.exists(tk.PROBE), "%s not built (make -C barcode_amd/csrc)" % tk.PROBE
    L = C.CDLL(tk.PROBE)
    vp, i, d, ull = C.c_void_p, C.c_int, C.c_double, C.c_ulonglong
    L.fftp_row_stride.argtypes = [i, i]
    L.fftp_step_boundary_x.argtypes = [i, i, d, i, i, i] + [vp] * 7 + [vp, vp, vp, vp, vp, vp, vp, d, ull]
    L.fftp_step_boundary_x_xtile.argtypes = [i, i, d, i, i] + [vp] * 7 + [vp, vp, vp, vp, vp, vp, vp, d, ull, i, vp]
    L.fftp_xtile_weights.argtypes = [i, i, vp, vp, vp]
    return L


@pytest.fixture
def padded(monkeypatch):
    monkeypatch.setenv("BCHMC_FFT_PAD", "1")


def run_tiled(lib, inp, mode, two_tile=False, ctl=None):
    """run_planes of tests/test_gpu_kstep.py through the XT instantiation; outputs come back un-permuted."""
    ctl = ctl or tk.Ctl()
    n, nhp = inp["n"], inp["nhp"]
    kbv = ki.pass_kb(ki.types(inp["prec"])[0])
    assert lib.fftp_row_stride(n, tk.pcode(inp["prec"])) == nhp
    ck = inp["Ck"].copy()
    nat = mode == BX_FIRST  # the opening reads the natural state
    q_in = inp["q"] if nat else tile(inp["q"], kbv)
    p_in = inp["p"] if nat else tile(inp["p"], kbv)
    qo, po, go = tk.filled(inp), tk.filled(inp), tk.filled(inp)  # a constant: the same array in either layout
    wpair = tile(np.stack([inp["wS"], inp["wM"]], axis=-1), kbv)
    guard = tk.dbl(0.0)
    sc = tk.dbl(inp["a"], inp["b"], inp["half_eps"], inp["eps"], inp["c_za"])
    ptr = tk.ptr
    st = lib.fftp_step_boundary_x_xtile(tk.pcode(inp["prec"]), n, inp["L"], mode, int(two_tile), ptr(ck), ptr(q_in), ptr(p_in),
                                        ptr(inp["g_in"]) if mode == BX_FIRST else None,
                                        ptr(qo) if mode != BX_LAST else None, ptr(po), ptr(go) if mode == BX_LAST else None,
                                        ptr(inp["wS"]), ptr(inp["wM"]), ptr(sc), ptr(guard), *ctl.args(), 0, ptr(wpair))
    tk.check_status(st)
    if mode != BX_LAST:
        qo, po = untile(qo, n, nhp, kbv), untile(po, n, nhp, kbv)
    got = {"Ck0": ck[0], "Ck1": ck[1], "Ck2": ck[2], "q_out": qo, "p_out": po, "g_out": go, "guard": float(guard[0])}
    return got, ctl


KERNELS = {"first": (BX_FIRST, False), "interior": (BX_INTERIOR, False), "last": (BX_LAST, False),
           "two_tile": (BX_INTERIOR, True)}


def finite_padding(n, prec):
    """The white set with finite data, not NaN, in the padding columns of every array."""
    d = ki.white(n, prec, seed=3, pad=True)
    rng = np.random.default_rng(77 + n)
    for name in ("Ck", "q", "p", "g_in", "wS", "wM"):
        bad = np.isnan(d[name])
        fill = rng.standard_normal(d[name].shape)
        d[name][bad] = (fill + 1j * fill[::-1] if np.iscomplexobj(d[name]) else np.abs(fill))[bad].astype(d[name].dtype)
    return d


def xtile_sets(n, prec):
    """tests/test_gpu_kstep.py's choice per n, without the set that has no wM (the tiled kernels take the pair), and
    the white set with finite padding."""
    yield from ((s, d) for s, d in tk.planes_sets(n, prec) if d["wM"] is not None)
    yield "white, finite padding", finite_padding(n, prec)


@pytest.fixture(scope="module")
def references():
    """(n, prec, set, mode) -> (reference, bounds): computed once, shared by the one-tile and the two-tile interior case."""
    cache = {}

    def get(inp, n, prec, sname, mode):
        key = (n, prec, sname, mode)
        if key not in cache:
            rdt = ki.types(prec)[0]
            r = ref.planes_step(inp, mode, False)
            cache[key] = (r, kb.planes_step_bound(r, inp, mode, False, rdt, nblocks=n * (inp["nhp"] // ki.pass_kb(rdt))))
        return cache[key]
    return get


# k_step_boundary_x2 has rows for n = 128 and 256 only
KERNEL_CASES = [(n, k) for n in (32, 64, 128) for k in ("first", "interior", "last")] + [(128, "two_tile")]


@pytest.mark.parametrize("n,kname", KERNEL_CASES, ids=["%d-%s" % c for c in KERNEL_CASES])
@pytest.mark.parametrize("prec", PRECS)
def test_tiled_kernel_has_the_bits_of_the_natural_one(lib, padded, references, prec, n, kname):
    mode, two_tile = KERNELS[kname]
    for sname, inp in xtile_sets(n, prec):
        nat, _ = tk.run_planes(lib, inp, mode, False, two_tile)
        got, _ = run_tiled(lib, inp, mode, two_tile)
        for name in ("Ck0", "Ck1", "Ck2", "q_out", "p_out", "g_out"):
            assert np.array_equal(got[name], nat[name], equal_nan=sname != "white, finite padding"), (sname, name)
        if mode == BX_FIRST:
            assert got["guard"] == 0.0 and nat["guard"] == 0.0
            continue
        if sname == "white, finite padding":
            assert np.isfinite(got["guard"])
            continue
        r, b = references(inp, n, prec, sname, mode)
        c = tk.consts("planes_step", prec)["guard"]
        fr = kb.scalar_fraction(got["guard"], r["guard"], c * b["guard"])
        fn = kb.scalar_fraction(nat["guard"], r["guard"], c * b["guard"])
        print("\nXTILE %s<%s> n=%d %s: guard, fraction of the bound: tiled %.3f natural %.3f" % (kname, prec, n, sname, fr, fn))
        assert fr <= 1.0


@pytest.mark.parametrize("prec", PRECS)
def test_control_path_tiled(lib, padded, prec):
    inp = ki.white(32, prec, pad=True)
    for kname, written in (("interior", ("Ck0", "q_out", "p_out")), ("first", ("Ck0", "q_out", "p_out")),
                           ("last", ("g_out", "p_out"))):
        mode, _ = KERNELS[kname]
        tk.check_control(lambda ctl: run_tiled(lib, inp, mode, False, ctl), inp, tk.ALL_OUT, written)


@pytest.mark.parametrize("prec", PRECS)
def test_control_path_tiled_two_tile(lib, prec):
    inp = ki.white(128, prec)
    tk.check_control(lambda ctl: run_tiled(lib, inp, BX_INTERIOR, True, ctl), inp, tk.ALL_OUT, ("Ck0", "q_out", "p_out"))


def test_tiled_entry_refuses_what_has_no_instantiation(lib, padded):
    inp = ki.white(32, "fp64", pad=True)
    kbv = 8
    wpair = tile(np.stack([inp["wS"], inp["wM"]], axis=-1), kbv)
    sc, g, ptr = tk.dbl(0.7, 1.3, 0.05, 0.1, -1e-5), tk.dbl(0.0), tk.ptr

    def call(n, mode, two_tile, wM=inp["wM"], wp=wpair):
        ctl = tk.Ctl()
        return lib.fftp_step_boundary_x_xtile(0, n, 0.0, mode, two_tile, ptr(inp["Ck"].copy()), ptr(inp["q"]), ptr(inp["p"]),
                                              ptr(inp["g_in"]), ptr(tk.filled(inp)), ptr(tk.filled(inp)), ptr(tk.filled(inp)),
                                              ptr(inp["wS"]), ptr(wM), ptr(sc), ptr(g), *ctl.args(), 0, ptr(wp))

    assert call(48, BX_INTERIOR, 0) == -1 and call(32, BX_INTERIOR, 1) == -1 and call(32, 3, 0) == -1
    assert call(32, BX_INTERIOR, 0, wM=None) == -1  # the pair holds wM: a tiled launch without a mass does not exist
    assert call(32, BX_INTERIOR, 0, wp=None) == -1


@pytest.mark.parametrize("n", [32, 64, 128])
@pytest.mark.parametrize("prec", PRECS)
def test_weight_pair_is_the_permuted_weights(lib, padded, prec, n):
    inp = ki.white(n, prec, pad=True)  # 1e12 of dynamic range, zeros, NaN in the padding columns
    kbv = ki.pass_kb(ki.types(prec)[0])
    assert lib.fftp_row_stride(n, tk.pcode(prec)) == inp["nhp"]
    pair = np.full((n * n * inp["nhp"], 2), -7.5)
    tk.check_status(lib.fftp_xtile_weights(tk.pcode(prec), n, tk.ptr(inp["wS"]), tk.ptr(inp["wM"]), tk.ptr(pair)))
    want = tile(np.stack([inp["wS"], inp["wM"]], axis=-1), kbv).reshape(-1, 2)
    assert tk.same_bits(pair, want)
    assert np.isnan(pair).any() and (pair == 0.0).any()  # the padding and the holes of the spectrum went through


# ---- trajectories at 128^3 ------------------------------------------------------------------------------------------------

class Work:
    """A seeded workload: parameters, fields, mock data, step size."""

    def __init__(self, p, f, window, noise, nobs, eps):
        self.p, self.f, self.eps = p, f, eps
        self.arrays = dict(signal_PS=f["signal_PS"], mass_f=f["mass_f"], window=window, noise=noise, nobs=nobs)
        self.q0, self.p0 = f["q0"], f["p0"]


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BCHMC_ZBIN_128", "1")  # 128^3 keeps rocFFT's C2R by default
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def engine(monkeypatch, w, env, precision=0):
    from barcode_amd.engine import Engine
    set_env(monkeypatch, env)
    e = Engine(w.p, precision=precision)
    e.upload(**w.arrays)
    return e


@pytest.fixture(scope="module")
def work128():
    """128^3, Zel'dovich + plane-parallel RSD, Gaussian likelihood, k-space mass: the benchmark's configuration, mock data
    from the engine's own forward model (as the 256^3 fixture of tests/test_gpu_two_array_passes.py makes them)."""
    import os
    from barcode_amd.engine import Engine
    saved = os.environ.get("BCHMC_ZBIN_128")
    os.environ["BCHMC_ZBIN_128"] = "1"
    try:
        p = HamilParams(Nx=128, L=200.0, likelihood=1, rsd_model=1)
        f = inputs.make_fields(p)
        e = Engine(p)
        e.upload(signal_PS=f["signal_PS"], mass_f=f["mass_f"], nobs=np.zeros(p.N), window=np.ones(p.N), noise=np.ones(p.N))
        e.forward(f["truth"], 1)
        dX = e.fetch("deltaX").reshape((p.Nx,) * 3)
        e.close()
    finally:
        if saved is None:
            del os.environ["BCHMC_ZBIN_128"]
        else:
            os.environ["BCHMC_ZBIN_128"] = saved
    window, noise, nobs = inputs.mock_observations(p, dX)
    return Work(p, f, window, noise, nobs, 0.5 * p.eps_heuristic())


DET = dict(BCHMC_DETERMINISTIC="1")
OFF = dict(BCHMC_NO_XTILE="1")


def run(monkeypatch, w, env, precision, neps, **kw):
    e = engine(monkeypatch, w, env, precision)
    q1, p1, done = e.leapfrog(kw.get("q0", w.q0), kw.get("p0", w.p0), kw.get("eps", w.eps), neps)
    e.close()
    return q1, p1, done


@pytest.mark.parametrize("neps", [1, 2, 3])
@pytest.mark.parametrize("precision", [0, 1], ids=["fp64", "fp32"])
def test_trajectory_is_the_natural_layouts_bit_for_bit(monkeypatch, work128, precision, neps):
    new = run(monkeypatch, work128, DET, precision, neps)
    old = run(monkeypatch, work128, dict(DET, **OFF), precision, neps)
    assert new[2] == old[2] == neps
    assert np.all(np.isfinite(new[0])) and np.all(np.isfinite(new[1])) and np.ptp(new[0]) > 0
    assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1])


@pytest.mark.parametrize("switch", ["BCHMC_BX_V2", "BCHMC_NO_PAIR", "BCHMC_NO_VPAIR"])
def test_trajectory_with_the_other_formulations(monkeypatch, work128, switch):
    """fp64 through the two-tile interior kernel, and the tiled kernels with three arrays on either side of them."""
    env = dict(DET, **{switch: "1"})
    new = run(monkeypatch, work128, env, 0, 3)
    old = run(monkeypatch, work128, dict(env, **OFF), 0, 3)
    assert new[2] == old[2] == 3
    assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1])


def test_trajectory_in_the_default_mode(monkeypatch, work128):
    new = run(monkeypatch, work128, {}, 0, 3)
    old = run(monkeypatch, work128, OFF, 0, 3)
    assert new[2] == old[2] == 3
    rq, rp = rel_l2(new[0], old[0]), rel_l2(new[1], old[1])
    print("\nXTILE 128x3 fp64 default mode against BCHMC_NO_XTILE=1: rel-L2 q %.3e (%.0e) p %.3e (%.0e)" % ((rq, NOISE[0][0], rp, NOISE[0][1])))
    assert rq < NOISE[0][0] and rp < NOISE[0][1]


def guard_case(monkeypatch, w, name):
    """(q0, p0, eps, neps, steps_done expected)."""
    p_bad = w.p0.copy().ravel()
    p_bad[0] = 1e60
    if name == "odd_boundary":
        return w.q0, p_bad, 1e-6, 6, 1
    if name == "last_boundary":
        return w.q0, p_bad, 1e-6, 2, 1
    # an even boundary: the prior force of a huge q0[0] moves p(x = 0) by eps g(0) per step (a step a hundred times shorter
    # than the workload's: q, and with it g, stays what it was to 1e-4), and the guard compares |sum_k hw Re p^_k| =
    # N |p(0)| with 1e50 N.  g(0) is linear in q0[0] up to the likelihood's part, which is nothing beside 1e50: measured at
    # 1e56, then q0[0] is set so that eps |g(0)| is 0.7e50 -- under the limit after step 0, over it after step 1.
    eps = 0.01 * w.eps
    e = engine(monkeypatch, w, dict(DET, **OFF))
    q_bad = w.q0.copy().ravel()
    q_bad[0] = 1e56
    g0 = e.gradient(q_bad)[0]
    assert np.isfinite(g0) and g0 != 0.0, g0
    q_bad[0] = 1e56 * 0.7e50 / (eps * abs(g0))
    kick = eps * abs(e.gradient(q_bad)[0])
    e.close()
    print("\nXTILE guard stop, even boundary: q0[0] %.3e, eps |g(0)| %.3e of the limit" % (q_bad[0], kick / 1e50))
    assert 0.6e50 < kick < 0.8e50
    return q_bad, w.p0, eps, 6, 2


@pytest.mark.parametrize("name", ["odd_boundary", "even_boundary", "last_boundary"])
def test_guard_stop(monkeypatch, work128, name):
    w = work128
    q0, p0, eps, neps, want = guard_case(monkeypatch, w, name)
    outs = []
    for env in (dict(DET, **OFF), DET):
        e = engine(monkeypatch, w, env)
        qb, pb, doneb = e.leapfrog(q0, p0, eps, neps)
        q1, p1, done = e.leapfrog(w.q0, w.p0, w.eps, 3)
        e.close()
        print("\nXTILE guard stop, %s, %s: steps_done %d of %d" % (name, "tiled" if env is DET else "natural", doneb, neps))
        assert doneb == want and done == 3
        assert np.all(np.isfinite(qb)) and np.all(np.isfinite(q1))
        outs.append((qb, pb, q1, p1))
    for a_, b_ in zip(outs[0], outs[1]):
        assert np.array_equal(a_, b_)


def test_weights_uploaded_between_trajectories_reach_the_tiled_pair(monkeypatch, work128):
    w = work128
    mass2 = np.ravel(w.f["mass_f"]) * (1.5 + 0.5 * np.cos(np.arange(w.p.N) * 0.37))
    ps2 = np.ravel(w.f["signal_PS"]) * 0.6
    e = engine(monkeypatch, w, DET)
    first = e.leapfrog(w.q0, w.p0, w.eps, 2)
    e.upload(mass_f=mass2, signal_PS=ps2)
    again = e.leapfrog(w.q0, w.p0, w.eps, 2)
    e.close()
    f = engine(monkeypatch, w, dict(DET, **OFF))
    f.upload(mass_f=mass2, signal_PS=ps2)
    fresh = f.leapfrog(w.q0, w.p0, w.eps, 2)
    f.close()
    assert first[2] == again[2] == fresh[2] == 2
    assert not np.array_equal(first[0], again[0])  # the new weights matter
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1])


@pytest.mark.parametrize("precision", [0, 1], ids=["fp64", "fp32"])
def test_early_q_and_late_q_come_out_of_the_tiles(monkeypatch, work128, precision):
    old = run(monkeypatch, work128, dict(DET, **OFF), precision, 2)
    early = run(monkeypatch, work128, DET, precision, 2)
    late = run(monkeypatch, work128, dict(DET, BCHMC_NO_DOWNLOAD_OVERLAP="1"), precision, 2)
    for new in (early, late):
        assert new[2] == 2
        assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1])
