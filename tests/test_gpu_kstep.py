"""The kernels that advance the state in k-space, each run alone on the GPU through libbchmc_fft_probe.so (the engine's
kernels on the engine's launches: barcode_amd/csrc/fft_probe.hip) and held per element and per x-column to the bound of
tests/kstep_bound.py against the longdouble reference of tests/kstep_reference.py, on the input sets of
tests/kstep_inputs.py.  tests/test_kstep_bounds.py measures the constants and shows on the CPU that the checker rejects
the plausible bugs.

- k_step_boundary_x at n = 32 (small block, PER 4), 64 (small block, PER 8) and 128 (big block, PER 4), fp64 and fp32,
  in every mode the engine instantiates: FIRST with and without g_in, FIRST ALPT, INTERIOR, INTERIOR ALPT, LAST with and
  without p_out; k_step_boundary_x2 at 128; at 256 one white-plus-impulses case each for the one-tile <double, 512, 4>
  (the benchmark's) and the two-tile fp32 kernel (the fp32 default), against float64 over the whole array plus
  longdouble on the columns of the first and last lane of the first and last k-group at j in {0, 1, n/2 - 1, n/2,
  n/2 + 1, n - 1} (the padding columns of those k-groups hold NaN on entry and may hold anything on exit: they are
  judged by the canaries alone).
  512 is left out: its arrays alone take a test out of the seconds range; the (2 x big block, PER 8) row of the launch
  table stays with the 512^3 trajectories of tests/test_gpu_large.py.  n = 32 and 64 run with padded rows
  (BCHMC_FFT_PAD=1), which the planes kernels need; 32 sees every input set, 64 and 128 the white set and impulses.
- k_alpt_mix_x at 32, 64, 128.
- the 3-D twins k_kick_drift_za, k_assemble, k_step_boundary, k_alpt_poisson, k_alpt_mix, k_prepare_mult, k_parseval,
  k_rollback at n = 8, 9, 15, 16, 32 (16 also with padded rows).
- the control path: *stop set, guard_prev just under / just over the limit, +-inf and NaN (NaN does not trip:
  fabs(NaN) > x is false, as upstream's comparison).
- cross-checks without a reference: one-tile and two-tile interior outputs bitwise equal on k < nh; the planes kernel
  against the inverse x-DFT of the 3-D kernel's output within the sum of their bounds.

Every input array carries NaN in its row padding (white sets); output arrays go in filled with a pattern, so that what
a kernel must leave alone is compared bitwise.  Every check prints a line `KSTEP ...` with its worst fraction of the
bound and where it occurred, then asserts <= 1.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import kstep_bound as kb
from tests import kstep_inputs as ki
from tests import kstep_reference as ref
from tests.kstep_reference import BX_FIRST, BX_INTERIOR, BX_LAST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "barcode_amd", "libbchmc_fft_probe.so")
PRECS = ["fp64", "fp32"]
FILL = 7.25 - 3.5j
LIMIT = 1e50


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the process-wide HIP runtime first, as barcode_amd.engine does)
    assert os.path.exists(PROBE), "%s not built (make -C barcode_amd/csrc)" % PROBE
    L = C.CDLL(PROBE)
    vp, i, d, ull, ll = C.c_void_p, C.c_int, C.c_double, C.c_ulonglong, C.c_longlong
    L.fftp_row_stride.argtypes = [i, i]
    L.fftp_step_boundary_x.argtypes = [i, i, d, i, i, i] + [vp] * 7 + [vp, vp, vp, vp, vp, vp, vp, d, ull]
    L.fftp_alpt_mix_x.argtypes = [i, i, d, vp, d, d, d]
    L.fftp_kick_drift_za.argtypes = [i, i, d, i] + [vp] * 7 + [vp, vp, vp, d, ull]
    L.fftp_assemble.argtypes = [i, i, d, i] + [vp] * 6 + [i, vp, vp]
    L.fftp_step_boundary.argtypes = [i, i, d, i] + [vp] * 9 + [i, vp, vp, vp, vp, d, ull]
    L.fftp_alpt_poisson.argtypes = [i, i, d, vp, vp, vp, d]
    L.fftp_alpt_mix.argtypes = [i, i, d, vp, d, d, d]
    L.fftp_prepare_mult.argtypes = [i, i, vp, vp, d]
    L.fftp_parseval.argtypes = [i, i, vp, vp, vp]
    L.fftp_rollback.argtypes = [i, ll] + [vp] * 8
    return L


@pytest.fixture
def padded(monkeypatch):
    """Row padding forced on: the planes kernels need whole k-groups, which n < 128 has only then."""
    monkeypatch.setenv("BCHMC_FFT_PAD", "1")


def ptr(a):
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


def check_status(st):
    assert st == 0, {-1: "arguments outside the engine's instantiations", -2: "HIP error"}.get(
        st, "canary after device array %d overwritten" % st)


def pcode(prec):
    return 0 if prec == "fp64" else 1


def dbl(*v):
    return np.array(v, np.float64)


class Ctl:
    """The control words of one call."""

    def __init__(self, stop=0, guard_prev=None, limit=LIMIT, step_index=3, steps_done=99):
        self.stop = np.array([stop], np.int32)
        self.done = np.array([steps_done], np.uint64)
        self.prev = None if guard_prev is None else dbl(guard_prev)
        self.limit, self.step_index = limit, step_index

    def args(self):
        return [ptr(self.stop), ptr(self.done), ptr(self.prev), self.limit, self.step_index]


def filled(inp):
    return np.full((inp["n"], inp["n"], inp["nhp"]), FILL, inp["q"].dtype)


def run_planes(lib, inp, mode, alpt, two_tile=False, ctl=None):
    """One launch of the planes step kernel; returns the outputs by the reference's names, the raw arrays and ctl."""
    ctl = ctl or Ctl()
    assert lib.fftp_row_stride(inp["n"], pcode(inp["prec"])) == inp["nhp"]
    ck = inp["Ck"].copy()
    qo, po, go = filled(inp), filled(inp), filled(inp)
    guard = dbl(0.0)
    p_in = inp["p"]
    p_out = po if p_in is not None else None
    sc = dbl(inp["a"], inp["b"], inp["half_eps"], inp["eps"], inp["c_za"])
    st = lib.fftp_step_boundary_x(pcode(inp["prec"]), inp["n"], inp["L"], mode, int(alpt), int(two_tile), ptr(ck),
                                  ptr(inp["q"]), ptr(p_in), ptr(inp["g_in"]) if mode == BX_FIRST else None,
                                  ptr(qo) if mode != BX_LAST else None, ptr(p_out), ptr(go) if mode == BX_LAST else None,
                                  ptr(inp["wS"]), ptr(inp["wM"]), ptr(sc), ptr(guard), *ctl.args())
    check_status(st)
    got = {"Ck0": ck[0], "Ck1": ck[1], "Ck2": ck[2], "q_out": qo, "p_out": po, "g_out": go, "guard": float(guard[0])}
    return got, ctl


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def judge(got, r, bounds, nh, consts, slicer=None):
    return kb.judge(got, r, bounds, nh, consts, slicer=slicer)


def report(kernel, prec, n, sname, worst):
    print("\nKSTEP %s<%s> n=%d %s: worst fraction of the bound %.3f at %s %s" % (
        kernel, prec, n, sname, worst[0], worst[1], ki.mode_name(worst[2])))
    assert worst[0] <= 1.0


def consts(family, prec):
    return kb.C[family][np.dtype(ki.types(prec)[0]).name]


MODES, with_, alpt_inputs = ki.MODES, ki.with_, ki.alpt_inputs


def untouched_outputs(got, inp, r, mode):
    """What the mode does not write comes back as it went in: the pattern, or the input of Ck."""
    for name in ("q_out", "p_out", "g_out"):
        if name not in r:
            assert same_bits(got[name], filled(inp)), name
    for c in range(3):
        if "Ck%d" % c not in r:
            assert same_bits(got["Ck%d" % c], inp["Ck"][c]), "Ck%d" % c


def check_planes(lib, inp, mode, alpt, two_tile, kernel, sname):
    rdt = ki.types(inp["prec"])[0]
    n, nh = inp["n"], inp["n"] // 2 + 1
    got, _ = run_planes(lib, inp, mode, alpt, two_tile)
    r = ref.planes_step(inp, mode, alpt)
    b = kb.planes_step_bound(r, inp, mode, alpt, rdt, nblocks=n * (inp["nhp"] // ki.pass_kb(rdt)))
    untouched_outputs(got, inp, r, mode)
    report(kernel, inp["prec"], n, sname, judge(got, r, b, nh, consts("planes_step", inp["prec"])))
    return got


def planes_sets(n, prec):
    """32 sees every set; 64 the white set and the first layer of impulses; 128 and above one rotation of it."""
    if n == 32:
        return ki.planes_sets(n, prec)
    return ki.planes_sets(n, prec, 1, 5 if n == 64 else 1, False)


@pytest.mark.parametrize("mname", sorted(MODES))
@pytest.mark.parametrize("n", [32, 64, 128])
@pytest.mark.parametrize("prec", PRECS)
def test_k_step_boundary_x(lib, padded, prec, n, mname):
    mode, alpt, ch = MODES[mname]
    for sname, inp in planes_sets(n, prec):
        check_planes(lib, with_(inp, ch), mode, alpt, False, "k_step_boundary_x[%s]" % mname, sname)


@pytest.mark.parametrize("prec", PRECS)
def test_k_step_boundary_x2_and_one_tile_bitwise(lib, prec):
    """The two-tile kernel at 128 against the reference, and against the one-tile kernel bit for bit on k < nh ("the
    same arithmetic per element"; the guard sums differ in the order of their additions only)."""
    n = 128
    for sname, inp in planes_sets(n, prec):
        two = check_planes(lib, inp, BX_INTERIOR, False, True, "k_step_boundary_x2", sname)
        one, _ = run_planes(lib, inp, BX_INTERIOR, False, False)
        for name in ("Ck0", "Ck1", "Ck2", "q_out", "p_out"):
            assert same_bits(one[name][:, :, :n // 2 + 1], two[name][:, :, :n // 2 + 1]), name


def sample_columns(n, nhp, rdt):
    """First and last lane of the first and the last k-group and every padding column, at the six edge values of j."""
    nh, kbv = n // 2 + 1, ki.pass_kb(rdt)
    ks = sorted({0, kbv - 1, (nhp // kbv - 1) * kbv, nh - 1, nhp - 1} | set(range(nh, nhp)))
    return [(j, k) for j in (0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1) for k in ks]


@pytest.mark.parametrize("case", ["one_tile_fp64", "two_tile_fp32"])
def test_k_step_boundary_x_256(lib, case):
    """White data with the impulses of the first layer added on top in their own columns, interior boundary.

    Cost: the slowest test of the file.  On the host about 6 s go into building the seven 256^2 x 136 input arrays, about
    7 s into the float64 reference and bound over the whole array (eight slabs of j, which keep the memory at an eighth)
    and 1 s into the longdouble columns; the launch with its copies is well under a second.  The whole array is what
    finds an index slip in a column no sample holds, so none of it is skipped."""
    n, prec, two_tile = 256, case[-4:], case.startswith("two")
    rdt, cdt = ki.types(prec)
    nh = n // 2 + 1
    inp = ki.white(n, prec)
    imp = next(ki.impulse_sets(n, prec, max_layers=1, rots=range(1)))[1]
    layer = ki.layers(n, inp["nhp"], rdt)[0]
    for (i, j, k) in layer:  # the impulse's column replaces the white one in every field
        for name in ("Ck", "q", "p"):
            inp[name][..., j, k] = imp[name][..., j, k]
    kernel = "k_step_boundary_x2" if two_tile else "k_step_boundary_x[interior]"
    got, _ = run_planes(lib, inp, BX_INTERIOR, False, two_tile)
    cs = dict(consts("planes_step", prec))
    nblocks = n * (inp["nhp"] // ki.pass_kb(rdt))
    # float64 over the whole array, in slabs of j (columns are independent; the guard sum and its bound add up).  The
    # float64 reference has the kernel's own round-off at T = double: twice the bound there.
    slack = 2.0 if prec == "fp64" else 1.0
    worst, guard_ref, guard_bound = (0.0, None, ()), 0.0, 0.0
    for j0 in range(0, n, 32):
        cols = [(j, k) for j in range(j0, j0 + 32) for k in range(nh)]
        r = ref.planes_step(inp, BX_INTERIOR, False, np.float64, cols)
        b = kb.planes_step_bound(r, inp, BX_INTERIOR, False, rdt, c=slack, nblocks=nblocks)
        guard_ref += float(r.pop("guard"))
        guard_bound += b.pop("guard")
        w = judge(got, r, b, nh, cs, slicer=lambda a: a[:, j0:j0 + 32, :nh].reshape(n, -1))
        if w[0] > worst[0]:
            worst = (w[0], w[1], (w[2][0], j0 + w[2][1] // nh, w[2][1] % nh) if w[2] else ())
    report(kernel, prec, n, "white+impulses float64", worst)
    gf = kb.scalar_fraction(got["guard"], guard_ref, cs["guard"] * guard_bound)
    report(kernel, prec, n, "guard sum", (gf, "guard", ()))
    cols = sample_columns(n, inp["nhp"], rdt)
    data = [c for c in cols if c[1] < nh]
    r = ref.planes_step(inp, BX_INTERIOR, False, np.longdouble, data)
    b = kb.planes_step_bound(r, inp, BX_INTERIOR, False, rdt, nblocks=nblocks)
    b.pop("guard")
    jj, kk = [c[0] for c in data], [c[1] for c in data]
    w = judge(got, r, b, nh, cs, slicer=lambda a: a[:, jj, kk])
    report(kernel, prec, n, "sampled columns longdouble", (w[0], w[1], (w[2][0],) + data[w[2][1]] if w[2] else ()))
    for name in ("Ck0", "Ck1", "Ck2", "q_out", "p_out"):
        assert np.isfinite(got[name][:, :, :nh]).all(), name
    assert np.isfinite(got["guard"])


def test_arguments_outside_the_tables_are_refused(lib, padded):
    """-1, with nothing launched: an n without a row in the launch table, the two-tile kernel where it has none, ALPT on
    the last boundary, a mode that does not exist, rows that are not whole k-groups."""
    inp = ki.white(32, "fp64", pad=True)

    def call(n, mode, alpt, two_tile):
        ctl = Ctl()
        sc = dbl(0.7, 1.3, 0.05, 0.1, -1e-5)
        g = dbl(0.0)
        return lib.fftp_step_boundary_x(0, n, 0.0, mode, alpt, two_tile, ptr(inp["Ck"]), ptr(inp["q"]), ptr(inp["p"]),
                                        ptr(inp["g_in"]), ptr(filled(inp)), ptr(filled(inp)), ptr(filled(inp)),
                                        ptr(inp["wS"]), ptr(inp["wM"]), ptr(sc), ptr(g), *ctl.args())

    assert call(48, BX_INTERIOR, 0, 0) == -1 and call(16, BX_INTERIOR, 0, 0) == -1
    assert call(32, BX_INTERIOR, 0, 1) == -1 and call(64, BX_INTERIOR, 0, 1) == -1
    assert call(32, BX_LAST, 1, 0) == -1 and call(32, 3, 0, 0) == -1 and call(32, -1, 0, 0) == -1
    assert lib.fftp_alpt_mix_x(0, 48, 0.0, ptr(inp["Ck"]), 1.0, 1.0, 1.0) == -1
    assert lib.fftp_alpt_mix(0, 1, 0.0, ptr(inp["Ck"]), 1.0, 1.0, 1.0) == -1


def test_unpadded_rows_are_refused_by_the_planes_entries(lib, monkeypatch):
    monkeypatch.setenv("BCHMC_FFT_PAD", "0")
    inp = ki.white(32, "fp64", pad=False)
    assert lib.fftp_alpt_mix_x(0, 32, 0.0, ptr(inp["Ck"]), 1.0, 1.0, 1.0) == -1


# ---- k_alpt_mix_x ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [32, 64, 128])
@pytest.mark.parametrize("prec", PRECS)
def test_k_alpt_mix_x(lib, padded, prec, n):
    rdt = ki.types(prec)[0]
    for sname, inp in planes_sets(n, prec):
        d = alpt_inputs(inp)
        ck = d["Ck"].copy()
        check_status(lib.fftp_alpt_mix_x(pcode(prec), n, d["L"], ptr(ck), d["smol"], d["inv_wtot"], d["inv_n"]))
        r = ref.alpt_mix(d, True)
        b = kb.alpt_mix_bound(r, d, True, rdt)
        got = {"Ck0": ck[0], "Ck1": ck[1], "Ck2": ck[2]}
        report("k_alpt_mix_x", prec, n, sname, judge(got, r, b, n // 2 + 1, consts("alpt_mix_x", prec)))


# ---- the 3-D twins -----------------------------------------------------------------------------------------------------

def twin_sets(n, prec, pad):
    return ki.twin_sets(n, prec, pad, None if n <= 16 else 1)


def run_kick_drift_za(lib, d, drift, ctl=None):
    ctl = ctl or Ctl()
    q, p, ck = d["q"].copy(), d["p"].copy(), np.full_like(d["Ck"], FILL)
    sc = dbl(d["half_eps"], d["eps"], d["c_za"])
    check_status(lib.fftp_kick_drift_za(pcode(d["prec"]), d["n"], d["L"], int(drift), ptr(q), ptr(p), ptr(d["g_in"]),
                                        ptr(d["wM"]), ptr(d.get("extra")), ptr(ck), ptr(sc), *ctl.args()))
    return {"q_out": q, "p_out": p, "Ck0": ck[0], "Ck1": ck[1], "Ck2": ck[2]}, ctl


def run_assemble(lib, d, kick, like_mode, stop=0):
    g, p, guard = filled(d), d["p"].copy(), dbl(0.0)
    sc = dbl(d["a"], d["b"], d["c_kick"])
    st = np.array([stop], np.int32)
    check_status(lib.fftp_assemble(pcode(d["prec"]), d["n"], d["L"], int(kick), ptr(d["Ck"]), ptr(d["q"]), ptr(d["wS"]),
                                   ptr(g), ptr(p), ptr(sc), like_mode, ptr(guard), ptr(st)))
    return {"g_out": g, "p_out": p, "guard": float(guard[0])}


def run_step_boundary(lib, d, last, like_mode, ctl=None):
    ctl = ctl or Ctl()
    ck, qo, po, g, guard = d["Ck"].copy(), filled(d), filled(d), filled(d), dbl(0.0)
    sc = dbl(d["a"], d["b"], d["half_eps"], d["eps"], d["c_za"])
    check_status(lib.fftp_step_boundary(pcode(d["prec"]), d["n"], d["L"], int(last), ptr(ck), ptr(d["q"]), ptr(d["p"]),
                                        ptr(qo), ptr(po), ptr(g), ptr(d["wS"]), ptr(d["wM"]), ptr(sc), like_mode,
                                        ptr(guard), *ctl.args()))
    return {"Ck0": ck[0], "Ck1": ck[1], "Ck2": ck[2], "q_out": qo, "p_out": po, "g_out": g, "guard": float(guard[0])}, ctl


def twin_checks(lib, inp):
    """Every 3-D twin on one input -> {kernel: worst}."""
    prec, n = inp["prec"], inp["n"]
    rdt = ki.types(prec)[0]
    nh, cs = n // 2 + 1, consts("twins", prec)
    res = {}
    for drift in (False, True):
        for extra in ((False, True) if drift else (False,)):
            d = with_(inp, dict(extra=np.ascontiguousarray(inp["Ck"][2]) if extra else None))
            got, _ = run_kick_drift_za(lib, d, drift)
            r = ref.kick_drift_za(d, drift)
            if not drift:
                assert same_bits(got["q_out"], d["q"]) and same_bits(got["p_out"], d["p"])
            res["k_kick_drift_za[%d%s]" % (drift, ",extra" if extra else "")] = judge(
                got, r, kb.kick_drift_za_bound(r, d, drift, rdt), nh, cs)
    for like_mode in (0, 1, 2):
        for kick in (False, True):
            d = with_(inp, dict(c_kick=inp["half_eps"]))
            got = run_assemble(lib, d, kick, like_mode)
            r = ref.assemble(d, kick, like_mode)
            if not kick:
                assert same_bits(got["p_out"], d["p"]) and got["guard"] == 0.0
            res["k_assemble[%d] like_mode %d" % (kick, like_mode)] = judge(
                got, r, kb.assemble_bound(r, d, kick, rdt, nblocks=2048), nh, cs)
        for last in (False, True):
            got, _ = run_step_boundary(lib, inp, last, like_mode)
            r = ref.step_boundary(inp, last, like_mode)
            for name in ("q_out", "g_out"):
                if name not in r:
                    assert same_bits(got[name], filled(inp)), name
            if last:
                assert same_bits(np.stack([got["Ck0"], got["Ck1"], got["Ck2"]]), inp["Ck"])
            res["k_step_boundary[%d] like_mode %d" % (last, like_mode)] = judge(
                got, r, kb.step_boundary_bound(r, inp, last, rdt, nblocks=2048), nh, cs)
    d = with_(inp, dict(scale=0.77 / float(n) ** 3))
    d1, phi = filled(d), filled(d)
    check_status(lib.fftp_alpt_poisson(pcode(prec), n, d["L"], ptr(d["q"]), ptr(d1), ptr(phi), d["scale"]))
    r = ref.alpt_poisson(d)
    res["k_alpt_poisson"] = judge({"d1": d1, "phi": phi}, r, kb.alpt_poisson_bound(r, rdt), nh, cs)
    d = alpt_inputs(inp)
    ck = d["Ck"].copy()
    check_status(lib.fftp_alpt_mix(pcode(prec), n, d["L"], ptr(ck), d["smol"], d["inv_wtot"], d["inv_n"]))
    r = ref.alpt_mix(d, False)
    res["k_alpt_mix"] = judge({"Ck0": ck[0], "Ck1": ck[1], "Ck2": ck[2]}, r, kb.alpt_mix_bound(r, d, False, rdt), nh, cs)
    return res


@pytest.mark.parametrize("case", ["8", "9", "15", "16", "16pad", "32"])
@pytest.mark.parametrize("prec", PRECS)
def test_3d_twins(lib, monkeypatch, prec, case):
    n, pad = int(case[:2].rstrip("p")), case.endswith("pad")
    if pad:
        monkeypatch.setenv("BCHMC_FFT_PAD", "1")
    worst = {}
    for sname, inp in twin_sets(n, prec, True if pad else None):
        assert lib.fftp_row_stride(n, pcode(prec)) == inp["nhp"]
        for kname, w in twin_checks(lib, inp).items():
            if kname not in worst or w[0] > worst[kname][1][0]:
                worst[kname] = (sname, w)
    for kname, (sname, w) in sorted(worst.items()):
        report(kname, prec, n, "worst of the sets (%s)" % sname, w)


@pytest.mark.parametrize("case", ["8", "9", "15", "16", "16pad", "32"])
@pytest.mark.parametrize("prec", PRECS)
def test_k_prepare_mult(lib, monkeypatch, prec, case):
    """corr depends on i, j and k separately, with zeros and negative entries; the row padding of mult must come back
    as it went in, the columns k < nh are normFS / corr to two roundings or exactly 0."""
    n, pad = int(case[:2].rstrip("p")), case.endswith("pad")
    if pad:
        monkeypatch.setenv("BCHMC_FFT_PAD", "1")
    nhp, nh = lib.fftp_row_stride(n, pcode(prec)), n // 2 + 1
    corr = ki.corr_grid(n)
    mult = np.full((n, n, nhp), -7.0)
    check_status(lib.fftp_prepare_mult(pcode(prec), n, ptr(corr), ptr(mult), 0.37))
    want = ref.prepare_mult(corr, n, 0.37)
    assert np.all(mult[:, :, nh:] == -7.0)
    fr, at = kb.fraction(mult[:, :, :nh], want, 2 * kb.UD * np.abs(want))
    report("k_prepare_mult", prec, n, "corr(i,j,k)", (fr, "mult", at))


@pytest.mark.parametrize("case", ["8", "9", "15", "16", "16pad", "32"])
@pytest.mark.parametrize("prec", PRECS)
def test_k_parseval(lib, monkeypatch, prec, case):
    """sum of hw w |x|^2 over k < nh, NaN in the row padding of x and w; bound: 4 operations per term and the additions of
    any order, u_d times the sum of the absolute terms."""
    n, pad = int(case[:2].rstrip("p")), case.endswith("pad")
    if pad:
        monkeypatch.setenv("BCHMC_FFT_PAD", "1")
    inp = ki.white(n, prec, pad=True if pad else None, planes=False)
    assert lib.fftp_row_stride(n, pcode(prec)) == inp["nhp"]
    parts = np.full(lib.fftp_parseval_blocks(), np.nan)
    check_status(lib.fftp_parseval(pcode(prec), n, ptr(inp["q"]), ptr(inp["wS"]), ptr(parts)))
    want, sabs = ref.parseval(inp["q"], inp["wS"], n)
    terms = n * n * (n // 2 + 1)
    fr = kb.scalar_fraction(float(np.sum(parts.astype(np.longdouble))), want, (4 + terms) * kb.UD * float(sabs))
    report("k_parseval", prec, n, "white", (fr, "sum", ()))


@pytest.mark.parametrize("s", [0, 1, 2, 3])
@pytest.mark.parametrize("prec", PRECS)
def test_k_rollback(lib, prec, s):
    """s >= 1 with *stop set: (q_read, (p_read + p_written) / 2) of the pair boundary s - 1 read, one rounding of the mean;
    s = 0 means *stop clear: nothing written."""
    rdt, cdt = ki.types(prec)
    rng = np.random.default_rng(40 + s)
    count = 70001  # several workgroups and a ragged end
    q0, p0, q1, p1 = ((rng.standard_normal(count) + 1j * rng.standard_normal(count)).astype(cdt) for _ in range(4))
    qd, pd = np.full(count, FILL, cdt), np.full(count, FILL, cdt)
    stop, done = np.array([1 if s else 0], np.int32), np.array([max(s, 1)], np.uint64)
    check_status(lib.fftp_rollback(pcode(prec), count, ptr(stop), ptr(done), ptr(q0), ptr(p0), ptr(q1), ptr(p1), ptr(qd), ptr(pd)))
    if s == 0:
        assert same_bits(qd, np.full(count, FILL, cdt)) and same_bits(pd, np.full(count, FILL, cdt))
        return
    qw, pw = ref.rollback(s, q0, p0, q1, p1)
    assert same_bits(qd, qw.astype(cdt))
    uT = kb.unit_roundoff(rdt)
    fr, at = kb.fraction(pd, pw, (uT + 2 * kb.UD) * (0.5 * np.abs(p0.astype(np.clongdouble)) + 0.5 * np.abs(p1.astype(np.clongdouble))))
    report("k_rollback", prec, count, "s=%d" % s, (fr, "p_dst", at))


# ---- the control path --------------------------------------------------------------------------------------------------

TRIP = {"just_under": (np.nextafter(LIMIT, 0), False), "at": (LIMIT, False), "just_over": (np.nextafter(LIMIT, np.inf), True),
        "minus_over": (-np.nextafter(LIMIT, np.inf), True), "inf": (np.inf, True), "minus_inf": (-np.inf, True),
        "nan": (np.nan, False)}  # NaN does not trip: fabs(NaN) > x is false, as upstream's comparison


def assert_left_alone(got, inp, names):
    for name in names:
        if name.startswith("Ck"):
            assert same_bits(got[name], inp["Ck"][int(name[2])]), name
        elif name == "guard":
            assert got["guard"] == 0.0
        else:
            assert same_bits(got[name], filled(inp)), name


def control_cases():
    yield "stop_set", dict(stop=1, guard_prev=0.0), "skip"
    for name, (val, trips) in TRIP.items():
        yield name, dict(stop=0, guard_prev=val), "trip" if trips else "run"


def check_control(run, inp, outputs, written):
    for cname, kw, expect in control_cases():
        got, ctl = run(Ctl(**kw))
        if expect == "run":
            assert ctl.stop[0] == 0 and ctl.done[0] == 99, cname
            for name in written:
                assert not same_bits(got[name], filled(inp) if not name.startswith("Ck") else inp["Ck"][int(name[2])]), (cname, name)
            continue
        assert_left_alone(got, inp, outputs)
        if expect == "skip":
            assert ctl.stop[0] == 1 and ctl.done[0] == 99, cname
        else:
            assert ctl.stop[0] == 1 and ctl.done[0] == 3, cname


ALL_OUT = ("Ck0", "Ck1", "Ck2", "q_out", "p_out", "g_out", "guard")


@pytest.mark.parametrize("prec", PRECS)
def test_control_path_planes(lib, padded, prec):
    inp = ki.white(32, prec, pad=True)
    for mname, written in (("interior", ("Ck0", "q_out", "p_out")), ("interior_alpt", ("Ck0", "q_out", "p_out")),
                           ("first", ("Ck0", "q_out", "p_out")), ("first_alpt", ("Ck0", "q_out")), ("last", ("g_out", "p_out"))):
        mode, alpt, ch = MODES[mname]
        check_control(lambda ctl: run_planes(lib, inp, mode, alpt, False, ctl), inp, ALL_OUT, written)
    # the two uncontrolled uses ignore the control words altogether
    for mname, written in (("first_za_only", ("Ck0",)), ("last_g_only", ("g_out",))):
        mode, alpt, ch = MODES[mname]
        d = with_(inp, ch)
        got, ctl = run_planes(lib, d, mode, alpt, False, Ctl(stop=1, guard_prev=np.inf))
        assert ctl.stop[0] == 1 and ctl.done[0] == 99
        for name in written:
            assert not same_bits(got[name], filled(d) if name != "Ck0" else d["Ck"][0]), name


@pytest.mark.parametrize("prec", PRECS)
def test_control_path_two_tile(lib, prec):
    inp = ki.white(128, prec)
    check_control(lambda ctl: run_planes(lib, inp, BX_INTERIOR, False, True, ctl), inp, ALL_OUT, ("Ck0", "q_out", "p_out"))


@pytest.mark.parametrize("prec", PRECS)
def test_control_path_twins(lib, prec):
    inp = ki.white(16, prec, planes=False)
    for last in (False, True):
        check_control(lambda ctl: run_step_boundary(lib, inp, last, 0, ctl), inp, ALL_OUT,
                      ("g_out", "p_out") if last else ("Ck0", "q_out", "p_out"))
    for cname, kw, expect in control_cases():
        got, ctl = run_kick_drift_za(lib, inp, True, Ctl(**kw))
        if expect == "run":
            assert ctl.stop[0] == 0 and not same_bits(got["q_out"], inp["q"]), cname
            continue
        assert same_bits(got["q_out"], inp["q"]) and same_bits(got["p_out"], inp["p"]), cname
        assert same_bits(np.stack([got["Ck0"], got["Ck1"], got["Ck2"]]), np.full_like(inp["Ck"], FILL)), cname
        assert ctl.stop[0] == 1 and ctl.done[0] == (99 if expect == "skip" else 3), cname
    # k_assemble<KICK> tests *stop only
    d = with_(inp, dict(c_kick=0.05))
    got = run_assemble(lib, d, True, 0, stop=1)
    assert same_bits(got["g_out"], filled(d)) and same_bits(got["p_out"], d["p"]) and got["guard"] == 0.0


# ---- planes kernel against the 3-D kernel ------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_planes_kernel_agrees_with_x_dft_of_3d_kernel(lib, padded, prec):
    """The same k-space input through k_step_boundary (3-D, like_mode 0) and, in planes space, through
    k_step_boundary_x<INTERIOR>: q', p' and the guard sum agree within the sum of the two bounds, and Psi in planes space
    is the inverse x-DFT (longdouble) of the 3-D kernel's Psi^ within the planes bound plus sqrt(n) times the column
    norm of the 3-D bound."""
    n = 32
    rdt, cdt = ki.types(prec)
    nh = n // 2 + 1
    k3 = ki.white(n, prec, pad=True, planes=False)
    pl = with_(k3, dict(Ck=ki.to_planes(k3["Ck"], cdt)))
    # both kernels must see the same V^: hand the 3-D kernel the x-DFT (longdouble, rounded once) of the planes input
    vk = np.zeros_like(k3["Ck"])
    vk[..., :nh] = np.fft.fft(pl["Ck"][..., :nh].astype(np.clongdouble), axis=1).astype(cdt)
    k3 = with_(k3, dict(Ck=vk))
    got3, _ = run_step_boundary(lib, k3, False, 0)
    gotp, _ = run_planes(lib, pl, BX_INTERIOR, False)
    r3, rp = ref.step_boundary(k3, False, 0), ref.planes_step(pl, BX_INTERIOR, False)
    b3 = kb.step_boundary_bound(r3, k3, False, rdt, nblocks=2048)
    bp = kb.planes_step_bound(rp, pl, BX_INTERIOR, False, rdt, nblocks=n * (pl["nhp"] // ki.pass_kb(rdt)))
    c3, cp = consts("twins", prec), consts("planes_step", prec)
    uT = kb.unit_roundoff(rdt)
    # rounding V^ to T for the 3-D kernel moves g^ by |f| u_T (|kx V^_x| + |ky V^_y| + |kz V^_z|) <= u_T |gabs|: p', q' follow
    slackg = uT * r3["_gabs"] * 2 * abs(k3["half_eps"])
    worst = (0.0, None, ())
    for name, extra in (("p_out", slackg), ("q_out", slackg * np.abs(r3.get("_ew", 0)))):
        bound = c3[name] * b3[name][0] + cp[name] * bp[name][0] + extra
        d = np.abs(got3[name][:, :, :nh].astype(np.clongdouble) - gotp[name][:, :, :nh].astype(np.clongdouble))
        fr = float(np.max(np.where(bound > 0, d / np.where(bound > 0, bound, 1), np.where(d > 0, np.inf, 0))))
        fr = fr if np.isfinite(fr) else np.inf
        if fr > worst[0]:
            worst = (fr, name, np.unravel_index(int(np.argmax(np.where(bound > 0, d / np.where(bound > 0, bound, 1), 0))), d.shape))
    mz = np.abs(r3["_mz"])
    G = r3["_G"]
    for c, kk in enumerate((G.kx, G.ky, G.kz)):
        name = "Ck%d" % c
        psi3 = np.fft.ifft(got3[name][:, :, :nh].astype(np.clongdouble), axis=0, norm="forward")
        e3 = c3[name] * b3[name][0] + np.abs(kk) * mz * slackg * np.abs(r3.get("_ew", 0))
        colb = cp[name] * bp[name][1] + np.sqrt(n) * kb.col2(e3)
        d = np.abs(gotp[name][:, :, :nh].astype(np.clongdouble) - psi3)
        e2 = kb.col2(d)
        with np.errstate(divide="ignore", invalid="ignore"):
            fr = float(np.max(np.where(colb > 0, e2 / np.where(colb > 0, colb, 1), np.where(e2 > 0, np.inf, 0))))
        fr = fr if np.isfinite(fr) else np.inf
        if fr > worst[0]:
            worst = (fr, name, ())
    # the guard sums: p_end moves by half_eps times the same rounding of V^, slackg / 2 per element
    gbound = c3["guard"] * b3["guard"] + cp["guard"] * bp["guard"] + float(np.sum(G.hw * slackg / 2))
    fr = kb.scalar_fraction(got3["guard"], gotp["guard"], gbound)
    if fr > worst[0]:
        worst = (fr, "guard", ())
    report("k_step_boundary_x[interior] vs x-DFT of k_step_boundary", prec, n, "white", worst)
