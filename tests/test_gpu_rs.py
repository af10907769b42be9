"""The real-space ALPT kernels (alpt.hpp: k_alpt_grad, k_alpt_sources, k_alpt_kernel_table) and the calc_h 0 / 3 kernels
(variants.hpp: k_findif_mul, k_gradfft_mult, k_mul3, k_conv_kernel, k_interp_tsc), each run alone on the GPU through
libbchmc_fft_probe.so (the engine's kernels on the engine's launches: barcode_amd/csrc/fft_probe.hip) and held per cell to
the bound of tests/rs_bound.py against the longdouble reference of tests/rs_reference.py, on the cases of
tests/rs_cases.py.  tests/test_rs_bounds.py measures the constants and shows on the CPU that the checker rejects the
plausible bugs.

Sizes, the smallest at which each code path differs: 4 (aliased stencil arms), 5 and 9 (stencil_row's odd branch, nyq_keep's
weight 1/2), 8 (slab of 1), 16 and 24 (slab of 3 at 24), 83 (odd, n^2 > 4096 row slots and N > 2048 x 256: the slot loop and
the grid stride both take a second round) and 88 (the same on the slab branch, slab 11).  Every input set runs at 16, the
white set and the impulses at the other sizes.  n > 256, where the k loop of the stencil kernels takes a second round,
stays with the 512^3 trajectories of tests/test_gpu_large.py: its arrays alone take a test out of the seconds range.

Output arrays go in filled with a pattern and every row must come back written; a cell whose bound is 0 must be exact
(the cells an impulse's stencil does not reach, the padding of the kernel table, the planes nyq_keep zeroes, a particle
failing pos_ok); a reference value that is not finite must come back as the same class.  k_alpt_sources runs with both
pointer layouts of alpt_middle.  The half-complex inputs carry NaN in their row padding (BCHMC_FFT_PAD=1 gives small grids
padded rows); what the kernels leave in the padding of their outputs is judged by the canaries alone.  Every check prints
a line `RS ...` with its worst fraction of the bound and where it occurred, then asserts <= 1.

One engine-level case meets the spherical-collapse branch on the real path: sfmodel = 2 on a field scaled so that
D1 delta(1) >= 1.5 in about 12 % of the cells (tests/test_rs_bounds.py holds the conditions on the field), psi, positions
and rho against the oracle at TOL_FIELD, on the 3-D plans at 16^3 and on the planes path at 32^3.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import rs_bound as rb
from tests import rs_cases as rc
from tests import rs_inputs as ri
from tests import rs_reference as ref
from tests.kstep_inputs import box, types

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "barcode_amd", "libbchmc_fft_probe.so")
PRECS = ["fp64", "fp32"]
SIZES = list(ri.SIZES)
FILL = -7.25


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the process-wide HIP runtime first, as barcode_amd.engine does)
    assert os.path.exists(PROBE), "%s not built (make -C barcode_amd/csrc)" % PROBE
    L = C.CDLL(PROBE)
    vp, i, d, ll = C.c_void_p, C.c_int, C.c_double, C.c_longlong
    L.fftp_row_stride.argtypes = [i, i]
    L.fftp_stencil_grid.argtypes = [i]
    L.fftp_alpt_grad.argtypes = [i, i, d, vp, vp]
    L.fftp_alpt_sources.argtypes = [i, i, d, i, vp, vp, vp, d, d]
    L.fftp_alpt_kernel_table.argtypes = [i, i, d, vp, d]
    L.fftp_findif_mul.argtypes = [i, i, d, i, d, d, vp, vp, vp]
    L.fftp_gradfft_mult.argtypes = [i, i, d, vp, vp, d]
    L.fftp_conv_kernel.argtypes = [i, i, d, vp, vp, vp, d, d]
    L.fftp_mul3.argtypes = [i, ll, vp, vp, vp]
    L.fftp_interp_tsc.argtypes = [i, i, d, i, vp, d, vp, vp, vp]
    return L


@pytest.fixture
def padded(monkeypatch):
    """Row padding forced on, so that the small grids have padding columns to poison."""
    monkeypatch.setenv("BCHMC_FFT_PAD", "1")


def ptr(a):
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


def check_status(st):
    if st == -2:   # nothing more runs on a device that has reported an error
        pytest.exit("HIP error in a probe call", returncode=3)
    assert st == 0, {-1: "arguments outside the engine's instantiations", -2: "HIP error"}.get(
        st, "canary after device array %d overwritten" % st)


def pcode(prec):
    return 0 if prec == "fp64" else 1


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def report(kernel, prec, n, sname, got, case):
    worst = rb.judge(got, case["r"], case["bound"], rb.consts(kernel[len("alpt_"):] if kernel == "alpt_kernel_table" else kernel,
                                                              types(prec)[0]))
    print("\nRS k_%s<%s> n=%d %s: worst fraction of the bound %.3f at %s %s" % (kernel, prec, n, sname, worst[0], worst[1],
                                                                              worst[2]))
    assert worst[0] <= 1.0


# ---- k_alpt_grad --------------------------------------------------------------------------------------------------------
def run_grad(lib, phi, n, prec):
    g3 = np.full((3, n, n, n), FILL, phi.dtype)
    check_status(lib.fftp_alpt_grad(pcode(prec), n, box(n), ptr(phi), ptr(g3)))
    return g3


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_k_alpt_grad(lib, prec, n):
    assert lib.fftp_stencil_grid(n) == max(min(n * n, 4096) // 8 * 8, 8)
    for case in rc.grad_cases(n, prec):
        g3 = run_grad(lib, case["phi"], n, prec)
        report("alpt_grad", prec, n, case["name"], {"g3": g3}, case)
        if case["name"].startswith("impulse"):
            # the response is the stencil itself: 4 cells per axis, 2 at n = 4 where ll and rr are one cell and cancel
            assert [int(np.count_nonzero(g)) for g in g3] == [2 if n == 4 else 4] * 3


@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("prec", PRECS)
def test_k_alpt_grad_nonfinite(lib, prec, n):
    """One NaN and one +inf in phi: exactly the cells whose stencil reaches them change class, every other cell is bitwise
    as without them."""
    clean, dirty, cells = ri.nonfinite(n, prec)
    g0, g1 = run_grad(lib, clean, n, prec), run_grad(lib, dirty, n, prec)
    r = ref.alpt_grad(dirty, n, box(n))
    case = dict(r=r, bound=rb.alpt_grad_bound(r, types(prec)[0]))
    report("alpt_grad", prec, n, "nonfinite", {"g3": g1}, case)
    bad = np.zeros((n, n, n), bool)
    for at in cells:
        bad[at] = True
    for c in range(3):
        reach = ref.stencil_reach(bad, c)
        assert not np.isfinite(g1[c][reach]).any() and np.isfinite(g1[c][~reach]).all()
        assert same_bits(g1[c][~reach], g0[c][~reach])


# ---- k_alpt_sources -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_k_alpt_sources(lib, prec, n):
    """layout 0: a_out == d1, b_out separate (alpt_middle on the planes path); layout 1: b_out == d1, a_out separate."""
    for case in rc.sources_cases(n, prec):
        for layout, lname in enumerate(("planes layout", "3-D layout")):
            d1 = case["d1"].copy()
            other = np.full((n, n, n), FILL, d1.dtype)
            check_status(lib.fftp_alpt_sources(pcode(prec), n, box(n), layout, ptr(case["g3"]), ptr(d1), ptr(other), ri.D1,
                                               ri.D2))
            got = {"a": other, "b": d1} if layout else {"a": d1, "b": other}
            report("alpt_sources", prec, n, "%s, %s" % (case["name"], lname), got, case)
            if case["name"].startswith("impulse"):
                at = ri.impulse_cells(n)[case["name"][len("impulse_"):]]
                assert not got["a"][~ref.m2v_support(n, at)].any()


# ---- the k-space kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_k_alpt_kernel_table(lib, padded, prec, n):
    case = rc.table_case(n, prec)
    assert lib.fftp_row_stride(n, pcode(prec)) == case["nhp"]
    tab = np.full((n, n, case["nhp"]), FILL + 2.5j, types(prec)[1])
    check_status(lib.fftp_alpt_kernel_table(pcode(prec), n, box(n), ptr(tab), rc.SMOL))
    report("alpt_kernel_table", prec, n, "table", {"tab": tab}, case)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_k_gradfft_mult(lib, padded, prec, n):
    nh = n // 2 + 1
    for case in rc.gradfft_cases(n, prec):
        fk = case["fk"]
        assert lib.fftp_row_stride(n, pcode(prec)) == fk.shape[2]
        ck = np.full((3,) + fk.shape, FILL + 2.5j, fk.dtype)
        check_status(lib.fftp_gradfft_mult(pcode(prec), n, box(n), ptr(fk), ptr(ck), 1.0 / n ** 3))
        report("gradfft_mult", prec, n, case["name"], {"Ck": ck[:, :, :, :nh]}, case)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_k_conv_kernel(lib, padded, prec, n):
    nh = n // 2 + 1
    for case in rc.conv_cases(n, prec):
        pl = case["pl"]
        assert lib.fftp_row_stride(n, pcode(prec)) == pl.shape[2]
        ck = np.full((3,) + pl.shape, FILL + 2.5j, pl.dtype)
        check_status(lib.fftp_conv_kernel(pcode(prec), n, box(n), ptr(pl), ptr(case["F"]), ptr(ck), rc.HH, 1.0 / n ** 3))
        report("conv_kernel", prec, n, case["name"], {"Ck": ck[:, :, :, :nh]}, case)


# ---- k_mul3, k_findif_mul, k_interp_tsc ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 16, 83])
@pytest.mark.parametrize("prec", PRECS)
def test_k_mul3(lib, prec, n):
    case = rc.mul3_case(n, prec)
    out = np.full((3, n ** 3), FILL, case["a"].dtype)
    check_status(lib.fftp_mul3(pcode(prec), n ** 3, ptr(case["a"]), ptr(case["b3"]), ptr(out)))
    report("mul3", prec, n, case["name"], {"out3": out}, case)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_k_findif_mul(lib, prec, n):
    for case in rc.findif_cases(n, prec):
        V = np.full((3, n, n, n), FILL, case["dX"].dtype)
        check_status(lib.fftp_findif_mul(pcode(prec), n, box(n), case["code"], ri.LN_RHO_C, ri.LN_DELTA_MIN, ptr(case["dX"]),
                                         ptr(case["pl"]), ptr(V)))
        report("findif_mul", prec, n, case["name"], {"V": V}, case)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_k_interp_tsc(lib, prec, n):
    pos = np.array([ri.TSC_POS["cpecvel"], ri.TSC_POS["v_norm"]], np.float64)
    for case in rc.tsc_cases(n, prec):
        psi, conv = np.ascontiguousarray(case["psi"]), np.ascontiguousarray(case["conv"])
        V = np.full((3, n ** 3), FILL, psi.dtype)
        check_status(lib.fftp_interp_tsc(pcode(prec), n, box(n), case["rsd"], ptr(pos), rc.F1, ptr(psi), ptr(conv), ptr(V)))
        assert (~case["r"]["_ok"]).sum() >= 3 and not V[:, ~case["r"]["_ok"]].any()
        report("interp_tsc", prec, n, case["name"], {"V": V}, case)


def test_probe_refuses_what_the_engine_does_not_launch(lib):
    z = np.zeros(3 * 8 ** 3)
    assert lib.fftp_alpt_grad(0, 3, 0.0, ptr(z), ptr(z)) == -1
    assert lib.fftp_alpt_grad(0, 8, 0.0, None, ptr(z)) == -1
    assert lib.fftp_alpt_sources(0, 8, 0.0, 2, ptr(z), ptr(z), ptr(z), 1.0, 1.0) == -1
    assert lib.fftp_findif_mul(0, 8, 0.0, 3, 1.0, -0.5, ptr(z), ptr(z), ptr(z)) == -1
    assert lib.fftp_mul3(0, 0, ptr(z), ptr(z), ptr(z)) == -1
    assert lib.fftp_interp_tsc(0, 8, 0.0, 2, ptr(z), 0.0, ptr(z), ptr(z), ptr(z)) == -1
    assert lib.fftp_alpt_kernel_table(0, 1, 0.0, ptr(z), 1.0) == -1


# ---- the collapse branch on the real path -------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,planes", [(16, 0), (32, 1)], ids=["3d_plans_16", "planes_32"])
def test_engine_alpt_with_collapsed_cells(monkeypatch, nx, planes):
    from tests.util import TOL_FIELD, rel_l2
    if planes:
        monkeypatch.setenv("BCHMC_FFT_PAD", "1")   # planes mode needs whole 128-byte k-groups per row
    else:
        monkeypatch.setenv("BCHMC_NO_ALPT_PLANES", "1")
    c, delta = ri.collapse_case(nx)
    e = c.engine()
    assert e.tile_info()["alpt_planes"] == planes
    o = c.oracle
    dX, px, py, pz = o.Lag2Eul(delta, rsd=0)
    e.forward(delta, 0)
    want = dict(zip(("psix", "psiy", "psiz"), o.alpt_displacement(delta)), posx=px, posy=py, posz=pz,
                rho=o.getDensity(c.p.mk, px, py, pz))
    for name, w in want.items():
        lvl = rel_l2(e.fetch(name), w)
        print("RS engine collapse n=%d %s: rel-L2 %.2e" % (nx, name, lvl))
        assert lvl < TOL_FIELD, name
    e.close()
