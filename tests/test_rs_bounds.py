"""The bound of tests/rs_bound.py on the CPU: every real-space ALPT kernel and calc_h 0 / 3 kernel restated in numpy
(storage in float32 / float64, arithmetic in float64, operation by operation as alpt.hpp and variants.hpp write it), run on
the cases of tests/rs_cases.py and judged against the longdouble reference of tests/rs_reference.py.

- test_measured_constants: the worst fraction of the bound at C = 1 per kernel, type and output, over n = 4, 5, 8, 9, 16, 24,
  83, 88; asserted equal (rounded up to two digits) to rs_bound.MEASURED, whose 4-fold is the constant the HIP kernels
  are held to.  Measured against the longdouble reference, never against the GPU.
- test_reference_*: the reference against closed forms (plane waves, impulse supports).
- test_stencil_row_*: stencil_row over slots [0, n^2) is a bijection onto (i, j), the slots of workgroup b lie in the slab of
  b & 7 for n divisible by 8; tests/host/stencil_row_check.cpp runs the real stencil_row / stencil_grid for the same table
  (stand-alone, address and undefined-behaviour sanitizers).
- test_mutant_*: the checker, at the constants the GPU test uses, rejects each plausible bug by the factor MUTANT_FLOOR
  states (the measured worst fraction of the bound, rounded down; inf: a wrong class or a non-zero where the bound is 0).
"""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import rs_bound as rb
from tests import rs_cases as rc
from tests import rs_inputs as ri
from tests import rs_reference as ref
from tests.kstep_inputs import box, types
from tests.kstep_reference import kval, nyq_keep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ["fp64", "fp32"]
FILL = -7.25
STENCIL_SIZES = (4, 5, 8, 9, 16, 24, 66, 72, 83, 88, 128, 256)
quiet = dict(invalid="ignore", over="ignore", divide="ignore")


# ---- the launch mapping of the stencil passes (launch_grid.hpp: stencil_row, stencil_grid) ---------------------------
def stencil_row(slot, n):
    if n & 7 == 0:
        slab, x, loc = n >> 3, slot & 7, slot >> 3
        return loc // slab, x * slab + loc % slab
    return slot // n, slot % n


def stencil_grid(n):
    return max(min(n * n, 4096) // 8 * 8, 8)


def rows_visited(n, skip_slot=None):
    """(n, n) bool: the rows (i, j) the slot loop of every workgroup reaches."""
    seen = np.zeros((n, n), bool)
    grid = stencil_grid(n)
    for b in range(grid):
        for slot in range(b, n * n, grid):
            if slot != skip_slot:
                seen[stencil_row(slot, n)] = True
    return seen


# ---- the kernels restated -----------------------------------------------------------------------------------------------
def arm_nowrap(A, off, axis):
    """a[o + (c + off) stride] without the wrap: the flat array rolled, so that the upper edge reads the next row."""
    stride = (A.shape[1] * A.shape[2], A.shape[2], 1)[axis]
    return np.roll(A.reshape(-1), -off * stride).reshape(A.shape)


def findif_axis(a, axis, n, L, mut=None):
    fac = n / (2.0 * L)
    A = a.astype(np.float64)
    l, r, ll = (ref.arm(A, o, axis) for o in (-1, 1, -2))
    rr = arm_nowrap(A, 2, axis) if mut == "rr_nowrap" else ref.arm(A, 2, axis)
    c1, c2 = (1.0 / 6, 4.0 / 3) if mut == "swap_consts" else (4.0 / 3, 1.0 / 6)
    with np.errstate(**quiet):
        return -(fac * (c1 * (l - r) - c2 * (ll - rr)))


def stored(values, rdt, n, skip_slot=None):
    """What a stencil kernel leaves in an output array that went in filled: the rows its slot loop reaches."""
    out = np.full(values.shape, FILL, rdt)
    seen = rows_visited(n, skip_slot)[:, :, None]
    with np.errstate(**quiet):
        return np.where(seen, values.astype(rdt), out)


def k_alpt_grad(phi, n, L, mut=None, skip_slot=None):
    rdt = phi.dtype
    return {"g3": np.array([stored(findif_axis(phi, c, n, L, mut), rdt, n, skip_slot) for c in range(3)])}


def k_alpt_sources(g3, d1, n, L, D1, D2, mut=None, skip_slot=None):
    rdt = d1.dtype
    gx, gy, gz = g3
    xx, xy, xz = (findif_axis(gx, ax, n, L) for ax in (0, 2 if mut == "xy_stride" else 1, 2))
    yy, yz, zz = findif_axis(gy, 1, n, L), findif_axis(gy, 2, n, L), findif_axis(gz, 2, n, L)
    with np.errstate(**quiet):
        m2v = xx * yy - xy * xy + xx * zz - xz * xz + yy * zz
        if mut != "drop_term":
            m2v = m2v - yz * yz
        dl = d1.astype(np.float64)
        a = D1 * dl - D2 * m2v
        psilin = -D1 * dl
        arg = 1.0 + 2.0 / 3.0 * psilin
        take = (arg >= -1e-9) if mut == "branch_late" else (arg > 0.0)
        psisc = np.where(take, 3.0 * (np.sqrt(arg) - 1.0), 3.0 if mut == "plus3" else -3.0)
    return {"a": stored(a, rdt, n, skip_slot), "b": stored(-psisc, rdt, n, skip_slot)}


def kgrid64(n, nk, L):
    kv = kval(n, L, max(n, nk))
    return kv[:n, None, None], kv[None, :n, None], kv[None, None, :nk]


def k_alpt_kernel_table(n, nhp, L, smol, cdt, mut=None):
    kx, ky, kz = kgrid64(n, nhp, L)
    k = np.arange(nhp)[None, None, :]
    val = np.exp(-(kx * kx + ky * ky + kz * kz) * smol * smol / 2.0)
    return {"tab": np.where((k < n // 2 + 1) | (mut == "padding"), val, 0.0).astype(cdt)}


def k_gradfft_mult(fk, n, L, inv_n, mut=None):
    nh = n // 2 + 1
    v = fk[:, :, :nh].astype(np.complex128)
    keep = nyq_keep(n, nh)
    if mut == "plain_mask":
        h = n // 2
        i, j, k = np.arange(n)[:, None, None], np.arange(n)[None, :, None], np.arange(nh)[None, None, :]
        keep = np.where((i == h) | (j == h) | (k == h), 0.0, 1.0)
    keep = keep * inv_n
    with np.errstate(**quiet):
        out = [np.where(keep == 0.0, 0.0, (-kk * v.imag * keep) + 1j * (kk * v.real * keep)) for kk in kgrid64(n, nh, L)]
    return {"Ck": np.array(out).astype(fk.dtype)}


def k_conv_kernel(pl, F, n, L, hh, inv_n, mut=None):
    nh = n // 2 + 1
    v = pl[:, :, :nh].astype(np.complex128)
    f = F[:, :, :nh]
    s = -1.0 if mut == "rotation" else 1.0
    with np.errstate(**quiet):
        out = [(hh * kk * (s * -v.imag) * f * inv_n) + 1j * (hh * kk * (s * v.real) * f * inv_n) for kk in kgrid64(n, nh, L)]
    return {"Ck": np.array(out).astype(pl.dtype)}


def k_mul3(a, b3):
    with np.errstate(**quiet):
        return {"out3": a[None] * b3}


def k_findif_mul(dX, plike, n, L, code, rho_c, delta_min, mut=None):
    fac = n / (2.0 * L)
    v = dX.astype(np.float64)
    with np.errstate(**quiet):
        if code == 2:
            if mut == "no_clamp":
                v = np.log(rho_c * (1.0 + v))
            elif mut == "clamp_after":
                v = np.log(rho_c * (1.0 + v))
                v = np.where(v < delta_min, delta_min, v)
            else:
                v = np.log(rho_c * (1.0 + np.where(v < delta_min, delta_min, v)))
        pl = plike.astype(np.float64)
        out = []
        for c in range(3):
            l, r, ll, rr = (ref.arm(v, o, c) for o in ref.OFFSETS)
            out.append((pl * -(fac * ((4.0 / 3) * (l - r) - (1.0 / 6) * (ll - rr)))).astype(dX.dtype))
    return {"V": np.array(out)}


def k_interp_tsc(psi, conv, geo, rsd, f1, cpecvel, v_norm, mut=None):
    rdt = psi.dtype
    n, N = geo.n, geo.N
    pos, ok = ref.tsc_positions(psi, geo, rsd, rdt, cpecvel, v_norm)
    xk = [np.where(ok, x.astype(np.float64), 0.5) / geo.d for x in pos]
    c = [np.trunc(x).astype(np.int64) for x in xk]
    d = [x - (ci.astype(np.float64) + 0.5) for x, ci in zip(xk, c)]
    w = [[0.5 * ((1.5 - np.abs(dd + 1)) * (1.5 - np.abs(dd + 1))), 0.75 - dd * dd,
          0.5 * ((1.5 - np.abs(du - 1)) * (1.5 - np.abs(du - 1)))]
         for dd, du in zip(d, d if mut == "fix_dz" else (d[2], d[2], d[2]))]
    cv = conv.reshape(3, n, n, n)
    o = np.zeros((3, N))
    for a in range(3):
        for b in range(3):
            for e in range(3):
                ww = w[0][a] * w[1][b] * w[2][e]
                ia, ib, ie = (c[0] % n + n + a - 1) % n, (c[1] % n + n + b - 1) % n, (c[2] % n + n + e - 1) % n
                for comp in range(3):
                    o[comp] += ww * cv[comp][ia, ib, ie].astype(np.float64)
    if rsd:
        comp = 1 if mut == "f1_component" else 2
        o[comp] += f1 * o[comp]
    o[:, ~ok] = 0.0
    return {"V": o.astype(rdt)}


# ---- running a case through a restatement ------------------------------------------------------------------------------
def run(kernel, case, n, prec, mut=None, skip_slot=None):
    L = box(n)
    if kernel == "alpt_grad":
        return k_alpt_grad(case["phi"], n, L, mut, skip_slot)
    if kernel == "alpt_sources":
        return k_alpt_sources(case["g3"], case["d1"], n, L, ri.D1, ri.D2, mut, skip_slot)
    if kernel == "kernel_table":
        return k_alpt_kernel_table(n, case["nhp"], L, rc.SMOL, types(prec)[1], mut)
    if kernel == "gradfft_mult":
        return k_gradfft_mult(case["fk"], n, L, 1.0 / n ** 3, mut)
    if kernel == "conv_kernel":
        return k_conv_kernel(case["pl"], case["F"], n, L, rc.HH, 1.0 / n ** 3, mut)
    if kernel == "mul3":
        return k_mul3(case["a"], case["b3"])
    if kernel == "findif_mul":
        return k_findif_mul(case["dX"], case["pl"], n, L, case["code"], ri.LN_RHO_C, ri.LN_DELTA_MIN, mut)
    if kernel == "interp_tsc":
        return k_interp_tsc(case["psi"], case["conv"], case["geo"], case["rsd"], rc.F1, mut=mut, **ri.TSC_POS)
    raise KeyError(kernel)


def cases(kernel, n, prec):
    one = {"kernel_table": rc.table_case, "mul3": rc.mul3_case}
    if kernel in one:
        return [one[kernel](n, prec)]
    return {"alpt_grad": rc.grad_cases, "alpt_sources": rc.sources_cases, "gradfft_mult": rc.gradfft_cases,
            "conv_kernel": rc.conv_cases, "findif_mul": rc.findif_cases, "interp_tsc": rc.tsc_cases}[kernel](n, prec)


def worst_over(kernel, n, prec, consts=None, mut=None, skip_slot=None, only=None, per=None):
    worst = 0.0
    for case in cases(kernel, n, prec):
        if only is not None and not only(case):
            continue
        got = run(kernel, case, n, prec, mut, skip_slot)
        worst = max(worst, rb.judge(got, case["r"], case["bound"], consts, per)[0])
    return worst


def round_up(x):
    if x == 0 or not math.isfinite(x):
        return x
    e = 10.0 ** (math.floor(math.log10(x)) - 1)
    return round(math.ceil(x / e - 1e-9) * e, 12)


@pytest.mark.parametrize("kernel", sorted(rb.MEASURED))
@pytest.mark.parametrize("prec", PRECS)
def test_measured_constants(kernel, prec):
    per = {}
    for n in ri.SIZES:
        worst_over(kernel, n, prec, per=per)
    tname = np.dtype(types(prec)[0]).name
    figures = {o: round_up(f) for o, f in per.items()}
    print("\nRS measured %s<%s>: %s" % (kernel, tname, figures))
    assert all(math.isfinite(f) for f in figures.values()), figures
    assert figures == rb.MEASURED[kernel][tname]


# ---- the reference against closed forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 16])
def test_reference_plane_wave(n):
    L = box(n)
    for axis in range(3):
        phi = ri.wave(n, axis)
        r = ref.alpt_grad(phi, n, L)
        want = ri.wave_response(n, L, axis)
        for c in range(3):
            if c == axis:
                # phi itself is cos() in double: off by 2^-53 (its own rounding and that of the argument, <= 2 pi + 0.3)
                assert np.max(np.abs(r["g3"][c] - want)) <= 2.0 ** -52 * 8 * np.max(r["_S"][c])
            else:
                assert not r["g3"][c].any()


@pytest.mark.parametrize("n", [4, 5, 8, 16])
def test_reference_impulse_supports(n):
    """The response of the first pass to an impulse is the stencil: 12 cells (9 at n = 4, where ll and rr are one cell and
    cancel), everything else exactly 0; m2v through both passes lives inside m2v_support."""
    L = box(n)
    for at in ri.impulse_cells(n).values():
        phi = np.zeros((n, n, n))
        phi[at] = 1
        r = ref.alpt_grad(phi, n, L)
        reach = ref.grad_support(n, at)
        assert [int(m.sum()) for m in reach] == [3 if n == 4 else 4] * 3
        for c in range(3):
            assert not r["g3"][c][~reach[c]].any() and not r["_S"][c][~reach[c]].any()
            # at n = 4 the aliased arm cancels: the value there is 0 although the stencil reaches it
            assert int(np.count_nonzero(r["g3"][c])) == (2 if n == 4 else 4)
        s = ref.alpt_sources(r["g3"], np.zeros((n, n, n)), n, L, ri.D1, ri.D2)
        sup = ref.m2v_support(n, at)
        assert not s["_m2v"][~sup].any() and not s["_X"][~sup].any() and not s["_P"][~sup].any()
        assert sup.sum() < n ** 3 or n <= 5


def test_collapse_branch_cells_are_in_the_sets():
    """The special delta(1) values take both branches, on both sides of the edge, in both types, and one is NaN."""
    for prec in PRECS:
        arg = rc.sources_cases(ri.FULL, prec)[0]["r"]["_arg"]
        fin = np.isfinite(arg)
        assert (arg[fin] <= 0).sum() >= 3 and (arg[fin] > 0).sum() >= 3 and np.isnan(arg).sum() == 1
        assert np.abs(arg[fin]).min() < 4 * float(np.finfo(types(prec)[0]).eps)


@pytest.mark.parametrize("nx", [16, 32])
def test_collapse_case_reaches_the_branch(nx):
    """The engine-level case of tests/test_gpu_rs.py: D1 delta(1) >= 1.5 in at least 1 % and at most 50 % of the cells, and
    no cell with |1 - 2/3 D1 delta(1)| < 1e-6, so that the square root amplifies round-off by no more than about 1e3."""
    c, delta = ri.collapse_case(nx)
    assert c.p.D1 == ri.D1 and c.p.D2 == ri.D2
    t = c.p.D1 * np.asarray(delta).ravel()
    frac = float(np.mean(t >= 1.5))
    edge = float(np.abs(1.0 - 2.0 / 3.0 * t).min())
    print("\nRS collapse case n=%d: D1 delta >= 1.5 in %.1f %% of the cells, nearest to the edge %.2e" % (nx, 100 * frac, edge))
    assert 0.01 <= frac <= 0.5 and edge >= 1e-6


# ---- stencil_row --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", STENCIL_SIZES)
def test_stencil_row_is_a_bijection(n):
    rows = [stencil_row(s, n) for s in range(n * n)]
    assert len(set(rows)) == n * n and all(0 <= i < n and 0 <= j < n for i, j in rows)
    grid = stencil_grid(n)
    assert grid % 8 == 0 and 8 <= grid <= max(n * n, 8) and grid <= 4096
    assert rows_visited(n).all()
    if n % 8 == 0:
        slab = n // 8
        for b in range(grid):
            assert all(stencil_row(s, n)[1] // slab == b & 7 for s in range(b, n * n, grid)), b


def test_stencil_row_host_program(tmp_path):
    """The real stencil_row / stencil_grid of launch_grid.hpp, compiled as plain C++ with the address and undefined-behaviour
    sanitizers into a stand-alone program, check themselves and print the table (n, grid, slot -> i, j) this file's restatement must equal."""
    exe = str(tmp_path / "stencil_row_check")
    # the sanitizer runtimes are linked statically, so the program does not care what else the process has preloaded
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "host", "stencil_row_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(n) for n in STENCIL_SIZES], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    out = r.stdout
    lines = out.split("\n")
    pos = 0
    for n in STENCIL_SIZES:
        head = lines[pos].split()
        assert head == ["n", str(n), "grid", str(stencil_grid(n))], head
        got = np.array(lines[pos + 1].split(), dtype=np.int64).reshape(n * n, 2)
        want = np.array([stencil_row(s, n) for s in range(n * n)])
        assert np.array_equal(got, want), n
        pos += 2


# ---- mutants ------------------------------------------------------------------------------------------------------------
def mutant(kernel, mut, prec, n=ri.FULL, skip_slot=None, only=None):
    c = rb.consts(kernel, types(prec)[0])
    assert worst_over(kernel, n, prec, c, only=only) <= 1.0
    return worst_over(kernel, n, prec, c, mut, skip_slot, only)


MUTANTS = [
    ("alpt_sources", "plus3", PRECS, {}),          # the -3 branch returning +3
    ("alpt_sources", "branch_late", ["fp64"], {}),  # taken at arg < -1e-9: float32 has no delta(1) with arg in [-1e-9, 0)
    ("alpt_sources", "drop_term", PRECS, {}),      # yz^2 dropped
    ("alpt_sources", "xy_stride", PRECS, {}),      # xy = d g_x / d z: the wrong stride
    ("alpt_grad", "swap_consts", PRECS, {}),       # 4/3 and 1/6 swapped
    ("alpt_grad", "rr_nowrap", PRECS, {}),         # rr = c + 2 without the wrap at the upper edge
    ("alpt_grad", None, PRECS, dict(skip_slot=37)),     # a slot of stencil_row skipped: stale fill
    ("alpt_sources", None, PRECS, dict(skip_slot=200)),
    ("findif_mul", "no_clamp", PRECS, {}),
    ("findif_mul", "clamp_after", PRECS, {}),
    ("interp_tsc", "fix_dz", PRECS, {}),           # the upstream dz bug "fixed"
    ("interp_tsc", "f1_component", PRECS, {}),     # f1 on the y component
    ("conv_kernel", "rotation", PRECS, {}),        # (Im, -Re) for (-Im, Re)
    ("gradfft_mult", "plain_mask", PRECS, dict(n=9)),   # the plain Nyquist mask at odd n
    ("kernel_table", "padding", PRECS, {}),        # a non-zero value in the padding column
]
# the smallest factor over the bound, over the types, by which each mutant is rejected (measured, rounded down)
MUTANT_FLOOR = {
    ("alpt_sources", "plus3"): 8e6, ("alpt_sources", "branch_late"): math.inf, ("alpt_sources", "drop_term"): 5e8,
    ("alpt_sources", "xy_stride"): 5e9, ("alpt_grad", "swap_consts"): 3e10, ("alpt_grad", "rr_nowrap"): math.inf,
    ("alpt_grad", None): math.inf, ("alpt_sources", None): math.inf, ("findif_mul", "no_clamp"): math.inf,
    ("findif_mul", "clamp_after"): math.inf, ("interp_tsc", "fix_dz"): 2e10, ("interp_tsc", "f1_component"): 2e6,
    ("conv_kernel", "rotation"): 8e6, ("gradfft_mult", "plain_mask"): 4e6, ("kernel_table", "padding"): math.inf,
}


@pytest.mark.parametrize("kernel,mut,precs,kw", MUTANTS, ids=["%s-%s" % (m[0], m[1] or "skip_slot") for m in MUTANTS])
def test_mutant_is_rejected(kernel, mut, precs, kw):
    for prec in precs:
        f = mutant(kernel, mut, prec, **kw)
        print("\nRS mutant %s %s <%s>: %.3g x the bound" % (kernel, mut or "skip_slot", prec, f))
        assert f >= MUTANT_FLOOR[(kernel, mut)], (prec, f)
