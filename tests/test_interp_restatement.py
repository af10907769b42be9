"""CPU-only: the numpy restatement of interpolate_CIC / interpolate_TSC / interpolate_TSC_multi
(tests/interp_restatement.py) that the GPU tests compare bchmc_interp_particles with -- the literal loop against the
vectorised form bit for bit on the edge set, closed forms, the mutants the edge set must tell apart -- and the
declarations of the feature through every layer (header, ctypes signatures, the C++ shim, shim.py, hamil.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import interp_restatement as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = ((4, 4.0), (5, 3.0), (8, 8.0), (9, 1.0), (16, 50.0))


def fields_of(n, count=3, seed=1):
    return np.random.default_rng(seed + n).standard_normal((count, n ** 3))


# ---- loop against vectorised form ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
@pytest.mark.parametrize("kernel", (ir.CIC, ir.TSC), ids=("cic", "tsc"))
@pytest.mark.parametrize("n,L", GRIDS)
def test_loop_and_vectorised_form_agree_bitwise_on_the_edge_set(n, L, kernel, dtype):
    x, y, z = ir.edge_set(n, L, seed=n, n_uniform=200)
    f = fields_of(n)
    a, lost_a = ir.interpolate_loops(kernel, n, L, x, y, z, f, dtype)
    b, lost_b = ir.interpolate(kernel, n, L, x, y, z, f, dtype)
    assert np.array_equal(lost_a, lost_b) and 0 < lost_a.sum() < lost_a.size
    assert np.array_equal(ir.bits(a), ir.bits(b))
    assert np.array_equal(np.isnan(a), np.broadcast_to(lost_a, a.shape))  # NaN exactly where lost
    # one field of a multi-field call is the single-field call
    one, _ = ir.interpolate(kernel, n, L, x, y, z, f[1:2], dtype)
    assert np.array_equal(ir.bits(one[0]), ir.bits(b[1]))


def test_the_named_entry_points():
    n, L = 8, 8.0
    x, y, z = ir.edge_set(n, L, n_uniform=50)
    f = fields_of(n)
    assert np.array_equal(ir.bits(ir.interpolate_CIC(n, L, x, y, z, f[0])), ir.bits(ir.interpolate(ir.CIC, n, L, x, y, z, f[:1])[0][0]))
    assert np.array_equal(ir.bits(ir.interpolate_TSC(n, L, x, y, z, f[0])), ir.bits(ir.interpolate_TSC_multi(n, L, x, y, z, f)[0]))


# ---- the domain ---------------------------------------------------------------------------------------------------------

def test_the_domain_of_each_kernel():
    n, L = 9, 1.0
    d = L / n
    top = np.nextafter(L, 0.0)
    assert top < L and top / d == 9.0  # x < L is not enough: the double below 1.0 lands in cell 9
    f = fields_of(n, 1)
    half = np.full(8, 0.5)
    x = np.array([top, L, -1e-300, -0.0, 0.0, np.nan, np.inf, 2.5 * L])
    for axis in range(3):
        cols = [half, half, half]
        cols[axis] = x
        _, lost = ir.interpolate(ir.TSC, n, L, cols[0], cols[1], cols[2], f)
        assert np.array_equal(lost, [True, True, True, False, False, True, True, True])
        _, lost = ir.interpolate(ir.CIC, n, L, cols[0], cols[1], cols[2], f)
        assert np.array_equal(lost, [False, False, False, False, False, True, True, False])  # CIC folds what is finite
    # fp32 handles: a double beyond the float range is an infinity there, and the position decides as the float
    big = np.array([1e300])
    assert ir.interpolate(ir.CIC, n, L, big, half[:1], half[:1], f, np.float32)[1][0]
    assert not ir.interpolate(ir.CIC, n, L, big, half[:1], half[:1], f, np.float64)[1][0]
    x32 = np.array([np.nextafter(np.float32(L), np.float32(0.0), dtype=np.float32)], dtype=np.float64)  # a float below L
    near = np.array([L * (1 - 2.0 ** -30)])  # rounds to L as a float: kept as a double, lost as a float
    assert not ir.interpolate(ir.TSC, n, L, near, half[:1], half[:1], f, np.float64)[1][0]
    assert ir.interpolate(ir.TSC, n, L, near, half[:1], half[:1], f, np.float32)[1][0]
    assert ir.interpolate(ir.TSC, n, L, x32, half[:1], half[:1], f, np.float32)[1][0] == (float(x32[0]) / d >= n)


# ---- closed forms -------------------------------------------------------------------------------------------------------

def test_a_particle_at_a_cell_centre():
    n, L = 8, 8.0
    f = fields_of(n, 2)
    g = f.reshape(2, n, n, n)
    c = (3, 1, 6)
    x, y, z = (np.array([k + 0.5]) for k in c)
    cic, _ = ir.interpolate(ir.CIC, n, L, x, y, z, f)
    assert np.array_equal(cic[:, 0], g[:, 3, 1, 6])  # cell-centred CIC: that cell's value
    # TSC at a centre: dx = dy = dz = 0, weights 0.125 / 0.75 / 0.125 per axis (the slip changes nothing when dz = dx = dy)
    w = np.array([0.125, 0.75, 0.125])
    want = np.zeros(2)
    for i in range(3):
        for j in range(3):
            for k in range(3):
                want += w[i] * w[j] * w[k] * g[:, c[0] - 1 + i, c[1] - 1 + j, c[2] - 1 + k]
    tsc, _ = ir.interpolate(ir.TSC, n, L, x, y, z, f)
    assert np.array_equal(tsc[:, 0], want)


def test_cic_reproduces_a_linear_field_away_from_the_wrap():
    n, L = 16, 50.0
    d = L / n
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    rng = np.random.default_rng(2)
    x, y, z = rng.uniform(d, L - d, size=(3, 500))  # between the first and the last cell centre
    for axis, idx in enumerate((i, j, k)):
        centre = (idx + 0.5) * d
        field = 2.0 + 3.0 * centre  # linear in one coordinate
        got = ir.interpolate_CIC(n, L, x, y, z, field.reshape(-1))
        want = 2.0 + 3.0 * (x, y, z)[axis]
        # eight products of values up to 2 + 3 L, each rounded three times, and the rounding of xpos / d - c at |xpos / d|
        # up to n: a few ulps of the largest value
        assert np.max(np.abs(got - want)) <= 64 * 2.0 ** -53 * (2.0 + 3.0 * L)


def test_tsc_of_a_constant_field_is_the_product_of_the_slipped_weight_sums():
    """c (sum wx)(sum wy)(sum wz) with wx[2] = wy[2] = wz[2] from dz: only sum wz is 1."""
    n, L, c = 8, 8.0, 3.0
    x, y, z = np.array([2.25]), np.array([5.5]), np.array([1.875])
    dx, dy, dz = -0.25, 0.0, 0.375
    # by hand: w[1] = 0.75 - t^2, w[0] = (0.5 - t)^2 / 2, w[2] = (0.5 + dz)^2 / 2 = 0.3828125 on every axis
    up = 0.5 * 0.875 ** 2
    sx = (0.75 - 0.0625) + 0.5 * 0.75 ** 2 + up
    sy = 0.75 + 0.5 * 0.5 ** 2 + up
    sz = (0.75 - 0.140625) + 0.5 * 0.125 ** 2 + up
    assert (sx, sy, sz) == (1.3515625, 1.2578125, 1.0) and (dx, dy, dz) == (2.25 - 2.5, 5.5 - 5.5, 1.875 - 1.5)
    got = ir.interpolate_TSC(n, L, x, y, z, np.full(n ** 3, c))
    assert abs(got[0] - c * sx * sy * sz) <= 27 * 2.0 ** -52 * c * sx * sy * sz
    no_slip = ir.interpolate(ir.TSC, n, L, x, y, z, [np.full(n ** 3, c)], mutant="no_slip")[0][0]
    assert abs(no_slip[0] - c) <= 27 * 2.0 ** -52 * c  # without the slip the weights are a partition of one


# ---- mutants ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutant,kernel", [("no_slip", ir.TSC), ("no_half_shift", ir.CIC), ("no_second_fold", ir.CIC),
                                          ("domain_x_lt_L", ir.TSC)])
def test_the_edge_set_tells_the_restatement_from_each_mutant(mutant, kernel):
    grids = ((9, 1.0),) if mutant == "domain_x_lt_L" else GRIDS
    for n, L in grids:
        x, y, z = ir.edge_set(n, L, seed=n)
        f = fields_of(n)
        right, lost = ir.interpolate(kernel, n, L, x, y, z, f)
        wrong, lost_w = ir.interpolate(kernel, n, L, x, y, z, f, mutant=mutant)
        if mutant != "no_second_fold":  # (that one leaves coordinates far outside the box, where int64 and int part ways)
            loops, lost_l = ir.interpolate_loops(kernel, n, L, x, y, z, f, mutant=mutant)
            assert np.array_equal(ir.bits(wrong), ir.bits(loops)) and np.array_equal(lost_w, lost_l)
        differ = np.any(ir.bits(right) != ir.bits(wrong), axis=0) | (lost != lost_w)
        assert differ.any(), (mutant, n)
        if mutant == "domain_x_lt_L":  # the mutant keeps nextafter(1, 0), which the restatement loses
            top = np.nextafter(L, 0.0)
            assert np.any((x == top) & lost & ~lost_w)


# ---- declarations through every layer -----------------------------------------------------------------------------------

def header():
    return open(os.path.join(ROOT, "include", "bchmc.h")).read()


def header_args(name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    decl = re.search(r"\bint %s\(([^)]*)\);" % name, text).group(1)
    out = []
    for a in decl.split(","):
        a = " ".join(a.split())
        out.append(re.match(r"^(.*?)(\w+)$", a).group(1).strip())
    return out


def struct_fields(struct):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\}" % struct, text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            t, names = decl.rsplit(" ", 1) if "," not in decl else decl.split(" ", 1)
            out += [(nm.strip().lstrip("*"), t + (" *" if nm.strip().startswith("*") else "")) for nm in names.split(",")]
    return out


def test_the_header_declares_the_entry_points_and_their_properties():
    text = header()
    assert "#define BCHMC_ABI_VERSION 4" in text  # new functions only: no struct or entry point changed
    assert header_args("bchmc_interp_release") == ["bchmc_handle *"]
    assert header_args("bchmc_interp_particles") == [
        "bchmc_handle *", "bchmc_part_source", "const double *", "const double *", "const double *", "uint64_t",
        "const bchmc_interp_field *", "int32_t", "const bchmc_interp_opts *", "double *", "bchmc_interp_stats *"]
    assert "BCHMC_INTERP_MAX_FIELDS = 4" in text and "BCHMC_INTERP_HANDLE_FIELD = 3" in text
    doc = text[:text.index("enum { BCHMC_INTERP_MAX_FIELDS")].rsplit("/* ----", 1)[1]
    for k in range(1, 8):
        assert re.search(r"\bI%d\b" % k, doc), "property I%d" % k
    for word in ("BCHMC_ERR_UNSUPPORTED", "BCHMC_ERR_STATE", "BCHMC_ERR_ARG", "interpolate_grid.cpp", ":166-167",
                 "quiet NaN", "bchmc_interp_release"):
        assert word in doc, word
    assert struct_fields("bchmc_interp_field") == [("source", "int32_t"), ("field", "int32_t"), ("host", "const double *")]
    assert struct_fields("bchmc_interp_opts") == [("kernel", "int32_t"), ("path", "int32_t"), ("reserved[2]", "int32_t")]
    assert struct_fields("bchmc_interp_stats") == [("n_in", "uint64_t"), ("n_lost", "uint64_t"), ("max_per_tile", "uint64_t"),
                                                   ("path_used", "int32_t"), ("reserved", "int32_t")]


def test_engine_mirrors_the_structs_and_binds_the_entry_points():
    from barcode_amd import engine
    dp = C.POINTER(C.c_double)
    assert list(engine.InterpField._fields_) == [("source", C.c_int32), ("field", C.c_int32), ("host", dp)]
    assert [n for n, _ in engine.InterpOpts._fields_] == ["kernel", "path", "reserved"]
    assert [n for n, _ in engine.InterpStats._fields_] == ["n_in", "n_lost", "max_per_tile", "path_used", "reserved"]
    assert C.sizeof(engine.InterpField) == 16 and C.sizeof(engine.InterpOpts) == 16 and C.sizeof(engine.InterpStats) == 32
    assert engine.INTERP_MAX_FIELDS == 4 and engine.INTERP_HANDLE_FIELD == 3 and engine.INTERP_KERNELS == dict(cic=1, tsc=2)
    lib = engine.load()
    ctype = {"bchmc_handle *": C.c_void_p, "bchmc_part_source": C.c_int, "const double *": dp, "double *": dp,
             "uint64_t": C.c_uint64, "int32_t": C.c_int32, "const bchmc_interp_field *": C.POINTER(engine.InterpField),
             "const bchmc_interp_opts *": C.POINTER(engine.InterpOpts), "bchmc_interp_stats *": C.POINTER(engine.InterpStats)}
    assert list(lib.bchmc_interp_particles.argtypes) == [ctype[t] for t in header_args("bchmc_interp_particles")]
    assert list(lib.bchmc_interp_release.argtypes) == [C.c_void_p]
    for name in ("bchmc_interp_particles", "bchmc_interp_release"):
        assert name in engine.EXPORTS and hasattr(C.CDLL(engine.LIB_PATH), name)
    params = list(inspect.signature(engine.Engine.interp_particles).parameters)
    assert params == ["self", "x", "y", "z", "fields", "kernel", "path", "source"]
    assert callable(engine.Engine.interp_release)
    # a null handle: BCHMC_ERR_ARG without touching a device
    x = np.zeros(1)
    p = x.ctypes.data_as(dp)
    fd = (engine.InterpField * 1)(engine.InterpField(0, 0, p))
    o = engine.InterpOpts(1, 0)
    assert lib.bchmc_interp_particles(None, 0, p, p, p, 1, fd, 1, C.byref(o), p, None) == 1
    assert lib.bchmc_interp_release(None) == 1


def test_shim_and_hamil_bind_the_new_names():
    from barcode_amd import hamil, shim
    lib = shim.load()
    assert "bchmc_shim_interpolate" in shim.SHIM_EXPORTS and lib.bchmc_shim_interpolate.argtypes
    text = open(os.path.join(ROOT, "include", "bchmc_shim.hpp")).read()
    assert "-> bchmc_shim::interpolate_CIC" in text[:text.index("#ifndef BCHMC_SHIM_HPP")]  # the opening name map
    # upstream's argument lists behind the view (interpolate_grid.cpp:108-112, 194-195, 271-273)
    assert re.search(r"void interpolate_CIC\(HamilView \*hd, ULONG N1, ULONG N2, ULONG N3, real_prec L1.*?real_prec d3, "
                     r"const real_prec \*xp.*?const real_prec \*field_grid, ULONG N_OBJ,\s*real_prec \*interpolation\);",
                     text, flags=re.S)
    assert re.search(r"void interpolate_TSC\(HamilView \*hd, ULONG N1, ULONG N2, ULONG N3, real_prec d1.*?"
                     r"const real_prec \*field_grid, ULONG N_OBJ,\s*real_prec \*interpolation\);", text, flags=re.S)
    assert re.search(r"void interpolate_TSC_multi\(HamilView \*hd, ULONG N1.*?ULONG N_OBJ, real_prec \*\*field_grids,\s*"
                     r"real_prec \*\*interpolations, int N_fields\);", text, flags=re.S)
    assert "bchmc_shim_interpolate" in text
    for name in ("interpolate_CIC", "interpolate_TSC", "interpolate_TSC_multi"):
        assert callable(getattr(shim.ShimHamil, name)) and callable(getattr(hamil, name))
        assert list(inspect.signature(getattr(hamil, name)).parameters)[:4] == ["hd", "xp", "yp", "zp"]


def test_documents_name_the_feature():
    for doc, words in (("README.md", ("bchmc_interp_particles",)), ("INTEGRATION.md", ("bchmc_interp_particles", "interpolate_TSC_multi")),
                       ("DESIGN.md", ("9.8", "k_itp_gather_tile", "interp_bench", "SPH-kernel gather for free lists"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
