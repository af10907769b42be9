"""bchmc_density_particles without a GPU: the declarations through every layer (header, library, engine.py, the C++ shim,
shim.py, hamil.py, io.py), the refusal of a null handle, the file writer, and closed forms of the longdouble reference
(tests/catalogue_reference.py) that the GPU tests compare the kernels with.

Upstream's CIC is cell-centred (getCICcells shifts the coordinate by d / 2, interpolate_grid.cpp:31-33): a particle at a
cell CENTRE puts weight 1 into that one cell, and a particle at a cell CORNER splits into eight times 1/8.  Both are
asserted.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import catalogue_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
CTYPE = {"bchmc_handle *": C.c_void_p, "bchmc_part_source": C.c_int, "const double *": C.POINTER(C.c_double),
         "double *": C.POINTER(C.c_double), "uint64_t": C.c_uint64}


def header():
    return open(os.path.join(ROOT, "include", "bchmc.h")).read()


def header_args(name):
    """The parameter types of a prototype in bchmc.h, comments removed."""
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    decl = re.search(r"\bint %s\(([^)]*)\);" % name, text).group(1)
    out = []
    for a in decl.split(","):
        a = " ".join(a.split())
        m = re.match(r"^(.*?)(\w+)$", a)
        out.append(m.group(1).strip())
    return out


def test_the_header_declares_the_entry_points_and_their_properties():
    text = header()
    assert "#define BCHMC_ABI_VERSION 4" in text  # new functions only: no struct or entry point changed
    assert header_args("bchmc_catalogue_release") == ["bchmc_handle *"]
    args = header_args("bchmc_density_particles")
    assert args == ["bchmc_handle *", "bchmc_part_source", "const double *", "const double *", "const double *",
                    "const double *", "uint64_t", "const bchmc_density_opts *", "double *", "bchmc_density_stats *"]
    assert re.search(r"BCHMC_PART_HOST = 0", text) and re.search(r"BCHMC_PART_FORWARD = 1", text)
    doc = text[:text.index("typedef enum { BCHMC_PART_HOST")].rsplit("/* ----", 1)[1]
    for k in range(1, 8):
        assert re.search(r"\bD%d\b" % k, doc), "property D%d" % k
    for word in ("BCHMC_ERR_UNSUPPORTED", "BCHMC_ERR_STATE", "BCHMC_ERR_ARG", "massFunctions.cc:195", "LAG2EULer"):
        assert word in doc, word


def _fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\}" % struct, re.sub(r"/\*.*?\*/", "", header(), flags=re.S), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            t, names = decl.split(" ", 1)
            out += [(nm.strip(), t) for nm in names.split(",")]
    return out


def test_engine_mirrors_the_structs_and_binds_the_entry_points():
    from barcode_amd import engine
    ct = {"int32_t": C.c_int32, "double": C.c_double, "uint64_t": C.c_uint64}
    assert [(n, ct[t]) for n, t in _fields("bchmc_density_opts")] == list(engine.DensityOpts._fields_)
    assert [(n, ct[t]) for n, t in _fields("bchmc_density_stats")] == list(engine.DensityStats._fields_)
    assert C.sizeof(engine.DensityOpts) == 24 and C.sizeof(engine.DensityStats) == 24
    lib = engine.load()
    want = [CTYPE.get(t) or {"const bchmc_density_opts *": C.POINTER(engine.DensityOpts),
                             "bchmc_density_stats *": C.POINTER(engine.DensityStats)}[t]
            for t in header_args("bchmc_density_particles")]
    assert list(lib.bchmc_density_particles.argtypes) == want
    assert list(lib.bchmc_catalogue_release.argtypes) == [C.c_void_p]
    for name in ("bchmc_density_particles", "bchmc_catalogue_release"):
        assert name in engine.EXPORTS and hasattr(C.CDLL(engine.LIB_PATH), name)
    assert engine.PART_SOURCES == dict(host=0, forward=1) and engine.F_NOBS == engine.FIELDS["nobs"]
    import inspect
    params = list(inspect.signature(engine.Engine.density_particles).parameters)
    assert params == ["self", "x", "y", "z", "w", "mk", "kernel_h", "to_nobs", "source", "download"]
    with pytest.raises(ValueError):
        engine.Engine.density_particles(None, download=False)  # nowhere to put the field
    assert callable(engine.Engine.catalogue_release)
    # a null handle, or no options: BCHMC_ERR_ARG without touching a device
    x = np.zeros(1)
    dp = x.ctypes.data_as(C.POINTER(C.c_double))
    o = engine.DensityOpts(1, 0, 0.0, -1, 0)
    assert lib.bchmc_density_particles(None, 0, dp, dp, dp, None, 1, C.byref(o), dp, None) == 1
    assert lib.bchmc_catalogue_release(None) == 1


def test_shim_hamil_and_io_bind_the_new_names(tmp_path, monkeypatch):
    from barcode_amd import hamil, io, shim
    lib = shim.load()
    assert "bchmc_shim_getDensity" in shim.SHIM_EXPORTS and lib.bchmc_shim_getDensity.argtypes
    text = open(os.path.join(ROOT, "include", "bchmc_shim.hpp")).read()
    for kernel in ("NGP", "CIC", "TSC", "SPH"):
        assert re.search(r"\bvoid getDensity_%s\(HamilView \*hd" % kernel, text)
    assert "-> bchmc_shim::getDensity_NGP" in text[:text.index("#ifndef BCHMC_SHIM_HPP")]  # the opening name map
    assert "bchmc_shim_getDensity" in text
    # upstream's argument lists behind the view (massFunctions.cc:49-51, 100-101, 167-169, 392-396)
    assert re.search(r"getDensity_CIC\(HamilView \*hd, ULONG N1.*?real_prec \*delta,\s*bool weightmass\);", text, flags=re.S)
    assert re.search(r"getDensity_SPH\(HamilView \*hd, ULONG N1.*?bool weightmass, real_prec kernel_h\);", text, flags=re.S)
    assert callable(shim.ShimHamil.getDensity) and callable(hamil.getDensity)
    with pytest.raises(ValueError):
        hamil.getDensity(None, 1, [0.5], [0.5], [0.5], None, True)  # weightmass without Par_mass
    # quick_dump_scalar(density, N1, fname_out, 0, false) of tools/density.cc: the raw array, default name "density"
    rho = np.arange(27, dtype=np.float64) * 0.25
    # The writer's extension rule is upstream's (IOfunctionsGen.cc:185-191): ".dat" only when the name holds no '.' at
    # all, directories included -- so the name is given relative to the working directory, as the tool is run
    monkeypatch.chdir(tmp_path)
    path = io.dump_density(rho)
    assert path == "density.dat" and os.path.getsize(tmp_path / "density.dat") == 27 * 8
    assert np.array_equal(io.read_array("density", 27), rho)
    os.makedirs("run.1")
    dotted = io.dump_density(rho, os.path.join("run.1", "density"))  # a '.' anywhere in the name: taken as given
    assert dotted == os.path.join("run.1", "density") and os.path.getsize(dotted) == 27 * 8
    import inspect
    assert inspect.signature(io.dump_density).parameters["fname_out"].default == "density"


def test_documents_name_the_feature():
    for doc, words in (("README.md", ("bchmc_density_particles",)), ("INTEGRATION.md", ("bchmc_density_particles", "getDensity_SPH")),
                       ("DESIGN.md", ("9.7", "k_cat_scatter", "catalogue_bench"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)


# ---- closed forms of the reference --------------------------------------------------------------------------------------

N, MINS = 8, (-1.5, 0.25, 3.0)


def one(mk, point, w=None, mins=(0.0, 0.0, 0.0), h=None):
    geo = cr.Geometry(N, float(N), mins)
    pos = [np.array([c]) for c in point]
    return cr.density(mk, pos, None if w is None else np.array([w]), geo, h), geo


def test_one_particle_at_a_cell_centre():
    centre = (3.5, 1.5, 6.5)
    cell = 6 + N * (1 + N * 3)
    ref, geo = one(0, centre)
    assert ref.S[cell] == 1 and ref.S.sum() == 1 and ref.cnt.sum() == 1 and ref.n_in == 1
    ref, geo = one(1, centre)  # cell-centred CIC: all of it in the particle's own cell
    assert ref.S[cell] == 1 and np.count_nonzero(ref.S) == 1 and ref.cnt.sum() == 8
    ref, geo = one(1, (3.0, 1.0, 6.0))  # a cell corner: eight times 1/8
    assert np.count_nonzero(ref.S) == 8 and np.all(ref.S[ref.S != 0] == LD(1) / 8)
    ref, geo = one(2, centre)  # 27 values: (1/8, 3/4, 1/8) per axis
    w1 = np.array([LD(1) / 8, LD(3) / 4, LD(1) / 8])
    want = np.sort((w1[:, None, None] * w1[None, :, None] * w1[None, None, :]).ravel())
    assert np.count_nonzero(ref.S) == 27 and np.array_equal(np.sort(ref.S[ref.S != 0]), want)
    assert ref.S[cell] == LD(27) / 64
    for h in (1.0, 1.3):  # W(0) / (pi h^3) at the home cell
        ref, geo = one(3, centre, h=h)
        pi = LD("3.14159265358979323846264338327950288")
        assert abs(ref.S[cell] - 1 / (pi * LD(h) ** 3)) <= LD(2) ** -60 and ref.S[cell] == ref.S.max()
        assert ref.cnt[cell] == 1


def test_cic_and_tsc_conserve_the_weight_exactly():
    for mins in ((0.0, 0.0, 0.0), MINS):
        geo = cr.Geometry(N, float(N), mins)
        pos, w = cr.catalogue_sets(geo, np.float64, names=("weights",))["weights"]
        inside = np.ones(len(w), dtype=bool)
        for x, m in zip(pos, geo.mins):
            inside &= (x >= m) & (x < m + geo.L)
        assert inside.all()
        total = np.sum(w.astype(LD))
        for mk in (1, 2):
            ref = cr.density(mk, pos, w, geo)
            # every coordinate is a double and d = 1: each particle's eight (27) longdouble weights add to its w up to
            # the rounding of the products, 2^-64 relative to sum |w W| = A
            assert abs(ref.S.sum() - total) <= LD(2) ** -60 * ref.A.sum(), mk
            assert ref.n_in == len(w) and ref.cnt.sum() == len(w) * (8 if mk == 1 else 27)
        unit = cr.density(1, pos, None, geo)
        assert np.array_equal(unit.A, unit.S) and np.array_equal(unit.M, unit.cnt.astype(LD))


def test_domain_tests_and_the_upper_face():
    """NGP, CIC and SPH lose x == min + L; TSC keeps it, in cell 0, with upstream's weights of a particle n - 1/2 cells
    from that cell's centre.  NaN and infinities are lost everywhere; SPH does not subtract min from its cell index."""
    geo = cr.Geometry(N, float(N), (0.0, 0.0, 0.0))
    top = [np.array([float(N)]), np.array([3.5]), np.array([3.5])]
    for mk in (0, 1, 3):
        assert cr.density(mk, top, None, geo, 1.0).n_in == 0
    t = cr.density(2, top, None, geo)
    dd = LD(N) - LD(0.5)
    assert t.n_in == 1 and t.S[3 + N * 3] == (LD(0.75) - dd * dd) * LD(0.75) * LD(0.75)
    bad = [np.array([np.nan, np.inf, -np.inf, 1.0]), np.array([1.0, 1.0, 1.0, 1.0]), np.array([1.0, 1.0, 1.0, np.nan])]
    for mk in (0, 1, 2, 3):
        r = cr.density(mk, bad, None, geo, 1.0)
        assert r.n_in == 0 and not r.S.any()
    shifted, geo2 = one(3, (3.5, 1.5, 6.5), mins=(2.5, 0.25, 5.0), h=1.0)
    assert shifted.S.argmax() == 6 + N * (1 + N * 3)  # the cell of x / d, not of (x - min) / d
