"""The bispectrum's definition, bounds and bindings without a GPU: the float64 restatement of tests/bispec_reference.py
agrees with the enumerated definition under the bounds of tests/bispec_bound.py at n = 4, 5, 8, 9, 12, 16, its counts are
the enumeration's integers, four wrong variants each miss a bound or an exact count, and B4's rule never drops a triplet
that holds a triangle."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import bispec_bound as bb
from tests import bispec_reference as br

# (n, k_min / k_f, dk / k_f, n_shell): the smallest grid with the shells of the issue; odd grids; edges that fall exactly on
# mode lengths (k_min = dk = k_f and k_min = k_f, dk = k_f / 2); shells below 2/3 k_Nyquist (B4's rule active) and up to
# sqrt(3) k_Nyquist (aliased triangles, rule inactive); n_shell = 1 and 32
CASES = ((4, 0.5, 1.0, 3), (5, 0.5, 1.0, 3), (5, 1.0, 1.0, 2), (8, 0.5, 0.7, 3), (8, 0.0, 0.22, 32), (8, 1.5, 2.0, 1),
         (9, 1.0, 0.5, 4), (9, 1.0, 1.0, 7), (12, 0.5, 1.0, 3), (16, 0.5, 1.5, 3), (16, 0.5, 1.0, 6))
ACTIVE = {(8, 0.5, 0.7, 3), (9, 1.0, 0.5, 4), (12, 0.5, 1.0, 3), (16, 0.5, 1.5, 3)}


def ident(case):
    return "%d-%g-%g-%d" % case


@functools.lru_cache(maxsize=None)
def both(case):
    """(restatement, definition) of the seeded white field of the case's grid."""
    n, kmin_kf, dk_kf, ns = case
    L = br.box_of(n)
    k_min, dk = br.edges(n, kmin_kf, dk_kf)
    x = br.field(n)
    return x, L, br.restatement(x, L, k_min, dk, ns), br.definition(x, L, k_min, dk, ns)


def misses(x, L, got, want):
    """What of a restated result misses the float64 bound or an exact count against the enumeration: a list of names."""
    b = bb.bounds(x, L, got, np.float64)
    out = []
    if not np.array_equal(got["nmode"].astype(np.int64), want["nmode"]):
        out.append("nmode")
    if not np.array_equal(np.rint(got["ntri"]).astype(np.int64), want["ntri"]):
        out.append("ntri")
    if bb.fraction(np.abs(got["b"] - want["b"]).astype(np.float64), b["b"]) > 1.0:
        out.append("b")
    if bb.fraction(np.abs(got["power"] - want["power"]).astype(np.float64), b["power"]) > 1.0:
        out.append("power")
    return out


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_restatement_agrees_with_the_enumeration(case):
    n, kmin_kf, dk_kf, ns = case
    x, L, got, want = both(case)
    assert br.rule_active(n, L, *br.edges(n, kmin_kf, dk_kf), ns) == (case in ACTIVE)
    b = bb.bounds(x, L, got, np.float64)
    fb = bb.fraction(np.abs(got["b"] - want["b"]).astype(np.float64), b["b"])
    fn = bb.fraction(np.abs(got["ntri"] - want["ntri"]), b["ntri"])
    fp = bb.fraction(np.abs(got["power"] - want["power"]).astype(np.float64), b["power"])
    print("%s: error / bound B %.3g, ntri %.3g, power %.3g; largest ntri bound %.3g"
          % (ident(case), fb, fn, fp, float(np.max(b["ntri"]))))
    assert fb <= 1.0 and fn <= 1.0 and fp <= 1.0
    assert float(np.max(b["ntri"])) < 0.5  # so rint(ntri) must be the count
    assert misses(x, L, got, want) == []
    assert np.all(np.abs(got["kmean"] - want["kmean"]) <= b["kmean"])
    assert np.any(want["ntri"] > 0) and np.any(want["b"] != 0)


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_enumerated_counts_are_symmetric_and_the_restatement_rounds_to_them(case):
    _, _, got, want = both(case)
    cnt = want["count_all"]
    for perm in itertools.permutations(range(3)):
        assert np.array_equal(cnt, np.transpose(cnt, perm))
    assert np.array_equal(np.rint(got["ntri"]).astype(np.int64), want["ntri"])
    # every ordered pair of modes of two shells closes with exactly one k3, in some shell or none
    assert np.all(cnt.sum(axis=2) <= np.outer(want["nmode"], want["nmode"]))


def mutant_of(case, **switch):
    n, kmin_kf, dk_kf, ns = case
    x, L, _, want = both(case)
    k_min, dk = br.edges(n, kmin_kf, dk_kf)
    return misses(x, L, br.restatement(x, L, k_min, dk, ns, **switch), want)


def test_lower_edge_compared_strictly_misses_the_counts():
    """Mutant: |k| > k_min in place of >=.  With k_min = k_f the six modes of length k_f leave shell 0."""
    for case in ((5, 1.0, 1.0, 2), (9, 1.0, 0.5, 4)):
        assert mutant_of(case) == []
        m = mutant_of(case, lower_edge_strict=True)
        assert "nmode" in m and "ntri" in m, m


def test_zero_mode_admitted_misses_the_counts():
    """Mutant: k = 0 in shell 0 at k_min = 0."""
    case = (8, 0.0, 0.22, 32)
    assert mutant_of(case) == []
    m = mutant_of(case, admit_zero_mode=True)
    assert "nmode" in m and "ntri" in m, m


def test_hermitian_weight_dropped_misses_nmode():
    for case in ((4, 0.5, 1.0, 3), (9, 1.0, 1.0, 7)):
        m = mutant_of(case, hermitian_weight=False)
        assert "nmode" in m and "ntri" not in m, m


def test_one_power_of_n_off_misses_the_bound():
    for case in ((5, 0.5, 1.0, 3), (16, 0.5, 1.5, 3)):
        assert mutant_of(case, n_power=2) == ["b"]
        assert mutant_of(case, n_power=4) == ["b"]


RULE_GRIDS = (4, 5, 8, 9, 12, 16)
RULE_EDGES = tuple(itertools.product((0.0, 0.5, 1.0, 1.0 / 3.0), (0.5, 0.7, 1.0, np.sqrt(2.0) / 2.0)))


@pytest.mark.parametrize("n", RULE_GRIDS)
def test_the_empty_rule_never_drops_a_triangle(n):
    """B4, exhaustively: for every (k_min, dk) of the set and the largest n_shell that keeps the rule active, no triplet
    the rule marks empty has an enumerated triple; and the rule does drop something where three shells allow it."""
    L = br.box_of(n)
    dropped = checked = 0
    for kmin_kf, dk_kf in RULE_EDGES:
        k_min, dk = br.edges(n, kmin_kf, dk_kf)
        ns = min(32, int(np.floor(((2.0 / 3.0) * (n / 2.0) - kmin_kf) / dk_kf)))
        while ns >= 1 and not br.rule_active(n, L, k_min, dk, ns):
            ns -= 1
        if ns < 1:
            continue
        comp = br.computed(n, L, k_min, dk, ns)
        count, _ = br.enumerate_direct(n, L, k_min, dk, ns)
        cnt = br.sorted_table(count)
        assert np.all(cnt[~comp] == 0), (n, kmin_kf, dk_kf, ns)
        dropped += int(np.count_nonzero(~comp))
        checked += 1
    assert checked > 0
    if n >= 12:
        assert dropped > 0


def test_an_inactive_rule_computes_everything():
    n = 8
    L = br.box_of(n)
    k_min, dk = br.edges(n, 0.5, 1.0)
    assert not br.rule_active(n, L, k_min, dk, 4) and np.all(br.computed(n, L, k_min, dk, 4))
    # aliased triangles: shells (0, 0, 3) hold none on an infinite grid (3.5 k_f > 1.5 + 1.5) but do modulo the grid
    count, _ = br.enumerate_direct(n, L, k_min, dk, 4)
    assert count[0, 0, 3] == 0 and count[3, 3, 3] > 0 and count[2, 3, 3] > 0


def test_library_exports_and_bindings():
    from barcode_amd import engine, hamil, io, shim
    raw = C.CDLL(engine.LIB_PATH)
    for name in ("bchmc_bispectrum", "bchmc_bispec_release"):
        assert name in engine.EXPORTS and hasattr(raw, name)
    lib = engine.load()
    assert lib.bchmc_bispectrum.argtypes and C.sizeof(engine.BispecOpts) == 24
    # a NULL handle is refused without touching a device
    assert lib.bchmc_bispectrum(None, 0, None, None, None, None, None, None, None, None) == 1
    assert lib.bchmc_bispec_release(None) == 1
    assert callable(engine.Engine.bispectrum) and callable(engine.Engine.bispec_release)
    assert callable(hamil.measure_bispectrum) and callable(io.dump_bispec)
    assert np.array_equal(engine.bispec_triplets(5), br.triplets(5)) and len(engine.bispec_triplets(32)) == 5984
    slib = shim.load()
    assert "bchmc_shim_measure_bispectrum" in shim.SHIM_EXPORTS and slib.bchmc_shim_measure_bispectrum.argtypes
    probe = C.CDLL(engine.LIB_PATH.replace("libbarcode_hip.so", "libbchmc_fft_probe.so"))
    assert hasattr(probe, "fftp_bispec_triple")


def test_dump_bispec_round_trip(tmp_path):
    from barcode_amd import io
    x, L, got, _ = both((5, 0.5, 1.0, 3))
    path = io.dump_bispec(got, str(tmp_path), "deltaLAG")
    assert path.endswith("deltaLAG_bispec.txt")
    back = io.read_bispec(path)
    assert np.array_equal(back["triplets"], got["triplets"])
    for key in ("b", "ntri", "q"):
        assert np.array_equal(back[key], got[key])
    assert np.array_equal(back["kmean"], got["kmean"][got["triplets"]])
