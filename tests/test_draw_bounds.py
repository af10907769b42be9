"""The bounds of tests/draw_bound.py on the CPU: the constants are what the restated kernels reach (and no more), the
checker rejects twelve plausible wrong draws, and the engine's two Philox counter maps share no counter.  No GPU."""
import functools

import numpy as np
import pytest

from tests import draw_bound as db
from tests import draw_restatement as dr
from tests.util import Case

DTYPES = (np.float32, np.float64)
FILL = -7.25


@functools.lru_cache(maxsize=None)
def masses(n, m):
    """(L, mass_f or None, mass_r or None) of Case(Nx=n, mass_type=m), the entry-point cases of tests/test_gpu_draw.py."""
    c = Case(Nx=n, mass_type=m)
    return c.p.L, (c.mass_f if m in (1, 5) else None), (c.mass_r if m in (0, 5) else None)


def white_run(n, attempt, stream, with_var, dtype, mut=None):
    var = db.white_var(n, dtype) if with_var else None
    buf = np.full(n + 1, FILL, dtype=dtype)
    dr.white_storage(buf, n, db.SEED, attempt, stream, var, dtype, mut)
    ref = dr.white_ref(n, db.SEED, attempt, stream, var)
    if buf[n] != dtype(FILL):  # what the probe's canary sees on the device
        return np.inf, n
    return db.white_fraction(buf[:n], ref, dtype, c=1.0)


def color_run(nh, with_wM, accumulate, dtype, mut=None):
    wk, wM, old = db.color_inputs(nh, dtype)
    wM = wM if with_wM else None
    got = dr.color_storage(wk, wM, old, accumulate, dtype, mut)
    ref, a = dr.color_ref(wk, wM, old, accumulate)
    return db.color_fraction(got, ref, wk, a, old if accumulate else None, dtype, c=1.0)


def draw_run(n, m, dtype, mut=None):
    L, mf, mr = masses(n, m)
    got = dr.draw_storage(n, L, db.DRAW_SEED, db.DRAW_ATTEMPT, mf, mr, dtype, mut)
    return max(db.draw_fractions(got, dr.draw_ref(n, L, db.DRAW_SEED, db.DRAW_ATTEMPT, mf, mr), n, dtype, c=1.0))


def measure(dtype):
    white = max(white_run(n, a, s, v, dtype)[0] for n in db.WHITE_N for a, s, v in db.white_params(n))
    color = max(color_run(nh, w, acc, dtype)[0] for nh in db.COLOR_NH for w in (False, True) for acc in (0, 1))
    draw = max(draw_run(n, m, dtype) for n in db.DRAW_N for m in db.DRAW_MASS_TYPES)
    return dict(white=white, color=color, draw=draw)


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_constants_are_the_measured_ones(dtype):
    """The restatements reach MEASURED on the GPU tests' own sets, not more, and not much less (a figure three times too
    large would be a bound three times too loose); every C is four times its figure."""
    got = measure(dtype)
    name = np.dtype(dtype).name
    for kind, f in got.items():
        rec = db.MEASURED[kind][name]
        print("\nDRAW %s %s: worst fraction at C = 1 %.4f (recorded %.4f)" % (kind, name, f, rec))
        assert f <= rec, (kind, f, rec)
        assert f >= rec / 1.5, (kind, f, rec)
        assert db.C[kind][name] == 4.0 * rec


def test_exact_zeros_and_infinities():
    """var <= 0 and wM <= 0 give exact zeros in the reference; var = +inf gives the infinity of g's sign."""
    for dtype in DTYPES:
        n = 729
        var = db.white_var(n, dtype)
        ref = dr.white_ref(n, db.SEED, 1, 1, var)
        dead = ~(var > 0)
        assert dead.sum() >= 6 and np.all(ref["g"][dead] == 0) and np.all(ref["g"][~dead] != 0)
        assert np.array_equal(np.isinf(ref["g"]), np.isinf(var))
        assert np.isinf(var).any() == (dtype is np.float32)
        wk, wM, old = db.color_inputs(257, dtype)
        for acc in (0, 1):
            ref, a = dr.color_ref(wk, wM, old, acc)
            z = ~(wM > 0)
            assert z.sum() > 50 and np.all(a[z] == 0)
            assert np.all(ref[z] == (old[z].astype(np.clongdouble) if acc else 0))


MUTANT_RUNS = {
    "swap_attempt_stream": lambda dt: white_run(4096, 1, 0, False, dt, "swap_attempt_stream")[0],
    "no_domain": lambda dt: white_run(4096, 0, 0, False, dt, "no_domain")[0],
    "pair_plus_one": lambda dt: white_run(4096, 0, 0, False, dt, "pair_plus_one")[0],
    "swap_u": lambda dt: white_run(4096, 0, 0, False, dt, "swap_u")[0],
    "swap_sincos": lambda dt: white_run(4096, 0, 1, False, dt, "swap_sincos")[0],
    "shift12": lambda dt: white_run(4096, 0, 0, False, dt, "shift12")[0],
    # half a unit of the 53-bit grid: visible where u1 is small, so on the large set
    "no_half": lambda dt: white_run(db.WHITE_N[-1], 0, 0, False, dt, "no_half")[0],
    "var_not_sqrt": lambda dt: white_run(4096, 0, 1, True, dt, "var_not_sqrt")[0],
    "odd_tail": lambda dt: white_run(729, 0, 0, False, dt, "odd_tail")[0],
    "inv_wM_not_sqrt": lambda dt: color_run(257, True, 0, dt, "inv_wM_not_sqrt")[0],
    "no_accumulate": lambda dt: color_run(257, True, 1, dt, "no_accumulate")[0],
    "one_stream": lambda dt: draw_run(8, 5, dt, "one_stream"),
}


@pytest.mark.parametrize("mut", dr.MUTANTS)
def test_checker_rejects(mut):
    """Each wrong draw misses its bound -- at the constants the tests use, four times the measured figure -- in both
    storage types.  One exception: the dropped + 0.5 moves u1 by 2^-54, that is g by 2^-54 / (u1 rad^2) of itself, which a
    float32 store (2^-24 of g) hides unless u1 < 2^-35; a set that holds such a u1 has 2^35 pairs.  float64 sees it on the
    largest set (test_the_largest_set_has_small_u1), and the kernel computes g in double on every handle."""
    for dtype in DTYPES if mut != "no_half" else (np.float64,):
        kind = "color" if mut in ("inv_wM_not_sqrt", "no_accumulate") else "draw" if mut == "one_stream" else "white"
        f = MUTANT_RUNS[mut](dtype) / db.constant(kind, dtype)
        print("\nDRAW mutant %s %s: %.3g of the bound" % (mut, np.dtype(dtype).name, f))
        assert f > 1.0, (mut, dtype, f)


def test_the_largest_set_has_small_u1():
    """Why the no_half mutant runs on the largest set: 2^-54 of u1 shows in g only where u1 is small."""
    u1, _ = dr.uniforms(np.arange((db.WHITE_N[-1] + 1) // 2, dtype=np.uint64), db.SEED, 0, 0)
    assert u1.min() < 2.0 ** -18


def _tuples(words):
    return set(zip(*(w.ravel().tolist() for w in words)))


def counter_sets(mut=None):
    """Both maps of include/bchmc.h enumerated at n = 8: every pair and every cell."""
    n3 = 8 ** 3
    pairs, cells = np.arange((n3 + 1) // 2, dtype=np.uint64), np.arange(n3, dtype=np.uint64)
    mom, poi = set(), set()
    for attempt in (0, 1, 63, 2 ** 32 - 1):
        for s in (dr.FOURIER, dr.REAL):
            mom |= _tuples(dr.counters(pairs, attempt, s, mut))
    n_mom = 4 * 2 * pairs.size
    for stream in (0, 1, 2 ** 31 - 1):
        for j in range(64):
            poi |= _tuples(dr.poisson_counters(cells, j, stream, positions=False))
        for kk in (0, 1, 255):
            poi |= _tuples(dr.poisson_counters(cells, kk, stream, positions=True))
    n_poi = 3 * (64 + 3) * cells.size
    return mom, n_mom, poi, n_poi


def test_counter_maps_are_disjoint():
    """The momentum draw and the Poisson sampler share no Philox counter (so a mock drawn with the chain's seed is
    independent of the momenta), and neither map repeats one within itself."""
    mom, n_mom, poi, n_poi = counter_sets()
    assert len(mom) == n_mom and len(poi) == n_poi
    assert not (mom & poi)
    assert all(c[1] & 0x80000000 for c in mom) and not any(c[1] & 0x80000000 for c in poi)
    # the words above 2^32 that no device test reaches: the domain bit joins the index's high word, the Poisson map has none
    big = np.array([2 ** 32 + 5, 2 ** 62 + 1], dtype=np.uint64)
    c = dr.counters(big, 3, 1)
    assert [int(x) for x in c[0]] == [5, 1] and [int(x) for x in c[1]] == [0x80000001, 0xC0000000]
    assert [int(x) for x in c[2]] == [3, 3] and [int(x) for x in c[3]] == [1, 1]
    p = dr.poisson_counters(big, 3, 1, positions=True)
    assert [int(x) for x in p[1]] == [1, 0x40000000] and [int(x) for x in p[3]] == [3, 3]


def test_without_the_domain_bit_the_maps_meet():
    """What the domain bit is for: without it, pair c of attempt j of the Fourier part is cell c of iteration j of Poisson
    stream 0, and the real-space part meets stream 0's positions."""
    mom, _, poi, _ = counter_sets("no_domain")
    shared = mom & poi
    assert (5, 0, 63, 0) in shared and (5, 0, 1, 1) in shared
    assert len(shared) == 256 * (3 + 2)  # attempts 0, 1, 63 against j; attempts 0, 1 against kk


def test_restatement_uses_the_poisson_samplers_uniform_convention():
    """u53 is shared with the Poisson restatement: one definition of the 53-bit uniform for both consumers."""
    from tests import poisson_restatement as pr
    assert dr.u53 is pr.u53 and dr.philox4x32_10 is pr.philox4x32_10
    hi, lo = np.array([0xFFFFFFFF], dtype=np.uint64), np.array([0xFFFFFFFF], dtype=np.uint64)
    assert dr.u53(hi, lo)[0] == 1.0 and dr.u53(hi * 0, lo * 0)[0] == 2.0 ** -54  # the ends: (2^53 - 1 + 0.5) rounds to 2^53
