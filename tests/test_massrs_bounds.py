"""The bounds of tests/massrs_bound.py on the CPU: the restated kernels stay inside the counted bounds on every set of
tests/test_gpu_massrs.py (worst fractions printed and held against MEASURED), no cell is excluded and no value stands near an
edge, the checker rejects thirteen wrong kernels, and the oracle's trajectories on the entry-point cases of the GPU test are
well conditioned.  No GPU."""
import functools

import numpy as np
import pytest

from tests import mass_restatement as mr
from tests import massrs_bound as mb
from tests import massrs_reference as ref
from tests.util import Case

DTYPES = (np.float32, np.float64)
IDS = ["float32", "float64"]


def kin_run(count, dtype, mut=None, sum_mut=None, sets=mb.SUM_SETS):
    """The worse of the sum sets (the mutants run on the confined one, which holds every edge)."""
    worst = (0.0, 0)
    for kind in sets:
        p, m = mb.mass_inputs(count, dtype, confined=kind)
        worst = max(worst, mb.check_kin_rs(mb.block_sum64(mb.kin_terms64(p, m, mut), sum_mut), p, m))
    return worst


def loglike_run(count, dtype, mut=None, sum_mut=None, sets=mb.SUM_SETS):
    worst = (0.0, 0)
    for kind in sets:
        a = mb.grf_inputs(count, dtype, confined=kind)
        worst = max(worst, mb.check_grf_loglike(mb.block_sum64(mb.grf_terms64(*a, mut=mut), sum_mut), *a))
    return worst


def div_run(count, dtype, mut=None):
    p, m = mb.mass_inputs(count, dtype)
    return mb.check_div_mass_r(mb.div_mass_r64(p, m, dtype, mut), p, m, dtype)


def grad_run(count, dtype, mut=None):
    a = mb.grf_inputs(count, dtype)
    return mb.check_grf_grad(mb.grf_grad64(*a, dtype, mut), *a, dtype)


def scale_run(count, dtype):
    z, s = mb.scale_inputs(count, dtype)
    return mb.check_scale_c(mb.scale_c64(z, s, dtype), z, s, dtype)


def add_run(count, dtype):
    a, b = mb.add_inputs(count, dtype)
    return mb.check_add_r(mb.add_r64(a, b, dtype), a, b, dtype)


RUNS = {"div_mass_r": (div_run, mb.COUNTS), "grf_grad": (grad_run, mb.COUNTS), "scale_c": (scale_run, mb.COUNTS),
        "add_r": (add_run, mb.COUNTS), "kin_rs": (kin_run, mb.SUM_COUNTS), "grf_loglike": (loglike_run, mb.SUM_COUNTS)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kernel", sorted(RUNS))
def test_restatements_stay_inside_the_counted_bounds(kernel, dtype):
    """Every set, every cell: at most 1 -- the bound has no constant to tune -- and what MEASURED records (not more, and not
    much less: a record three times too large would hide a change)."""
    run, counts = RUNS[kernel]
    ref.near_edge(reset=True)
    worst = (0.0, 0, 0)
    for count in counts:
        f, at = run(count, dtype)
        print("\nMASSRS restated %s<%s> count=%d: worst fraction %.4f at element %d" % (kernel, np.dtype(dtype).name, count, f, at))
        worst = max(worst, (f, count, at))
    rec = mb.MEASURED[kernel][np.dtype(dtype).name][0]
    print("\nMASSRS restated %s<%s>: worst fraction %.4f (recorded %.4f) at count %d, element %d"
          % ((kernel, np.dtype(dtype).name, worst[0], rec) + worst[1:]))
    assert ref.near_edge() == 0, "a set holds a value near an edge of double's or the storage type's range"
    assert worst[0] <= 1.0
    assert worst[0] <= rec and worst[0] >= rec / 1.5


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_sets_stand_on_the_edges(dtype):
    """What the sets promise: every guard value and both extremes in mass_r, every window value, q == nobs, noise = 0, 0 * inf
    and 0 / 0 cells; the reference has exact zeros in every closed cell and the upstream non-finite class elsewhere."""
    fi = np.finfo(dtype)
    for confined in (False, True):
        n = 4096
        p, m = mb.mass_inputs(n, dtype, confined)
        assert all(np.any((m == v) & (np.signbit(m) == np.signbit(dtype(v)))) for v in (0.0, -0.0, -1.0, np.inf, fi.max,
                                                                                          fi.smallest_subnormal))
        assert np.isnan(m).sum() > 50 and np.any(p == 0) and np.any(np.signbit(p) & (p == 0)) and np.any(p < 0)
        assert np.log10(m[m > 0].astype(np.float64).max() / m[m > 0].astype(np.float64).min()) > (500 if dtype is np.float64 else 60)
        closed = ~(m > 0)
        want = ref.div_mass_r(p, m)
        assert 0.08 < closed.mean() < 0.2 and np.all(want[closed] == 0) and np.all(ref.kin_terms(p, m)[closed] == 0)
        on_tiny = (m == fi.smallest_subnormal) & (p == 0)
        assert on_tiny.any() and np.all(np.isnan(want[on_tiny]) == (dtype is np.float64))
        assert np.isinf(ref.as_storage(want, dtype)).any()
        q, nobs, noise, w = mb.grf_inputs(n, dtype, confined)
        assert all(np.any((w == v) & (np.signbit(w) == np.signbit(dtype(v)))) for v in (0.0, -0.0, -1.0, 0.5, 1.0,
                                                                                          fi.smallest_subnormal))
        assert np.isnan(w).any() and np.any(noise == 0) and np.any((q == nobs) & (w > 0)) and np.any(q == 0)
        g, t = ref.grf_grad(q, nobs, noise, w), ref.grf_terms(q, nobs, noise, w)
        shut = ~(w > 0)
        assert 0.3 < shut.mean() < 0.6 and np.all(g[shut] == 0) and np.all(t[shut] == 0)
        zero_over_zero = (q == nobs) & (noise == 0) & (w > 0)
        assert zero_over_zero.any() and np.all(np.isnan(g[zero_over_zero])) and np.all(np.isnan(t[zero_over_zero]))
        assert np.isposinf(g).any() and np.isneginf(g).any() and np.isposinf(t).any()
        assert np.any((g == 0) & (q == nobs) & (w > 0) & (noise > 0))
        if confined:   # three partials in four stay finite and are judged by value (a float mass has no infinite 1 / m)
            for terms, some in ((ref.kin_terms(p, m), dtype is np.float64), (t, True)):
                bad = ~np.isfinite(ref.block_sums(terms))
                assert bad.any() == some and not bad[np.arange(ref.RED_BLOCKS) % 4 != 1].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_moderate_sets_have_finite_totals(dtype):
    """Every term of the "moderate" sum sets is finite at every size, closed cells and masked cells included, so the total
    is judged by value; a total with the sign of one term in a thousand flipped misses its bound."""
    for count in mb.SUM_COUNTS:
        p, m = mb.mass_inputs(count, dtype, "moderate")
        a = mb.grf_inputs(count, dtype, "moderate")
        for terms in (ref.kin_terms(p, m), ref.grf_terms(*a)):
            assert np.all(np.isfinite(terms)) and (count < 255 or (np.any(terms > 0) and np.any(terms == 0)))
    t = mb.kin_terms64(p, m)
    t[3::1000] = -t[3::1000]   # (every fifth cell has p = 0)
    f, at = mb.check_kin_rs(mb.block_sum64(t), p, m)
    assert f > 1.0


def test_ownership_and_turns():
    """Block b owns i = b 256 + t (mod 1024 * 256); the sizes of the GPU test fill a thread 0, 1, 2 and 3 times and leave
    blocks idle."""
    assert ref.owner_block(mb.FULL + 3)[[0, 255, 256, mb.FULL - 1, mb.FULL, mb.FULL + 2]].tolist() == [0, 0, 1, 1023, 0, 0]
    assert ref.trips(257)[:3].tolist() == [1, 1, 0] and ref.trips(256)[:2].tolist() == [1, 0]
    assert ref.trips(mb.FULL + 3)[[0, 1, 1023]].tolist() == [2, 1, 1] and ref.trips(2 * mb.FULL + 3)[[0, 1]].tolist() == [3, 2]
    t = np.arange(mb.FULL + 3, dtype=np.float64)
    s = ref.block_sums(t)
    assert s[0] == t[:256].sum() + t[mb.FULL:].sum() and s[5] == t[5 * 256: 6 * 256].sum()
    assert np.array_equal(mb.block_sum64(t), s.astype(np.float64))   # integers: every order gives the same sum


REJECT = (
    [("div_mass_r", m, lambda dt, m=m: div_run(4096, dt, m)) for m in mb.MASS_MUTANTS]
    + [("kin_rs", m, lambda dt, m=m: kin_run(4096, dt, m)) for m in mb.KIN_MUTANTS]
    + [("grf_grad", m, lambda dt, m=m: grad_run(4096, dt, m)) for m in mb.GRAD_MUTANTS]
    + [("grf_loglike", m, lambda dt, m=m: loglike_run(4096, dt, m)) for m in mb.LOGLIKE_MUTANTS]
    + [(k, "second_trip_dropped", lambda dt, r=r: r(mb.FULL + 3, dt, None, "second_trip_dropped"))
       for k, r in (("kin_rs", kin_run), ("grf_loglike", loglike_run))]
    + [(k, "idle_blocks_unwritten", lambda dt, r=r: r(729, dt, None, "idle_blocks_unwritten"))
       for k, r in (("kin_rs", kin_run), ("grf_loglike", loglike_run))]
)


@pytest.mark.parametrize("kernel,mut,run", REJECT, ids=["%s-%s" % r[:2] for r in REJECT])
def test_checker_rejects(kernel, mut, run):
    for dtype in DTYPES:
        f, at = run(dtype)
        print("\nMASSRS mutant %s of %s<%s>: fraction %.3g at element %d" % (mut, kernel, np.dtype(dtype).name, f, at))
        assert f > 1.0, (kernel, mut, dtype, f)


def test_second_trip_mutant_is_seen_in_the_three_cells_alone():
    """The dropped turn at 1024 * 256 + 3 is wrong in block 0 only, by three cells: the partial of block 0 is what fails."""
    for run in (kin_run, loglike_run):
        f, at = run(mb.FULL + 3, np.float64, None, "second_trip_dropped", sets=("moderate",))
        assert f > 1.0 and at in (0, ref.RED_BLOCKS)


# ---- the entry-point cases of tests/test_gpu_massrs.py: conditioning of the oracle's trajectories ---------------------------
@functools.lru_cache(maxsize=None)
def entry_case(kind, n):
    if kind != "jasche":
        return mb.entry_case(kind, n)
    c = Case(Nx=n, likelihood=1, mass_type=6, window_zero_fraction=0.3, eps_scale=mb.JASCHE_EPS_SCALE)
    c.mass_r = mr.hamiltonian_mass(c.p, c.oracle, c.q0, c.signal_PS, c.window, c.noise)[1]
    c.oracle.set(mass_r=c.mass_r)
    return c


CONDITIONING = [(k, n) for k in ("mass0", "mass5", "grf") for n in mb.ENTRY_N] + [("jasche", 8)]


@pytest.mark.parametrize("kind,n", CONDITIONING, ids=["%s_%d" % kn for kn in CONDITIONING])
def test_oracle_conditioning(kind, n):
    """A 1e-13 perturbation of q0 grows by less than 100 over the ten steps (tests/util.py::Case's criterion), and the run
    stays finite although mass_r holds zeros, negatives and NaN: TOL_TRAJ_10 applies to these cases.  The Jasche case keeps
    Case's step (JASCHE_EPS_SCALE = 0.1 of the heuristic)."""
    c = entry_case(kind, n)
    if kind == "jasche":
        m = np.asarray(c.mass_r).ravel()
        assert np.all(m[c.window.ravel() == 0] == 0) and np.all(m[c.window.ravel() > 0] > 0)
    elif kind != "grf":
        m = np.asarray(c.mass_r).ravel()
        assert 0.15 < (m == 0).mean() < 0.25 and 0.02 < (m < 0).mean() < 0.08 and 0.005 < np.isnan(m).mean() < 0.04
        assert np.array_equal(m.astype(np.float32).astype(np.float64)[~np.isnan(m)], m[~np.isnan(m)])
    q1, p1, done = c.oracle.Hamiltonian_EoM(c.q0, c.p0, c.eps, 10)
    rng = np.random.Generator(np.random.Philox(99))
    dq = 1e-13 * np.linalg.norm(c.q0) / np.sqrt(c.q0.size) * rng.standard_normal(c.q0.shape)
    q1b, p1b, _ = c.oracle.Hamiltonian_EoM(c.q0 + dq, c.p0, c.eps, 10)
    assert done == 10 and np.all(np.isfinite(q1)) and np.all(np.isfinite(p1))
    rel_in = np.linalg.norm(dq) / np.linalg.norm(c.q0)
    gq = np.linalg.norm(q1b - q1) / np.linalg.norm(q1) / rel_in
    gp = np.linalg.norm(p1b - p1) / np.linalg.norm(p1) / rel_in
    print("\nMASSRS conditioning %s n=%d: growth of a 1e-13 perturbation of q0 %.2f in q1, %.2f in p1" % (kind, n, gq, gp))
    assert gq < 100 and gp < 100
