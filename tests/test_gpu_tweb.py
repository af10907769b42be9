"""bchmc_tweb_* on the device: the tensor against the longdouble reference of tests/tweb_reference.py, the eigenvalues
against numpy.linalg.eigvalsh of the device's own tensor, types on the cells the two bounds of tests/tweb_bound.py decide,
counts, masses, the trace identity, known answers, k_tweb_eigen alone on chosen tensors (libbchmc_fft_probe.so), bitwise
repeatability, the posterior counters against a bincount restatement, the contracts of include/bchmc.h and the upper
layers.  Grids: 4 (smallest), 5 and 9 (odd), 8 and 16 (even, more than one workgroup), 32 once, and 96 once (the
grid-stride tail: the kernels' grids are capped at 2048 workgroups)."""
import ctypes as C
import functools
import gc
import os

import numpy as np
import pytest

from barcode_amd import engine as engine_mod
from barcode_amd import hamil, io
from barcode_amd.engine import BchmcError, Engine
from barcode_amd.params import HamilParams
from tests import tweb_bound as tb
from tests import tweb_reference as tr
from tests.test_gpu_ensemble import samples_of
from tests.util import Case

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "barcode_amd", "libbchmc_fft_probe.so")
PREC = pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))
DTYPE = (np.float64, np.float32)
GRIDS = (4, 5, 8, 9, 16)


def engine_of(n, precision=0):
    return Engine(HamilParams(Nx=n, L=tr.box_of(n)), precision=precision)


@functools.lru_cache(maxsize=None)
def reference(n, cells):
    """(field, longdouble tensor, float64 smoothed field) of the host field of (n, cells); shared read-only."""
    x = tr.host_field(n, cells)
    L = tr.box_of(n)
    t = tr.tensor_longdouble(x, L, cells * L / n)
    xs = tr.tensor(x, L, cells * L / n)[1]
    for a in (x, t, xs):
        a.setflags(write=False)
    return x, t, xs


def check(e, res, x, t_ref, xs, lambda_th, dtype, host, tag, ref_float64=False):
    """Every output of one classify against the reference of its source x (n, n, n), at the bounds of tweb_bound.
    ref_float64: t_ref comes from numpy's float64 transforms, which obey the float64 tensor bound themselves
    (tests/test_tweb_bounds.py), so that bound is added to the device's."""
    n = x.shape[0]
    N = n ** 3
    t_ref64 = np.asarray(t_ref, dtype=np.float64)
    b6 = tb.tensor_bound(x, t_ref64, dtype)
    if ref_float64:
        b6 = b6 + tb.tensor_bound(x, t_ref64, np.float64)
    t_dev = np.stack([e.tweb_tensor(c) for c in range(6)])
    err = np.max(np.abs(t_dev.reshape(6, n, n, n).astype(np.longdouble) - t_ref).reshape(6, -1), axis=1).astype(np.float64)
    print("%s: tensor error / bound %s" % (tag, np.array2string(err / b6, precision=3)))
    assert np.all(err <= b6), tag
    # eigenvalues against eigvalsh of the device's own tensor
    lam, typ = res["lambda"], res["type"]
    lam_ref = tr.eigenvalues(t_dev)
    eb = tb.eigen_bound(t_dev)
    worst = float(np.max(np.abs(lam - lam_ref) / np.where(eb > 0, eb, 1)))
    print("%s: eigenvalue error / bound %.3f" % (tag, worst))
    assert np.all(np.abs(lam - lam_ref) <= eb), tag
    assert np.all(lam[0] >= lam[1]) and np.all(lam[1] >= lam[2])
    # types on decided cells, against the reference tensor's
    lam_true = tr.eigenvalues(t_ref64.reshape(6, -1))
    und = tb.undecided(lam_true, lambda_th, tb.eigen_bound(t_ref64.reshape(6, -1)) + tb.tensor_shift(b6))
    n_und = int(np.count_nonzero(und))
    print("%s: %d of %d cells undecided" % (tag, n_und, N))
    assert n_und <= tb.UNDECIDED_CAP * N, tag
    type_ref = tr.web_type(lam_true, lambda_th)
    assert np.array_equal(typ[~und], type_ref[~und]), tag
    assert np.array_equal(typ, tr.web_type(lam, lambda_th))  # the type is the count of the returned eigenvalues
    # counts: exactly the device's own map, and the reference's within the undecided cells
    assert res["n_nonfinite"] == 0
    assert np.array_equal(res["n_type"], np.bincount(typ, minlength=4).astype(np.uint64)), tag
    n_ref = np.bincount(type_ref, minlength=4)
    assert np.all(np.abs(res["n_type"].astype(np.int64) - n_ref) <= n_und), tag
    # masses of the device's own map under the summation bound
    for ty in range(4):
        cells_ty = typ == ty
        want = float(np.sum(1.0 + x.ravel()[cells_ty].astype(np.longdouble)))
        assert abs(res["mass_type"][ty] - want) <= tb.mass_bound(x, cells_ty, dtype, host), (tag, ty)
    # the trace identity
    want = (xs - np.mean(xs)).ravel()
    slack = 3.0 * eb + b6[0] + b6[3] + b6[5] + 1e-13 * float(np.max(np.abs(x)))
    assert np.all(np.abs(lam.sum(axis=0) - want) <= slack), tag
    assert np.all(np.abs(t_dev[0] + t_dev[3] + t_dev[5] - want) <= b6[0] + b6[3] + b6[5] + 1e-13 * float(np.max(np.abs(x)))), tag


# ---- known answers --------------------------------------------------------------------------------------------------------
@PREC
@pytest.mark.parametrize("n", GRIDS)
def test_plane_waves_along_each_axis(n, precision):
    """x = A cos(2 pi m i / n), m = 1 and the Nyquist wave m = n / 2: T_aa = x, the five other components 0 within bound,
    eigenvalues (x, 0, 0) sorted, types 0 and 1 only and equal to the reference's at lambda_th = 0.25 A."""
    A, dt = 1.5, DTYPE[precision]
    e = engine_of(n, precision)
    for m in (1,) + ((n // 2,) if n % 2 == 0 else ()):
        for axis in range(3):
            x = tr.plane_wave(n, (axis,), m, A)
            t_ref = np.zeros((6, n, n, n))
            t_ref[(0, 3, 5)[axis]] = x
            res = e.tweb_classify(x, lambda_th=0.25 * A)
            b6 = tb.tensor_bound(x, t_ref, dt)
            t_dev = np.stack([e.tweb_tensor(c) for c in range(6)]).reshape(6, n, n, n)
            assert np.all(np.max(np.abs(t_dev - t_ref).reshape(6, -1), axis=1) <= b6), (m, axis)
            want = np.sort(np.stack([x, 0 * x, 0 * x]), axis=0)[::-1].reshape(3, -1)
            slack = tb.eigen_bound(t_dev.reshape(6, -1)) + tb.tensor_shift(b6)
            assert np.all(np.abs(res["lambda"] - want) <= slack), (m, axis)
            assert set(np.unique(res["type"])) <= {0, 1}
            assert np.array_equal(res["type"], tr.web_type(want, 0.25 * A)), (m, axis)
    e.close()


@PREC
@pytest.mark.parametrize("n", (8, 9, 16))
def test_wave_along_the_diagonal(n, precision):
    """The wave along (1, 1, 0): T_xy = T_xx = T_yy = x / 2 -- the sign and the indexing of an off-diagonal component --
    and the same eigenvalues (x, 0, 0)."""
    A, dt = 1.5, DTYPE[precision]
    e = engine_of(n, precision)
    x = tr.plane_wave(n, (0, 1), 1, A)
    t_ref = np.stack([x / 2, x / 2, 0 * x, x / 2, 0 * x, 0 * x])
    res = e.tweb_classify(x, lambda_th=0.25 * A)
    b6 = tb.tensor_bound(x, t_ref, dt)
    t_dev = np.stack([e.tweb_tensor(c) for c in range(6)]).reshape(6, n, n, n)
    assert np.all(np.max(np.abs(t_dev - t_ref).reshape(6, -1), axis=1) <= b6)
    want = np.sort(np.stack([x, 0 * x, 0 * x]), axis=0)[::-1].reshape(3, -1)
    assert np.all(np.abs(res["lambda"] - want) <= tb.eigen_bound(t_dev.reshape(6, -1)) + tb.tensor_shift(b6))
    assert np.array_equal(res["type"], tr.web_type(want, 0.25 * A))
    e.close()


@PREC
def test_three_waves_give_all_four_types(precision):
    """x = A (cos 2 pi i / n + cos 2 pi 2 j / n + cos 2 pi 3 k / n) at n = 16: T is the diagonal of the three terms, all
    four types occur and the counts are the reference's exactly."""
    n, A = 16, 1.0
    terms = [tr.plane_wave(n, (0,), 1, A), tr.plane_wave(n, (1,), 2, A), tr.plane_wave(n, (2,), 3, A)]
    want = np.sort(np.stack(terms), axis=0)[::-1].reshape(3, -1)
    types = tr.web_type(want, 0.25 * A)
    e = engine_of(n, precision)
    res = e.tweb_classify(sum(terms), lambda_th=0.25 * A)
    assert set(np.unique(res["type"])) == {0, 1, 2, 3}
    assert np.array_equal(res["type"], types)
    assert np.array_equal(res["n_type"], np.bincount(types, minlength=4).astype(np.uint64))
    e.close()


# ---- random fields, every source ---------------------------------------------------------------------------------------
@PREC
@pytest.mark.parametrize("cells", (0.0, 2.0))
@pytest.mark.parametrize("n", GRIDS)
def test_host_field(n, cells, precision):
    x, t_ref, xs = reference(n, cells)
    e = engine_of(n, precision)
    res = e.tweb_classify(x, smoothing_scale=cells * tr.box_of(n) / n, lambda_th=0.0)
    check(e, res, x, t_ref, xs, 0.0, DTYPE[precision], True, "host %d^3 R = %g cells %s" % (n, cells, DTYPE[precision].__name__))
    e.close()


def test_host_field_128_workgroups():
    """32^3: 128 workgroups in the eigen pass, 128 partial rows in the reduction (two per lane)."""
    n = 32
    x, t_ref, xs = reference(n, 0.0)
    e = engine_of(n, 0)
    res = e.tweb_classify(x)
    check(e, res, x, t_ref, xs, 0.0, np.float64, True, "host 32^3")
    e.close()


def test_host_field_grid_stride_tail():
    """96^3 = 884736 cells against grids capped at 2048 x 256 = 524288 threads: every kernel of the call makes a second,
    partial trip, and 96 is no power of two.  The direct longdouble DFT is out of reach at this size; the reference is
    numpy's float64 transform with its own bound added."""
    n = 96
    x = tr.field(n)
    L = tr.box_of(n)
    t_ref, xs, _ = tr.tensor(x, L, 0.0)
    e = engine_of(n, 0)
    res = e.tweb_classify(x)
    check(e, res, x, t_ref, xs, 0.0, np.float64, True, "host 96^3", ref_float64=True)
    e.close()


@PREC
@pytest.mark.parametrize("n", (9, 16))
def test_chain_state_and_deltax(n, precision):
    """The chain state after chain_set_state, and deltaX after a forward model of it, with R = 0 and R = 2 cells."""
    c = Case(Nx=n, likelihood=1)
    e = c.engine(precision=precision)
    e.chain_set_state(c.q0)
    e.chain_forward(0)
    L = c.p.L
    for src, x in (("chain", c.q0), ("deltaX", e.fetch("deltaX"))):
        x = np.asarray(x, dtype=np.float64).reshape((n,) * 3)
        for cells in (0.0, 2.0):
            R = cells * L / n
            res = e.tweb_classify(source=src, smoothing_scale=R, lambda_th=0.0)
            check(e, res, x, tr.tensor_longdouble(x, L, R), tr.tensor(x, L, R)[1], 0.0, DTYPE[precision], False,
                  "%s %d^3 R = %g cells %s" % (src, n, cells, DTYPE[precision].__name__))
    e.close()


# ---- k_tweb_eigen alone ----------------------------------------------------------------------------------------------------
def probe_eigen(prec, t6, x, lambda_th, want_lam=True):
    lib = C.CDLL(PROBE)
    vp = C.c_void_p
    lib.fftp_tweb_eigen.argtypes = [C.c_int, C.c_longlong, vp, vp, C.c_double, vp, vp, vp]
    t6 = np.ascontiguousarray(t6, dtype=DTYPE[prec])
    M = t6.shape[1]
    lam = np.full((3, M), -7.0)
    typ = np.full(M, 9, dtype=np.uint8)
    res = np.zeros(9, dtype=np.uint64)
    xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    rc = lib.fftp_tweb_eigen(prec, M, t6.ctypes.data, None if xx is None else xx.ctypes.data, float(lambda_th),
                             lam.ctypes.data if want_lam else None, typ.ctypes.data, res.ctypes.data)
    assert rc == 0, rc
    return lam, typ, res[:5].copy(), res[5:].view(np.float64).copy(), t6.astype(np.float64)


@PREC
def test_eigen_probe_on_chosen_tensors(precision):
    """The degenerate set ((lambda, 0, 0) and (lambda, lambda, 0) in general position, lambda I, diagonal tensors; on
    fp64 also scaled by 1e+-100), random tensors and one NaN and one infinite tensor."""
    rng = np.random.Generator(np.random.Philox(21))
    deg, _ = tr.degenerate_set(rng, 80)
    if precision == 1:
        deg = deg[:, : deg.shape[1] // 3]  # float storage cannot hold the scaled ones
    t = np.concatenate([deg, rng.standard_normal((6, 1500))], axis=1)
    bad = (5, t.shape[1] - 1)
    t[2, bad[0]] = np.nan
    t[3, bad[1]] = np.inf
    x = rng.standard_normal(t.shape[1])
    lam, typ, counts, masses, t_used = probe_eigen(precision, t, x, 0.1)
    good = np.ones(t.shape[1], dtype=bool)
    good[list(bad)] = False
    assert np.all(typ[~good] == 255) and np.all(np.isnan(lam[:, ~good])) and counts[4] == 2
    ref = tr.eigenvalues(t_used[:, good])
    eb = tb.eigen_bound(t_used[:, good])
    print("probe %s: worst eigenvalue error / bound %.3f" % (DTYPE[precision].__name__,
                                                               float(np.max(np.abs(lam[:, good] - ref) / eb))))
    assert np.all(np.abs(lam[:, good] - ref) <= eb)
    assert np.array_equal(typ[good], tr.web_type(lam[:, good], 0.1))
    assert np.array_equal(counts[:4], np.bincount(typ[good], minlength=4).astype(np.uint64))
    for ty in range(4):
        sel = good & (typ == ty)
        assert abs(masses[ty] - float(np.sum(1.0 + x[sel]))) <= tb.mass_bound(x, sel, np.float64, True) + 1e-300
    # diagonal tensors come back as their diagonal, bit for bit
    d = rng.standard_normal((3, 300))
    td = np.zeros((6, 300))
    td[0], td[3], td[5] = d
    lam_d, _, _, masses_d, used = probe_eigen(precision, td, None, 0.0)
    assert np.array_equal(lam_d, np.sort(np.stack([used[0], used[3], used[5]]), axis=0)[::-1])
    assert masses_d.sum() == 300.0  # without a source every weight is 1
    # no eigenvalue array: the types are the same
    assert np.array_equal(probe_eigen(precision, t, x, 0.1, want_lam=False)[1], typ)


# ---- repeatability ---------------------------------------------------------------------------------------------------------
def same_result(a, b):
    return (np.array_equal(a["lambda"], b["lambda"]) and np.array_equal(a["type"], b["type"])
            and np.array_equal(a["n_type"], b["n_type"]) and np.array_equal(a["mass_type"].view(np.uint64),
                                                                             b["mass_type"].view(np.uint64)))


@PREC
def test_bitwise_repeatable(precision):
    """Two calls, a call across bchmc_tweb_release and two handles give identical lambda, type and stats, for a host
    field and for the chain state."""
    n = 16
    x = reference(n, 0.0)[0]
    R = 2.0 * tr.box_of(n) / n
    e, f = engine_of(n, precision), engine_of(n, precision)
    e.chain_set_state(x)
    f.chain_set_state(x)
    for kw in (dict(signal=x), dict(source="chain")):
        a = e.tweb_classify(smoothing_scale=R, **kw)
        assert same_result(a, e.tweb_classify(smoothing_scale=R, **kw))
        e.tweb_release()
        assert same_result(a, e.tweb_classify(smoothing_scale=R, **kw))
        assert same_result(a, f.tweb_classify(smoothing_scale=R, **kw))
    e.close()
    f.close()


# ---- the posterior accumulator ---------------------------------------------------------------------------------------------
class Counters:
    """The restatement: a bincount per cell."""

    def __init__(self, N):
        self.cnt = np.zeros((4, N), dtype=np.uint32)
        self.samples = 0

    def add(self, types):
        self.cnt[types, np.arange(types.size)] += 1
        self.samples += 1


def equal_to(e, w, tag=""):
    assert e.tweb_samples() == w.samples, tag
    for ty in range(4):
        assert np.array_equal(e.tweb_fetch(ty), w.cnt[ty]), (tag, ty)
        if w.samples:
            assert np.array_equal(e.tweb_fetch(ty, as_probability=True), w.cnt[ty].astype(np.float64) / float(w.samples)), (tag, ty)


@PREC
@pytest.mark.parametrize("n", (9, 16))
def test_accumulator_after_every_add_and_merge(n, precision):
    """Seven samples: counters and probabilities equal the restatement after every add; 3 + 4 samples on two handles
    merged in either order give the single handle's counters; a merge of nothing is a no-op."""
    s = samples_of(n)
    R = 2.0 * tr.box_of(n) / n
    e, a, b = (engine_of(n, precision) for _ in range(3))
    w = Counters(n ** 3)
    equal_to(e, w, "empty")
    for i, x in enumerate(s):
        res = e.tweb_classify(x, smoothing_scale=R, accumulate=True)
        w.add(res["type"])
        equal_to(e, w, "%d^3 sample %d" % (n, i))
        (a if i < 3 else b).tweb_classify(x, smoothing_scale=R, accumulate=True, want_lambda=False, want_type=False)
    assert np.all(w.cnt.sum(axis=0) == 7) and len(np.unique(w.cnt)) > 2
    na, ca = a.tweb_export()
    nb, cb = b.tweb_export()
    assert (na, nb) == (3, 4)
    a.tweb_merge(nb, cb)
    b.tweb_merge(na, ca)
    b.tweb_merge(0, None)
    for h in (a, b):
        equal_to(h, w, "merged")
    c = engine_of(n, precision)  # into a handle that never classified
    c.tweb_merge(na, ca)
    c.tweb_merge(nb, cb)
    equal_to(c, w, "merged into an empty handle")
    for h in (e, a, b, c):
        h.close()


def test_accumulator_reset_parameters_and_non_finite_sample():
    n = 9
    s = samples_of(n)
    e = engine_of(n)
    w = Counters(n ** 3)
    w.add(e.tweb_classify(s[0], smoothing_scale=1.0, lambda_th=0.1, accumulate=True)["type"])
    for kw in (dict(smoothing_scale=2.0, lambda_th=0.1), dict(smoothing_scale=1.0, lambda_th=0.2)):
        with pytest.raises(BchmcError) as err:
            e.tweb_classify(s[1], accumulate=True, **kw)
        assert err.value.code == STATE and "lambda_th" in str(err.value)
        equal_to(e, w, "after a refused pair")
    e.tweb_classify(s[1], smoothing_scale=2.0, lambda_th=0.2)  # not accumulating: any pair
    bad = np.array(s[2])
    bad[77] = np.nan
    with pytest.raises(BchmcError) as err:
        e.tweb_classify(bad, smoothing_scale=1.0, lambda_th=0.1, accumulate=True)
    assert err.value.code == ARG and "not finite" in str(err.value)
    res = err.value.result
    assert res["n_nonfinite"] == n ** 3 and np.all(res["type"] == 255) and np.all(np.isnan(res["lambda"]))
    equal_to(e, w, "after a non-finite sample")
    e.tweb_reset()
    equal_to(e, Counters(n ** 3), "reset")
    w2 = Counters(n ** 3)
    w2.add(e.tweb_classify(s[1], smoothing_scale=2.0, lambda_th=0.2, accumulate=True)["type"])  # another pair after reset
    equal_to(e, w2, "after reset")
    e.close()


# ---- contracts -----------------------------------------------------------------------------------------------------------
def test_refusals_and_resources():
    gc.collect()
    start = engine_mod.live_resources()
    n = 8
    N = n ** 3
    e = engine_of(n)
    created = engine_mod.live_resources()
    lib, dp = e.lib, C.POINTER(C.c_double)
    x = np.array(reference(n, 0.0)[0]).ravel()
    xp = x.ctypes.data_as(dp)
    out = np.zeros(N)
    op = out.ctypes.data_as(dp)

    def opts(R=0.0, lth=0.0, acc=0):
        return C.byref(engine_mod.TwebOpts(R, lth, acc, 0))

    def refused(rc, code, word):
        assert rc == code and word in lib.bchmc_last_error(e.h).decode(), (rc, lib.bchmc_last_error(e.h))

    refused(lib.bchmc_tweb_classify(e.h, 0, xp, None, None, None, None), ARG, "opts")
    for R in (-1.0, np.nan, np.inf):
        refused(lib.bchmc_tweb_classify(e.h, 0, xp, opts(R=R), None, None, None), ARG, "smoothing_scale")
    for lth in (np.nan, -np.inf):
        refused(lib.bchmc_tweb_classify(e.h, 0, xp, opts(lth=lth), None, None, None), ARG, "lambda_th")
    for acc in (2, -1):
        refused(lib.bchmc_tweb_classify(e.h, 0, xp, opts(acc=acc), None, None, None), ARG, "accumulate")
    refused(lib.bchmc_tweb_classify(e.h, 1, xp, opts(), None, None, None), ARG, "signal")
    refused(lib.bchmc_tweb_classify(e.h, 0, None, opts(), None, None, None), ARG, "signal")
    refused(lib.bchmc_tweb_classify(e.h, 3, None, opts(), None, None, None), ARG, "source")
    refused(lib.bchmc_tweb_classify(e.h, 1, None, opts(), None, None, None), STATE, "chain state")
    refused(lib.bchmc_tweb_classify(e.h, 2, None, opts(), None, None, None), STATE, "forward evaluation")
    for comp in (-1, 6):
        refused(lib.bchmc_tweb_tensor(e.h, comp, op), ARG, "component")
    refused(lib.bchmc_tweb_tensor(e.h, 0, op), STATE, "classify")
    for ty in (-1, 4):
        refused(lib.bchmc_tweb_fetch(e.h, ty, 0, op), ARG, "type")
    refused(lib.bchmc_tweb_fetch(e.h, 0, 1, op), STATE, "samples")
    cb = np.zeros(4 * N, dtype=np.uint32)
    cbp = cb.ctypes.data_as(C.POINTER(C.c_uint32))
    refused(lib.bchmc_tweb_merge(e.h, 1, None), ARG, "counts_b")
    refused(lib.bchmc_tweb_merge(e.h, 2 ** 32, cbp), ARG, "n_b")
    assert engine_mod.live_resources() == created and not out.any()  # nothing was taken or written
    e.tweb_classify(x, want_lambda=False)
    first = engine_mod.live_resources()
    # six real arrays, the type map, the partials and the half-complex array of a host source
    assert first[0] == created[0] + 9 and first[2:] == created[2:]
    e.tweb_classify(x, accumulate=True)
    full = engine_mod.live_resources()
    assert full[0] == first[0] + 2 and full[1] == first[1] + 24 * N + 16 * N  # the eigenvalue staging and the counters
    refused(lib.bchmc_tweb_merge(e.h, 2 ** 32 - 1, cbp), ARG, "n_b")
    e.tweb_reset()
    assert engine_mod.live_resources() == full and e.tweb_samples() == 0
    e.tweb_release()
    assert engine_mod.live_resources() == created
    refused(lib.bchmc_tweb_tensor(e.h, 0, op), STATE, "classify")
    e.chain_set_state(x)
    with_state = engine_mod.live_resources()
    e.tweb_classify(source="chain", want_lambda=False)  # the chain state needs no half-complex array
    assert engine_mod.live_resources()[0] == with_state[0] + 8
    e.close()
    assert engine_mod.live_resources() == start


def test_a_call_leaves_the_chain_as_it_was():
    """A deterministic handle at 16^3: two attempts with classifications of all three sources between them -- one set
    with the proposal pending -- give dH, terms and the proposal bit for bit as a twin that classified nothing."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)

    def run(classify):
        e = Engine(c.p, deterministic=1)
        e.upload(**c.arrays())
        e.chain_set_state(c.q0)
        e.chain_set_momenta(c.p0)
        out = [e.chain_attempt(c.eps, 3)]
        before = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + (e.fetch("deltaX"),)
        if classify:
            for kw in (dict(source="chain"), dict(source="deltaX"), dict(signal=c.truth)):
                e.tweb_classify(smoothing_scale=3.0, accumulate=True, **kw)
        after = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + (e.fetch("deltaX"),)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        out.append(e.chain_get_proposal())
        e.chain_accept(1)
        if classify:
            e.tweb_classify(source="chain", smoothing_scale=3.0, accumulate=True)
            assert e.tweb_samples() == 4 and np.array_equal(e.chain_get_state(), before[2])
        e.chain_set_momenta(0.9 * c.p0)
        out.append(e.chain_attempt(c.eps, 3))
        out.append(e.chain_get_proposal())
        e.close()
        return out

    plain, web = run(False), run(True)
    for k in (0, 2):
        assert plain[k][0] == web[k][0] and np.array_equal(plain[k][1], web[k][1]) and plain[k][2] == web[k][2] == 3
    for k in (1, 3):
        assert all(np.array_equal(x, y) for x, y in zip(plain[k], web[k]))


# ---- upper layers ----------------------------------------------------------------------------------------------------------
def test_hamil_shim_and_io_layers(tmp_path, monkeypatch):
    from barcode_amd.shim import ShimHamil
    monkeypatch.chdir(tmp_path)
    n = 9
    c = Case(Nx=n, likelihood=1)
    e = c.engine()
    e.chain_set_state(c.q0)

    class View:  # what hamil.py's functions read of a HamilData
        engine = e
    R = 2.0 * c.p.L / n
    direct = Engine(c.p)
    w = Counters(n ** 3)
    for x in (c.truth, c.q0):
        got = hamil.tweb_classify(View, x, smoothing_scale=R, lambda_th=0.05, accumulate=True)
        w.add(got["type"])
    assert same_result(got, direct.tweb_classify(c.q0, smoothing_scale=R, lambda_th=0.05))
    assert same_result(hamil.tweb_classify(View, smoothing_scale=R, lambda_th=0.05),
                       e.tweb_classify(source="chain", smoothing_scale=R, lambda_th=0.05))
    for ty, name in enumerate(("void", "sheet", "filament", "knot")):
        assert np.array_equal(hamil.tweb_probability(View, name), w.cnt[ty] / 2.0)
    paths = io.dump_tweb(e, "", "deltaLAG")
    assert paths == ("deltaLAG_pvoid.dat", "deltaLAG_psheet.dat", "deltaLAG_pfilament.dat", "deltaLAG_pknot.dat",
                     "deltaLAG_tweb.txt")
    for ty, path in enumerate(paths[:4]):
        assert np.array_equal(io.read_array(path[:-4], n ** 3), w.cnt[ty] / 2.0)
    line = open(paths[4]).read().split()
    assert int(line[0]) == 2 and float(line[1]) == R and float(line[2]) == 0.05
    direct.close()
    hd = ShimHamil(c.p, **c.arrays())
    lam, typ, nt, mt = hd.tweb_classify(c.q0, R, 0.05, accumulate=True)
    assert np.array_equal(lam, got["lambda"]) and np.array_equal(typ, got["type"])
    assert np.array_equal(nt, got["n_type"]) and np.array_equal(mt, got["mass_type"])
    assert np.array_equal(hd.tweb_probability(1), (got["type"] == 1).astype(np.float64))
    hd.close()
    e.close()
