"""The Philox momentum draw value by value: k_white_noise and k_color_momenta run alone through libbchmc_fft_probe.so (the
engine's kernels on chain_draw's launches: barcode_amd/csrc/fft_probe.hip), and bchmc_chain_draw_momenta itself, each
compared element by element with the longdouble restatement of tests/draw_restatement.py under the bounds of
tests/draw_bound.py.  tests/test_draw_bounds.py measures the constants and shows on the CPU that the checker rejects the
plausible bugs (a counter word in the wrong slot, the pair index off by one, the odd tail, a 52-bit uniform, sine for
cosine, one stream for both parts, a wrong power of the mass).

Sizes.  k_white_noise: 1, 2, 3 (one pair, the odd tail alone), 729 and 4096 (several blocks, odd and even), and
2 * 2048 * 256 + 3, where nblk_stride's cap of 2048 blocks makes the first threads take a second stride iteration and the
last pair is half a pair.  k_color_momenta: 1, 257, 2048 * 256 + 5 for the same reasons.  The entry point: 8^3, 9^3, 16^3 with
a Fourier-space mass, a real-space mass and both, on fp64 and fp32 handles.

Every value is compared; nothing is excluded (the draw decides only var > 0 and wM > 0, on exact inputs).  Values that must
be exactly zero (var <= 0, wM <= 0) have a zero bound.  Output arrays go in filled with a pattern, and the probe's canaries
stand behind every device array.  Every check prints a line `DRAW ...` with its worst fraction of the bound, then asserts
<= 1.

Not pinned on the device: pair indices >= 2^32 (the i_hi counter word), which no array that fits a test of seconds reaches.
The restatement and the disjointness test of tests/test_draw_bounds.py cover that word on the CPU.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import draw_bound as db
from tests import draw_restatement as dr
from tests.util import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "barcode_amd", "libbchmc_fft_probe.so")
PRECS = ["fp64", "fp32"]
FILL = -7.25
BCHMC_ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the process-wide HIP runtime first, as barcode_amd.engine does)
    assert os.path.exists(PROBE), "%s not built (make -C barcode_amd/csrc)" % PROBE
    L = C.CDLL(PROBE)
    vp, i, u, ll = C.c_void_p, C.c_int, C.c_uint, C.c_longlong
    L.fftp_white_noise.argtypes = [i, ll, u, u, u, u, vp, vp]
    L.fftp_color_momenta.argtypes = [i, ll, vp, vp, vp, i]
    yield L
    white_reference.cache_clear()
    draw_case.cache_clear()


def ptr(a):
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


def check_status(st):
    if st == -2:   # nothing more runs on a device that has reported an error
        pytest.exit("HIP error in a probe call", returncode=3)
    assert st == 0, {-1: "arguments outside the probe's range"}.get(st, "canary after device array %d overwritten" % st)


def storage(prec):
    return np.dtype(np.float64 if prec == "fp64" else np.float32)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- k_white_noise ------------------------------------------------------------------------------------------------------
def run_white(lib, prec, n, attempt, stream, var, seed=db.SEED):
    out = np.full(n, FILL, storage(prec))
    check_status(lib.fftp_white_noise(PRECS.index(prec), n, seed & 0xFFFFFFFF, seed >> 32, attempt, stream, ptr(var), ptr(out)))
    return out


@functools.lru_cache(maxsize=4)
def white_reference(n, attempt, stream, with_var, prec):
    """The reference is the same for both precisions without var; with var it is that precision's var array."""
    var = db.white_var(n, storage(prec)) if with_var else None
    return var, dr.white_ref(n, db.SEED, attempt, stream, var)


@pytest.mark.parametrize("prec", PRECS)   # the precisions of one size follow each other: they share references
@pytest.mark.parametrize("n", db.WHITE_N)
def test_k_white_noise(lib, prec, n):
    dt = storage(prec)
    for attempt, stream, with_var in db.white_params(n):
        var, ref = white_reference(n, attempt, stream, with_var, prec if with_var else "fp64")
        got = run_white(lib, prec, n, attempt, stream, var)
        f, at = db.white_fraction(got, ref, dt)
        print("\nDRAW k_white_noise<%s> n=%d attempt=%d stream=%d var=%s: worst fraction of the bound %.3f at value %d"
              % (prec, n, attempt, stream, "array" if with_var else "null", f, at))
        assert f <= 1.0
        if with_var:
            dead = ~(var > 0)
            assert np.all(got[dead] == 0), "var <= 0 must give exactly 0"
            assert np.array_equal(np.isinf(got), np.isinf(var))


@pytest.mark.parametrize("prec", PRECS)
def test_white_noise_streams_differ_and_odd_tail_is_a_prefix(lib, prec):
    """Stream 0 and stream 1 differ in every value, and so do two attempts; the first n - 1 values of an odd n are those of
    n + 1 bit for bit, at a one-block size and across the second stride iteration."""
    for n in (729, db.WHITE_N[-1]):
        a = run_white(lib, prec, n, 1, 0, None)
        b = run_white(lib, prec, n, 1, 1, None)
        c = run_white(lib, prec, n, 2, 0, None)
        assert np.all(a != b) and np.all(a != c) and np.all(b != c)
        assert same_bits(a, run_white(lib, prec, n, 1, 0, None))
        even = run_white(lib, prec, n + 1, 1, 0, None)
        assert same_bits(a[: n - 1], even[: n - 1]) and same_bits(a[n - 1:], even[n - 1: n])
    # the key's two words are separate: swapping them, or dropping the high one, changes every value
    a = run_white(lib, prec, 729, 0, 0, None)
    lo, hi = db.SEED & 0xFFFFFFFF, db.SEED >> 32
    assert np.all(a != run_white(lib, prec, 729, 0, 0, None, seed=(lo << 32) | hi))
    assert np.all(a != run_white(lib, prec, 729, 0, 0, None, seed=lo))


# ---- k_color_momenta ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh", db.COLOR_NH)
@pytest.mark.parametrize("prec", PRECS)
def test_k_color_momenta(lib, prec, nh):
    dt = storage(prec)
    wk, wM_set, old = db.color_inputs(nh, dt)
    for with_wM in (False, True):
        wM = wM_set if with_wM else None
        for accumulate in (0, 1):
            pk = old.copy()
            check_status(lib.fftp_color_momenta(PRECS.index(prec), nh, ptr(wk), ptr(wM), ptr(pk), accumulate))
            ref, a = dr.color_ref(wk, wM, old, accumulate)
            f, at = db.color_fraction(pk, ref, wk, a, old if accumulate else None, dt)
            print("\nDRAW k_color_momenta<%s> nh=%d wM=%s accumulate=%d: worst fraction of the bound %.3f at element %d"
                  % (prec, nh, "array" if with_wM else "null", accumulate, f, at))
            assert f <= 1.0
            if with_wM:
                z = ~(wM > 0)
                assert same_bits(pk[z], old[z]) if accumulate else np.all(pk[z] == 0), "wM <= 0 must add exactly nothing"


# ---- bchmc_chain_draw_momenta -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def draw_case(n, m):
    c = Case(Nx=n, mass_type=m)
    mf, mr = (c.mass_f if m in (1, 5) else None), (c.mass_r if m in (0, 5) else None)
    return c, dr.draw_ref(n, c.p.L, db.DRAW_SEED, db.DRAW_ATTEMPT, mf, mr)


def device_draw(c, prec, seed=db.DRAW_SEED, attempt=db.DRAW_ATTEMPT):
    e = c.engine(precision=PRECS.index(prec))
    try:
        e.chain_draw_momenta(seed, attempt)
        return e.chain_get_momenta()
    finally:
        e.close()


@pytest.mark.parametrize("n", db.DRAW_N)
@pytest.mark.parametrize("prec", PRECS)
def test_chain_draw_momenta_every_value(prec, n):
    """Fourier only (mass_type 1), real-space only (0) and both (5): every momentum against the reference under the
    whole-draw bound, and the mixed draw is the sum of the two others (same seed and attempt, the masses are the same
    arrays) within twice the bound."""
    dt = storage(prec)
    got = {}
    for m in db.DRAW_MASS_TYPES:
        c, ref = draw_case(n, m)
        got[m] = device_draw(c, prec)
        fmax, f2 = db.draw_fractions(got[m], ref, n, dt)
        print("\nDRAW chain_draw_momenta<%s> n=%d mass_type=%d: max error %.3f, l2 error %.3f of the bound" % (prec, n, m, fmax, f2))
        assert fmax <= 1.0 and f2 <= 1.0
    ref5 = draw_case(n, 5)[1]
    assert np.array_equal(ref5["pf"], draw_case(n, 1)[1]["p"]) and np.array_equal(ref5["pr"], draw_case(n, 0)[1]["p"])
    both = got[1].astype(np.longdouble) + got[0].astype(np.longdouble)
    fmax, f2 = db.draw_fractions(got[5], (both, ref5["S"]), n, dt, scale=2.0)
    print("\nDRAW chain_draw_momenta<%s> n=%d: mixed against the sum of its parts, max %.3f, l2 %.3f of twice the bound"
          % (prec, n, fmax, f2))
    assert fmax <= 1.0 and f2 <= 1.0


@pytest.mark.parametrize("prec", PRECS)
def test_attempt_is_one_counter_word(prec):
    """attempt 2^32 - 1 is accepted and is its own draw; 2^32 is BCHMC_ERR_ARG with a message and leaves the resident
    momenta as they were (it used to wrap onto attempt 0)."""
    from barcode_amd.engine import BchmcError
    n, m = 8, 5
    c, _ = draw_case(n, m)
    e = c.engine(precision=PRECS.index(prec))
    try:
        e.chain_draw_momenta(db.DRAW_SEED, 2 ** 32 - 1)
        last = e.chain_get_momenta()
        ref = dr.draw_ref(n, c.p.L, db.DRAW_SEED, 2 ** 32 - 1, c.mass_f, c.mass_r)
        fmax, f2 = db.draw_fractions(last, ref, n, storage(prec))
        print("\nDRAW chain_draw_momenta<%s> attempt 2^32 - 1: max error %.3f, l2 error %.3f of the bound" % (prec, fmax, f2))
        assert fmax <= 1.0 and f2 <= 1.0
        for attempt in (2 ** 32, 2 ** 32 + 7, 2 ** 64 - 1):
            with pytest.raises(BchmcError) as err:
                e.chain_draw_momenta(db.DRAW_SEED, attempt)
            assert err.value.code == BCHMC_ERR_ARG and "attempt" in str(err.value)
            assert same_bits(last, e.chain_get_momenta())
        e.chain_draw_momenta(db.DRAW_SEED, 0)
        assert np.all(e.chain_get_momenta() != last)
    finally:
        e.close()
