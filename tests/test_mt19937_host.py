"""Host side of the exact momentum draw (no GPU): the MT19937 jump-ahead of bchmc_mt19937_jump, the closed form of
the resolution_independent_random_grid_FS walk (bchmc_garfield_walk_index), and GslMT19937 against the oracle's
restatement of GSL's stream."""
from fractions import Fraction

import numpy as np
import pytest

from barcode_amd import engine
from barcode_amd.gsl_mt19937 import GslMT19937

TWO32 = 4294967296.0


def _start(kind):
    r = GslMT19937(20241016)
    if kind == "mid":
        r.raw(377)
    elif kind == "pos0":
        r.raw(624)  # the block is used up (mti = 624); the same words as mti = 0 after its regeneration
        r.uniform()
        mt, _ = r.get_state()
        r.set_state(mt, 0)
    return r


@pytest.mark.parametrize("kind", ["seeded", "mid", "pos0"])
@pytest.mark.parametrize("steps", [0, 1, 623, 624, 625, 19937, 10 ** 6 + 7, 2 ** 26 + 3])
def test_jump_equals_serial_generation(kind, steps):
    r = _start(kind)
    mt, mti = r.get_state()
    mo, mio = engine.mt19937_jump(mt, mti, steps)
    ref = r.copy()
    if steps:
        ref._bg.random_raw(steps)
    mr, mir = ref.get_state()
    assert mio == mir and np.array_equal(mo, mr)
    j = GslMT19937()
    j.set_state(mo, mio)
    assert np.array_equal(j.raw(1000), ref.raw(1000))


def test_library_exports_the_mt19937_entry_points():
    import ctypes
    import re
    lib = ctypes.CDLL(engine.LIB_PATH)
    text = open(engine.os.path.join(engine.os.path.dirname(engine._HERE), "include", "bchmc.h")).read()
    for sym in engine.EXPORTS_MT19937 + ("bchmc_garfield_walk_index",):
        assert re.search(r"\b%s\s*\(" % sym, text) and hasattr(lib, sym), sym


def test_jump_rejects_an_invalid_state():
    with pytest.raises(engine.BchmcError):
        engine.mt19937_jump(np.zeros(624, dtype=np.uint32), 625, 5)


def _walk_loops(n):
    """random.hpp:64-112 (half_size = false), transcribed: cell -> position in the walk."""
    out = np.full((n, n, n), -1, dtype=np.int64)
    c, m = 0, n - 1
    for i in range(n // 2):
        for k in range(i + 1):
            for j in range(i):
                for cell in ((i, j, k), (m - i, j, k), (i, m - j, k), (m - i, m - j, k), (i, j, m - k),
                             (m - i, j, m - k), (i, m - j, m - k), (m - i, m - j, m - k)):
                    out[cell] = c
                    c += 1
            for j in range(i + 1):
                for cell in ((j, i, k), (m - j, i, k), (j, m - i, k), (m - j, m - i, k), (j, i, m - k),
                             (m - j, i, m - k), (j, m - i, m - k), (m - j, m - i, m - k)):
                    out[cell] = c
                    c += 1
        for j in range(i):
            for k in range(i):
                for cell in ((j, k, i), (m - j, k, i), (j, m - k, i), (m - j, m - k, i), (j, k, m - i),
                             (m - j, k, m - i), (j, m - k, m - i), (m - j, m - k, m - i)):
                    out[cell] = c
                    c += 1
    return out


@pytest.mark.parametrize("n", [2, 4, 8, 16, 32])
def test_walk_index_is_the_reference_walk(n):
    ref = _walk_loops(n)
    got = np.array([engine.garfield_walk_index(n, i, j, k) for i in range(n) for j in range(n) for k in range(n)])
    assert np.array_equal(got, ref.reshape(-1))
    assert np.array_equal(np.sort(got), np.arange(n ** 3))  # a bijection onto [0, n^3)
    with pytest.raises(engine.BchmcError):
        engine.garfield_walk_index(n + 1, 0, 0, 0)


def test_gsl_mt19937_equals_the_oracle_stream():
    from oracle import oracle as orc
    for seed in (0, 1, 5489, 4357, 2 ** 32 - 1):
        r = GslMT19937(seed)
        w = orc.mt19937_stream(seed, 3000)
        assert np.array_equal(r.raw(3000), w)
    assert [int(x) for x in GslMT19937(5489).raw(2)] == [3499211612, 581869302]
    # gsl_rng_uniform, state round trip
    r = GslMT19937(7)
    a = [r.uniform() for _ in range(700)]
    assert a == [x / TWO32 for x in orc.mt19937_stream(7, 700)]
    mt, mti = r.get_state()
    assert mti == 76 and mt.dtype == np.uint32 and mt.size == 624
    s = GslMT19937()
    s.set_state(mt, mti)
    assert s.uniform() == r.uniform()


def test_gsl_mt19937_gaussians_equal_the_oracle():
    """gsl_ran_ugaussian (polar Box-Muller) through a vectorised restatement of GslMT19937 words."""
    from oracle import oracle as orc
    n = 5000
    w = GslMT19937(99).raw(3 * n).astype(np.float64)
    u = w[w != 0] / TWO32
    x, y = -1 + 2 * u[0::2][:u.size // 2], -1 + 2 * u[1::2][:u.size // 2]
    r2 = x * x + y * y
    ok = ~((r2 > 1) | (r2 == 0))
    y, r2 = y[ok][:n], r2[ok][:n]
    g = y * np.sqrt(-2 * np.log(r2) / r2)
    ref = orc.ugaussian_stream(99, n)
    # same words, pairs and decisions; numpy's log may differ from the C library's by an ulp
    assert np.all(np.abs(g - ref) <= 1e-15 * np.maximum(np.abs(ref), 1e-300) + 1e-300)


def test_r2_boundary_words_of_the_device_tests():
    """The crafted pair of tests/test_gpu_mt19937_draw.py: separately rounded r2 == 1 (accepted), fused > 1."""
    x = ((1 << 32) - 25) / TWO32 * 2 - 1
    y = ((1 << 31) + 327680) / TWO32 * 2 - 1
    assert x * x + y * y == 1.0 and float(Fraction(x) ** 2 + Fraction(y * y)) > 1.0
