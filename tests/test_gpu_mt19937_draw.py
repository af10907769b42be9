"""The exact momentum draw: bchmc_chain_draw_momenta_mt19937 writes into the resident chain the momenta that
draw_momenta (HMC_momenta.cc:42-94) makes from a GSL mt19937 state, and returns the state GSL holds afterwards.
Pinned against the oracle's restatement of the reference's draw (oracle/orc_random.c) and against a numpy
restatement of the stream arithmetic (zero-word skip, pairing, accept mask)."""
import numpy as np
import pytest

from tests.util import Case, rel_l2

pytestmark = pytest.mark.gpu

TWO32 = 4294967296.0


def untemper(y):
    """Inverse of MT19937's output tempering, so that a state can be written to produce chosen outputs."""
    y = int(y)
    y ^= y >> 18
    y ^= (y << 15) & 0xefc60000
    x = y
    for _ in range(5):
        x = y ^ ((x << 7) & 0x9d2c5680)
    y = x & 0xFFFFFFFF
    x = y
    for _ in range(3):
        x = y ^ (x >> 11)
    return x & 0xFFFFFFFF


def restate_stream(rng, n_gauss):
    """numpy restatement of n_gauss calls of gsl_ran_ugaussian from a copy of ``rng``: (words used, Gaussians)."""
    r = rng.copy()
    n_words = int(2.6 * n_gauss) + 4096
    while True:
        w = r.copy().raw(n_words).astype(np.float64)
        pos = np.flatnonzero(w)
        u = w[pos] / TWO32
        npair = u.size // 2
        x = -1.0 + 2.0 * u[0:2 * npair:2]
        y = -1.0 + 2.0 * u[1:2 * npair:2]
        r2 = x * x + y * y  # numpy: separately rounded, like a non-FMA GSL build
        ok = ~((r2 > 1.0) | (r2 == 0))
        if np.count_nonzero(ok) >= n_gauss:
            break
        n_words *= 2
    acc = np.flatnonzero(ok)[:n_gauss]
    g = y[acc] * np.sqrt(-2.0 * np.log(r2[acc]) / r2[acc])
    used = int(pos[2 * acc[-1] + 1]) + 1
    return used, g


def garfield(n, L, mass_f, g):
    """create_GARFIELD (random.cpp:48-511, as oracle/orc_random.c states it) from the Gaussians g (2 n^3 of them, in
    draw order), placed by the walk of resolution_independent_random_grid_FS."""
    from barcode_amd.engine import garfield_walk_index
    N = n ** 3
    idx = np.array([garfield_walk_index(n, i, j, k) for i in range(n) for j in range(n) for k in range(n)])
    G = (g[2 * idx] + 1j * g[2 * idx + 1]).reshape(n, n, n)
    out = np.zeros((n, n, n), dtype=complex)
    amp = float(N) * float(N) / (L * L * L)
    P = np.asarray(mass_f).reshape(n, n, n)
    h = n // 2
    for i in range(h + 1):
        for j in range(h + 1):
            for k in range(h + 1):
                sigma = np.sqrt(amp * P[i, j, k] / 2.)
                fr = [a for a, v in enumerate((i, j, k)) if 0 < v < h]
                if not fr:
                    out[i, j, k] = 0 if i == j == k == 0 else G[i, j, k].real * (np.sqrt(2.) * sigma)
                    continue
                for r in range({3: 4, 2: 2, 1: 1}[len(fr)]):
                    a = [i, j, k]
                    if r:
                        ax = fr[r - 1] if len(fr) == 3 else fr[0]
                        a[ax] = n - a[ax]
                    b = tuple((n - t) % n for t in a)
                    v = G[tuple(a)] * sigma
                    out[tuple(a)] = v
                    out[b] = np.conj(v)
    return np.fft.ifftn(out).real.reshape(-1)


def restate_draw(c, rng):
    """draw_momenta from ``rng`` (not advanced): (words used, momenta)."""
    p = c.p
    fs, rs = p.mass_type in (1, 2, 3, 4, 5), p.mass_type in (0, 5, 6, 60)
    N = p.N
    used, g = restate_stream(rng, 2 * N * fs + N * rs)
    mom = garfield(p.Nx, p.L, c.mass_f, g[:2 * N]) if fs else np.zeros(N)
    if rs:
        mom = mom + np.sqrt(np.asarray(c.mass_r).reshape(-1)) * g[2 * N * fs:]
    return used, mom


def check_state(rng_before, used, rng_after):
    """rng_after == rng_before advanced by `used` words: same (mt, mti) and the same next 1000 uniforms."""
    ref = rng_before.copy()
    ref.raw(used)
    m1, i1 = ref.get_state()
    m2, i2 = rng_after.get_state()
    assert i1 == i2 and np.array_equal(m1, m2)
    a, b = ref.copy(), rng_after.copy()
    assert [a.uniform() for _ in range(1000)] == [b.uniform() for _ in range(1000)]


def close(p, pr):
    assert rel_l2(p, pr) < 1e-13
    assert np.max(np.abs(p - pr)) <= 1e-12 * np.max(np.abs(pr))


@pytest.mark.parametrize("n", [8, 16, 32, 64])
@pytest.mark.parametrize("mass_type", [1, 0, 5])
def test_first_draw_equals_the_reference_draw(n, mass_type):
    """A seeded generator's first draw == orc.draw_momenta (the reference's draw restated), and the state after it
    is the serial stream's."""
    from barcode_amd.gsl_mt19937 import GslMT19937
    from oracle import oracle as orc
    c = Case(Nx=n, mass_type=mass_type)
    e = c.engine()
    seed = 1000 + n + mass_type
    rng = GslMT19937(seed)
    before = rng.copy()
    used = e.chain_draw_momenta_mt19937(rng)
    close(e.chain_get_momenta(), orc.draw_momenta(c.p, c.mass_f, c.mass_r, seed))
    used_r, _ = restate_stream(before, (2 * c.p.N if mass_type else 0) + (c.p.N if mass_type in (0, 5) else 0))
    assert used == used_r
    check_state(before, used, rng)
    e.close()


def test_consecutive_draws_and_mid_block_states():
    """Draws from mid-block states (mti != 624, and mti == 0) match the restatement, word count and state exact."""
    from barcode_amd.gsl_mt19937 import GslMT19937
    c = Case(Nx=16, mass_type=5)
    e = c.engine()
    rng = GslMT19937(4242)
    rng.raw(333)
    for _ in range(3):
        before = rng.copy()
        used = e.chain_draw_momenta_mt19937(rng)
        used_r, mom = restate_draw(c, before)
        assert used == used_r
        close(e.chain_get_momenta(), mom)
        check_state(before, used, rng)
        rng.uniform()
    mt, _ = GslMT19937(9).get_state()
    rng.set_state(mt, 0)
    before = rng.copy()
    used = e.chain_draw_momenta_mt19937(rng)
    assert used == restate_draw(c, before)[0]
    check_state(before, used, rng)
    e.close()


# chosen outputs: 3 zero words (the pairing parity shifts), a pair with u = 1/2 twice (r2 == 0: rejected), a pair
# whose separately rounded r2 is exactly 1 (accepted) while a fused x*x + y*y rounds to 1 + 2^-52 (rejected)
CRAFTED = [0, 0, 0, 1 << 31, 1 << 31, (1 << 32) - 25, (1 << 31) + 327680, 0, 12345, 0, 1 << 31, 1 << 31]


@pytest.mark.parametrize("mti,mass_type", [(600, 1), (0, 5), (611, 0)])
def test_rare_paths_from_crafted_states(mti, mass_type):
    """Zero words, r2 == 0 and r2 == 1: word count, state and momenta equal the numpy restatement."""
    from barcode_amd.gsl_mt19937 import GslMT19937
    c = Case(Nx=8, mass_type=mass_type)
    e = c.engine()
    mt, _ = GslMT19937(77).get_state()
    mt = mt.copy()
    for t, v in enumerate(CRAFTED):
        mt[mti + t] = untemper(v)
    rng = GslMT19937()
    rng.set_state(mt, mti)
    assert [int(w) for w in rng.copy().raw(len(CRAFTED))] == CRAFTED
    before = rng.copy()
    used = e.chain_draw_momenta_mt19937(rng)
    used_r, mom = restate_draw(c, before)
    assert used == used_r
    check_state(before, used, rng)
    close(e.chain_get_momenta(), mom)
    e.close()


def test_segment_boundaries_and_continuation_are_invisible(monkeypatch):
    """Segments of one 624-word block (hundreds of boundaries at 32^3) and a pass capacity far below the stream
    (the continuation path) give bitwise the momenta and the state of the default layout."""
    from barcode_amd.gsl_mt19937 import GslMT19937
    c = Case(Nx=32, mass_type=5)
    out = []
    for env in ({}, {"BCHMC_MT_SEGMENT_WORDS": "624"}, {"BCHMC_MT_CAPACITY": "40000"},
                {"BCHMC_MT_SEGMENT_WORDS": "1248", "BCHMC_MT_CAPACITY": "30000"}):
        for k in ("BCHMC_MT_SEGMENT_WORDS", "BCHMC_MT_CAPACITY"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = c.engine()
        rng = GslMT19937(31337)
        rng.raw(101)
        used = e.chain_draw_momenta_mt19937(rng)
        out.append((used, rng.get_state(), e.chain_get_momenta()))
        e.close()
    for used, (mt, mti), p in out[1:]:
        assert used == out[0][0] and mti == out[0][1][1] and np.array_equal(mt, out[0][1][0])
        assert np.array_equal(p, out[0][2])


def test_hamiltonian_mc_with_the_exact_draw_equals_the_host_restatement():
    """HamiltonianMC(momenta="mt19937") == the same loop fed momenta= a host restatement of the draw from the same
    GslMT19937: same Neps, epsilon and accept sequence, dH to 1e-9."""
    from barcode_amd import hamil
    from barcode_amd.gsl_mt19937 import GslMT19937
    c = Case(Nx=16, likelihood=1)
    logs = []
    for exact in (True, False):
        hd = hamil.HamilData(c.p, N_eps_fac=4.0, eps_fac=4 * c.eps, **c.arrays())
        hd.engine.chain_set_state(c.q0)
        rng = GslMT19937(2024)

        def host_draw():
            used, mom = restate_draw(c, rng)
            rng.raw(used)
            return mom

        log = []
        for _ in range(5):
            log += hamil.HamiltonianMC(hd, rng, itmax=50, momenta="mt19937" if exact else host_draw)
        logs.append((log, rng.get_state()))
        hd.engine.close()
    # the C++ shim's entry: the caller's generator state crosses through the mt19937_state_fn hook every attempt
    from barcode_amd.shim import ShimHamil
    hs = ShimHamil(c.p, N_eps_fac=4.0, eps_fac=4 * c.eps, **c.arrays())
    hs.chain_set_state(c.q0)
    rng = GslMT19937(2024)
    log = []
    for _ in range(5):
        log += hs.HamiltonianMC_mt19937(rng, itmax=50)
    hs.close()
    logs.append((log, rng.get_state()))
    (a, sa), (b, sb), (s, ss) = logs
    assert len(a) == len(b) == len(s) and any(r["accepted"] for r in a)
    for ra, rb, rs in zip(a, b, s):
        assert ra["Neps"] == rb["Neps"] == rs["Neps"] and ra["epsilon"] == rb["epsilon"] == rs["epsilon"]
        assert ra["accepted"] == rb["accepted"] == bool(rs["accepted"])
        assert abs(ra["dH"] - rb["dH"]) <= 1e-9 * max(1.0, abs(rb["dH"]))
        assert abs(rs["dH"] - rb["dH"]) <= 1e-9 * max(1.0, abs(rb["dH"]))
    assert sa[1] == sb[1] == ss[1] and np.array_equal(sa[0], sb[0]) and np.array_equal(ss[0], sb[0])


def test_fp32_handle_draws_the_same_stream():
    from barcode_amd.gsl_mt19937 import GslMT19937
    c = Case(Nx=64, mass_type=5)
    res = []
    for precision in (0, 1):
        e = c.engine(precision=precision)
        rng = GslMT19937(555)
        used = e.chain_draw_momenta_mt19937(rng)
        res.append((used, rng.get_state(), e.chain_get_momenta()))
        e.close()
    (u0, s0, p0), (u1, s1, p1) = res
    assert u0 == u1 and s0[1] == s1[1] and np.array_equal(s0[0], s1[0])
    assert rel_l2(p1, p0) < 1e-6


def _big(n, L, precision):
    from barcode_amd import inputs
    from barcode_amd.engine import Engine
    from barcode_amd.params import HamilParams
    p = HamilParams(Nx=n, L=L, likelihood=1, mass_type=1)
    mass_f = inputs.inverse_power_mass(inputs.power_grid(p))
    e = Engine(p, precision=precision)
    e.upload(mass_f=mass_f)
    return p, mass_f, e


def test_256_fp64_draw_equals_the_reference_draw():
    from barcode_amd.gsl_mt19937 import GslMT19937
    from oracle import oracle as orc
    p, mass_f, e = _big(256, 800.0, 0)
    rng = GslMT19937(256)
    e.chain_draw_momenta_mt19937(rng)
    close(e.chain_get_momenta(), orc.draw_momenta(p, mass_f, None, 256))
    e.close()


def test_512_fp32_draw_completes_with_the_expected_statistics():
    from barcode_amd.gsl_mt19937 import GslMT19937
    p, mass_f, e = _big(512, 1600.0, 1)
    rng = GslMT19937(512)
    used = e.chain_draw_momenta_mt19937(rng)
    G = 2 * p.N
    # words per Gaussian: 2 x (pairs per accepted one), geometric with success pi/4: mean 8/pi, variance 4 (1-pi/4)/(pi/4)^2
    mean, var = 8 / np.pi, 4 * (1 - np.pi / 4) / (np.pi / 4) ** 2
    assert abs(used - mean * G) < 6 * np.sqrt(var * G)
    K = e.kinetic_term(e.chain_get_momenta())
    assert abs(K - p.N / 2) < 5 * np.sqrt(p.N / 2)
    e.close()
