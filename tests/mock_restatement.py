"""numpy restatement of setup_random_test and make_initial_guess (barlib/src/barcoderunner.cc:42-247) on a
``GslMT19937``: the truth field by ``garfield()`` from the stream's Gaussians, its forward model by the oracle's
``Lag2Eul``, the three windows, both data models, and ``gsl_ran_gaussian(r, sigma) = sigma * y * sqrt(-2 log r2 / r2)``
in GSL's product order (numpy rounds every product on its own, like a non-FMA GSL build).

Also the list of cases tests/test_gpu_mock.py runs, with the distance of every case from the three thresholds that are
conditions and not tolerances (``delta_eul > 3``, ``Lambda + g < 0``, ``delta_eul < delta_min``): the CPU test asserts
the margins on this restatement alone, the GPU test then demands exact masks."""
from dataclasses import dataclass

import numpy as np

from barcode_amd import inputs
from barcode_amd.params import HamilParams
from oracle.oracle import Oracle
from tests.test_gpu_mt19937_draw import TWO32, garfield, restate_stream

EDGE = 1e-9   # no cell of a case may lie this close to a threshold (three orders above TOL_FIELD x the O(10) values)


@dataclass
class MockOpts:
    """The scalars of NUMERICAL / OBSERVATIONAL the stage reads; defaults: data/input.par."""
    window_type: int = 1
    data_model: int = 0
    negative_obs: bool = False
    random_test_rsd: bool = False
    sigma_min: float = 1.0
    sigma_fac: float = 0.0


def split_stream(rng, n):
    """The next n accepted polar pairs of ``rng`` (advanced in place): (words used, y, sqrt(-2 log r2 / r2))."""
    if n == 0:
        return 0, np.zeros(0), np.zeros(0)
    n_words = int(2.6 * n) + 4096
    while True:
        w = rng.copy().raw(n_words).astype(np.float64)
        pos = np.flatnonzero(w)
        u = w[pos] / TWO32
        npair = u.size // 2
        x = -1.0 + 2.0 * u[0:2 * npair:2]
        y = -1.0 + 2.0 * u[1:2 * npair:2]
        r2 = x * x + y * y
        ok = ~((r2 > 1.0) | (r2 == 0))
        if np.count_nonzero(ok) >= n:
            break
        n_words *= 2
    acc = np.flatnonzero(ok)[:n]
    used = int(pos[2 * acc[-1] + 1]) + 1
    rng.raw(used)
    return used, y[acc], np.sqrt(-2.0 * np.log(r2[acc]) / r2[acc])


def gsl_ran_gaussian(sigma, y, root):
    return sigma * y * root   # (sigma * y) * root, each product rounded


def unit_stream(rng, n):
    """n calls of gsl_ran_ugaussian, ``rng`` advanced in place: (words used, Gaussians)."""
    used, g = restate_stream(rng, n)
    rng.raw(used)
    return used, g


def window_of(window_type, delta_eul):
    N = delta_eul.size
    if window_type == 1:
        return np.ones(N)
    if window_type == 10:
        w = np.ones(N)
        w[:N // 2] = 0.
        return w
    if window_type == 23:   # upstream's code: ones where delta_eul > 3 (its comment says the opposite)
        return (delta_eul > 3).astype(np.float64)
    raise ValueError("in barcoderunner: window_type = %d is not a valid choice!" % window_type)


def check_opts(p, o):
    """What upstream (and the engine) refuses before it draws."""
    if o.window_type not in (1, 10, 23):
        raise ValueError("in barcoderunner: window_type = %d is not a valid choice!" % o.window_type)
    if o.data_model not in (0, 1):
        raise ValueError("in barcoderunner: data_model = %d is not a valid choice!" % o.data_model)
    if o.data_model == 0 and p.likelihood == 0:
        raise NotImplementedError("Poissonian mock data")
    if o.data_model == 0 and p.likelihood == 2:
        raise ValueError("in barcoderunner: linear data model was chosen (additive error), but incompatible likelihood!")


def observe(p, o, delta_lag, delta_eul, window, y, root):
    """nobs, noise (0 where unwindowed: upstream leaves those cells unwritten), the clamp mask and the margins, from the
    split Gaussians of the windowed cells in cell order (barcoderunner.cc:117-198)."""
    N = delta_eul.size
    idx = np.flatnonzero(window > 0)
    nobs, noise = np.zeros(N), np.zeros(N)
    clamped = np.zeros(N, dtype=bool)
    edges = {}
    if o.window_type == 23:
        edges["window"] = float(np.min(np.abs(delta_eul - 3)))
    if o.data_model == 0:
        Lam = p.rho_c * (1. + delta_eul)
        if p.likelihood == 1:
            sigma = o.sigma_min + o.sigma_fac * Lam[idx]
            v = Lam[idx] + gsl_ran_gaussian(sigma, y, root)
            if not o.negative_obs:
                if v.size:
                    edges["clamp"] = float(np.min(np.abs(v)))
                clamped[idx] = v < 0
                v = np.where(v < 0, 0., v)
        else:
            sigma = o.sigma_min + o.sigma_fac * (delta_lag[idx] * delta_lag[idx])
            v = delta_lag[idx] + gsl_ran_gaussian(sigma, y, root)
        nobs[idx], noise[idx] = v, sigma
    else:
        edges["delta_min"] = float(np.min(np.abs(delta_eul - p.delta_min)))
        Lam = np.log(p.rho_c * (1. + np.maximum(delta_eul, p.delta_min)))
        b = p.rho_c * (1 + p.delta_min)
        nobs[:] = np.log(b * b)
        sigma = np.full(idx.size, o.sigma_fac)
        nobs[idx], noise[idx] = Lam[idx] + gsl_ran_gaussian(sigma, y, root), sigma
    if p.likelihood in (1, 3):
        zero = idx[noise[idx] == 0.]
        if zero.size:
            raise RuntimeError("in barcoderunner(): noise = 0 found! Index %d" % zero[0])
    return nobs, noise, clamped, edges


def setup_random_test(p, signal_PS, rng, o, oracle=None, lag2eul=None, delta_lag=None):
    """setup_random_test from ``rng`` (advanced in place).  ``lag2eul(delta, rsd)`` defaults to the oracle's;
    ``delta_lag``: the truth made elsewhere from the first 2 N Gaussians (the 256^3 case: orc.create_GARFIELD), the
    generator then only skips them.  Returns a dict of the arrays, ``words`` and ``edges``."""
    check_opts(p, o)
    N = p.N
    used1, g = unit_stream(rng, 2 * N)
    if delta_lag is None:
        delta_lag = garfield(p.Nx, p.L, signal_PS, g)
    if lag2eul is None:
        orc = oracle or Oracle(p)
        lag2eul = lambda d, rsd: orc.Lag2Eul(d, rsd=rsd)[0]
    delta_eul = np.asarray(lag2eul(delta_lag, 1 if o.random_test_rsd else 0)).reshape(-1)
    window = window_of(o.window_type, delta_eul)
    used2, y, root = split_stream(rng, int(np.count_nonzero(window > 0)))
    nobs, noise, clamped, edges = observe(p, o, delta_lag, delta_eul, window, y, root)
    return dict(delta_lag=delta_lag, delta_eul=delta_eul, window=window, nobs=nobs, noise=noise, clamped=clamped,
                words=used1 + used2, edges=edges, gaussians=y * root)


def make_initial_guess(p, signal_PS, rng, initial_guess, file_field=None, smoothing_type=1, smoothing_scale=0.,
                       oracle=None):
    """make_initial_guess from ``rng`` (advanced in place): (words used, signal)."""
    N = p.N
    if initial_guess == 0:
        return 0, np.zeros(N)
    if initial_guess == 1:
        return 0, np.array(file_field, dtype=np.float64).reshape(-1)
    if initial_guess in (2, 3):
        used, g = unit_stream(rng, 2 * N)
        sig = garfield(p.Nx, p.L, signal_PS, g)
        if initial_guess == 3:
            if smoothing_type != 1:
                raise ValueError("only the Gaussian kernel is restated")
            sig = (oracle or Oracle(p)).convcomp(sig, smoothing_scale)
        return used, sig
    if initial_guess == 4:
        used, y, root = split_stream(rng, N)
        return used, 0. + gsl_ran_gaussian(1.e-1, y, root)
    raise ValueError("In barcoderunner: invalid choice of initial_guess (%d)!" % initial_guess)


# ---- the cases of tests/test_gpu_mock.py ---------------------------------------------------------------------------
def params(n, sfmodel=1, likelihood=1, **kw):
    return HamilParams(Nx=n, L=200.0 * n / 64.0, sfmodel=sfmodel, likelihood=likelihood, **kw)


def power(p):
    return inputs.power_grid(p)


# (n, seed, HamilParams keywords, MockOpts keywords)
GRID = [(n, seed, dict(sfmodel=sf), dict(random_test_rsd=bool(rsd)))
        for n in (16, 32) for seed in (1, 2, 3) for sf, rsd in ((1, 0), (1, 1), (2, 0))]
VARIANTS = [
    (16, 1, dict(), dict(window_type=10)),
    (16, 1, dict(), dict(window_type=23)),
    (32, 2, dict(), dict(window_type=23, random_test_rsd=True)),
    (16, 2, dict(), dict(negative_obs=True)),
    (16, 1, dict(), dict(sigma_fac=0.3)),
    (32, 3, dict(), dict(sigma_fac=0.3, window_type=10)),
    (16, 3, dict(), dict(sigma_fac=0.3, negative_obs=True)),
    (16, 1, dict(likelihood=3), dict(sigma_fac=0.3)),
    (16, 2, dict(likelihood=3), dict(window_type=23)),
    (16, 1, dict(likelihood=2), dict(data_model=1, sigma_fac=0.1)),
    (32, 2, dict(likelihood=2), dict(data_model=1, sigma_fac=0.1, window_type=23)),
    (16, 1, dict(mk=1, calc_h=1), dict()),
    (32, 2, dict(mk=1, calc_h=1), dict()),
]


def case_id(c):
    n, seed, pk, ok = c
    return "n%d-s%d-%s" % (n, seed, "-".join("%s%s" % (k, v) for k, v in sorted({**pk, **ok}.items())) or "default")


_CACHE = {}


def restate_case(c):
    """(params, signal_PS, MockOpts, restated dict, generator after) of a case; cached per process."""
    from barcode_amd.gsl_mt19937 import GslMT19937
    key = case_id(c)
    if key not in _CACHE:
        n, seed, pk, ok = c
        p = params(n, **pk)
        P = power(p)
        o = MockOpts(**ok)
        rng = GslMT19937(seed)
        r = setup_random_test(p, P, rng, o)
        _CACHE[key] = (p, P, o, r, rng)
    return _CACHE[key]


def assert_margins(r):
    for name, v in r["edges"].items():
        assert v > EDGE, "a cell lies %.3g from the %s threshold: change the seed of this case" % (v, name)


def words_for(rng, n, chunk=1 << 24):
    """Words that n calls of gsl_ran_ugaussian consume from a copy of ``rng``, counted chunk by chunk (the 256^3 case:
    5 x 10^7 Gaussians, whose stream does not fit one numpy pass comfortably)."""
    r = rng.copy()
    base, need, carry = 0, int(n), np.zeros(0)
    while True:
        w = r.raw(chunk).astype(np.float64)
        pos = np.flatnonzero(w)
        vals = np.concatenate([carry, w[pos] / TWO32])
        pos = np.concatenate([np.full(carry.size, -1, dtype=pos.dtype), pos])
        npair = vals.size // 2
        x = -1.0 + 2.0 * vals[0:2 * npair:2]
        y = -1.0 + 2.0 * vals[1:2 * npair:2]
        r2 = x * x + y * y
        ok = ~((r2 > 1.0) | (r2 == 0))
        c = int(np.count_nonzero(ok))
        if c >= need:
            a = np.flatnonzero(ok)[need - 1]
            return base + int(pos[2 * a + 1]) + 1
        need -= c
        carry = vals[-1:] if vals.size % 2 else np.zeros(0)
        base += chunk
