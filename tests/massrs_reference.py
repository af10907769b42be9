"""Longdouble reference of the generic trajectory's real-space mass and GRF kernels (k_div_mass_r, k_kin_rs, k_grf_grad,
k_grf_loglike, k_scale_c, k_add_r of barcode_amd/csrc/kspace_force.hpp), written from the upstream lines and not from the
kernels:

  the mass term of a drift      HMC.cc:317-327        invM = 0 unless mass_r > 0, then 1 / mass_r;  dummy += momenta invM
  kinetic_term, real-space part HMC.cc:88-110         dummy += invM momenta (the same guard);  value += 0.5 momenta dummy
  grf_likelihood_grad_log_like  gaussian_random_field.cpp:25-37   (delta - nobs) / (noise noise) where window > 0, else 0
  grf_likelihood_log_like       gaussian_random_field.cpp:39-52   sum over window > 0 of 0.5 ((delta - nobs) / noise)^2

Inputs are arrays of the handle's storage type and are taken exactly; every value is numpy longdouble (64-bit mantissa).

Upstream computes in double (real_prec).  The reference does not round to double, but it keeps double's RANGE at every
upstream operation (`as_double`): a longdouble intermediate beyond the largest double is the infinity upstream gets there,
one below half the smallest subnormal is its zero.  That is what makes 0 * (1 / 5e-324) a NaN and x / (1e-170)^2 an
infinity, as upstream has them, and where the upstream formula is not finite the expected value is that non-finite class
(tests/like_bound.py::worst_fraction judges classes).  A stored output gets the storage type's range the same way
(`as_storage`).  An intermediate within a factor 1 +- 2^-40 of one of these edges could be classed either way by a correct
double evaluation; `near_edge` counts them, and tests/test_massrs_bounds.py asserts that the sets hold none.
"""
import numpy as np

LD = np.longdouble
RED_BLOCKS, RED_THREADS = 1024, 256          # k_kin_rs / k_grf_loglike: kRedBlocks workgroups of 256 threads

_OVER = {np.dtype(np.float64): LD(2.0) ** 1024 * (1 - LD(2.0) ** -54),    # rounds to infinity from here on
         np.dtype(np.float32): LD(2.0) ** 128 * (1 - LD(2.0) ** -25)}
_ZERO = {np.dtype(np.float64): LD(2.0) ** -1075, np.dtype(np.float32): LD(2.0) ** -150}   # rounds to zero up to here
_EDGE = LD(2.0) ** -40
_near = [0]


def near_edge(reset=False):
    """Number of intermediates since the last reset that lay within 2^-40 (relative) of a range edge."""
    n = _near[0]
    if reset:
        _near[0] = 0
    return n


def _range(x, dtype, flush):
    over, zero = _OVER[np.dtype(dtype)], _ZERO[np.dtype(dtype)]
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(x)
        _near[0] += int(np.count_nonzero(np.abs(a - over) <= _EDGE * over))
        x = np.where(a >= over, np.copysign(LD(np.inf), x), x)
        if flush:
            _near[0] += int(np.count_nonzero(np.abs(a - zero) <= _EDGE * zero))
            x = np.where((a <= zero) & (a > 0), np.copysign(LD(0), x), x)
    return x


def as_double(x):
    """A longdouble value as upstream's double holds it, up to rounding: overflow to +-inf, underflow to +-0."""
    return _range(x, np.float64, True)


def as_storage(x, dtype):
    """The class a value takes when stored as `dtype`: +-inf beyond its largest finite value (an underflow moves the value
    by less than a subnormal, which the bounds carry)."""
    return _range(x, dtype, False)


def ld(a):
    return np.ascontiguousarray(a).ravel().astype(LD)


def inv_mass(mass_r):
    """invM of HMC.cc:94-95 and :323-324: 0 unless mass_r > 0 (a NaN is not > 0)."""
    m = ld(mass_r)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        on = m > 0
        return np.where(on, as_double(LD(1) / np.where(on, m, LD(1))), LD(0))


def div_mass_r(p, mass_r):
    """momenta invM of HMC.cc:325 (dummy is zero before it on this path), in double's range."""
    with np.errstate(invalid="ignore", over="ignore"):
        return as_double(ld(p) * inv_mass(mass_r))


def kin_terms(p, mass_r):
    """The term of every cell in kinetic_term's sum: 0.5 momenta (invM momenta), HMC.cc:97 and :109."""
    p = ld(p)
    with np.errstate(invalid="ignore", over="ignore"):
        return as_double(LD(0.5) * p * as_double(inv_mass(mass_r) * p))


def grf_grad(q, nobs, noise, window):
    """gaussian_random_field.cpp:33-36."""
    q, nobs, noise, w = ld(q), ld(nobs), ld(noise), ld(window)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(w > 0, as_double(as_double(q - nobs) / as_double(noise * noise)), LD(0))


def grf_terms(q, nobs, noise, window):
    """The term of every cell in grf_likelihood_log_like's sum, gaussian_random_field.cpp:48-49."""
    q, nobs, noise, w = ld(q), ld(nobs), ld(noise), ld(window)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = as_double(as_double(q - nobs) / noise)
        return np.where(w > 0, as_double(LD(0.5) * as_double(t * t)), LD(0))


def scale_c(z, s):
    """z s per component (the generic path's 1 / N of an unnormalised transform); returns (real, imag)."""
    z = np.ascontiguousarray(z).ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        return as_double(z.real.astype(LD) * LD(s)), as_double(z.imag.astype(LD) * LD(s))


def add_r(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return ld(a) + ld(b)


def owner_block(count):
    """The workgroup that sums cell i: thread t of block b takes i = b 256 + t (mod 1024 * 256)."""
    return (np.arange(count, dtype=np.int64) // RED_THREADS) % RED_BLOCKS


def trips(count):
    """Per block: the largest number of cells one of its threads sums (the turns of the grid-stride loop that reach it)."""
    first = np.arange(RED_BLOCKS, dtype=np.int64) * RED_THREADS
    return np.maximum(0, -(-(count - first) // (RED_BLOCKS * RED_THREADS)))


def block_sums(terms):
    """Longdouble sum, per block, of exactly the cells the block owns (NaN and infinities propagate as in any sum);
    a block without cells has 0."""
    terms = np.asarray(terms, dtype=LD).ravel()
    full = RED_BLOCKS * RED_THREADS
    pad = np.zeros(-(-terms.size // full) * full, dtype=LD)
    pad[:terms.size] = terms
    with np.errstate(invalid="ignore", over="ignore"):
        return pad.reshape(-1, RED_BLOCKS, RED_THREADS).sum(axis=(0, 2))
