"""Running mean and scatter of small per-sample arrays on the host.

The engine keeps the posterior mean and variance of whole fields on the device (``Engine.ensemble_add``).  The binned
statistics of a sample -- P(k), xi(r), P(k_perp, k_par) from the ``measure_*`` calls -- are a few hundred numbers, so
their mean and scatter over the ensemble are kept here, in numpy, with the same arithmetic in the same operand order:
Welford's update for one more sample, Chan, Golub & LeVeque's pairwise update for another accumulator.  No GPU needed.
"""
import numpy as np


class RunningBins:
    """``add(values)`` per sample; ``mean``, ``variance`` (ddof = 1), ``std``; ``merge(other)`` or
    ``merge_parts(count, mean, m2)`` for another chain's accumulator.  The shape is fixed by the first sample."""

    def __init__(self, shape=None):
        self.count = 0
        self.mean = None if shape is None else np.zeros(shape)
        self.m2 = None if shape is None else np.zeros(shape)

    def _take(self, shape):
        if self.mean is None:
            self.mean, self.m2 = np.zeros(shape), np.zeros(shape)
        elif self.mean.shape != tuple(shape):
            raise ValueError("sample of shape %s into an accumulator of shape %s" % (tuple(shape), self.mean.shape))

    def add(self, values):
        """d = x - mean;  mean = mean + d / c;  m2 = m2 + d * (x - mean), c = count + 1.  A value that is not finite
        makes its element NaN for good."""
        x = np.asarray(values, dtype=np.float64)
        self._take(x.shape)
        c = float(self.count + 1)
        with np.errstate(invalid="ignore", over="ignore"):
            d = x - self.mean
            self.mean = self.mean + d / c
            self.m2 = self.m2 + d * (x - self.mean)
        bad = ~np.isfinite(x)
        self.mean[bad] = np.nan
        self.m2[bad] = np.nan
        self.count += 1
        return self

    def merge_parts(self, count, mean, m2):
        """d = mean_b - mean;  mean = mean + d * w;  m2 = (m2 + m2_b) + (d * d) * c, with w = nb / (na + nb) and
        c = na * nb / (na + nb).  ``count == 0`` is a no-op; into an empty accumulator it is a copy."""
        nb = int(count)
        if nb == 0:
            return self
        mean_b, m2_b = np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64)
        self._take(mean_b.shape)
        if m2_b.shape != mean_b.shape:
            raise ValueError("mean and m2 differ in shape")
        na = self.count
        if na == 0:
            self.mean, self.m2 = mean_b.copy(), m2_b.copy()
        else:
            w = float(nb) / float(na + nb)
            c = float(na) * float(nb) / float(na + nb)
            with np.errstate(invalid="ignore", over="ignore"):
                d = mean_b - self.mean
                self.mean = self.mean + d * w
                self.m2 = (self.m2 + m2_b) + (d * d) * c
        self.count = na + nb
        return self

    def merge(self, other):
        return self.merge_parts(other.count, other.mean, other.m2) if other.count else self

    @property
    def variance(self):
        if self.count < 2:
            raise ValueError("the variance needs two samples, the accumulator holds %d" % self.count)
        return self.m2 / float(self.count - 1)

    @property
    def std(self):
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.variance)
