"""GSL's ``gsl_rng_mt19937`` (rng/mt.c) on the host, backed by numpy's MT19937.

The reference draws the momenta, ``Neps``, ``epsilon`` and the Metropolis uniform of every HMC attempt from one
``gsl_rng`` (HMC.cc:449, 260-261, 480).  ``GslMT19937`` is that generator: seeded as ``gsl_rng_set`` seeds it, with
its state in GSL's own form ``(unsigned long mt[624], int mti)`` so that it can be handed to the device draw
(``Engine.chain_draw_momenta_mt19937``) and taken back from it.  numpy's ``MT19937`` with ``_legacy_seeding`` is the
same generator (Matsumoto & Nishimura's 2002 seeding), and its ``state['state']`` ``{'key', 'pos'}`` is GSL's
``(mt, mti)`` under the same convention: the next output is ``temper(key[pos])``, a block is regenerated first when
``pos == 624``.
"""
import numpy as np
from numpy.random import MT19937

_TWO32 = 4294967296.0


class GslMT19937:
    """``gsl_rng`` of type ``gsl_rng_mt19937``; ``uniform()`` / ``__call__`` are ``gsl_rng_uniform``."""

    def __init__(self, seed=0):
        self._bg = MT19937(0)
        self.set(seed)

    def set(self, seed):
        """``gsl_rng_set(r, seed)``: seed 0 means 4357 (rng/mt.c), the seed is taken modulo 2^32."""
        s = int(seed) & 0xFFFFFFFF
        self._bg._legacy_seeding(4357 if s == 0 else s)

    def get(self):
        """``gsl_rng_get``: the next 32-bit output."""
        return int(self._bg.random_raw())

    def raw(self, n):
        """The next ``n`` 32-bit outputs (uint32)."""
        return self._bg.random_raw(int(n)).astype(np.uint32)

    def uniform(self):
        """``gsl_rng_uniform``: word / 2^32, in [0, 1)."""
        return int(self._bg.random_raw()) / _TWO32

    __call__ = uniform

    def uniform_pos(self):
        """``gsl_rng_uniform_pos``: as ``uniform`` but a zero word is redrawn, in (0, 1)."""
        while True:
            w = int(self._bg.random_raw())
            if w:
                return w / _TWO32

    def get_state(self):
        """GSL's state: ``(mt, mti)`` with ``mt`` a copy as uint32[624] and ``0 <= mti <= 624``."""
        st = self._bg.state["state"]
        return np.array(st["key"], dtype=np.uint32), int(st["pos"])

    def set_state(self, mt, mti):
        mt = np.ascontiguousarray(mt, dtype=np.uint32).reshape(-1)
        if mt.size != 624 or not 0 <= int(mti) <= 624:
            raise ValueError("an mt19937 state is 624 words and 0 <= mti <= 624")
        self._bg.state = {"bit_generator": "MT19937", "state": {"key": mt.copy(), "pos": int(mti)}}

    def copy(self):
        other = GslMT19937.__new__(GslMT19937)
        other._bg = MT19937(0)
        other.set_state(*self.get_state())
        return other
