"""Which path a trajectory takes on a handle (barcode_amd/csrc/eval_plan.hpp decides, bchmc.hip launches), seen from
outside: the launch count of each of the nine profile classes after one 3-step bchmc_leapfrog, for the path switches and
configurations that change what is launched.  The parity tests compare one path with another, so a change that silently
stops taking a path passes all of them; these counts do not.

The expected counts are literals.  They were recorded by running this file on the commit before eval_plan.hpp existed
(it uses nothing but the ABI of that commit) and are not derived from the code they now check.  What equal counts cannot
tell apart -- planes mode against the 3-D plans where both launch as often, the one-tile against the two-tile boundary,
the z pass inside the binning against rocFFT's -- is in tests/host/eval_plan_check.cpp's table."""
import dataclasses
import functools

import pytest

from barcode_amd.engine import Engine
from tests.util import Case

pytestmark = pytest.mark.gpu

CLASSES = ("rocfft_c2r", "rocfft_r2c", "k_kick_drift_za", "k_scatter_sph", "k_sum+k_partial_like", "k_gather_sph",
           "k_assemble", "k_bin+k_scan_tiles+k_reorder", "other")
SWITCHES = ("BCHMC_NO_FUSE", "BCHMC_NO_PLANES", "BCHMC_NO_PLANES_ENDS", "BCHMC_NO_ALPT_PLANES")

ZELDOVICH_RSD = dict(likelihood=1, rsd_model=1)
ALPT = dict(likelihood=1, rsd_model=0, sfmodel=2)
# name: (Nx, configuration, mass_type, environment); 32^3 with BCHMC_FFT_PAD=1 has planes mode, 16^3 has not
CASES = {
    "default": (32, ZELDOVICH_RSD, 1, {}),
    "no_fuse": (32, ZELDOVICH_RSD, 1, {"BCHMC_NO_FUSE": "1"}),
    "no_planes": (32, ZELDOVICH_RSD, 1, {"BCHMC_NO_PLANES": "1"}),
    "no_planes_ends": (32, ZELDOVICH_RSD, 1, {"BCHMC_NO_PLANES_ENDS": "1"}),
    "alpt": (32, ALPT, 1, {}),
    "alpt_no_alpt_planes": (32, ALPT, 1, {"BCHMC_NO_ALPT_PLANES": "1"}),
    "mass_with_real_space_part": (32, ZELDOVICH_RSD, 5, {}),
    "n16_default": (16, ZELDOVICH_RSD, 1, {}),
}
# launches per class, in the order of CLASSES
EXPECTED = {
    "default": (6, 6, 2, 4, 4, 4, 4, 4, 3),
    "no_fuse": (6, 6, 4, 4, 4, 4, 4, 4, 2),
    "no_planes": (6, 6, 2, 4, 4, 4, 4, 4, 3),
    "no_planes_ends": (6, 6, 2, 4, 4, 4, 4, 4, 3),
    "alpt": (11, 10, 6, 4, 4, 4, 4, 4, 8),
    "alpt_no_alpt_planes": (15, 14, 11, 4, 4, 4, 4, 4, 7),
    "mass_with_real_space_part": (9, 9, 7, 4, 4, 4, 4, 4, 8),
    "n16_default": (6, 6, 2, 4, 4, 4, 4, 4, 3),
}


@functools.lru_cache(maxsize=None)
def _case(nx, cfg):
    return Case(Nx=nx, **dict(cfg))


def scope_counts(name, setenv, delenv):
    nx, cfg, mass_type, env = CASES[name]
    for k in SWITCHES:
        delenv(k)
    setenv("BCHMC_FFT_PAD", "1")
    for k, v in env.items():
        setenv(k, v)
    c = _case(nx, tuple(sorted(cfg.items())))
    e = Engine(dataclasses.replace(c.p, mass_type=mass_type))
    try:
        e.upload(**c.arrays())
        e.profile(True)
        _, _, done = e.leapfrog(c.q0, c.p0, c.eps, 3)
        prof = e.profile_read()
    finally:
        e.close()
    assert done == 3
    assert tuple(prof) == CLASSES
    return tuple(prof[k][1] for k in CLASSES)


@pytest.mark.parametrize("name", list(CASES))
def test_launches_per_class(monkeypatch, name):
    got = scope_counts(name, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    print("%s: %s" % (name, got))
    assert got == EXPECTED[name]


def test_the_fingerprint_tells_paths_apart():
    """Not vacuous: the counts every case above is held to differ where the path does."""
    assert EXPECTED["default"] != EXPECTED["no_fuse"]
    assert EXPECTED["alpt"] != EXPECTED["alpt_no_alpt_planes"]
