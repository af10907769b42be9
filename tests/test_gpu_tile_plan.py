"""The wiring from the environment through the tile plan (barcode_amd/csrc/tile_plan.hpp) to the handle: engines are
created, nothing is launched, and bchmc_tile_info must report the partition that tests/host/tile_plan_check.cpp works
out by hand for the same grids and switches (fp64, h = d, grid origin 0, mk = 3).  One engine at a time."""
import pytest

from barcode_amd.engine import Engine
from barcode_amd.params import HamilParams

pytestmark = pytest.mark.gpu

SWITCHES = ("BCHMC_SORT_CAP", "BCHMC_SORT_CAP_FIXED", "BCHMC_NO_TILES", "BCHMC_NO_TILES_LOW", "BCHMC_CHUNK")
FIELDS = ("tiled", "one_pass", "cap", "cap_alloc", "watch", "tile_shape", "unrolled81")
# without tiles the handle keeps its defaults: no slots, "watch" set (nothing polls it)
DIRECT = (0, 0, 0, 0, 1, (0, 0, 0), 0)
TABLE = [
    # n, environment, (tiled, one_pass, cap, cap_alloc, watch, tile shape, std81)
    (4, {}, (1, 1, 1024, 1024, 0, (4, 4, 4), 0)),
    (5, {}, DIRECT),
    (12, {}, (1, 1, 1024, 1024, 0, (4, 4, 4), 0)),
    (24, {}, (1, 1, 8192, 8192, 0, (8, 8, 8), 0)),
    (32, {}, (1, 1, 16384, 16384, 0, (8, 8, 16), 1)),
    (32, {"BCHMC_SORT_CAP": "64"}, (1, 1, 64, 16384, 1, (8, 8, 16), 1)),
    (32, {"BCHMC_SORT_CAP": "2048", "BCHMC_SORT_CAP_FIXED": "1"}, (1, 1, 2048, 2048, 0, (8, 8, 16), 1)),
    (32, {"BCHMC_NO_TILES": "1"}, DIRECT),
    (32, {"BCHMC_CHUNK": "64"}, (1, 1, 16384, 16384, 0, (8, 8, 16), 1)),
]


@pytest.mark.parametrize("n, env, expect", TABLE, ids=["%d-%s" % (n, "+".join(sorted(env)) or "default")
                                                       for n, env, _ in TABLE])
def test_tile_info_is_the_plan_worked_out_by_hand(n, env, expect, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = Engine(HamilParams(Nx=n, L=200.0 * n / 64.0), device=0, precision=0)
    try:
        info = e.tile_info()
    finally:
        e.close()
    print("n = %d %s: %s" % (n, env, info))
    assert tuple(info[k] for k in FIELDS) == expect, info
