"""Cost of reading grid fields at a free particle catalogue on the device: bchmc_interp_particles on
an fp64 handle at 256^3, N_part = 2^16, 2^20 and 2^24, one field (deltaX) and three (Psi x, y, z), CIC and TSC, a uniform
catalogue and a clustered one (the handle's own particles after a forward model, a random subset of them below 2^24), the
direct kernel (path 0) against the tile kernel (path 1).  The rule for path = -1 (barcode_amd/csrc/interp_plan.hpp) is read
from these figures.

Per case: the host clock around the whole call and the engine's own event time (bchmc_profile) of the same calls, split
into the staging of the sources (fetch of the handle's fields into the feature's own arrays), the binning (count, scan,
fill; nothing on path 0), and the gather; what the host clock holds beyond the events is the transfers (columns in,
results out, through the pinned staging) and the host's part in them.  Warm-ups, then the median and quartiles of --reps
calls.  Beside them, up to --host-max particles, the route that existed before: bchmc_fetch of the fields plus the numpy
restatement of the interpolator (tests/interp_restatement.py), one repetition, with a bitwise comparison of the results.
Writes profiles/interp_bench.json (--out).

    python scripts/interp_bench.py [--reps 7] [--n 256] [--host-max 1048576]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from barcode_amd.engine import Engine  # noqa: E402
from barcode_amd.params import HamilParams  # noqa: E402

def stats(ms):
    q1, med, q3 = (float(x) for x in np.percentile(ms, [25, 50, 75]))
    return dict(median_ms=med, q1_ms=q1, q3_ms=q3, reps=len(ms))


# the engine's profile classes that a call books its binning and its gather under (BCHMC_K_SORT, BCHMC_K_GATHER)
BINNING, GATHER = "k_bin+k_scan_tiles+k_reorder", "k_gather_sph"


def split(prof):
    """Event time of one call by what it was spent on; prof is a whole profile_read(), every class present."""
    missing = {BINNING, GATHER} - set(prof)
    if missing:  # a renamed class would otherwise land in "staging" without a word
        raise KeyError("the engine's profile has no class %s" % ", ".join(sorted(missing)))
    out = dict(staging=0.0, binning=0.0, gather=0.0)
    for name, (ms, cnt) in prof.items():
        if cnt:
            out["binning" if name == BINNING else "gather" if name == GATHER else "staging"] += ms
    return out


def measure(e, pos, fields, kernel, path, reps, warmup=2):
    e.profile(True)
    host, parts = [], dict(staging=[], binning=[], gather=[])
    for r in range(warmup + reps):
        e.profile_read()
        t0 = time.perf_counter()
        vals, st = e.interp_particles(pos[0], pos[1], pos[2], fields, kernel=kernel, path=path)
        dt = 1e3 * (time.perf_counter() - t0)
        prof = split(e.profile_read())
        if r >= warmup:
            host.append(dt)
            for k, ms in prof.items():
                parts[k].append(ms)
    e.profile(False)
    ev = {k: float(np.median(v)) for k, v in parts.items()}
    row = dict(host_clock=stats(host), events_median_ms=ev, n_in=st["n_in"], n_lost=st["n_lost"],
               max_per_tile=st["max_per_tile"], path_used=st["path_used"])
    row["events_total_ms"] = sum(ev.values())
    row["transfers_and_host_ms"] = row["host_clock"]["median_ms"] - row["events_total_ms"]
    row["binning_plus_gather_ns_per_particle"] = 1e6 * (ev["binning"] + ev["gather"]) / pos.shape[1]
    return row, vals


def host_route(e, p, pos, fields, kernel):
    """What a user did before: fetch the fields, loop (here: numpy) on the host."""
    from tests import interp_restatement as ir
    t0 = time.perf_counter()
    arrays = [e.fetch("deltaX" if f == "deltax" else f) for f in fields]
    t1 = time.perf_counter()
    vals, _ = ir.interpolate(ir.KERNELS[kernel], p.Nx, p.L, pos[0], pos[1], pos[2], arrays)
    return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1), vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20, 1 << 24])
    ap.add_argument("--host-max", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_bench.json"))
    a = ap.parse_args()
    n = a.n
    p = HamilParams(Nx=n, L=200.0 * n / 64)
    rng = np.random.default_rng(7)
    e = Engine(p)
    e.forward(rng.standard_normal(p.N) * 1.5, 0)  # a displacement field strong enough to cluster the particles
    own = np.stack([e.fetch(k) for k in ("posx", "posy", "posz")])
    tiles = e.tile_info()
    res = []
    for n_part in a.sizes:
        cats = (("uniform", rng.random((3, n_part)) * p.L),
                ("clustered", own if n_part >= p.N else own[:, rng.choice(p.N, n_part, replace=False)]))
        for name, pos in cats:
            pos = np.ascontiguousarray(pos)
            for fields in (["deltax"], ["psix", "psiy", "psiz"]):
                for kernel in ("cic", "tsc"):
                    rows = {}
                    for path in (0, 1):
                        row = dict(n=n, dtype="f64", catalogue=name, n_part=int(pos.shape[1]), kernel=kernel,
                                   n_fields=len(fields), path=path, tile_shape=tiles["tile_shape"])
                        m, vals = measure(e, pos, fields, kernel, path, a.reps)
                        row.update(m)
                        rows[path] = (row, vals)
                    same = bool(np.array_equal(rows[0][1].view(np.uint64), rows[1][1].view(np.uint64)))
                    for path in (0, 1):
                        rows[path][0]["paths_agree_bitwise"] = same
                    d0, d1 = (sum(rows[k][0]["events_median_ms"][c] for c in ("binning", "gather")) for k in (0, 1))
                    rows[1][0]["tile_over_direct_binning_plus_gather"] = d1 / d0
                    if pos.shape[1] <= a.host_max:
                        fetch_ms, numpy_ms, host_vals = host_route(e, p, pos, fields, kernel)
                        hb = host_vals.view(np.uint64).copy()
                        hb[np.isnan(host_vals)] = np.uint64(0x7ff8000000000000)
                        for path in (0, 1):
                            rows[path][0].update(host_route_fetch_ms=fetch_ms, host_route_numpy_ms=numpy_ms,
                                                 host_route_agrees_bitwise=bool(np.array_equal(hb, rows[path][1].view(np.uint64))))
                    for path in (0, 1):
                        res.append(rows[path][0])
                        print(json.dumps(rows[path][0]), flush=True)
    e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X; host_clock: around the whole call; events_median_ms: bchmc_profile's event time of the "
                                "same calls by purpose; transfers_and_host_ms: the rest of the host clock; medians and "
                                "quartiles after 2 warm-ups; host_route: bchmc_fetch of the fields plus the numpy "
                                "restatement, one repetition", results=res), f, indent=1)


if __name__ == "__main__":
    main()
