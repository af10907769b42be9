"""Cost of the RSD multipoles on the device, at 64^3 ... 512^3 on fp64 and fp32 handles, beside
``measure_spectrum2d`` at the same grid and n_bin:

* ``measure_multipoles`` and ``measure_cross_multipoles`` of the resident chain state (no transform: the calls are the
  class sums, the shell sums and the read-back), ``measure_corr_multipoles`` of it (|x^|^2, one C2R, then the same two
  stages on A(r)) and ``measure_spectrum2d`` of it, called in alternation -- one of each per round -- so that clock
  and thermal drift hit all four alike; 3 warm-up rounds (the first builds every table and the geometry), then the median
  and quartiles of --reps rounds, host clock around calls that end in their own synchronise;
* the engine's own event times (bchmc_profile) per kernel class for each call;
* the ratio of the auto call to ``measure_spectrum2d``;
* the route it replaces: ``chain_get_state`` and tests/multipole_reference.py's numpy restatement on the host, once per
  grid up to --host-max.

Writes profiles/multipoles_bench.json (--out) and prints one JSON line per grid and precision.

    python scripts/multipole_bench.py [--reps 9] [--sizes 64,128,256,512] [--n-bin 64] [--host-max 256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from barcode_amd.engine import BchmcError, Engine  # noqa: E402
from barcode_amd.params import HamilParams  # noqa: E402
from scripts.ensemble_bench import field, profiled  # noqa: E402


def quartiles(ms):
    q1, med, q3 = (float(x) for x in np.percentile(ms, [25, 50, 75]))
    return dict(median_ms=med, q1_ms=q1, q3_ms=q3, reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="64,128,256,512")
    ap.add_argument("--n-bin", type=int, default=64)
    ap.add_argument("--host-max", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multipoles_bench.json"))
    a = ap.parse_args()
    nb = a.n_bin
    res = []
    for n in (int(s) for s in a.sizes.split(",")):
        L = 200.0 * n / 64
        for precision in (0, 1):
            row = dict(n=n, n_bin=nb, dtype="f32" if precision else "f64", lib=os.environ.get("BCHMC_LIB", ""))
            try:
                e = Engine(HamilParams(Nx=n, L=L), precision=precision)
                e.chain_set_state(field(n))
                calls = dict(spectrum2d=lambda: e.measure_spectrum2d(None, nb),
                             multipoles=lambda: e.measure_multipoles(n_bin=nb),
                             cross_multipoles=lambda: e.measure_cross_multipoles(n_bin=nb),
                             corr_multipoles=lambda: e.measure_corr_multipoles(n_bin=nb))
                ms = {k: [] for k in calls}
                for r in range(3 + a.reps):
                    for k, fn in calls.items():
                        t0 = time.perf_counter()
                        fn()
                        if r >= 3:
                            ms[k].append(1e3 * (time.perf_counter() - t0))
                for k, fn in calls.items():
                    row[k] = quartiles(ms[k])
                    row[k]["event_ms"] = profiled(e, fn, 3)
                row["ratio_multipoles_to_spectrum2d"] = row["multipoles"]["median_ms"] / row["spectrum2d"]["median_ms"]
                if precision == 0 and n <= a.host_max:
                    from tests import multipole_reference as mr
                    t0 = time.perf_counter()
                    x = e.chain_get_state()
                    t1 = time.perf_counter()
                    mr.power(x, n, L, nb)
                    t2 = time.perf_counter()
                    row["host_route_ms"] = dict(get_state=1e3 * (t1 - t0), numpy_restatement=1e3 * (t2 - t1))
                e.close()
            except BchmcError as err:
                row["skipped"] = str(err)
            print(json.dumps(row), flush=True)
            res.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X, the resident chain state, host clock around calls that end in their own "
                                "synchronise, the four calls in alternation; medians and quartiles; event_ms: "
                                "bchmc_profile's event time per call by kernel class",
                       results=res), f, indent=1)


if __name__ == "__main__":
    main()
