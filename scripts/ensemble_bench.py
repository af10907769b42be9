"""Cost of the ensemble accumulators on the device, at 256^3 on fp64 and fp32 handles:

* one ``ensemble_add`` from each source -- a host field, the resident chain state, the handle's deltaX;
* the path it replaces: ``chain_get_state`` plus the same Welford update in numpy on the host;
* one ``ensemble_merge`` of two host arrays and one ``ensemble_fetch`` of the standard deviation;
* the floor of the update kernel: 40 bytes per cell (8 read from a double source, 16 read and 16 written of mean and
  m2; 36 from a float source) at --hbm-tbs, the copy bandwidth measured on the box class.

Timing: host clock around a call that ends in its own synchronise; 3 warm-ups, then the median and quartiles of --reps
calls (the protocol of scripts/corr_bench.py).  The engine's own event times (bchmc_profile) per kernel class are read as
well: for a host source class "other" is the update kernel alone (the upload is not a kernel), for the chain state it is
the 1 / N scaling plus the update, beside the C2R.  Run it once per build of the streaming hints
(make -C barcode_amd/csrc variant NAME=ensnt0 DEFS=-DBCHMC_NT_ENSEMBLE=0, then BCHMC_LIB=...) for the A/B.  Writes
profiles/ensemble_bench.json (--out).

    python scripts/ensemble_bench.py [--reps 20] [--sizes 256] [--hbm-tbs 6.3]
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


def timed(fn, reps, warmup=3):
    ms = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if r >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    q1, med, q3 = (float(x) for x in np.percentile(ms, [25, 50, 75]))
    return dict(median_ms=med, q1_ms=q1, q3_ms=q3, reps=reps)


def profiled(e, fn, reps):
    """Mean event time per call of every kernel class that ran, over `reps` calls."""
    e.profile(True)
    e.profile_read()
    for _ in range(reps):
        fn()
    out = {k: ms / reps for k, (ms, cnt) in e.profile_read().items() if cnt}
    e.profile(False)
    return out


def field(n):
    rng = np.random.default_rng(3)
    x = np.arange(n) * (2 * np.pi / n)
    return 0.05 * (rng.standard_normal((n, n, n)) + np.cos(3 * x)[None, None, :]).reshape(-1)


class HostWelford:
    """The update the device replaces, on the host in numpy, in place."""

    def __init__(self, size):
        self.count, self.mean, self.m2 = 0, np.zeros(size), np.zeros(size)
        self.d, self.t = np.empty(size), np.empty(size)

    def add(self, x):
        c = float(self.count + 1)
        np.subtract(x, self.mean, out=self.d)
        np.divide(self.d, c, out=self.t)
        self.mean += self.t
        np.subtract(x, self.mean, out=self.t)
        self.t *= self.d
        self.m2 += self.t
        self.count += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="256")
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    a = ap.parse_args()
    res = []
    for n in (int(s) for s in a.sizes.split(",")):
        for precision in (0, 1):
            N = n ** 3
            src_bytes = 4 if precision else 8
            row = dict(n=n, dtype="f32" if precision else "f64", lib=os.environ.get("BCHMC_LIB", ""),
                       floor_ms=dict(host=40. * N / (a.hbm_tbs * 1e9), device=(32. + src_bytes) * N / (a.hbm_tbs * 1e9),
                                     merge=48. * N / (a.hbm_tbs * 1e9)))
            try:
                e = Engine(HamilParams(Nx=n, L=200.0 * n / 64), precision=precision)
                sig = field(n)
                e.chain_set_state(sig)
                e.chain_forward(0)
                r = {}
                for name, call in (("host", lambda: e.ensemble_add(0, sig)), ("chain", lambda: e.ensemble_add(1, source="chain")),
                                   ("deltaX", lambda: e.ensemble_add(2, source="deltaX"))):
                    r[name] = timed(call, a.reps)
                    r[name + "_event_ms"] = profiled(e, call, a.reps)
                cnt, mean, m2 = e.ensemble_export(0)
                r["merge"] = timed(lambda: e.ensemble_merge(3, cnt, mean, m2), a.reps)
                r["merge_event_ms"] = profiled(e, lambda: e.ensemble_merge(3, cnt, mean, m2), a.reps)
                r["fetch_std"] = timed(lambda: e.ensemble_fetch(0, "std"), a.reps)
                w = HostWelford(N)
                reps_host = max(3, a.reps // 4)
                r["host_path_get_state"] = timed(e.chain_get_state, reps_host, warmup=1)
                r["host_path_get_state_plus_numpy"] = timed(lambda: w.add(e.chain_get_state()), reps_host, warmup=1)
                row["ensemble"] = r
                e.close()
            except BchmcError as err:
                row = dict(n=n, dtype=row["dtype"], skipped=str(err))
            res.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X, host clock around calls that end in their own synchronise; medians and quartiles; "
                                "*_event_ms: bchmc_profile's event time per call by kernel class; floor_ms: bytes per cell "
                                "over --hbm-tbs",
                       results=res), f, indent=1)


if __name__ == "__main__":
    main()
