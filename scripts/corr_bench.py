"""Cost of the correlation-function measurement on the device: bchmc_measure_corr and
bchmc_measure_corr2d with the tools' automatic bin count at 64^3, 128^3, 256^3 fp64 and 512^3 fp32, for the resident
chain state and for a host array; the first call for a bin count (which builds the geometry) and later calls.  Beside
them what the engine offered for the same result before: chain_get_state plus the vectorised restatement of the tool on
the host (tests/corr_restatement.py), medians of --host-reps.

Timing: host clock around a call that ends in its own synchronise; 3 warm-ups, then the median and quartiles of --reps
calls (the protocol of scripts/mock_bench.py).  A "first" call is made first again by asking for another bin count in
between.  Writes profiles/corr_bench.json.

    python scripts/corr_bench.py [--reps 20] [--sizes 64,128,256,512] [--host-sizes 64,128,256] [--host-reps 5]
    python scripts/corr_bench.py --trace 256     # a few later calls only: the run to put under a kernel trace
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from barcode_amd.engine import BchmcError, Engine, corr_auto_nbin  # noqa: E402
from barcode_amd.params import HamilParams  # noqa: E402
from tests import corr_restatement as cr  # noqa: E402


def timed(fn, reps, warmup=3, before=None):
    ms = []
    for r in range(warmup + reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if r >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    q1, med, q3 = (float(x) for x in np.percentile(ms, [25, 50, 75]))
    return dict(median_ms=med, q1_ms=q1, q3_ms=q3, reps=reps)


def field(n):
    rng = np.random.default_rng(3)
    x = np.arange(n) * (2 * np.pi / n)
    return (rng.standard_normal((n, n, n)) + np.cos(3 * x)[None, None, :]).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="64,128,256,512")
    ap.add_argument("--host-sizes", default="64,128,256")
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_bench.json"))
    a = ap.parse_args()
    if a.trace:
        n = a.trace
        e = Engine(HamilParams(Nx=n, L=200.0 * n / 64), precision=1 if n >= 512 else 0)
        e.chain_set_state(field(n))
        nb = corr_auto_nbin(n, e.params.L)
        for _ in range(6):
            e.measure_corr(None, nb)
            e.measure_corr2d(None, nb)
        e.close()
        return
    host_sizes = [int(s) for s in a.host_sizes.split(",") if s]
    res = []
    for n in (int(s) for s in a.sizes.split(",")):
        precision = 1 if n >= 512 else 0
        L = 200.0 * n / 64
        nb = corr_auto_nbin(n, L)
        row = dict(n=n, dtype="f32" if precision else "f64", n_bin=nb)
        try:
            e = Engine(HamilParams(Nx=n, L=L), precision=precision)
            sig = field(n)
            e.chain_set_state(sig)
            for name, fn in (("corr", e.measure_corr), ("corr2d", e.measure_corr2d)):
                r = {}
                r["chain_later"] = timed(lambda: fn(None, nb), a.reps)
                r["host_later"] = timed(lambda: fn(sig, nb), a.reps)
                r["chain_first"] = timed(lambda: fn(None, nb), max(3, a.reps // 4), warmup=1, before=lambda: fn(None, nb + 1))
                r["host_first"] = timed(lambda: fn(sig, nb), max(3, a.reps // 4), warmup=1, before=lambda: fn(None, nb + 1))
                if n in host_sizes:
                    tool = cr.corr_grid if name == "corr" else cr.corr2d
                    r["host_chain_get_state_plus_restatement"] = timed(lambda: tool(e.chain_get_state(), n, L, nb),
                                                                       a.host_reps, warmup=0)
                row[name] = r
            e.close()
        except BchmcError as err:
            row = dict(n=n, skipped=str(err))
        res.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X, host clock around calls that end in their own synchronise; medians and quartiles",
                       note="n_bin is the tools' automatic count; *_first rebuilds the geometry of the bin count (another "
                            "count is measured in between, outside the clock); the host column is chain_get_state plus "
                            "the numpy restatement of the tool",
                       results=res), f, indent=1)


if __name__ == "__main__":
    main()
