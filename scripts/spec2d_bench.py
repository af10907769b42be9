"""Cost of the 2-D power spectrum on the device: bchmc_measure_spectrum2d of the resident chain
state and of a host array with n_bin = 200, the first call for a bin count (which builds the tables and the sums of
|k|) and later calls, beside bchmc_measure_spectrum_src with the same n_bin on the same handle.

Timing: host clock around a call that ends in its own synchronise; 3 warm-ups, then the median and quartiles of --reps
calls (the protocol of scripts/corr_bench.py).  For the later calls from the chain state the engine's own event times
(bchmc_profile) of the kernels are read as well: class "other" holds the two slice/reduce launches and the copy of the
bin sums.  A "first" call is made first again by asking for another bin count in between.  Writes
profiles/spec2d_bench.json (--out).

    python scripts/spec2d_bench.py [--reps 20] [--sizes 128,256] [--n-bin 200]
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


def profiled(e, fn, reps):
    """Mean event time per call of every kernel class that ran, over `reps` calls."""
    e.profile(True)
    e.profile_read()
    for _ in range(reps):
        fn()
    out = {k: ms / reps for k, (ms, cnt) in e.profile_read().items() if cnt}
    e.profile(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--n-bin", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec2d_bench.json"))
    a = ap.parse_args()
    nb = a.n_bin
    res = []
    for n in (int(s) for s in a.sizes.split(",")):
        precision = 1 if n >= 512 else 0
        row = dict(n=n, dtype="f32" if precision else "f64", n_bin=nb, lib=os.environ.get("BCHMC_LIB", ""))
        try:
            e = Engine(HamilParams(Nx=n, L=200.0 * n / 64), precision=precision)
            sig = field(n)
            e.chain_set_state(sig)
            two_d = e.measure_spectrum2d
            r = {}
            r["chain_later"] = timed(lambda: two_d(None, nb), a.reps)
            r["chain_later_event_ms"] = profiled(e, lambda: two_d(None, nb), a.reps)
            r["host_later"] = timed(lambda: two_d(sig, nb), a.reps)
            r["chain_first"] = timed(lambda: two_d(None, nb), max(3, a.reps // 4), warmup=1, before=lambda: two_d(None, nb + 1))
            row["spectrum2d"] = r
            row["spectrum_src"] = dict(chain=timed(lambda: e.measure_spectrum(None, nb, "chain"), a.reps),
                                       host=timed(lambda: e.measure_spectrum(sig, nb, "host"), a.reps))
            e.close()
        except BchmcError as err:
            row = dict(n=n, skipped=str(err))
        res.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X, host clock around calls that end in their own synchronise; medians and quartiles; "
                                "*_event_ms: bchmc_profile's event time per call by kernel class",
                       results=res), f, indent=1)


if __name__ == "__main__":
    main()
