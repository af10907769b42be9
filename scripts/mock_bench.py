"""Cost of the start of a run on the device: bchmc_setup_random_test (defaults of data/input.par:
window of ones, Gaussian likelihood, Zel'dovich, SPH) and bchmc_make_initial_guess(2), at 64^3, 128^3, 256^3 fp64 and
512^3 fp32 when the device has room, beside what the engine offered for the same job before: inputs.mock_observations
on the host (Philox, from a delta_eul already on the host) plus the three bchmc_upload calls.

Timing: host clock, each call followed by bchmc_sync; 3 warm-ups, then the median and quartiles of --reps calls.  The
generator is re-seeded for every call (same stream every time).  Writes profiles/mock_bench.json.

    python scripts/mock_bench.py [--reps 20] [--sizes 64,128,256,512]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from barcode_amd import inputs  # noqa: E402
from barcode_amd.engine import BchmcError, Engine  # noqa: E402
from barcode_amd.gsl_mt19937 import GslMT19937  # noqa: E402
from barcode_amd.params import HamilParams  # noqa: E402


def timed(fn, sync, reps, warmup=3):
    for _ in range(warmup):
        fn()
        sync()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    q1, med, q3 = (float(x) for x in np.percentile(ms, [25, 50, 75]))
    return dict(median_ms=med, q1_ms=q1, q3_ms=q3, reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="64,128,256,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mock_bench.json"))
    a = ap.parse_args()
    res = []
    for n in (int(s) for s in a.sizes.split(",")):
        precision = 1 if n >= 512 else 0
        p = HamilParams(Nx=n, L=200.0 * n / 64, likelihood=1)
        P = inputs.power_grid(p)
        try:
            e = Engine(p, precision=precision)
            e.upload(signal_PS=P, mass_f=inputs.inverse_power_mass(P))
            row = dict(n=n, dtype="f32" if precision else "f64")
            state = GslMT19937(1).get_state()
            rng = GslMT19937()

            def built():
                rng.set_state(*state)
                e.setup_random_test(rng, deltas=False)

            def guess():
                rng.set_state(*state)
                e.make_initial_guess(rng, 2)

            row["setup_random_test"] = timed(built, e.sync, a.reps)
            row["make_initial_guess_2"] = timed(guess, e.sync, a.reps)
            dX = e.fetch("deltaX").reshape((n,) * 3)

            def host():
                window, noise, nobs = inputs.mock_observations(p, dX)
                e.upload(window=window, noise=noise, nobs=nobs)

            row["host_mock_observations_plus_uploads"] = timed(host, e.sync, max(3, a.reps // 4), warmup=1)
            e.close()
        except BchmcError as err:
            row = dict(n=n, skipped=str(err))
        res.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X, host clock, every call followed by bchmc_sync; medians and quartiles",
                       note="the host column starts from a delta_eul already on the host: it does not include the "
                            "truth field or its forward model, which setup_random_test includes",
                       results=res), f, indent=1)


if __name__ == "__main__":
    main()
