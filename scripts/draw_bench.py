"""Cost of getting momenta into the resident chain, three ways (DESIGN.md "Exact momentum draw"):

  exact   bchmc_chain_draw_momenta_mt19937: draw_momenta's own numbers from a GSL mt19937 state, on the device
  philox  bchmc_chain_draw_momenta: the counter-based stand-in (same spectrum, other numbers)
  set     bchmc_chain_set_momenta of a host array (how a host-drawn reference field gets in)

Sizes 64^3, 128^3, 256^3 fp64 and 512^3 fp32, mass_type 1 (mass_f = 1/P).  Timing: host clock around each call
after bchmc_sync (the exact draw and set_momenta synchronise themselves; the Philox draw is followed by bchmc_sync),
warm-up first, then `--reps` calls; median, quartiles and range in ms.  The first exact draw on a handle also
pays the one-time host precompute (jump polynomials); it is reported as `first_exact_ms` and, net of a steady
draw, as `precompute_ms`.  Writes profiles/draw_bench.json.

    python scripts/draw_bench.py [--reps 20] [--warmup 3] [--sizes 64,128,256,512]
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
from barcode_amd.engine import Engine  # noqa: E402
from barcode_amd.gsl_mt19937 import GslMT19937  # noqa: E402
from barcode_amd.params import HamilParams  # noqa: E402


def stats(ms):
    ms = np.asarray(ms)
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return dict(min=q[0], p25=q[1], median=q[2], p75=q[3], max=q[4], n=int(ms.size))


def timed(fn, e, reps, warmup):
    for _ in range(warmup):
        fn()
    e.sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        e.sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def bench(n, precision, reps, warmup):
    p = HamilParams(Nx=n, L=200.0 * n / 64, likelihood=1, mass_type=1)
    mass_f = inputs.inverse_power_mass(inputs.power_grid(p))
    e = Engine(p, precision=precision)
    e.upload(mass_f=mass_f)
    rng = GslMT19937(12345)
    t0 = time.perf_counter()
    words = e.chain_draw_momenta_mt19937(rng)
    e.sync()
    first = 1e3 * (time.perf_counter() - t0)
    exact = timed(lambda: e.chain_draw_momenta_mt19937(rng), e, reps, warmup)
    attempt = [0]

    def philox():
        attempt[0] += 1
        e.chain_draw_momenta(7, attempt[0])

    phil = timed(philox, e, reps, warmup)
    host_p = e.chain_get_momenta()
    setm = timed(lambda: e.chain_set_momenta(host_p), e, reps, warmup)
    e.close()
    r = dict(n=n, precision="fp32" if precision else "fp64", words_per_draw=int(words), first_exact_ms=first,
             precompute_ms=first - float(np.median(exact)), exact_ms=stats(exact), philox_ms=stats(phil),
             set_momenta_ms=stats(setm))
    print("%4d^3 %s  exact %.3f ms [%.3f, %.3f]  philox %.3f ms  set_momenta %.3f ms  first exact %.1f ms"
          % (n, r["precision"], r["exact_ms"]["median"], r["exact_ms"]["p25"], r["exact_ms"]["p75"],
             r["philox_ms"]["median"], r["set_momenta_ms"]["median"], first), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="64,128,256,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw_bench.json"))
    a = ap.parse_args()
    res = []
    for n in (int(s) for s in a.sizes.split(",")):
        res.append(bench(n, 1 if n >= 512 else 0, a.reps, a.warmup))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(timing="host clock after bchmc_sync, warm-up %d, %d reps" % (a.warmup, a.reps), results=res),
                  f, indent=1)


if __name__ == "__main__":
    main()
