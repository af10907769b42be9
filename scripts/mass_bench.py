"""Cost of Hamiltonian_mass on the device (bchmc_hamiltonian_mass), fp64, from the resident chain
state, Gaussian likelihood, Zel'dovich, SPH / calc_h 2:

  types 1, 2, 3 at 64^3 and 256^3, next to one bchmc_gradient of a host array (the likelihood force types 2 and 3
  evaluate once, plus its transfers);
  type 6 (the Jasche diagonal) at 32^3 and 64^3, and at 128^3 when the 64^3 time x 64 predicts under 60 s.

Timing: host clock around each call (both synchronise), warm-up first; the median of --reps calls (one call for type
6 beyond 32^3).  For type 6 the per-kernel-class split of bchmc_profile_read is kept too (the mass kernels are in the
"other" class; their launch count is the number of cell slices + the fixed passes).  Writes profiles/mass_bench.json.

    python scripts/mass_bench.py [--reps 5] [--sizes 64,256] [--jasche-sizes 32,64,128]
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
from barcode_amd.params import HamilParams  # noqa: E402


def setup(n, mass_type):
    p = HamilParams(Nx=n, L=200.0 * n / 64, likelihood=1, mass_type=mass_type)
    f = inputs.make_fields(p)
    dX = np.zeros((n,) * 3)
    window, noise, nobs = inputs.mock_observations(p, dX)
    e = Engine(p)
    e.upload(signal_PS=f["signal_PS"], mass_f=f["mass_f"], mass_r=np.ones(p.N), window=window, noise=noise, nobs=nobs)
    e.chain_set_state(f["q0"])
    return e, f["q0"]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--jasche-sizes", default="32,64,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mass_bench.json"))
    a = ap.parse_args()
    res = []
    for n in (int(s) for s in a.sizes.split(",")):
        for t in (1, 2, 3):
            e, q = setup(n, t)
            med, ms = timed(lambda: e.hamiltonian_mass(None), a.reps, 1)
            g_med, _ = timed(lambda: e.gradient(q), a.reps, 1)
            e.close()
            res.append(dict(n=n, mass_type=t, build_ms=med, build_ms_all=ms, gradient_ms=g_med))
            print("%4d^3 type %d  build %.2f ms  (one bchmc_gradient %.2f ms)" % (n, t, med, g_med), flush=True)
    last = None
    for n in (int(s) for s in a.jasche_sizes.split(",")):
        if last is not None and last[1] * (n / last[0]) ** 6 > 60e3:
            print("%4d^3 type 6 skipped: predicted %.0f s" % (n, last[1] * (n / last[0]) ** 6 / 1e3), flush=True)
            res.append(dict(n=n, mass_type=6, skipped="predicted over 60 s"))
            continue
        e, q = setup(n, 6)
        reps = a.reps if n <= 32 else 1
        e.profile(True)
        med, ms = timed(lambda: e.hamiltonian_mass(None), reps, 1 if n <= 32 else 0)
        prof = e.profile_read()
        e.close()
        last = (n, med)
        res.append(dict(n=n, mass_type=6, build_ms=med, build_ms_all=ms,
                        kernel_classes={k: dict(ms=v[0], launches=v[1]) for k, v in prof.items() if v[1]}))
        print("%4d^3 type 6  build %.1f ms" % (n, med), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X, fp64, host clock around each synchronising call", results=res), f, indent=1)


if __name__ == "__main__":
    main()
