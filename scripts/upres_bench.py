"""Cost of the up-resolved 2-D correlation function on the device: bchmc_measure_corr2d_interp in
both modes (0: CIC interpolation, without a cut; 1: zero padding) and bchmc_interp_upres at 64 -> 128, 128 -> 256 and
256 -> 512 in fp64 and 256 -> 512 in fp32, with the tool's automatic bin count, for the resident chain state and for a
host array; later calls (the fine grid and the bin tables are kept) and first calls (after bchmc_upres_release: buffers,
rocFFT plans and tables are rebuilt).  Beside them what the engine offered for the same numbers before: chain_get_state
plus the vectorised restatement of the tool on the host (tests/upres_restatement.py), medians of --host-reps.

Timing: host clock around a call that ends in its own synchronise; 3 warm-ups, then the median and quartiles of --reps
calls (the protocol of scripts/corr_bench.py).  Writes profiles/upres_bench.json.

    python scripts/upres_bench.py [--reps 20] [--cases 64:128:0,128:256:0,256:512:0,256:512:1] [--host-cases 64:128,128:256]
    python scripts/upres_bench.py --trace 256:512     # a few later calls only: the run to put under a kernel trace
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from barcode_amd.engine import BchmcError, Engine, corr_auto_nbin  # noqa: E402
from barcode_amd.params import HamilParams  # noqa: E402
from tests import upres_restatement as ur  # noqa: E402


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
    ap.add_argument("--cases", default="64:128:0,128:256:0,256:512:0,256:512:1")
    ap.add_argument("--host-cases", default="64:128,128:256")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--trace", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upres_bench.json"))
    a = ap.parse_args()
    if a.trace:
        n, n_out = (int(s) for s in a.trace.split(":"))
        e = Engine(HamilParams(Nx=n, L=200.0 * n / 64))
        e.chain_set_state(field(n))
        nb = corr_auto_nbin(n_out, e.params.L)
        for _ in range(6):
            e.measure_corr2d_interp(n_out, None, nb, 0)
            e.measure_corr2d_interp(n_out, None, nb, 1)
        e.close()
        return
    host_cases = [tuple(int(t) for t in s.split(":")) for s in a.host_cases.split(",") if s]
    res = []
    for n, n_out, precision in (tuple(int(t) for t in s.split(":")) for s in a.cases.split(",")):
        L = 200.0 * n / 64
        nb = corr_auto_nbin(n_out, L)
        row = dict(n=n, n_out=n_out, dtype="f32" if precision else "f64", n_bin=nb)
        try:
            e = Engine(HamilParams(Nx=n, L=L), precision=precision)
            sig = field(n)
            e.chain_set_state(sig)
            first = max(3, a.reps // 6)
            for mode in (0, 1):
                r = {}
                r["chain_later"] = timed(lambda: e.measure_corr2d_interp(n_out, None, nb, mode), a.reps)
                r["host_later"] = timed(lambda: e.measure_corr2d_interp(n_out, sig, nb, mode), a.reps)
                r["chain_first"] = timed(lambda: e.measure_corr2d_interp(n_out, None, nb, mode), first, warmup=1,
                                         before=e.upres_release)
                r["host_first"] = timed(lambda: e.measure_corr2d_interp(n_out, sig, nb, mode), first, warmup=1,
                                        before=e.upres_release)
                if (n, n_out) in host_cases and not precision:
                    tool = ((lambda q: ur.corr2d_interp_cic(q, n, L, n_out, nb, math.inf)) if mode == 0 else
                            (lambda q: ur.corr2d_zeropad(q, n, L, n_out, nb, "literal")))
                    r["host_chain_get_state_plus_restatement"] = timed(lambda: tool(e.chain_get_state()), a.host_reps,
                                                                       warmup=0)
                row["mode%d" % mode] = r
            row["interp_upres_chain"] = timed(lambda: e.interp_upres(n_out), max(3, a.reps // 4), warmup=1)
            e.close()
        except BchmcError as err:
            row = dict(n=n, n_out=n_out, skipped=str(err))
        res.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X, host clock around calls that end in their own synchronise; medians and quartiles",
                       note="n_bin is the tool's automatic count on the fine grid; mode 0 without a cut; *_first follows a "
                            "bchmc_upres_release made outside the clock, so it rebuilds buffers, plans and tables; the host "
                            "column is chain_get_state plus the numpy restatement of the tool; interp_upres includes the "
                            "download of n_out^3 doubles",
                       results=res), f, indent=1)


if __name__ == "__main__":
    main()
