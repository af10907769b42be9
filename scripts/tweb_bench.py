"""Cost of the T-web classification on the device, at 256^3 on fp64 and fp32 handles:

* one ``tweb_classify`` of the resident chain state and of a host field, with the eigenvalues and the type map fetched,
  and of the chain state with statistics only (what a run that only accumulates the posterior pays, plus the counter pass);
* the engine's own event times (bchmc_profile) per kernel class: the six C2Rs, the R2C of a host field, and class "other"
  = the six component passes, the eigenvalue pass, its reduction and, for the chain state, the 1 / N scaling in front of
  the C2R that recovers the unsmoothed field;
* the eigenvalue pass alone is not a class of its own in the hooks; its time comes from the kernel trace of a second
  run, ``rocprofv3 --kernel-trace --stats -- python scripts/tweb_bench.py --no-host-route`` (k_tweb_eigen's row).
  Here, beside it: the bytes it moves and a device-to-device copy reading and writing that many bytes in total, in the
  same process on the same device;
* the route it replaces: ``chain_get_state`` and tests/tweb_reference.py's numpy (fftn, eigvalsh) on the host, once.

Timing: host clock around a call that ends in its own synchronise; 3 warm-ups, then the median and quartiles of --reps
calls (the protocol of scripts/corr_bench.py).  Writes profiles/tweb_bench.json (--out).

    python scripts/tweb_bench.py [--reps 10] [--sizes 256] [--no-host-route]
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
from scripts.ensemble_bench import field, profiled, timed  # noqa: E402


def eigen_bytes(N, esz, src_bytes, with_lambda):
    """Bytes k_tweb_eigen moves: six tensor loads and the source per cell, the type and, when asked, three doubles."""
    return N * (6 * esz + src_bytes + 1 + (24 if with_lambda else 0))


def copy_ms(nbytes, reps):
    """A device-to-device copy that reads and writes `nbytes` in total (torch, events around each copy)."""
    import torch
    half = nbytes // 2
    a = torch.empty(half, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    a.zero_()
    ms = []
    for r in range(3 + reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        b.copy_(a)
        t1.record()
        t1.synchronize()
        if r >= 3:
            ms.append(t0.elapsed_time(t1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="256")
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tweb_bench.json"))
    a = ap.parse_args()
    res = []
    for n in (int(s) for s in a.sizes.split(",")):
        L = 200.0 * n / 64
        R = 2.0 * L / n
        for precision in (0, 1):
            N = n ** 3
            esz = 4 if precision else 8
            row = dict(n=n, dtype="f32" if precision else "f64", lib=os.environ.get("BCHMC_LIB", ""), smoothing_cells=2.0)
            try:
                e = Engine(HamilParams(Nx=n, L=L), precision=precision)
                sig = field(n)
                e.chain_set_state(sig)
                r = {}
                calls = (("chain", lambda: e.tweb_classify(source="chain", smoothing_scale=R)),
                         ("host", lambda: e.tweb_classify(sig, smoothing_scale=R)),
                         ("chain_stats_only", lambda: e.tweb_classify(source="chain", smoothing_scale=R, want_lambda=False,
                                                                       want_type=False)),
                         ("chain_accumulate", lambda: e.tweb_classify(source="chain", smoothing_scale=R, want_lambda=False,
                                                                       want_type=False, accumulate=True)))
                for name, call in calls:
                    r[name] = timed(call, a.reps)
                    r[name + "_event_ms"] = profiled(e, call, a.reps)
                r["fetch_probability"] = timed(lambda: e.tweb_fetch(1, as_probability=True), a.reps)
                st = e.tweb_classify(source="chain", smoothing_scale=R, want_lambda=False, want_type=False)
                r["type_fractions"] = [float(c) / N for c in st["n_type"]]
                for with_lambda in (True, False):
                    nb = eigen_bytes(N, esz, esz, with_lambda)
                    key = "eigen_with_lambda" if with_lambda else "eigen_stats_only"
                    r[key] = dict(bytes=nb, copy_same_bytes_ms=copy_ms(nb, a.reps))
                if not a.no_host_route:
                    from tests import tweb_reference as tr
                    t0 = time.perf_counter()
                    x = e.chain_get_state().reshape((n,) * 3)
                    t1 = time.perf_counter()
                    t6 = tr.tensor(x, L, R)[0]
                    t2 = time.perf_counter()
                    tr.web_type(tr.eigenvalues(t6.reshape(6, -1)), 0.0)
                    t3 = time.perf_counter()
                    r["host_route_ms"] = dict(get_state=1e3 * (t1 - t0), numpy_tensor=1e3 * (t2 - t1),
                                              numpy_eigvalsh=1e3 * (t3 - t2), total=1e3 * (t3 - t0))
                row["tweb"] = r
                e.close()
            except BchmcError as err:
                row = dict(n=n, dtype=row["dtype"], skipped=str(err))
            res.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X, host clock around calls that end in their own synchronise; medians and quartiles; "
                                "*_event_ms: bchmc_profile's event time per call by kernel class; copy_same_bytes_ms: a "
                                "device-to-device copy reading and writing k_tweb_eigen's byte count in total",
                       results=res), f, indent=1)


if __name__ == "__main__":
    main()
