"""Cost of the bispectrum on the device, at 256^3 on fp64 and fp32 handles, for n_shell = 8,
16 and 32 shells from 0.5 k_f up to 2/3 k_Nyquist (B4's rule active):

* one ``bispectrum`` of the resident chain state: the first call, which builds the table of triangle counts (n_shell
  indicator filter + C2R passes and a contraction of its own), and later calls (median and quartiles);
* the engine's own event times (bchmc_profile) per kernel class: the n_shell C2Rs, and class "other" = the shell
  statistics, the n_shell filter passes, the contraction and the two reductions;
* the contraction alone (k_bispec_triple + k_bispec_reduce) on random arrays of the same size through
  libbchmc_fft_probe.so, event time, with the rows cut as the engine cuts them, against its two floors: the bytes it must
  read (n_shell N esz) at the rate of a device-to-device copy in the same process, and 2 T_computed N flop at the
  78.6 TFLOP/s fp64 vector peak;
* the route it replaces: ``chain_get_state`` and tests/bispec_reference.py's numpy restatement on the host, once, for
  n_shell = 8 (its cost is linear in n_shell for the transforms and in T for the sums).

Timing: host clock around a call that ends in its own synchronise; 3 warm-ups, then the median and quartiles of --reps
calls (the protocol of scripts/corr_bench.py).  Writes profiles/bispec_bench.json (--out).

    python scripts/bispec_bench.py [--reps 5] [--sizes 256] [--shells 8,16,32] [--no-host-route] [--no-probe]
"""
import argparse
import ctypes as C
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
from scripts.tweb_bench import copy_ms  # noqa: E402

PEAK_FP64 = 78.6e12  # README.md: the fp64 vector peak of one MI355X
PROBE = os.path.join(ROOT, "barcode_amd", "libbchmc_fft_probe.so")


def row_ends(n, L, k_min, dk, ns):
    """s3_end of bchmc_bispectrum (B4): (32, 32) uint8, and the number of computed triplets."""
    kfac = 2.0 * np.pi / L
    active = k_min + float(ns) * dk <= (2.0 / 3.0) * (kfac * (0.5 * float(n)))
    end = np.zeros((32, 32), dtype=np.uint8)
    computed = 0
    for s1 in range(ns):
        for s2 in range(s1, ns):
            e = ns
            if active:
                reach = (k_min + (s1 + 1.0) * dk) + (k_min + (s2 + 1.0) * dk)
                e = s2
                while e < ns and not (k_min + float(e) * dk >= reach):
                    e += 1
            end[s1, s2] = e
            computed += e - s2
    return end, computed


def probe_ms(prec, ns, M, end, reps):
    """Event time of the contraction and its reduction on ns random arrays of M cells: median of `reps` after one warm-up."""
    lib = C.CDLL(PROBE)
    vp = C.c_void_p
    lib.fftp_bispec_triple.argtypes = [C.c_int, C.c_int, C.c_longlong, vp, vp, vp, vp]
    rng = np.random.default_rng(5)
    a = rng.standard_normal((ns, M), dtype=np.float32 if prec else np.float64)
    out = np.zeros(ns * (ns + 1) * (ns + 2) // 6)
    ms = C.c_float()
    got = []
    for r in range(1 + reps):
        rc = lib.fftp_bispec_triple(prec, ns, M, a.ctypes.data, end.ctypes.data, out.ctypes.data, C.byref(ms))
        if rc:
            raise RuntimeError("fftp_bispec_triple: %d" % rc)
        if r:
            got.append(ms.value)
    return float(np.median(got))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="256")
    ap.add_argument("--shells", default="8,16,32")
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--no-probe", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bispec_bench.json"))
    a = ap.parse_args()
    res = []
    for n in (int(s) for s in a.sizes.split(",")):
        L = 200.0 * n / 64
        kf = 2.0 * np.pi / L
        N = n ** 3
        for precision in (0, 1):
            esz = 4 if precision else 8
            row = dict(n=n, dtype="f32" if precision else "f64", lib=os.environ.get("BCHMC_LIB", ""), shells={})
            try:
                e = Engine(HamilParams(Nx=n, L=L), precision=precision)
                e.chain_set_state(field(n))
                for ns in (int(s) for s in a.shells.split(",")):
                    k_min, dk = 0.5 * kf, ((2.0 / 3.0) * (n / 2.0) - 0.5) * kf / ns * (1.0 - 1e-12)
                    end, computed = row_ends(n, L, k_min, dk, ns)
                    call = lambda: e.bispectrum(source="chain", k_min=k_min, dk=dk, n_shell=ns)  # noqa: E731
                    e.bispec_release()
                    t0 = time.perf_counter()
                    first = call()
                    r = dict(k_min=k_min, dk=dk, triplets=int(len(first["b"])), triplets_computed=int(computed),
                             triplets_filled=int(np.count_nonzero(first["ntri"] >= 0.5)),
                             first_call_ms=1e3 * (time.perf_counter() - t0))
                    r["later_calls"] = timed(call, a.reps)
                    r["later_calls_event_ms"] = profiled(e, call, a.reps)
                    nbytes, flop = ns * N * esz, 2.0 * computed * N
                    r["contraction"] = dict(bytes=nbytes, flop=flop, floor_flop_ms=1e3 * flop / PEAK_FP64,
                                            floor_bytes_ms=copy_ms(2 * nbytes, a.reps) / 2.0)
                    if not a.no_probe:
                        r["contraction"]["event_ms"] = probe_ms(precision, ns, N, end, 3)
                    if not a.no_host_route and ns == 8 and precision == 0:
                        from tests import bispec_reference as br
                        t0 = time.perf_counter()
                        x = e.chain_get_state().reshape((n,) * 3)
                        t1 = time.perf_counter()
                        br.restatement(x, L, k_min, dk, ns)
                        t2 = time.perf_counter()
                        r["host_route_ms"] = dict(get_state=1e3 * (t1 - t0), numpy_restatement=1e3 * (t2 - t1), total=1e3 * (t2 - t0))
                    row["shells"][str(ns)] = r
                    print(json.dumps(dict(n=n, dtype=row["dtype"], n_shell=ns, **r)), flush=True)
                e.close()
            except BchmcError as err:
                row["skipped"] = str(err)
                print(json.dumps(row), flush=True)
            res.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X, host clock around calls that end in their own synchronise; medians and quartiles; "
                                "*_event_ms: bchmc_profile's event time per call by kernel class; contraction.event_ms: "
                                "k_bispec_triple + k_bispec_reduce alone on random arrays, event time; floor_bytes_ms: half "
                                "the time of a device-to-device copy that reads and writes the contraction's bytes; "
                                "floor_flop_ms: 2 T_computed N flop at 78.6 TFLOP/s",
                       results=res), f, indent=1)


if __name__ == "__main__":
    main()
