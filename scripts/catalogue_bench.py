"""Cost of assigning a free particle catalogue to the grid on the device: bchmc_density_particles at
256^3 fp64 with SPH (h = d) and with CIC, for three catalogues -- N_part = N uniform, N_part = 8 N uniform, and N_part = N
drawn from a log-normal field (clustered).

Per case: the host clock around the whole call (the catalogue's way over PCIe included; the call ends in its own
synchronise) and, separately, the engine's own event time of the device work (bchmc_profile: the kernels of every batch
and the final conversion, without the transfers between them; also split into binning, scatter and the rest); 3 warm-ups, then the median and
quartiles of --reps calls.  Beside them the host cost of the same assignment by the route that existed before: the
oracle's OpenMP getDensity (the C restatement of massFunctions.cc) on the threads the machine grants, N particles at a
time, one repetition (not taken for SPH of 8 N particles, which would run for minutes).  Writes profiles/catalogue_bench.json (--out).

    python scripts/catalogue_bench.py [--reps 20] [--n 256] [--host-threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from barcode_amd.engine import Engine  # noqa: E402
from barcode_amd.params import HamilParams  # noqa: E402


def lognormal_catalogue(n, L, count, rng, sigma=1.5, smooth=2.0):
    """`count` particles drawn from exp(sigma g), g a unit-variance Gaussian field smoothed over `smooth` cells: the cell
    by inversion of the cumulative sum, the place inside the cell uniform."""
    k = np.fft.fftfreq(n) * 2 * np.pi
    k2 = k[:, None, None] ** 2 + k[None, :, None] ** 2 + np.fft.rfftfreq(n)[None, None, :] ** 2 * (2 * np.pi) ** 2
    g = np.fft.irfftn(np.fft.rfftn(rng.standard_normal((n, n, n))) * np.exp(-0.5 * k2 * smooth ** 2), s=(n, n, n))
    g /= g.std()
    cdf = np.cumsum(np.exp(sigma * g).reshape(-1))
    cell = np.searchsorted(cdf, rng.random(count) * cdf[-1])
    d = L / n
    idx = np.stack([cell // (n * n), (cell // n) % n, cell % n])
    return (idx + rng.random((3, count))) * d


def stats(ms):
    q1, med, q3 = (float(x) for x in np.percentile(ms, [25, 50, 75]))
    return dict(median_ms=med, q1_ms=q1, q3_ms=q3, reps=len(ms))


def measure(e, pos, mk, reps, warmup=3, w=None):
    """Host clock per call and the event time of its device work, the same calls; the event time also by kernel class:
    the binning (count, scan, fill), the scatter, and the rest (clearing, conversion)."""
    e.profile(True)
    host, dev, cls = [], [], {}
    for r in range(warmup + reps):
        e.profile_read()
        t0 = time.perf_counter()
        rho, st = e.density_particles(pos[0], pos[1], pos[2], w, mk=mk)
        dt = 1e3 * (time.perf_counter() - t0)
        prof = {k: ms for k, (ms, cnt) in e.profile_read().items() if cnt}
        if r >= warmup:
            host.append(dt)
            dev.append(sum(prof.values()))
            for k, ms in prof.items():
                cls.setdefault(k, []).append(ms)
    e.profile(False)
    return dict(host_clock=stats(host), device_events=stats(dev),
                device_events_by_class_median_ms={k: float(np.median(v)) for k, v in cls.items()}, n_in=st["n_in"],
                max_per_tile=st["max_per_tile"], sum_rho=float(rho.sum()))


def host_route(p, pos, mk, threads):
    """The oracle's getDensity, N particles at a time (it takes the handle's own particle count), summed."""
    os.environ["OMP_NUM_THREADS"] = str(threads)
    from oracle.oracle import Oracle
    o = Oracle(p)
    N = p.N
    t0 = time.perf_counter()
    rho = np.zeros(N)
    for s in range(0, pos.shape[1], N):
        rho += o.getDensity(mk, pos[0, s:s + N], pos[1, s:s + N], pos[2, s:s + N])
    return 1e3 * (time.perf_counter() - t0), rho


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "catalogue_bench.json"))
    a = ap.parse_args()
    n = a.n
    p = HamilParams(Nx=n, L=200.0 * n / 64)
    rng = np.random.default_rng(7)
    cats = (("uniform_N", rng.random((3, p.N)) * p.L), ("uniform_8N", rng.random((3, 8 * p.N)) * p.L),
            ("lognormal_N", lognormal_catalogue(n, p.L, p.N, rng)))
    e = Engine(p)
    res = []
    for name, pos in cats:
        pos = np.ascontiguousarray(pos)
        for mk, kernel in ((3, "SPH h=d"), (1, "CIC")):
            row = dict(n=n, dtype="f64", catalogue=name, n_part=int(pos.shape[1]), kernel=kernel,
                       tiled=bool(e.tile_info()["tiled"]))
            row.update(measure(e, pos, mk, a.reps))
            row["device_ns_per_particle"] = 1e6 * row["device_events"]["median_ms"] / pos.shape[1]
            # the host's SPH of 8 N particles alone would take minutes: not measured
            if not a.no_host and not (mk == 3 and pos.shape[1] > p.N):
                ms, rho_h = host_route(p, pos, mk, a.host_threads)
                row["host_route_ms"] = ms
                row["host_route_threads"] = a.host_threads
                row["host_route_over_host_clock"] = ms / row["host_clock"]["median_ms"]
                rho, _ = e.density_particles(pos[0], pos[1], pos[2], mk=mk)
                row["rel_l2_against_host_route"] = float(np.linalg.norm(rho - rho_h) / np.linalg.norm(rho_h))
            res.append(row)
            print(json.dumps(row), flush=True)
        if name == "uniform_N":  # the same catalogue with a weight column: its pass on the host and its 8 B per particle
            w = rng.standard_normal(pos.shape[1])
            row = dict(n=n, dtype="f64", catalogue=name + "_weighted", n_part=int(pos.shape[1]), kernel="CIC", tiled=True)
            row.update(measure(e, pos, 1, a.reps, w=w))
            row["device_ns_per_particle"] = 1e6 * row["device_events"]["median_ms"] / pos.shape[1]
            res.append(row)
            print(json.dumps(row), flush=True)
    e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X; host_clock: around the whole call, catalogue transfer included; device_events: "
                                "bchmc_profile's event time of the same calls' device work; medians and quartiles after 3 "
                                "warm-ups; host_route_ms: the oracle's OpenMP getDensity, one repetition",
                       results=res), f, indent=1)


if __name__ == "__main__":
    main()
