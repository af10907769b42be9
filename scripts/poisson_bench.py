"""Cost of Poisson-sampling a density field on the device: at 256^3 fp64, a lognormal-like field at
Nbar = 0.5, 8 and 64, three things, each after a warm-up call:

  * bchmc_poisson_draw of the 256^3 field (counts, scan, offsets);
  * bchmc_poisson_positions of one batch of 2^20 particles from the middle of that sample;
  * bchmc_poisson_density of a 128^3 field into the 256^3 grid, CIC (tools/poisson_upres.cc end to end).

Per case the engine's own event time of the device work (bchmc_profile: HIP events around every launch) and the host clock
around the whole call.  Beside them: the draw's bytes read and written against 8 TB/s; the same rates through
numpy.random.Generator.poisson on the host; and the host route the last entry point replaces -- the positions fetched to
the host, then bchmc_density_particles of them.  Writes profiles/poisson_bench.json (--out).

    python scripts/poisson_bench.py [--reps 5] [--n 256] [--no-host]
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

HBM_BYTES_PER_S = 8e12
# the draw from a staged host field: k_pois_counts reads x (8 B) and writes the count as a double and its offset inside the
# workgroup (16 B); k_pois_offsets reads and writes the offset (16 B); the two scans of the workgroup totals are 1 / 1024 of that
DRAW_BYTES_PER_CELL = 40


def lognormal_delta(n, rng, sigma=1.0, smooth=2.0):
    """exp(sigma g) / mean - 1, g a unit-variance Gaussian field smoothed over `smooth` cells."""
    k = np.fft.fftfreq(n) * 2 * np.pi
    k2 = k[:, None, None] ** 2 + k[None, :, None] ** 2 + np.fft.rfftfreq(n)[None, None, :] ** 2 * (2 * np.pi) ** 2
    g = np.fft.irfftn(np.fft.rfftn(rng.standard_normal((n, n, n))) * np.exp(-0.5 * k2 * smooth ** 2), s=(n, n, n))
    g /= g.std()
    rho = np.exp(sigma * g)
    return (rho / rho.mean() - 1.0).reshape(-1)


def timed(e, call, reps):
    """(median event ms of the call's device work, median host-clock ms, last result) after one warm-up call."""
    e.profile(True)
    ev, host, out = [], [], None
    for r in range(reps + 1):
        e.profile_read()
        t0 = time.perf_counter()
        out = call()
        dt = 1e3 * (time.perf_counter() - t0)
        prof = sum(ms for ms, cnt in e.profile_read().values() if cnt)
        if r:
            ev.append(prof)
            host.append(dt)
    e.profile(False)
    return float(np.median(ev)), float(np.median(host)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson_bench.json"))
    a = ap.parse_args()
    n, half = a.n, a.n // 2
    p = HamilParams(Nx=n, L=200.0 * n / 64, mk=1, calc_h=1)
    rng = np.random.default_rng(7)
    fine, coarse = lognormal_delta(n, rng), lognormal_delta(half, rng)
    e = Engine(p)
    res = []
    for nbar in (0.5, 8.0, 64.0):
        row = dict(n=n, Nbar=nbar)
        ev, host, (_, st) = timed(e, lambda: e.poisson_draw(fine, seed=1, scale=nbar, counts=False), a.reps)
        floor_ms = 1e3 * DRAW_BYTES_PER_CELL * p.N / HBM_BYTES_PER_S
        row["draw"] = dict(event_ms=ev, host_clock_ms=host, n_part=st["n_part"], max_count=st["max_count"],
                           n_capped=st["n_capped"], lambda_max=st["lambda_max"], bytes=DRAW_BYTES_PER_CELL * p.N,
                           floor_ms_at_8TBs=floor_ms, fraction_of_8TBs=floor_ms / ev,
                           cells_per_s=p.N / (1e-3 * ev))
        m = min(1 << 20, st["n_part"])
        first = (st["n_part"] - m) // 2
        ev, host, _ = timed(e, lambda: e.poisson_positions(first, m), a.reps)
        row["positions_batch"] = dict(m=m, event_ms=ev, host_clock_ms=host, particles_per_s=m / (1e-3 * ev))
        if not a.no_host:
            lam = nbar * (1.0 + fine)
            t0 = time.perf_counter()
            k = np.random.default_rng(1).poisson(lam)
            dt = time.perf_counter() - t0
            row["numpy_poisson"] = dict(ms=1e3 * dt, cells_per_s=p.N / dt, n_part=int(k.sum()))
        # up-resolving: n / 2 into n.  Nbar per coarse cell is 8 Nbar per fine cell of the same mean count
        _, st = e.poisson_draw(coarse, seed=2, scale=nbar, counts=False)
        ev, host, (rho, ds) = timed(e, lambda: e.poisson_density(mk=1), a.reps)
        row["density_upres"] = dict(n_in=half, n_part=st["n_part"], event_ms=ev, host_clock_ms=host, n_in_domain=ds["n_in"],
                                    sum_rho=float(rho.sum()), ns_per_particle=1e6 * ev / max(st["n_part"], 1))
        if not a.no_host:
            t0 = time.perf_counter()
            x, y, z = e.poisson_positions(0, st["n_part"])
            t1 = time.perf_counter()
            rho_h, _ = e.density_particles(x, y, z, mk=1)
            t2 = time.perf_counter()
            row["host_route"] = dict(positions_to_host_ms=1e3 * (t1 - t0), density_particles_ms=1e3 * (t2 - t1),
                                     total_ms=1e3 * (t2 - t0), over_density_upres_host_clock=1e3 * (t2 - t0) / host,
                                     rel_l2=float(np.linalg.norm(rho_h - rho) / max(np.linalg.norm(rho), 1e-300)))
            del x, y, z
        res.append(row)
        print(json.dumps(row), flush=True)
    e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(measured="MI355X; event_ms: bchmc_profile's event time of the call's device work, host_clock_ms: around "
                                "the whole call; medians of --reps calls after one warm-up; numpy_poisson and host_route: one "
                                "repetition", results=res), f, indent=1)


if __name__ == "__main__":
    main()
