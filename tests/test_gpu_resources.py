"""Everything a handle allocates comes back when it is closed: bchmc_live_resources (device buffers, their bytes,
pinned host buffers, other objects: events, streams, rocFFT plans and execution infos) before an engine is created,
while it is alive after every lazily allocating entry point has run, and after close().  Counts only: free device memory
moves under other processes and is not looked at.  Nx = 16 is the smallest grid on the tiled path (8 x 8 x 16 tiles)."""
import gc

import numpy as np
import pytest

from barcode_amd import engine
from barcode_amd.engine import BchmcError, Engine
from barcode_amd.gsl_mt19937 import GslMT19937
from barcode_amd.params import HamilParams
from tests.util import Case

pytestmark = pytest.mark.gpu

NX = 16


def _start():
    gc.collect()   # an engine some earlier test dropped without close() goes now, not between the two readings
    return engine.live_resources()


def _alive(start):
    now = engine.live_resources()
    print("live resources: start %s now %s" % (start, now))
    assert all(n > s for n, s in zip(now, start)), (start, now)
    return now


def _closed(e, start):
    e.close()
    assert engine.live_resources() == start


def test_every_lazy_allocation_of_a_chain_is_returned():
    """The resident chain (cq, cp, part6, cg, qk2, pk2, guard), gradient (gprior, glike), the three measurements with two
    bin counts each (spec_bins, corr1.acc, corr2.* regrow), the MT19937 draw and the mock data (mt.*, mock.*, the
    Gaussian buffer growing from the momenta's size to the truth field's), host-array trajectories (copy stream,
    early-download event), all with profiling on (the event pool)."""
    c = Case(Nx=NX, likelihood=1, rsd_model=1)
    start = _start()
    e = c.engine()
    created = _alive(start)
    e.profile(True)
    e.chain_set_state(c.q0)
    e.chain_draw_momenta(11, 0)
    _, _, done = e.chain_attempt(c.eps, 3)
    assert done == 3
    e.chain_accept(True)
    e.chain_draw_momenta(11, 1)
    e.chain_attempt(c.eps, 3)          # carries the gradient of the accepted state (cg)
    e.chain_accept(False)
    e.gradient(c.q0)
    for n_bin in (20, 50):
        e.measure_spectrum(None, n_bin)
    for n_bin in (8, 12):
        e.measure_corr(None, n_bin)
        e.measure_corr2d(None, n_bin)
    rng = GslMT19937(4242)
    assert e.chain_draw_momenta_mt19937(rng) > 0
    q1, p1, done, dH, terms = e.leapfrog_dh(c.q0, c.p0, c.eps, 3)
    assert done == 3 and np.isfinite(dH) and np.all(np.isfinite(q1))
    assert e.leapfrog(c.q0, c.p0, c.eps, 2)[2] == 2
    used, dl, de = e.setup_random_test(rng)
    assert used > 0 and np.all(np.isfinite(de))
    for guess in (2, 4):
        assert e.make_initial_guess(rng, guess) > 0
    assert sum(n for _, n in e.profile_read().values()) > 0
    now = _alive(start)
    # at least: cq, cp, part6, guard, 2 of gradient, spec_bins, corr1.acc, 4 of corr2, 11 of mt, 5 of mock; mt.h_io; the
    # copy stream, ev_q and two events of the pool
    assert now[0] >= created[0] + 28 and now[1] > created[1] and now[2] >= created[2] + 1 and now[3] >= created[3] + 4
    _closed(e, start)


def test_slot_polls_and_a_grown_partition_are_returned(monkeypatch):
    """BCHMC_SORT_CAP=64: a 20-step device trajectory polls the slot words (h_slots and its two events), and the forward
    model of a strongly clustered field re-partitions the records at the next synchronising call.  At this size the
    record array holds four times all particles from the start, so the partition grows inside the allocation; the
    reallocation's own order of release and allocation is what tests/host/owned_check.cpp exercises."""
    import torch
    monkeypatch.setenv("BCHMC_SORT_CAP", "64")
    c = Case(Nx=NX, likelihood=1, rsd_model=1)
    start = _start()
    e = c.engine()
    created = _alive(start)
    assert e.tile_info()["watch"] == 1
    dev = torch.device("cuda", 0)
    q0, p0 = torch.from_numpy(c.q0.reshape(-1)).to(dev), torch.from_numpy(c.p0.reshape(-1)).to(dev)
    q1, p1 = torch.empty_like(q0), torch.empty_like(p0)
    e.leapfrog_device(q0, p0, q1, p1, c.eps, 20)
    assert e.steps_done() == 20
    e.forward(40.0 * c.truth, 1)
    assert e.tile_info()["cap"] > 64
    now = _alive(start)
    assert now[2] == created[2] + 1 and now[3] == created[3] + 2   # h_slots, slot_ev[2]
    _closed(e, start)


def test_sph_convolution_tables_are_returned():
    """calc_h = 3: conv and convF."""
    c = Case(Nx=NX, likelihood=1, rsd_model=1, calc_h=3)
    start = _start()
    e = c.engine()
    created = _alive(start)
    e.gradient(c.q0)
    assert e.leapfrog_dh(c.q0, c.p0, c.eps, 2)[2] == 2
    now = _alive(start)
    assert now[0] >= created[0] + 2
    _closed(e, start)


@pytest.mark.parametrize("t", [5, 6])
def test_jasche_mass_scratch_is_returned(t):
    """hamiltonian_mass of a Jasche type allocates six scratch buffers and releases them before it returns."""
    c = Case(Nx=NX, likelihood=1, window_zero_fraction=0.3, mass_type=t)
    start = _start()
    e = c.engine()
    before = _alive(start)
    mf, mr = e.hamiltonian_mass(c.q0)
    assert mr is not None and np.all(np.isfinite(mr))
    after = _alive(start)
    assert after == before   # these types bin no spectrum: nothing of the call is kept
    _closed(e, start)


def test_a_staged_host_trajectory_is_returned(monkeypatch):
    """The one case above Nx = 16: arrays cross PCIe through the two pinned staging chunks and their events only above
    1 MiB, i.e. from 64^3 on.  One short host-array trajectory, no oracle."""
    from barcode_amd import inputs
    monkeypatch.setenv("BCHMC_STAGE_MB", "1")
    p = HamilParams(Nx=64, L=200.0, likelihood=1, rsd_model=1)
    f = inputs.make_fields(p)
    one = np.ones(p.N)
    start = _start()
    e = Engine(p)
    created = _alive(start)
    e.upload(signal_PS=f["signal_PS"], mass_f=f["mass_f"], window=one, noise=one, nobs=one)
    staged = _alive(start)
    assert staged[2] == created[2] + 2 and staged[3] == created[3] + 2   # the two chunks and their events
    assert e.leapfrog_dh(f["q0"], f["p0"], 1e-3 * p.eps_heuristic(), 2)[2] == 2
    _alive(start)
    _closed(e, start)


def test_a_refused_configuration_holds_nothing():
    start = _start()
    with pytest.raises(BchmcError):
        Engine(HamilParams(Nx=NX, mass_type=7))   # closes the handle it was given for the error text
    assert engine.live_resources() == start
    h = engine.C.c_void_p()
    cfg = engine.make_config(HamilParams(Nx=NX, mass_type=7))
    lib = engine.load()
    assert lib.bchmc_create(engine.C.byref(cfg), engine.C.byref(h)) != 0 and h
    assert engine.live_resources() == start
    lib.bchmc_destroy(h)
    assert engine.live_resources() == start
