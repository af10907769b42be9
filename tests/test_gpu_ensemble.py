"""bchmc_ensemble_* on the device against the numpy restatement of the same lines (tests/ensemble_restatement.py): the
kernels are compiled without FMA contraction, with IEEE divide and sqrt, in the operand order include/bchmc.h states, so
count, mean, variance, standard deviation and m2 are compared with ``numpy.array_equal`` -- after every sample, on fp64
and fp32 handles, for host fields and for the two device sources (whose fields the restatement is fed as the engine
itself hands them out; their parity with the oracle is what the existing tests pin)."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

from barcode_amd import engine as engine_mod
from barcode_amd import hamil, inputs, io
from barcode_amd.engine import BchmcError, Engine
from barcode_amd.params import HamilParams
from tests import ensemble_restatement as er
from tests.util import TOL_FIELD, Case

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 9
PREC = pytest.mark.parametrize("precision", (0, 1), ids=("fp64", "fp32"))


def box_of(n):
    return 200. * n / 64.


@functools.lru_cache(maxsize=None)
def samples_of(n):
    """make_fields' truth and q0 plus seeded perturbations of them: 7 samples up to 16^3, 3 at 128^3; shared read-only."""
    f = inputs.make_fields(HamilParams(Nx=n, L=box_of(n)))
    rng = np.random.Generator(np.random.Philox(1000 + n))
    count = 7 if n <= 16 else 3
    out = [f["truth"].ravel(), f["q0"].ravel()]
    sd = float(np.std(f["truth"]))
    while len(out) < count:
        out.append(f["truth"].ravel() + 0.3 * sd * rng.standard_normal(n ** 3))
    s = np.ascontiguousarray(out[:count])
    s.setflags(write=False)
    return s


def engine_of(n, precision=0):
    return Engine(HamilParams(Nx=n, L=box_of(n)), precision=precision)


def equal_to(e, slot, w, tag=""):
    """Every output of a slot against the restatement `w`, bit for bit."""
    assert e.ensemble_count(slot) == w.count, tag
    if w.count == 0:
        return
    assert np.array_equal(e.ensemble_fetch(slot, "mean"), w.mean), tag + " mean"
    assert np.array_equal(e.ensemble_fetch(slot, "m2"), w.m2), tag + " m2"
    if w.count >= 2:
        assert np.array_equal(e.ensemble_fetch(slot, "variance"), w.variance()), tag + " variance"
        assert np.array_equal(e.ensemble_fetch(slot, "std"), w.std()), tag + " std"


@PREC
@pytest.mark.parametrize("n", (4, 5, 9, 16, 128))
def test_host_fields_bit_for_bit_after_every_add(n, precision):
    """n = 4: the smallest grid; 5 and 9: odd N, the scalar tail; 16 and 128: more than one workgroup, 128 more pairs
    than the grid has threads on a small device.  A host field is accumulated from its staged doubles, so an fp32 handle
    gives the fp64 handle's bits."""
    e = engine_of(n, precision)
    w = er.Welford(n ** 3)
    assert e.ensemble_count(0) == 0
    for i, x in enumerate(samples_of(n)):
        e.ensemble_add(0, x)
        w.add(x)
        equal_to(e, 0, w, "%d^3 sample %d" % (n, i))
    assert np.all(w.variance() > 0)
    e.close()


@PREC
@pytest.mark.parametrize("n", (9, 16))
def test_chain_state_and_deltax_bit_for_bit(n, precision):
    """Three chain states, a forward model without and with RSD for each: the chain state into slot 0, the real-space
    deltaX into slot 1, the redshift-space one into slot 2."""
    c = Case(Nx=n, likelihood=1, rsd_model=1)
    e = c.engine(precision=precision)
    w = [er.Welford(n ** 3) for _ in range(3)]
    for state in (c.q0, c.truth, 0.5 * (c.q0 - c.truth)):
        e.chain_set_state(state)
        for rsd in (0, 1):
            e.chain_forward(rsd)
            e.ensemble_add(0, source="chain")
            w[0].add(e.chain_get_state())
            e.ensemble_add(1 + rsd, source="deltaX")
            w[1 + rsd].add(e.fetch("deltaX"))
            for slot in range(3):
                equal_to(e, slot, w[slot], "%d^3 slot %d" % (n, slot))
    assert w[0].count == 6 and w[1].count == w[2].count == 3
    assert not np.array_equal(w[1].mean, w[2].mean)  # two different fields were accumulated
    e.close()


@PREC
@pytest.mark.parametrize("n", (9, 16))
def test_merge(n, precision):
    """7 samples split 3 + 4 over two slots, one exported and merged into the other: bit for bit the Chan restatement
    of the two exported triples, within TOL_FIELD of the largest value of the sequential result; a merge of count 0 is
    a no-op, a merge into an empty slot a copy."""
    s = samples_of(n)
    e = engine_of(n, precision)
    seq = er.Welford(n ** 3)
    for i, x in enumerate(s):
        e.ensemble_add(0 if i < 3 else 1, x)
        seq.add(x)
    a, b = e.ensemble_export(0), e.ensemble_export(1)
    assert a[0] == 3 and b[0] == 4
    e.ensemble_merge(0, 0, None, None)
    e.ensemble_merge(0, 0, b[1], b[2])
    assert e.ensemble_count(0) == 3 and np.array_equal(e.ensemble_fetch(0, "mean"), a[1])
    e.ensemble_merge(0, *b)
    w = er.Welford(n ** 3).merge(*a).merge(*b)
    equal_to(e, 0, w, "merged")
    for got, want in ((w.mean, seq.mean), (w.variance(), seq.variance()), (w.std(), seq.std())):
        lvl = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print("%d^3 merged against sequential: %.2e of max" % (n, lvl))
        assert lvl <= TOL_FIELD
    e.ensemble_merge(2, *e.ensemble_export(0))  # into an empty slot
    equal_to(e, 2, w, "copied")
    assert e.ensemble_export(3)[0] == 0 and not e.ensemble_export(3)[1].any()
    e.close()


def test_slots_are_independent():
    n = 9
    s = samples_of(n)
    e = engine_of(n)
    for x in s[:3]:
        e.ensemble_add(0, x)
    before = [e.ensemble_fetch(0, what) for what in ("mean", "variance", "std")]
    for x in s[3:]:
        e.ensemble_add(1, x)
    e.ensemble_reset(1)
    e.ensemble_add(1, s[0])
    after = [e.ensemble_fetch(0, what) for what in ("mean", "variance", "std")]
    assert e.ensemble_count(0) == 3 and e.ensemble_count(1) == 1
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(e.ensemble_fetch(1, "mean"), s[0]) and not e.ensemble_fetch(1, "m2").any()
    e.close()


def test_an_add_leaves_the_state_alone():
    """A deterministic handle at 16^3: two attempts with adds from the chain state and from deltaX between them -- one
    pair between chain_attempt and chain_accept, with the proposal pending -- give dH, terms and the proposal bit for bit
    as a twin that accumulated nothing."""
    c = Case(Nx=16, likelihood=1, rsd_model=1)

    def run(accumulate):
        e = Engine(c.p, deterministic=1)
        e.upload(**c.arrays())
        e.chain_set_state(c.q0)
        e.chain_set_momenta(c.p0)
        out = [e.chain_attempt(c.eps, 3)]
        before = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + (e.fetch("deltaX"),)
        if accumulate:
            e.ensemble_add(0, source="chain")
            e.ensemble_add(1, source="deltaX")
            e.ensemble_add(2, c.truth)
            assert np.array_equal(e.ensemble_fetch(0), before[0]) and np.array_equal(e.ensemble_fetch(1), before[4])
        after = (e.chain_get_state(), e.chain_get_momenta()) + e.chain_get_proposal() + (e.fetch("deltaX"),)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        out.append(e.chain_get_proposal())
        e.chain_accept(1)
        if accumulate:
            e.ensemble_add(0, source="chain")
            e.ensemble_add(1, source="deltaX")
            assert e.ensemble_count(0) == 2 and np.array_equal(e.chain_get_state(), before[2])
        e.chain_set_momenta(0.9 * c.p0)
        out.append(e.chain_attempt(c.eps, 3))
        out.append(e.chain_get_proposal())
        e.close()
        return out

    plain, acc = run(False), run(True)
    for k in (0, 2):
        assert plain[k][0] == acc[k][0] and np.array_equal(plain[k][1], acc[k][1]) and plain[k][2] == acc[k][2] == 3
    for k in (1, 3):
        assert all(np.array_equal(x, y) for x, y in zip(plain[k], acc[k]))


@PREC
def test_one_nan_cell_stays_in_its_cell(precision):
    n = 9
    s = samples_of(n)
    for bad, cell in ((np.nan, 123), (np.inf, n ** 3 - 1)):  # the second in the scalar tail
        e = engine_of(n, precision)
        w = er.Welford(n ** 3)
        for i, x in enumerate(s[:4]):
            x = np.array(x)
            if i == 1:
                x[cell] = bad
            e.ensemble_add(0, x)
            w.add(x)
        mean, var = e.ensemble_fetch(0, "mean"), e.ensemble_fetch(0, "variance")
        nan = np.isnan(mean)
        assert nan[cell] and nan.sum() == 1 and np.array_equal(np.isnan(var), nan)
        assert np.array_equal(mean[~nan], w.mean[~nan]) and np.array_equal(var[~nan], w.variance()[~nan])
        e.close()


def test_refusals_and_resources():
    gc.collect()
    start = engine_mod.live_resources()
    n = 16
    N = n ** 3
    s = samples_of(n)
    e = engine_of(n)
    created = engine_mod.live_resources()
    lib, dp = e.lib, C.POINTER(C.c_double)
    x = np.array(s[0])
    xp = x.ctypes.data_as(dp)
    out = np.zeros(N)
    op = out.ctypes.data_as(dp)
    cnt = C.c_uint64(5)
    for slot in (4, -1):
        assert lib.bchmc_ensemble_add(e.h, slot, 0, xp) == ARG
        assert lib.bchmc_ensemble_count(e.h, slot, C.byref(cnt)) == ARG
        assert lib.bchmc_ensemble_fetch(e.h, slot, 0, op) == ARG
        assert lib.bchmc_ensemble_merge(e.h, slot, 1, xp, xp) == ARG
        assert lib.bchmc_ensemble_reset(e.h, slot) == ARG
    assert lib.bchmc_ensemble_add(e.h, 0, 1, xp) == ARG and lib.bchmc_ensemble_add(e.h, 0, 2, xp) == ARG
    assert lib.bchmc_ensemble_add(e.h, 0, 0, None) == ARG and lib.bchmc_ensemble_add(e.h, 0, 3, None) == ARG
    assert lib.bchmc_ensemble_add(e.h, 0, 1, None) == STATE  # no chain state
    assert lib.bchmc_ensemble_add(e.h, 0, 2, None) == STATE  # no forward evaluation
    assert lib.bchmc_ensemble_fetch(e.h, 0, 0, None) == ARG and lib.bchmc_ensemble_fetch(e.h, 0, 4, op) == ARG
    assert lib.bchmc_ensemble_merge(e.h, 0, 1, None, xp) == ARG and lib.bchmc_ensemble_merge(e.h, 0, 1, xp, None) == ARG
    assert lib.bchmc_ensemble_fetch(e.h, 0, 0, op) == STATE  # the mean of nothing
    assert engine_mod.live_resources() == created and not out.any() and cnt.value == 5  # nothing was taken or written
    e.ensemble_add(0, x)
    one = engine_mod.live_resources()
    assert one[0] == created[0] + 2 and one[1] == created[1] + 16 * N and one[2:] == created[2:]
    for what in ("variance", "std"):
        with pytest.raises(BchmcError) as err:
            e.ensemble_fetch(0, what)
        assert err.value.code == STATE
    assert np.array_equal(e.ensemble_fetch(0, "mean"), x) and not e.ensemble_fetch(0, "m2").any()
    e.ensemble_add(3, x)
    e.ensemble_add(3, s[1])
    two = engine_mod.live_resources()
    assert two[0] == created[0] + 4 and two[1] == created[1] + 32 * N
    e.ensemble_reset(3)  # keeps the buffers
    assert engine_mod.live_resources() == two and e.ensemble_count(3) == 0
    with pytest.raises(BchmcError) as err:
        e.ensemble_fetch(3, "mean")
    assert err.value.code == STATE
    e.ensemble_add(3, s[2])
    assert np.array_equal(e.ensemble_fetch(3), s[2])  # the reset zeroed the arrays
    e.ensemble_release()
    assert engine_mod.live_resources() == created and e.ensemble_count(0) == e.ensemble_count(3) == 0
    e.ensemble_add(1, x)  # and a later add takes them again
    assert engine_mod.live_resources()[0] == created[0] + 2
    e.close()
    assert engine_mod.live_resources() == start


def test_hamil_and_io_layers(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    n = 9
    s = samples_of(n)
    e = engine_of(n)

    class View:  # what hamil.py's functions read of a HamilData
        engine = e
    w = er.Welford(n ** 3)
    for x in s[:3]:
        hamil.ensemble_add(View, 2, x)
        w.add(x)
    assert np.array_equal(hamil.ensemble_fetch(View, 2), w.mean)
    assert np.array_equal(hamil.ensemble_fetch(View, 2, "std"), w.std())
    paths = io.dump_ensemble(e, "", 2, "deltaLAG")
    assert paths == ("deltaLAG_mean.dat", "deltaLAG_std.dat")
    assert np.array_equal(io.read_array("deltaLAG_mean", n ** 3), w.mean)
    assert np.array_equal(io.read_array("deltaLAG_std", n ** 3), w.std())
    e.close()
