"""The scalars off their defaults, without a GPU (tests/offdefault.py has the sets and why they are what they are):
the cosmology factors against the formula text, the two CPU restatements against each other, the force against finite
differences of the energy, every scalar shown to change what the GPU test compares, the per-cell likelihood formulas
with their bound (tests/like_bound.py), and the growth factors input_par.hamil_params computes.
The engine's side of the same comparisons is tests/test_gpu_offdefault.py."""
import dataclasses
import os

import numpy as np
import pytest

from barcode_amd import input_par
from barcode_amd.params import HamilParams
from oracle import oracle as orc
from oracle.np_restatement import NpHamil
from tests import like_bound as lb
from tests import offdefault as od
from tests import pm_reference as ref
from tests.offdefault import OFF, OFF_LN, scalars_for
from tests.util import GOLDEN_DIR, TOL_ENERGY, TOL_FIELD, Case, rel_l2

LD = np.longdouble


# ---- the sets themselves --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [OFF, OFF_LN], ids=["OFF", "OFF_LN"])
def test_the_sets_meet_their_conditions(s):
    assert set(s) == set(od.DEFAULTS) and len(s) == 9
    for k, v in s.items():
        assert v not in (0.0, 1.0) and v != od.DEFAULTS[k], k
    assert abs(s["OM"] + s["OL"] - 1) > 0.05 and s["ascale"] != 1
    assert abs(s["D2"] - od.derived_D2(s)) > 0.02          # not the derived D2 ...
    assert HamilParams(Nx=8, **s).D2 == s["D2"]            # ... and passed on as given
    assert s["biasE"] != round(s["biasE"])
    assert OFF_LN["biasP"] <= 1 < OFF["biasP"]


# ---- cosmology scalars from the formula text ------------------------------------------------------------------------
def cosmo_ld(a, OM, OL):
    """E_Hubble_a, fgrow (term 1), c_pecvel (cosmo.cc:26-31, 182-235) and Hub, v_norm (rsd.cc:26-42) in longdouble."""
    a, OM, OL = LD(a), LD(OM), LD(OL)
    OK = 1 - OM - OL
    E = np.sqrt(OM / (a * a * a) + OK / (a * a) + OL)
    Omega = OM / ((E * E) * (a * a * a))
    f = Omega ** (LD(5) / LD(9))
    hub = 100 * np.sqrt(OM / a / a / a + OL + OK / a / a)
    return dict(E=E, Omega=Omega, f=f, c_pecvel=f * 100 * E * a, Hub=hub, v_norm=1 / hub / a)


COSMOLOGIES = {"OFF": (OFF["ascale"], OFF["OM"], OFF["OL"]), "EdS": (0.37, 1.0, 0.0), "EdS_half": (0.5, 1.0, 0.0),
               "open": (0.4, 0.3, 0.0), "closed": (0.6, 0.4, 0.9), "WMAP7_z1": (0.5, 0.272, 0.728)}


def test_cosmology_scalars_against_the_formula_text():
    """orc_fgrow and orc_c_pecvel against longdouble; measured maximum over the cosmologies: 0.83 ulp of
    double (ulp = 2^-52 relative), held to 4 ulp.  Einstein-de Sitter: E = a^(-3/2), Omega = 1, f = 1, c_pecvel = 100 a^(-1/2)."""
    worst = 0.0
    for name, (a, OM, OL) in COSMOLOGIES.items():
        want = cosmo_ld(a, OM, OL)
        for got, key in ((orc.fgrow(a, OM, OL), "f"), (orc.c_pecvel(a, OM, OL), "c_pecvel")):
            err = float(abs(LD(got) - want[key]) / want[key]) / 2.0 ** -52
            worst = max(worst, err)
            assert err <= 4, (name, key, got, want[key])
        if name.startswith("EdS"):
            assert abs(orc.fgrow(a, OM, OL) - 1) <= 4 * 2.0 ** -52
            assert abs(orc.c_pecvel(a, OM, OL) / (100 / np.sqrt(a)) - 1) <= 4 * 2.0 ** -52
            assert abs(float(want["E"]) / a ** -1.5 - 1) < 1e-15 and abs(float(want["Omega"]) - 1) < 1e-15
        # c_pecvel v_norm = f: what calc_pos_rsd adds to z is f Psi_z, whatever a, OM, OL
        assert abs(float(want["c_pecvel"] * want["v_norm"] / want["f"]) - 1) < 1e-17
    print("cosmology scalars: worst %.2f ulp" % worst)
    # at ascale = 1, E = 1 for any OM, OL: the defaults cannot see them
    assert orc.fgrow(1.0, 0.3, 0.6) == pytest.approx(0.3 ** (5 / 9), rel=1e-15)
    assert orc.fgrow(OFF["ascale"], OFF["OM"], OFF["OL"]) != pytest.approx(OFF["OM"] ** (5 / 9), rel=0.05)


@pytest.mark.parametrize("name", list(COSMOLOGIES))
def test_hub_and_v_norm_through_the_redshift_space_shift(name):
    """The Hub / v_norm pair is not exported: it is seen through Lag2Eul's z_s - z = (c_pecvel Psi_z) v_norm = f Psi_z.
    The difference of two positions of size L carries their rounding: 1e-13 relative to the largest shift."""
    a, OM, OL = COSMOLOGIES[name]
    p = HamilParams(Nx=8, L=25.0, likelihood=1, rsd_model=1, **dict(OFF, ascale=a, OM=OM, OL=OL))
    o = orc.Oracle(p)
    z = (np.arange(8) * p.d)[None, None, :]
    delta = np.broadcast_to(0.2 * np.cos(2 * np.pi * z / p.L), (8, 8, 8)).copy()
    psi_z = o.theta2vel(-p.D1 * delta.ravel())[2]
    z0 = o.Lag2Eul(delta, rsd=0)[3]
    zs = o.Lag2Eul(delta, rsd=1)[3]
    shift = zs - z0
    shift = np.where(shift > p.L / 2, shift - p.L, np.where(shift < -p.L / 2, shift + p.L, shift))
    want = float(cosmo_ld(a, OM, OL)["f"]) * psi_z
    assert np.abs(want).max() > 0.05 and np.max(np.abs(shift - want)) < 1e-13 * p.L
    o.close()


# ---- two restatements agree off default -----------------------------------------------------------------------------
def _np(case):
    return NpHamil(case.p, case.signal_PS, case.mass_f, case.nobs, case.noise, case.window, mass_r=case.mass_r)


RESTATEMENT = [(name, "off") for name in od.RESTATEMENT_CASES] + [("calch3", "default"), ("calch3_rsd", "default")]


@pytest.mark.parametrize("name,scalars", RESTATEMENT, ids=["%s-%s" % r for r in RESTATEMENT])
def test_c_oracle_matches_numpy_restatement_off_default(name, scalars):
    """tests/test_oracle_cpu.py::test_c_oracle_matches_numpy_restatement, same assertions and tolerances, with every
    scalar off its default (and calc_h = 3, which NpHamil used to answer with calc_h = 2's numbers, at both)."""
    kw = od.RESTATEMENT_CASES[name]
    c = Case(Nx=8, **kw, **(scalars_for(kw) if scalars == "off" else {}))
    n = _np(c)
    o = c.oracle
    dX, px, py, pz = o.Lag2Eul(c.truth)
    dXn, posn = n.lag2eul(c.truth, bool(c.p.rsd_model))
    assert rel_l2(dX, dXn) < 1e-13
    for a, b in zip((px, py, pz), posn):
        assert rel_l2(a, b) < 1e-14
    g, gp, gl = o.gradient_psi(c.q0)
    gn, gpn, gln = n.gradient_psi(c.q0)
    assert rel_l2(gp, gpn) < 1e-13
    assert rel_l2(gl, gln) < 1e-12
    assert rel_l2(g, gn) < 1e-12
    q1, p1, done = o.Hamiltonian_EoM(c.q0, c.p0, c.eps, 3)
    q1n, p1n = n.leapfrog(c.q0, c.p0, c.eps, 3)
    assert done == 3
    assert rel_l2(q1, q1n) < 1e-11 and rel_l2(p1, p1n) < 1e-11
    dH, terms = o.delta_Hamiltonian(c.q0, c.p0, q1, p1)
    ref_ = [n.kinetic(c.p0), n.log_prior(c.q0), n.log_like(c.q0), n.kinetic(p1n), n.log_prior(q1n), n.log_like(q1n)]
    assert np.all(np.isfinite(terms))
    assert np.allclose(terms, ref_, rtol=1e-10)
    assert np.isclose(dH, sum(ref_[3:]) - sum(ref_[:3]), rtol=1e-8, atol=1e-8)


def test_np_restatement_refuses_what_it_does_not_restate():
    """calc_h = 1 (and with it NGP / CIC / TSC) exists in the C oracle only: NpHamil says so instead of answering with
    another variant's numbers."""
    c = Case(Nx=8, likelihood=1, calc_h=1)
    with pytest.raises(NotImplementedError):
        _np(c).gradient_psi(c.q0)


def test_lognormal_partial_is_not_finite_for_biasP_above_one():
    """lognormal_independent.cpp:49 takes log(rho_c (1 + biasP delta)^biasE) unguarded: with OFF's biasP = 1.3 a cell
    below delta = -1/1.3 gives NaN in the reference's own formula (both restatements agree on the class).  This is why
    log-normal trajectories run at OFF_LN."""
    c = Case(Nx=8, likelihood=2, **OFF)
    dX = np.linspace(-0.99, 2.0, c.p.N)
    pl = c.oracle.partial_f_delta_x_log_like(dX)
    with np.errstate(invalid="ignore"):
        pln = _np(c).partial_f(dX.reshape((8,) * 3)).ravel()
    bad = 1 + OFF["biasP"] * dX < 0
    assert bad.any() and np.all(np.isnan(pl[bad])) and np.all(np.isnan(pln[bad]))
    assert np.all(np.isfinite(pl[~bad])) and rel_l2(pl[~bad], pln[~bad]) < 1e-14
    c2 = Case(Nx=8, likelihood=2, **OFF_LN)
    assert np.all(np.isfinite(c2.oracle.partial_f_delta_x_log_like(dX)))


# ---- force against finite differences off default -------------------------------------------------------------------
def exact_partial_data(p, dX, window, nobs):
    """nobs' for which the reference's partial, times the rho_c that likelihood_calc_V_SPH multiplies in, IS minus the
    derivative of the cell's -log L term (with the data nobs) by delta_x.  See test_force_is_gradient_of_energy_off_default."""
    dens = 1 + p.biasP * dX
    if p.likelihood == 1:
        lam = window * p.rho_c * dens ** p.biasE
        return lam + (nobs - lam) * window * p.biasE * p.biasP * dens ** (p.biasE - 1)
    if p.likelihood == 0:
        lam = window * p.rho_c * dens ** p.biasE
        return lam * (1 - (1 - nobs / lam) / p.rho_c)
    lam_b = np.log(p.rho_c * dens ** p.biasE)
    lam_c = np.log(p.rho_c * (1 + np.maximum(dX, p.delta_min)))
    return lam_b + (nobs - lam_c) * (dX > p.delta_min) / ((1 + dX) * p.rho_c)


@pytest.mark.parametrize("kw", [dict(likelihood=1), dict(likelihood=1, rsd_model=1), dict(likelihood=0),
                                dict(likelihood=2), dict(likelihood=1, correct_delta=0)],
                         ids=["gauss", "gauss_rsd", "poisson", "lognormal", "gauss_nocorr"])
def test_force_is_gradient_of_energy_off_default(kw):
    """tests/test_oracle_cpu.py::test_force_is_gradient_of_energy with every scalar off its default, same margins.

    Off default the reference's force is no longer the gradient of its own energy, cell by cell.  With
    dens = 1 + biasP delta_x, the derivative of a cell's -log L term by delta_x and what the reference puts in its place
    (the partial, times normalize = rho_c L^3 / N of likelihood_calc_V_SPH, HMC_models.cc:224, where the chain rule has
    1 / mean(rho) = L^3 / N) are
      Gaussian     (Lambda - nobs) / sigma^2 * dLambda/ddelta, dLambda/ddelta = w rho_c biasE biasP dens^(biasE - 1);
                   the partial (gaussian_independent.cpp:33-38) carries no dLambda/ddelta and normalize supplies rho_c:
                   force / gradient = 1 / (w biasE biasP dens^(biasE - 1)) per cell;
      Poissonian   (1 - nobs / Lambda) dLambda/ddelta; the partial (poissonian.cpp:30) has all of it and normalize
                   supplies rho_c once more: force / gradient = -rho_c (the sign is the quirk the default test pins);
      log-normal   the energy takes Lambda_c = log(rho_c (1 + max(delta_x, delta_min))) without bias
                   (lognormal_independent.cpp:57-64) and the partial Lambda_b = log(rho_c dens^biasE) (:49):
                   force / gradient = rho_c (nobs - Lambda_b) (1 + delta_x) / (nobs - Lambda_c) per cell.
    The per-cell factors are taken out through the data: the force is evaluated with nobs' (exact_partial_data) for
    which rho_c times the partial equals the derivative above, and is then held against central differences of log_like
    with the data nobs.  What is left is the chain q -> Psi -> positions -> delta_x: D1 under correct_delta (without it
    the force is 1 / D1 too large, asserted for that case), rho_c of normalize, 1 + f1 under RSD.  A missing or doubled
    one is off by O(1)."""
    c = Case(Nx=8, **kw, **scalars_for(kw))
    o, p = c.oracle, c.p
    q = 0.3 * c.q0.ravel()  # gentle field: no shell crossing pile-ups
    dX = o.Lag2Eul(q, rsd=p.rsd_model if p.likelihood == 1 else 0)[0]
    assert dX.min() > p.delta_min and (1 + p.biasP * dX).min() > 0
    o.set(nobs=exact_partial_data(p, dX, c.window.ravel(), c.nobs.ravel()))
    gl = o.likelihood_grad_log_like(q)
    o.set(nobs=c.nobs)
    if not p.correct_delta:
        gl = gl * p.D1
    idx = np.argsort(-np.abs(gl))[:6]
    hstep = 1e-5
    for i in idx:
        e = np.zeros_like(q)
        e[i] = hstep
        fd = (o.log_like(q + e) - o.log_like(q - e)) / (2 * hstep)
        if p.likelihood == 0:
            fd = -fd
        tol = 0.3 if p.likelihood == 2 else 0.05
        assert abs(fd - gl[i]) <= tol * abs(gl[i]) + 1e-6, (i, fd, gl[i])


# ---- each scalar is observable --------------------------------------------------------------------------------------
OBSERVE_CASES = ("zeld_rsd", "alpt", "poisson", "lognormal", "calch0_lognormal")


def _observed(kw, s):
    """The quantities of one force evaluation and of psi that tests/test_gpu_offdefault.py compares, from the oracle."""
    c = Case(Nx=16, **kw, **s)
    o = c.oracle
    g, gp, gl = o.gradient_psi(c.q0)
    dX = o.get("deltaX")
    out = dict(posz=o.get("posz"), deltaX=dX, part_like=o.partial_f_delta_x_log_like(dX), grad_like=gl,
               psi_likeli=np.array([o.psi(c.q0)[1]]))
    o.close()
    return out


TOL_OF = dict(posz=TOL_FIELD, deltaX=TOL_FIELD, part_like=10 * TOL_FIELD, grad_like=10 * TOL_FIELD, psi_likeli=TOL_ENERGY)


def test_each_scalar_is_observable():
    """For every scalar of OFF: the oracle at OFF against the oracle at OFF with that one scalar back at its default
    (D2: at the value derived from D1).  In at least one case of the GPU comparison at least one compared quantity must
    move by >= 1e3 times its tolerance, else the GPU test would not notice an engine that ignores the scalar.  The same
    data (made at OFF) are used on both sides.  xobs / yobs / zobs are not read on this path and are not tested."""
    rows = []
    base = {}
    for name in OBSERVE_CASES:
        kw = od.INTERMEDIATE[name]
        base[name] = _observed(kw, scalars_for(kw))
    for scalar in od.SCALARS:
        best = (0.0, None, None)
        for name in OBSERVE_CASES:
            kw = od.INTERMEDIATE[name]
            full = scalars_for(kw)
            c_off = Case(Nx=16, **kw, **full)
            p2 = dataclasses.replace(c_off.p, **{scalar: od.with_default(full, scalar)[scalar]})
            o = orc.Oracle(p2)
            o.set(**c_off.arrays())
            g, gp, gl = o.gradient_psi(c_off.q0)
            dX = o.get("deltaX")
            got = dict(posz=o.get("posz"), deltaX=dX, part_like=o.partial_f_delta_x_log_like(dX), grad_like=gl,
                       psi_likeli=np.array([o.psi(c_off.q0)[1]]))
            o.close()
            for k, tol in TOL_OF.items():
                a, b = got[k], base[name][k]
                ok = np.isfinite(a) & np.isfinite(b)
                ratio = rel_l2(a[ok], b[ok]) / tol
                if ratio > best[0]:
                    best = (ratio, name, k)
        rows.append((scalar,) + best)
    print("scalar      case               quantity     change / tolerance")
    for scalar, ratio, name, k in rows:
        print("%-11s %-18s %-12s %.1e" % (scalar, name, k, ratio))
    for scalar, ratio, name, k in rows:
        assert ratio >= 1e3, (scalar, ratio)


def test_D2_and_delta_min_need_their_cases():
    """What the issue predicts: D2 is invisible without ALPT, delta_min without a log-normal energy or calc_h = 0."""
    for scalar, blind, seeing in (("D2", "zeld_rsd", "alpt"), ("delta_min", "zeld_rsd", "calch0_lognormal")):
        for name, visible in ((blind, False), (seeing, True)):
            kw = od.INTERMEDIATE[name]
            full = scalars_for(kw)
            c = Case(Nx=16, **kw, **full)
            o = orc.Oracle(dataclasses.replace(c.p, **{scalar: od.with_default(full, scalar)[scalar]}))
            o.set(**c.arrays())
            moved = rel_l2(o.gradient_psi(c.q0)[2], c.oracle.gradient_psi(c.q0)[2])
            assert (moved > 1e-6) if visible else (moved == 0), (scalar, name, moved)
            o.close()


# ---- per-cell likelihood formulas -----------------------------------------------------------------------------------
def density_sets(n=16):
    """rho of the four sets, from the oracle's SPH assignment (h = d) at the suite's geometry."""
    p = HamilParams(Nx=n, L=200.0 * n / 64.0)
    geo = ref.Geometry(n, p.L)
    o = orc.Oracle(p)
    sets = ref.position_sets(geo, np.float64, names=lb.DENSITY_SETS)
    out = {name: o.getDensity(3, *ref.positions(sets[name], geo, 0, np.float64)) for name in lb.DENSITY_SETS}
    o.close()
    return out


@pytest.fixture(scope="module")
def rho_sets():
    return density_sets()


def _scalars(bP, bE):
    return lb.Scalars(OFF["rho_c"], bP, bE, OFF["delta_min"])


def _evaluate(lik, s, rho, fp32, mutant=None):
    r = rho.astype(np.float32).astype(np.float64) if fp32 else rho
    dX = lb.overdens_ld(r)
    w, nobs, noise = lb.data_for(lik, s, np.asarray(dX, dtype=np.float64))
    if fp32:
        nobs = nobs.astype(np.float32).astype(np.float64)
    out, der = lb.partial_ld(lik, s, dX, w, nobs, noise)
    got = lb.partial_f64(lik, s, r, w, nobs, noise, mutant)
    if fp32:
        got = got.astype(np.float32).astype(np.float64)
    return dX, w, nobs, noise, out, der, got


def test_the_density_sets_reach_the_edges(rho_sets):
    """delta = -1 exactly, cells just above empty, cells hundreds of times the mean; no cell on a branch edge."""
    assert (rho_sets["collapse_inside"] == 0).sum() > 3000 and rho_sets["collapse_inside"].max() > 500 * rho_sets["collapse_inside"].mean()
    r = rho_sets["collapse_inside"]
    assert 0 < r[r > 0].min() < 1e-6 * r.mean()
    assert (rho_sets["sheet"] == 0).any() and (rho_sets["filament"] == 0).any() and not (rho_sets["uniform"] == 0).any()
    excluded = 0
    for rho in rho_sets.values():
        for fp32 in (False, True):
            for bP, bE in lb.BIAS_PAIRS + (lb.BIAS_EVEN,):
                for lik in (0, 1, 2):
                    dX, w = _evaluate(lik, _scalars(bP, bE), rho, fp32)[:2]
                    excluded += int(lb.edge_cells(lik, _scalars(bP, bE), dX, w).sum())
    assert excluded == 0


def test_likelihood_bound_constant_is_the_measured_one(rho_sets):
    """The float64 restatements of partial_like_value and of k_loglike's per-cell term against the longdouble formulas
    on every set, bias pair, likelihood and storage type: the worst fraction of the bound at C = 1 must not exceed
    like_bound.MEASURED (partial 5.0 for fp64 input, 0.99 for fp32 where the storage rounding dominates; -log L 4.31),
    C is four times that, and every non-finite cell of the reference is the same non-finite class."""
    worst = {"partial": 0.0, "partial_fp32": 0.0, "nll": 0.0}
    nonfinite = 0
    for name, rho in rho_sets.items():
        for fp32 in (False, True):
            for bP, bE in lb.BIAS_PAIRS + (lb.BIAS_EVEN,):
                s = _scalars(bP, bE)
                for lik in (0, 1, 2):
                    dX, w, nobs, noise, out, der, got = _evaluate(lik, s, rho, fp32)
                    nonfinite += int((~np.isfinite(out)).sum())
                    f, _ = lb.worst_fraction(got, out, lb.bound(out, der, dX, "partial", fp32, c=1))
                    key = "partial_fp32" if fp32 else "partial"
                    worst[key] = max(worst[key], f)
                    r = rho.astype(np.float32).astype(np.float64) if fp32 else rho
                    o2, d2 = lb.nll_ld(lik, s, dX, w, nobs, noise)
                    f2, _ = lb.worst_fraction(lb.nll_f64(lik, s, r, w, nobs, noise), o2, lb.bound(o2, d2, dX, "nll", c=1))
                    worst["nll"] = max(worst["nll"], f2)
                    # and the sum the engine's psi[1] is held to
                    assert abs(float(np.sum(lb.nll_f64(lik, s, r, w, nobs, noise)) / float(o2.sum())) - 1) < TOL_ENERGY
    print("likelihood bound, worst fraction at C = 1:", worst, "non-finite reference cells:", nonfinite)
    assert nonfinite > 1000                      # the log-normal's NaN (biasP = 1.3) and +inf (biasP = 1) classes occur
    assert worst["partial"] <= lb.MEASURED["partial"] and worst["partial_fp32"] <= lb.MEASURED["partial"]
    assert worst["nll"] <= lb.MEASURED["nll"]
    assert worst["partial"] > 0.5 * lb.MEASURED["partial"] and worst["nll"] > 0.5 * lb.MEASURED["nll"]
    assert lb.C == {k: 4 * v for k, v in lb.MEASURED.items()}


MUTANT_RUNS = {   # mutant -> (likelihoods it changes, (biasP, biasE))
    "bias_swapped": ((0, 1, 2), (1.3, 0.8)),
    "pow_biasE_in_derivative": ((0,), (1.3, 0.8)),
    "rho_c_dropped": ((0, 1, 2), (1.3, 0.8)),
    "clamp_in_partial": ((0, 1, 2), (0.8, 1.5)),
    "dens_test_for_gaussian": ((1,), lb.BIAS_EVEN),
}


@pytest.mark.parametrize("mutant", lb.MUTANTS)
@pytest.mark.parametrize("fp32", (False, True), ids=("fp64", "fp32"))
def test_the_checker_rejects_wrong_kernels(rho_sets, mutant, fp32):
    """Each mutant of partial_like_value is rejected, for every likelihood it changes, on the set where the GPU test
    would meet it (collapse_inside: empty cells, cells below delta_min, cells far above the mean); the correct
    restatement passes the same check.  "Lambda > 0" and "dens > 0" decide alike unless biasE is an even integer (dens < 0
    then has Lambda > 0): that mutant is shown at biasE = 2, which the GPU test runs for this reason."""
    liks, (bP, bE) = MUTANT_RUNS[mutant]
    s = _scalars(bP, bE)
    rho = rho_sets["collapse_inside"]
    for lik in liks:
        dX, w, nobs, noise, out, der, good = _evaluate(lik, s, rho, fp32)
        bnd = lb.bound(out, der, dX, "partial", fp32)
        assert lb.worst_fraction(good, out, bnd)[0] <= 1
        bad = _evaluate(lik, s, rho, fp32, mutant)[6]
        f, i = lb.worst_fraction(bad, out, bnd)
        assert f > 1e3, (mutant, lik, f, i)
        # the one fitted scalar of the default fp32 handle (like_bound.fit_mean_shift) does not rescue a wrong kernel
        r = rho.astype(np.float32).astype(np.float64) if fp32 else rho
        shift = lb.fit_mean_shift(lik, s, r, w, nobs, noise, bad, fp32)
        dXs = lb.overdens_ld(r, shift)
        outs, ders = lb.partial_ld(lik, s, dXs, w, nobs, noise)
        assert lb.worst_fraction(bad, outs, lb.bound(outs, ders, dXs, "partial", fp32))[0] > 1e3, (mutant, lik, shift)


@pytest.mark.parametrize("lik", (0, 1, 2))
def test_the_fitted_mean_shift_is_the_injected_one(rho_sets, lik):
    """A float64 evaluation whose mean is 1.7e-10 off the mean of the stored rho (what the default fp32 handle does)
    misses the bound taken with the stored mean, and meets it once the shift is fitted; the fit returns the shift."""
    s = _scalars(1.0, 0.8)
    rho = rho_sets["uniform"].astype(np.float32).astype(np.float64)
    inject = 1.7e-10
    dX = np.asarray(lb.overdens_ld(rho), dtype=np.float64)
    w, nobs, noise = lb.data_for(lik, s, dX)
    nobs = nobs.astype(np.float32).astype(np.float64)
    got = lb.partial_f64(lik, s, rho, w, nobs, noise, mean_shift=inject).astype(np.float32).astype(np.float64)
    dX0 = lb.overdens_ld(rho)
    out0, der0 = lb.partial_ld(lik, s, dX0, w, nobs, noise)
    assert lb.worst_fraction(got, out0, lb.bound(out0, der0, dX0, "partial", True))[0] > 1
    shift = lb.fit_mean_shift(lik, s, rho, w, nobs, noise, got, True)
    assert shift == pytest.approx(inject, rel=0.05)
    dX1 = lb.overdens_ld(rho, shift)
    out1, der1 = lb.partial_ld(lik, s, dX1, w, nobs, noise)
    assert lb.worst_fraction(got, out1, lb.bound(out1, der1, dX1, "partial", True))[0] <= 1
    geo = ref.Geometry(16, 50.0)
    pos = ref.positions(ref.position_sets(geo, np.float32, names=("uniform",))["uniform"], geo, 0, np.float32)
    cnt = ref.sph_density([a.astype(np.float64) for a in pos], geo, geo.d, 0.0, np.float32)[1]
    assert 1e-7 < lb.mean_shift_limit(rho, cnt, True) < 1e-5


# ---- input_par: the growth factors ----------------------------------------------------------------------------------
def _growth_second_opinion(a, OM, OL, panels=1 << 16):
    """D1 = E(a) I(a) / I(1), I(a) = int_0^a da' / (a' E(a'))^3, by composite Simpson in the variable s = a'^(1/4) (the
    integrand 4 s^9 / (OM + OK s^4 + OL s^12)^(3/2) is smooth) -- another rule, substitution and node count than
    input_par.growth_integral (one 64-node Gauss-Legendre rule in sqrt(a'))."""
    OK = 1.0 - OM - OL

    def integral(top):
        s = np.linspace(0.0, top ** 0.25, 2 * panels + 1)
        f = 4 * s ** 9 / (OM + OK * s ** 4 + OL * s ** 12) ** 1.5
        return (s[1] - s[0]) / 3 * (f[0] + f[-1] + 4 * f[1:-1:2].sum() + 2 * f[2:-1:2].sum())

    return np.sqrt(OM / a ** 3 + OK / a ** 2 + OL) * integral(a) / integral(1.0)


def test_growth_factor_definitions():
    """D1 = E(a) I(z) / I(0), I(z) = int_z^inf (1 + z') / E(z')^3 dz' (cosmo.cc:68-82, 124-176, init_par.cc:519-528).
    Pinned to the integral, not to a GSL build (the reference integrates at epsrel = 1e-8)."""
    for OM, OL in ((0.272, 0.728), (0.3, 0.6), (1.0, 0.0), (0.3, 0.0), (0.4, 0.9)):
        assert input_par.growth_factor(1.0, OM, OL) == pytest.approx(1.0, abs=1e-15)
    for a in (0.9, 0.5, 0.2, 0.05):
        assert input_par.growth_factor(a, 1.0, 0.0) == pytest.approx(a, rel=1e-12)   # Einstein-de Sitter: D1 = a
    got = input_par.growth_factor(0.5, 0.272, 0.728)                                    # WMAP7, z = 1
    assert got == pytest.approx(_growth_second_opinion(0.5, 0.272, 0.728), rel=1e-10)
    assert 0.60 < got < 0.64   # LCDM grows slower than EdS (0.5) towards late times: D1(z = 1) = 0.622
    for a, OM, OL in ((0.5, 0.3, 0.6), (0.25, 0.3, 0.0), (0.7, 0.4, 0.9)):
        assert input_par.growth_factor(a, OM, OL) == pytest.approx(_growth_second_opinion(a, OM, OL), rel=1e-10)
    # the rule has converged: twice the nodes change nothing
    assert input_par.growth_integral(0.5, 0.272, 0.728, 128) == pytest.approx(input_par.growth_integral(0.5, 0.272, 0.728), rel=1e-14)


def test_hamil_params_computes_the_growth_factors_from_z(tmp_path):
    template = os.path.join(GOLDEN_DIR, "reference_template_input.par")
    p0 = input_par.hamil_params(template)
    assert p0.ascale == 1.0 and p0.D1 == 1.0 and p0.D2 == HamilParams().D2      # z = 0: as before
    text = open(template).read()
    lines = [("z = 1.0  # redshift" if ln.split("=")[0].strip() == "z" else ln) for ln in text.splitlines()]
    assert lines != text.splitlines()
    par = tmp_path / "input.par"
    par.write_text("\n".join(lines) + "\n")
    p = input_par.hamil_params(str(par))
    assert p.ascale == 0.5
    assert p.D1 == input_par.growth_factor(0.5, p.OM, p.OL) == pytest.approx(0.6220391565627, rel=1e-12)
    E2 = p.OM / 0.125 + p.OL + (1 - p.OM - p.OL) / 0.25
    omega = p.OM / (E2 * 0.125)
    assert p.D2 == pytest.approx(-3.0 / 7.0 * p.D1 ** 2 * omega ** (-1.0 / 143.0), rel=1e-15)
    # an explicit D1 (and cosmology) still wins
    assert input_par.hamil_params(str(par), D1=0.7).D1 == 0.7
    assert input_par.hamil_params(str(par), OM=1.0, OL=0.0).D1 == pytest.approx(0.5, rel=1e-12)


# ---- the probed step sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(od.TRAJ))
def test_trajectory_cases_are_well_conditioned_and_finite(name):
    """Re-measures what tests/offdefault.TRAJ records: over the ten steps at 16^3 a 1e-13 perturbation of q0 grows by the
    recorded factor (< 100 for every case; held to within a factor 3 of the record, the direction of the perturbation
    being one draw), and trajectory and energies stay finite in the oracle."""
    kw, eps_scale, recorded = od.TRAJ[name]
    assert recorded < 100 and eps_scale <= Case.EPS_SCALE[kw["likelihood"]]
    c = od.traj_case(name)
    rng = np.random.default_rng(5)
    q0 = c.q0.ravel()
    dq = rng.standard_normal(q0.size)
    dq *= 1e-13 * np.linalg.norm(q0) / np.linalg.norm(dq)
    a = c.oracle.Hamiltonian_EoM(q0, c.p0, c.eps, 10)
    b = c.oracle.Hamiltonian_EoM(q0 + dq, c.p0, c.eps, 10)
    amp = max(rel_l2(b[0], a[0]), rel_l2(b[1], a[1])) / 1e-13
    dH, terms = c.oracle.delta_Hamiltonian(q0, c.p0, a[0], a[1])
    print("%s: eps_scale %g, amplification %.3g (recorded %.3g)" % (name, eps_scale, amp, recorded))
    assert a[2] == 10 and np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1])) and np.all(np.isfinite(terms))
    assert amp < 3 * recorded
