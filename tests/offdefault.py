"""The cosmology and observational scalars away from their defaults: the sets, the cases and the probed step sizes
that tests/test_offdefault_cpu.py (oracle, no GPU) and tests/test_gpu_offdefault.py (engine) share.

Every other test of the suite runs at D1 = 1, D2 derived from D1, ascale = 1, OM + OL = 1, rho_c = biasP = biasE = 1,
delta_min = -0.999, where a scalar that the engine forgets, applies twice or swaps with its neighbour changes nothing.
Two things hide at the defaults that putting one scalar off at a time would also miss, so all nine are off together:
at ascale = 1, E(a) = 1 for any OM, OL; and a D2 derived from D1 hides a swapped D1 / D2.

OFF      no scalar is 0, 1 or its default; OM + OL != 1 (curvature term of E(a) alive); ascale != 1; D2 is given and is
         not -3/7 D1^2 Omega^(-1/143) (= -0.1648 for these values); biasE is no integer, so every pow() is a real pow.
OFF_LN   the same with biasP <= 1 for log-normal trajectories: the reference's log-normal partial takes
         log(rho_c (1 + biasP delta)^biasE) without a guard (lognormal_independent.cpp:49), which is NaN wherever
         1 + biasP delta < 0; with biasP <= 1 the base stays positive wherever delta > -1.

xobs / yobs / zobs are not read on this path (plane-parallel RSD only; the oracle and the engine refuse planepar = 0),
so they are not part of the sets.
"""
DEFAULTS = dict(D1=1.0, D2=None, ascale=1.0, OM=0.272, OL=0.728, rho_c=1.0, biasP=1.0, biasE=1.0, delta_min=-0.999)
OFF = dict(D1=0.62, D2=-0.21, ascale=0.5, OM=0.3, OL=0.6, rho_c=1.7, biasP=1.3, biasE=0.8, delta_min=-0.5)
OFF_LN = dict(OFF, biasP=0.7)
SCALARS = tuple(OFF)


def scalars_for(kw):
    """The set a case runs at: OFF_LN for the log-normal likelihood, OFF otherwise."""
    return OFF_LN if kw.get("likelihood", 1) == 2 else OFF


def derived_D2(s):
    """init_par.cc:519-528: the D2 that HamilParams derives when none is given."""
    a = s["ascale"]
    omega = s["OM"] / (a ** 3 * (s["OM"] / a ** 3 + s["OL"] + (1.0 - s["OM"] - s["OL"]) / a ** 2))
    return -3.0 / 7.0 * s["D1"] ** 2 * omega ** (-1.0 / 143.0)


def with_default(s, name):
    """``s`` with the one scalar ``name`` put back to its default (D2: to the value derived from the set's D1)."""
    out = dict(s)
    out[name] = derived_D2(s) if name == "D2" else DEFAULTS[name]
    return out


# ---- one force evaluation: the cases whose intermediates the GPU test compares with the oracle ---------------------
# (ALPT additionally runs on the planes path at 32^3: the two forms of c_za, -D1 dq/N and dq/N.)
INTERMEDIATE = {
    "zeld":             dict(likelihood=1, rsd_model=0),
    "zeld_rsd":         dict(likelihood=1, rsd_model=1),
    "alpt":             dict(likelihood=1, rsd_model=0, sfmodel=2),
    "poisson_alpt":     dict(likelihood=0, rsd_model=0, sfmodel=2, kth=2.0),
    "calch0":           dict(likelihood=1, rsd_model=0, calc_h=0),
    "calch0_lognormal": dict(likelihood=2, rsd_model=0, calc_h=0),
    "calch1":           dict(likelihood=1, rsd_model=0, calc_h=1),
    "calch3_rsd":       dict(likelihood=1, rsd_model=1, calc_h=3),
    "ngp":              dict(likelihood=0, rsd_model=0, calc_h=1, mk=0),
    "cic":              dict(likelihood=1, rsd_model=0, calc_h=1, mk=1),
    "tsc":              dict(likelihood=1, rsd_model=1, calc_h=1, mk=2),
    "nocorr":           dict(likelihood=1, rsd_model=1, correct_delta=0),
    "poisson":          dict(likelihood=0, rsd_model=0),
    "lognormal":        dict(likelihood=2, rsd_model=0),
}


# ---- trajectory cases -------------------------------------------------------------------------------------------
# name -> (case keywords, eps_scale, amplification).  eps_scale is a fraction of the init_par.cc:259-261 heuristic,
# probed with the oracle at 16^3 as tests/util.Case describes: a 1e-13 relative perturbation of q0 must grow by less
# than 100x over the 10 steps, and the value is the largest of {Case.EPS_SCALE default, 0.03, 0.01, 0.003, 0.001} that
# qualifies.  amplification = rel-L2 change of (q1, p1) / 1e-13 measured at that value (tests/test_offdefault_cpu.py
# re-measures it for every case and holds it below 100).
TRAJ = {
    "gauss":        (dict(likelihood=1, rsd_model=0), 0.1, 0.51),
    "gauss_rsd":    (dict(likelihood=1, rsd_model=1), 0.1, 1.0),
    "poisson":      (dict(likelihood=0, rsd_model=0), 0.01, 98.0),     # 6e12 at the suite's 0.03
    "lognormal":    (dict(likelihood=2, rsd_model=0), 0.01, 0.42),
    "gauss_alpt":   (dict(likelihood=1, rsd_model=0, sfmodel=2), 0.1, 0.70),
    "poisson_alpt": (dict(likelihood=0, rsd_model=0, sfmodel=2, kth=2.0), 0.03, 29.0),
    "calch3_rsd":   (dict(likelihood=1, rsd_model=1, calc_h=3), 0.03, 0.55),   # 144 at the suite's 0.1
}

# The comparison of the two CPU restatements runs at 8^3 for three steps (tests/test_offdefault_cpu.py).  Probed the same
# way: every case qualifies at its Case.EPS_SCALE default; the largest amplifications over the three steps are 21
# (calc_h = 3 + RSD) and 6.9 (Poissonian), every other case stays below 1.
RESTATEMENT_CASES = {
    "gauss":            dict(likelihood=1, rsd_model=0),
    "gauss_rsd":        dict(likelihood=1, rsd_model=1),
    "poisson":          dict(likelihood=0, rsd_model=0),
    "lognormal":        dict(likelihood=2, rsd_model=0),
    "gauss_alpt":       dict(likelihood=1, rsd_model=0, sfmodel=2),
    "poisson_alpt":     dict(likelihood=0, rsd_model=0, sfmodel=2, kth=2.0),
    "gauss_calch0":     dict(likelihood=1, rsd_model=0, calc_h=0),
    "poisson_calch0":   dict(likelihood=0, rsd_model=0, calc_h=0),
    "lognormal_calch0": dict(likelihood=2, rsd_model=0, calc_h=0),
    "gauss_nocorr":     dict(likelihood=1, rsd_model=0, correct_delta=0),
    "calch3":           dict(likelihood=1, rsd_model=0, calc_h=3),
    "calch3_rsd":       dict(likelihood=1, rsd_model=1, calc_h=3),
}


def traj_case(name, Nx=16):
    """tests.util.Case of one TRAJ entry at its scalar set and probed step size."""
    from tests.util import Case
    kw, eps_scale, _ = TRAJ[name]
    return Case(Nx=Nx, eps_scale=eps_scale, **kw, **scalars_for(kw))


# ---- mock data (setup_random_test): (n, seed, HamilParams keywords, MockOpts keywords) as tests/mock_restatement.py ----
# Gaussian data model (rho_c in Lambda) and log-normal (rho_c and delta_min: 1033 of the 4096 cells lie below delta_min).
MOCK_CASES = [
    (16, 1, dict(OFF), dict()),
    (16, 1, dict(OFF, rsd_model=1), dict(random_test_rsd=True)),
    (16, 1, dict(OFF_LN, likelihood=2), dict(data_model=1, sigma_fac=0.1)),
]
