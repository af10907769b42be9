"""BASELINE config 3's model at 512^3 with fp64 fields, end to end against the OpenMP oracle.

Only here do the fp64 512^3 instantiations run inside the engine: k_step_boundary_x<double, 512, 8> on the interior
boundary, k_ypass<double, 512, 8> inverse, k_zbin_direct<double, 512> and <double, 512, true> with their 53 KB of LDS
(above 48 KiB: launch_dyn_lds of pass_launch.hpp raises the kernel's limit first), and with BCHMC_YFWD_F64=1 k_zr2c<double, 512> +
k_ypass<double, 512, 8, _, false>.  Component 2 of Ck starts 2.2 GB into the array at this size.

A module of its own: the fp64 record array alone is about 69 GB at create, so test_gpu_large.py's fp32 512^3 engine must
never be alive at the same time; one engine is open at a time here as well.  The oracle's 2-step trajectory (one
interior boundary), its energies, gradient and density are computed once; each engine path is compared with them,
not only with the other paths:
  default, BCHMC_YFWD_F64=1, BCHMC_SORT_CAP pinned low (k_zbin_direct<double, 512, true> hands Psi to the fallback
  sort on every evaluation), BCHMC_NO_ZBIN=1 (rocFFT's 2-D C2R + k_bin_direct).
Wall time of the module on one MI355X: 134 s, of which 112 s are the oracle's (16 host threads) and 4 x 3-8 s the
engine paths.
"""
import numpy as np
import pytest

from barcode_amd import inputs
from barcode_amd.params import HamilParams
from tests.util import TOL_ENERGY, TOL_TRAJ_10, rel_l2

pytestmark = pytest.mark.gpu

PATHS = {
    "default": {},
    "yfwd_f64": dict(BCHMC_YFWD_F64="1"),
    "sort_cap_pinned": dict(BCHMC_SORT_CAP="4096", BCHMC_SORT_CAP_FIXED="1"),
    "no_zbin": dict(BCHMC_NO_ZBIN="1"),
}
ENV_KEYS = ("BCHMC_YFWD_F64", "BCHMC_SORT_CAP", "BCHMC_SORT_CAP_FIXED", "BCHMC_NO_ZBIN")


@pytest.fixture(scope="module")
def ref512():
    """Inputs and the oracle's answers: 2-step trajectory, delta_Hamiltonian terms, gradient(q0), deltaX(q0)."""
    from oracle.oracle import Oracle
    p = HamilParams(Nx=512, L=200.0, likelihood=1, rsd_model=1, sfmodel=2)
    f = inputs.make_fields(p)
    o = Oracle(p, omp=True)
    o.set(signal_PS=f["signal_PS"], mass_f=f["mass_f"])
    dX = o.Lag2Eul(f["truth"], rsd=1)[0]
    window, noise, nobs = inputs.mock_observations(p, dX.reshape((p.Nx,) * 3))
    del dX
    o.set(window=window, noise=noise, nobs=nobs)
    eps = 0.5 * p.eps_heuristic()
    q1o, p1o, done_o = o.Hamiltonian_EoM(f["q0"], f["p0"], eps, 2)
    assert done_o == 2
    _, terms_o = o.delta_Hamiltonian(f["q0"], f["p0"], q1o, p1o)
    g_o = o.gradient_psi(f["q0"])[0]
    dX_o = o.get("deltaX")
    o.close()
    obs = dict(signal_PS=f["signal_PS"], mass_f=f["mass_f"], window=window, noise=noise, nobs=nobs)
    yield dict(p=p, q0=f["q0"], p0=f["p0"], eps=eps, obs=obs, q1=q1o, p1=p1o, terms=terms_o, g=g_o, dX=dX_o)


@pytest.fixture(scope="module")
def profiles():
    """profile_read of each path's trajectory, for the path checks at the end."""
    return {}


@pytest.mark.parametrize("path", list(PATHS))
def test_512_fp64_path_against_oracle(ref512, profiles, monkeypatch, path):
    from barcode_amd.engine import Engine
    r = ref512
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    e = Engine(r["p"], precision=0)
    try:
        e.upload(**r["obs"])
        e.profile(True)
        q1, p1, done = e.leapfrog(r["q0"], r["p0"], r["eps"], 2)
        profiles[path] = e.profile_read()
        e.profile(False)
        assert done == 2
        rq, rp = rel_l2(q1, r["q1"]), rel_l2(p1, r["p1"])
        del q1, p1
        _, t = e.delta_hamiltonian(r["q0"], r["p0"], r["q1"], r["p1"])
        g = e.gradient(r["q0"])
        rg = rel_l2(g, r["g"])
        del g
        rx = rel_l2(e.fetch("deltaX"), r["dX"])
    finally:
        e.close()
    re = float(np.max(np.abs(t - r["terms"]) / np.abs(r["terms"])))
    print("\n512^3 fp64 %s: rel-L2 q1 %.2e p1 %.2e, energies %.2e, gradient %.2e, deltaX %.2e" % (path, rq, rp, re, rg, rx))
    assert rq < TOL_TRAJ_10 and rp < TOL_TRAJ_10
    assert np.all(np.abs(t - r["terms"]) <= TOL_ENERGY * np.abs(r["terms"]))
    assert rg < 1e-11
    assert rx < 1e-12


def test_512_fp64_paths_ran(profiles):
    """The settings changed what ran (same launches per class, time moved between classes):
    - pinned record slots: every evaluation overflows and the two-pass fallback sort works inside the sort class
      (measured 21.0 against 9.5 ms per trajectory);
    - BCHMC_NO_ZBIN: the z pass is back in rocFFT's C2R, so the C2R class holds a larger share of C2R + sort
      (C2R 10.6 / sort 7.4 ms against 6.9 / 9.5 ms).
    BCHMC_YFWD_F64 leaves no such trace: in fp64 k_zr2c + k_ypass<forward> take what rocFFT's 2-D R2C takes."""
    if len(profiles) < len(PATHS):
        pytest.fail("the path tests did not all run before this one: %s" % sorted(profiles))
    ms = {k: {c: v[0] for c, v in prof.items()} for k, prof in profiles.items()}
    for k in PATHS:
        print("\n%s: %s" % (k, " ".join("%s %.2f ms / %d" % (c, v[0], v[1]) for c, v in profiles[k].items() if v[1])))
    sort_cls, c2r_cls = "k_bin+k_scan_tiles+k_reorder", "rocfft_c2r"  # BCHMC_K_SORT, BCHMC_K_FFT_C2R
    assert ms["sort_cap_pinned"][sort_cls] > 1.5 * ms["default"][sort_cls]

    def c2r_share(k):
        return ms[k][c2r_cls] / (ms[k][c2r_cls] + ms[k][sort_cls])
    assert c2r_share("no_zbin") > c2r_share("default") + 0.1
