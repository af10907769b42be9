"""CPU checks of the Hamiltonian_mass restatement (tests/mass_restatement.py) that the GPU tests compare the engine
with, and of hamil.HamiltonianMC's massnum schedule (HMC.cc:387-400)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from barcode_amd.hamil import massnum_due
from tests import mass_restatement as mr
from tests.util import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,kw", [(8, dict(rsd_model=1)), (8, dict(sfmodel=2)), (16, dict(rsd_model=1))],
                         ids=["rsd_8", "alpt_8", "rsd_16"])
def test_jasche_literal_equals_the_convolution_form(n, kw):
    """Per-cell R2C / grad_inv_lap / C2R (upstream) == the G-convolution form the engine runs, with a window with zeros
    and h = 1.5 cells (reach 4: at 8^3 the stencil wraps the box)."""
    c = Case(Nx=n, likelihood=1, window_zero_fraction=0.3, particle_kernel_h_rel=1.5, mass_type=6, **kw)
    _, px, py, pz = c.oracle.Lag2Eul(c.q0)
    if n == 8:
        a = mr.jasche_literal(c.p, px, py, pz, c.window, c.noise)
        b = mr.jasche_convolution(c.p, px, py, pz, c.window, c.noise)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(a))
        assert np.all(a[c.window.ravel() == 0] == 0) and np.all(a[c.window.ravel() > 0] > 0)
    else:  # 16^3: the two forms of D_l for a sample of cells (the full convolution form is slow in numpy)
        G = mr.glap_impulse_fields(n, c.p.L)
        shape = (n, n, n)
        for l in np.random.default_rng(1).choice(c.p.N, 24, replace=False):
            wx, wy, wz, _ = mr.wprime_il(c.p, px, py, pz, l)
            Ck = sum(mr.grad_inv_lap_FS(n, c.p.L, np.fft.rfftn(w.reshape(shape)), j + 1)
                     for j, w in enumerate((wx, wy, wz)))
            lit = np.fft.irfftn(Ck, s=shape, axes=(0, 1, 2)).ravel()
            conv = mr.jasche_D_convolution(c.p, px, py, pz, l, G)
            assert np.max(np.abs(lit - conv)) <= 1e-12 * np.max(np.abs(lit))


def test_pacman_sign_quirk():
    """pacman.cpp:42-47: a difference beyond +L/2 becomes L - d (positive), one below -L/2 becomes L + d."""
    d = mr.pacman_difference(np.array([0.7, -0.7, 0.3, -0.3]), 1.0)
    assert np.allclose(d, [0.3, 0.3, 0.3, -0.3])


@pytest.mark.parametrize("n_bin", [200, 7])
def test_type2_restatement_equals_the_direct_loop(n_bin):
    """The vectorised type-2 restatement == a full-grid loop of HMC_mass.cc:53-83 / 127-142, corner rule included."""
    c = Case(Nx=8, likelihood=1, mass_type=2)
    kmode, power = mr.force_power(c.oracle, c.q0, n_bin)
    a = mr.likeli_force_mass(c.p, c.signal_PS, power)
    b = mr.likeli_force_mass_loop(c.p, c.signal_PS, power)
    assert np.array_equal(a, b)
    # the corner mode is the only cell whose bin index reaches N_bin, and it reads an empty bin
    bins = mr.force_bins(8, c.p.L, n_bin)
    corner = 4 + 8 * (4 + 8 * 4)
    assert bins[corner] == n_bin and np.count_nonzero(bins >= n_bin) == 1
    invP = mr.inv_ps(c.signal_PS)[corner]
    assert a[corner] == 2 * invP


def test_force_power_is_the_likelihood_force_before_its_test_factor():
    """likelihood_grad_log_like = gradient_psi's likelihood term / grad_psi_likeli_factor."""
    c = Case(Nx=8, likelihood=1, grad_psi_likeli_factor=2.0, deltaQ_factor=0.7)
    _, _, gl = c.oracle.gradient_psi(c.q0)
    f = c.oracle.likelihood_grad_log_like(c.q0)
    assert np.allclose(gl, 2.0 * f, rtol=1e-14, atol=1e-14 * np.abs(f).max())


# (iGibbs, massnum_init, massnum_burn) -> rebuild?  HMC.cc:387-400 with massnum == 0 meaning never
SCHEDULE = [((1, 0, 0), False), ((1, 1, 10), True), ((5, 1, 10), True), ((10, 2, 10), True), ((11, 2, 10), False),
            ((20, 2, 10), True), ((1, 3, 10), True), ((2, 3, 10), False), ((3, 3, 10), True), ((7, 0, 5), False),
            ((10, 0, 5), True), ((3, 0, 5), False), ((1, 0, 5), False), ((6, 4, 5), False), ((5, 4, 5), False)]


def test_massnum_schedule_follows_hmc_cc():
    for (iG, init, burn), want in SCHEDULE:
        massnum = burn if iG > burn else init
        upstream = massnum != 0 and (iG % massnum == 0 or iG == 1)
        assert upstream == want, (iG, init, burn)
        assert massnum_due(iG, init, burn) == want, (iG, init, burn)


def test_mass_opts_layout_matches_the_header():
    from barcode_amd.engine import MassOpts
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "bchmc.h"
    int main(void) {
      printf("%zu %zu %zu %zu\n", sizeof(bchmc_mass_opts), offsetof(bchmc_mass_opts, mass_factor),
             offsetof(bchmc_mass_opts, iGibbs), offsetof(bchmc_mass_opts, s_eps_total));
      return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        cfile, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(cfile, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    assert vals == [C.sizeof(MassOpts), MassOpts.mass_factor.offset, MassOpts.iGibbs.offset,
                    MassOpts.s_eps_total.offset]
