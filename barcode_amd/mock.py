"""The start of a run: ``load_initial_fields`` (barlib/src/barcoderunner.cc:284-344) on the device.

``setup_random_test`` (:42-205) and ``make_initial_guess`` (:207-247) draw from the same ``GslMT19937`` the chain later
takes its momenta, Neps, epsilon and Metropolis uniforms from (``hamil.HamiltonianMC(momenta="mt19937")``), so a run
that starts from ``seed`` sees the arrays an upstream run seeded alike sees.  The Poissonian mock (``data_model`` 0 under
``likelihood`` 0) has no such form: ``gsl_ran_poisson`` consumes a data-dependent number of words per cell.  With
``MockParams.poisson_seed`` set it is drawn by the engine's counter-based sampler instead
(``Engine.setup_random_test_poisson``: truth, forward model and window still from ``rng``, nobs exact in distribution but
not upstream's stream); with ``None``, the default, it is refused as before (``BchmcError`` code 5).
"""
import os
from dataclasses import dataclass
from typing import Optional

from . import io


@dataclass
class MockParams:
    """The scalars of upstream's NUMERICAL / OBSERVATIONAL this stage reads (``input_par.mock_params`` fills them from
    an input.par); ``dir`` is NUMERICAL::dir, the directory of the dumps ('' = no files are written or read)."""
    seed: int = 1
    random_test: bool = True
    random_test_rsd: bool = False
    window_type: int = 1
    data_model: int = 0
    negative_obs: bool = False
    sigma_min: float = 1.0
    sigma_fac: float = 0.0
    initial_guess: int = 0
    initial_guess_file: str = ""
    initial_guess_smoothing_type: int = 1
    initial_guess_smoothing_scale: float = 0.0
    N_bin: int = 200
    likelihood: int = 1
    dir: str = ""
    poisson_seed: Optional[int] = None   # not upstream's: seed of the counter-based Poissonian mock (None: not drawn)


def setup_random_test(hd, rng, mock):
    """barcoderunner.cc:42-205: truth, forward model, window, nobs, noise_sf on the device; the engine of ``hd`` holds
    the three arrays afterwards as if they had been uploaded.  With ``mock.dir`` the dumps upstream writes
    (deltaLAGtest / deltaEULtest via dump_deltas, win, nobs, sigma).  Returns (delta_lag, delta_eul)."""
    e = hd.engine
    if mock.poisson_seed is not None and mock.likelihood == 0:
        _, dl, de = e.setup_random_test_poisson(rng, mock.poisson_seed, window_type=mock.window_type,
                                                random_test_rsd=mock.random_test_rsd)
    else:
        _, dl, de = e.setup_random_test(rng, window_type=mock.window_type, data_model=mock.data_model,
                                        negative_obs=mock.negative_obs, random_test_rsd=mock.random_test_rsd,
                                        sigma_min=mock.sigma_min, sigma_fac=mock.sigma_fac)
    if mock.dir:
        io.write_array(os.path.join(mock.dir, "deltaLAGtest"), dl)
        io.write_array(os.path.join(mock.dir, "deltaEULtest"), de)
        for name, field in (("win", "window"), ("nobs", "nobs"), ("sigma", "noise")):
            io.write_array(os.path.join(mock.dir, name), e.fetch(field))
    return dl, de


def make_initial_guess(hd, rng, mock):
    """barcoderunner.cc:207-247: sets the resident chain state of ``hd``; returns the words drawn from ``rng``."""
    ff = None
    if mock.initial_guess == 1:
        ff = io.read_array(os.path.join(mock.dir, mock.initial_guess_file), hd.engine.N)
    return hd.engine.make_initial_guess(rng, mock.initial_guess, file_field=ff,
                                        smoothing_type=mock.initial_guess_smoothing_type,
                                        smoothing_scale=mock.initial_guess_smoothing_scale)


def load_initial_fields(hd, rng, mock):
    """barcoderunner.cc:308-330 (a fresh run; the restart branch is the caller's): the random test, or win / nobs /
    sigma read from ``mock.dir``; then the initial guess, its dump and ``spec_initial_guess.dat``."""
    e = hd.engine
    if mock.random_test:
        setup_random_test(hd, rng, mock)
    else:
        e.upload(window=io.read_array(os.path.join(mock.dir, "win"), e.N),
                 nobs=io.read_array(os.path.join(mock.dir, "nobs"), e.N),
                 noise=io.read_array(os.path.join(mock.dir, "sigma"), e.N))
    make_initial_guess(hd, rng, mock)
    if mock.dir:
        io.write_array(os.path.join(mock.dir, "initial_guess"), e.chain_get_state())
        kmode, power = e.measure_spectrum(None, mock.N_bin)
        io.dump_measured_spec(kmode, power, os.path.join(mock.dir, "spec_initial_guess.dat"))
