"""``input.par`` reader with the reference's parsing rules, and the mapping of its keys onto ``HamilParams``.

``parameter_inifile`` follows ``barlib/src/ini_reader.cpp:14-44`` + ``barlib/include/ini_reader.hpp:16-28``: every
white-space character is removed from a line first, lines that are empty or start with ``#`` are skipped, a trailing
``# comment`` is cut, the rest is split at the first ``=``; ``find`` converts with the semantics of
``std::stringstream >> std::boolalpha >> value``.  ``hamil_params`` reads the keys of the leapfrog path as
``INIT_PARAMS`` does (``barlib/src/init_par.cc:52-186, 293-334``).
"""
import numpy as np

from .params import HamilParams


class parameter_inifile:
    def __init__(self, filename):
        self.parameters = {}
        try:
            f = open(filename)
        except OSError:
            # the reference only prints "Couldn't open config file ..." and goes on with an empty map
            return
        with f:
            for line in f:
                line = "".join(ch for ch in line if not ch.isspace())
                if not line or line[0] == "#":
                    continue
                cut = line.find("#")
                if cut != -1:
                    line = line[:cut]
                pos = line.find("=")
                key = line[:pos] if pos != -1 else line
                value = line[pos + 1:] if pos != -1 else line  # substr(npos + 1) == substr(0) upstream
                self.parameters[key] = value

    def find(self, kind, key):
        """``params.find<T>(key)``: ``kind`` is ``bool``, ``int``, ``float`` or ``str``.  A missing key yields the
        value-initialised result of a failed stream extraction (``False`` / 0 / 0.0 / ``""``), as upstream."""
        text = self.parameters.get(key, "")
        if kind is str:
            return text
        if kind is bool:
            return text == "true"  # std::boolalpha accepts exactly "true" / "false"
        try:
            if kind is int:
                # operator>> for integers stops at the first character that cannot continue the number
                digits = ""
                for i, ch in enumerate(text):
                    if ch.isdigit() or (i == 0 and ch in "+-"):
                        digits += ch
                    else:
                        break
                return int(digits)
            return float(_leading_float(text))
        except ValueError:
            return kind()


def _leading_float(text):
    """Longest prefix strtod would accept (enough for input.par: digits, sign, point, exponent)."""
    best = ""
    for end in range(1, len(text) + 1):
        try:
            float(text[:end])
            best = text[:end]
        except ValueError:
            if text[:end][-1] not in "eE+-.":
                break
    if not best:
        raise ValueError(text)
    return best


def growth_integral(a, OM, OL, nodes=64):
    """``I(z) = int_z^inf (1 + z') / E(z')^3 dz'`` at ``z = 1/a - 1`` (``growth_var``, cosmo.cc:68-82, integrated by
    ``D_growth``, cosmo.cc:124-176).  With ``z' = 1/a' - 1`` the integral is ``int_0^a da' / (a' E(a'))^3`` and
    ``(a' E)^2 = OM / a' + OK + OL a'^2``; ``a' = t^2`` removes the square root at the origin and leaves the smooth
    ``int_0^sqrt(a) 2 t^4 / (OM + OK t^2 + OL t^6)^(3/2) dt``, done with one Gauss-Legendre rule."""
    OK = 1.0 - OM - OL
    x, w = np.polynomial.legendre.leggauss(nodes)
    top = np.sqrt(a)
    t = 0.5 * top * (x + 1.0)
    f = 2.0 * t ** 4 / (OM + OK * t ** 2 + OL * t ** 6) ** 1.5
    return float(0.5 * top * np.dot(w, f))


def growth_factor(a, OM, OL):
    """``D1 = D_growth(ascale)`` of init_par.cc:519-528: ``E(a) I(z) / I(0)`` (cosmo.cc:124-176), 1 at ``a = 1`` for
    any cosmology and ``a`` for Einstein-de Sitter.  Pinned to the integral, not to a GSL build: the reference
    integrates with ``gsl_integration_qagiu`` at ``epsrel = 1e-8``, so the ``D1`` a reference run prints can differ
    from this one at the 1e-8 level."""
    E = np.sqrt(OM / a ** 3 + (1.0 - OM - OL) / a ** 2 + OL)
    return float(E * growth_integral(a, OM, OL) / growth_integral(1.0, OM, OL))


def hamil_params(filename, **overrides):
    """HamilParams from an ``input.par`` (keys and meaning: init_par.cc:52-186, 293-334; cubic grid: Nx, Lx only).
    ``ascale = 1 / (1 + z)`` (init_par.cc:143) and, unless overridden, ``D1 = D_growth(ascale, OM, OL)``
    (``growth_factor``); ``D2 = -3/7 D1^2 Omega(a)^(-1/143)`` is then derived from that ``D1`` by ``HamilParams``."""
    p = parameter_inifile(filename)
    kw = dict(
        Nx=p.find(int, "Nx"), L=p.find(float, "Lx"),
        min1=p.find(float, "xllc"), min2=p.find(float, "yllc"), min3=p.find(float, "zllc"),
        xobs=p.find(float, "xobs"), yobs=p.find(float, "yobs"), zobs=p.find(float, "zobs"),
        planepar=int(p.find(bool, "planepar")), periodic=int(p.find(bool, "periodic")),
        mk=p.find(int, "masskernel"), calc_h=p.find(int, "calc_h"),
        likelihood=p.find(int, "likelihood"), prior=p.find(int, "prior"),
        sfmodel=p.find(int, "sfmodel"), kth=p.find(float, "slength"),
        rsd_model=int(p.find(bool, "rsd_model")), mass_type=p.find(int, "mass_type"),
        correct_delta=int(p.find(bool, "correct_delta")), div_dH_by_N=int(p.find(bool, "div_dH_by_N")),
        particle_kernel=p.find(int, "particle_kernel"), particle_kernel_h_rel=p.find(float, "particle_kernel_h_rel"),
        grad_psi_prior_factor=p.find(float, "grad_psi_prior_factor"),
        grad_psi_likeli_factor=p.find(float, "grad_psi_likeli_factor"),
        deltaQ_factor=p.find(float, "deltaQ_factor"),
        sigma_min=p.find(float, "sigma_min"), delta_min=p.find(float, "delta_min"),
        ascale=1.0 / (1.0 + p.find(float, "z")),
    )
    kw.update(overrides)
    if "D1" not in kw:
        defaults = HamilParams.__dataclass_fields__
        kw["D1"] = growth_factor(kw["ascale"], kw.get("OM", defaults["OM"].default), kw.get("OL", defaults["OL"].default))
    return HamilParams(**kw)


def mock_params(filename, **overrides):
    """The keys of ``load_initial_fields`` (barcoderunner.cc:284-344) as ``INIT_PARAMS`` reads them (init_par.cc:61-67,
    99-102, 134, 149-150): a dict with ``seed``, ``random_test``, ``random_test_rsd``, ``window_type``, ``data_model``,
    ``negative_obs``, ``sigma_min``, ``sigma_fac``, ``initial_guess``, ``initial_guess_file``,
    ``initial_guess_smoothing_type``, ``initial_guess_smoothing_scale``, ``N_bin``, ``likelihood``.  Raises like
    init_par.cc:75-77 when ``data_model`` and ``likelihood`` do not go together."""
    p = parameter_inifile(filename)
    kw = dict(
        seed=p.find(int, "seed"),
        random_test=p.find(bool, "random_test"), random_test_rsd=p.find(bool, "random_test_rsd"),
        window_type=p.find(int, "window_type"), data_model=p.find(int, "data_model"),
        negative_obs=p.find(bool, "negative_obs"),
        sigma_min=p.find(float, "sigma_min"), sigma_fac=p.find(float, "sigma_fac"),
        initial_guess=p.find(int, "initial_guess"), initial_guess_file=p.find(str, "initial_guess_file"),
        initial_guess_smoothing_type=p.find(int, "initial_guess_smoothing_type"),
        initial_guess_smoothing_scale=p.find(float, "initial_guess_smoothing_scale"),
        N_bin=p.find(int, "N_bin"), likelihood=p.find(int, "likelihood"),
    )
    kw.update(overrides)
    if (kw["data_model"] == 1) != (kw["likelihood"] == 2):
        raise RuntimeError("Error: incompatible data_model and likelihood in input.par! Logarithmic and log-normal "
                           "must go together, or you must choose other models.")
    return kw
