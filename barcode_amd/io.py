"""On-disk formats next to the path.

* Field dumps: raw native-endian ``real_prec`` (double) arrays, no header -- ``write_array`` / ``read_array``
  (``barlib/src/IOfunctionsGen.cc:185-229``), including the ``.dat`` extension rule (`add_extension_if_missing`).
* Correlation-function tools: ``<name>_r`` / ``<name>_eta`` as such arrays (``tools/2D_corr_fct.cc:283-303``), and
  ``dump_deltas``' deltaLAG / deltaRSS / deltaEUL fields (``IOfunctionsGen.cc:136-171``).
* ``tools/2D_powspec.cc``: ``<name>_k`` / ``<name>_P`` as such arrays (:162-163).
* ``performance_log.txt``: one tab-separated row of 14 columns per attempt (``HMC.cc:40-60``) under the header
  written by ``barcoderunner.cc:357-358``.
"""
import os

import numpy as np

PERFORMANCE_LOG_COLUMNS = ("accepted", "epsilon", "Neps", "dH", "dK", "dE", "dprior", "dlikeli",
                           "psi_prior_i", "psi_prior_f", "psi_likeli_i", "psi_likeli_f", "H_kin_i", "H_kin_f")


def add_extension_if_missing(fn, ext=".dat"):
    """IOfunctionsGen.cc:185-191: append ``ext`` only when the name has no '.' at all."""
    return fn + ext if fn.rfind(".") == -1 else fn


def write_array(fname, a):
    """IOfunctionsGen.cc:216-229: N * sizeof(real_prec) raw bytes."""
    np.ascontiguousarray(a, dtype=np.float64).tofile(add_extension_if_missing(fname))


def read_array(fname, n):
    """IOfunctionsGen.cc:194-203: read exactly ``n`` doubles (raises if the file is short or missing)."""
    path = add_extension_if_missing(fname)
    if not os.path.isfile(path):
        raise RuntimeError("In read_array: error opening file " + path)
    a = np.fromfile(path, dtype=np.float64, count=n)
    if a.size != n:
        raise RuntimeError("In read_array: %s holds %d values, %d requested" % (path, a.size, n))
    return a


def performance_log_header():
    return "\t".join(PERFORMANCE_LOG_COLUMNS) + "\n"


def performance_log_row(rec):
    """``rec``: one record of ``barcode_amd.hamil.HamiltonianMC`` (or any mapping with the 14 columns).
    C++ ``operator<<`` formatting: bool as 0/1, integers plain, doubles with 6 significant digits (%g)."""
    out = []
    for k in PERFORMANCE_LOG_COLUMNS:
        v = rec[k]
        if k == "accepted":
            out.append("1" if v else "0")
        elif k == "Neps":
            out.append(str(int(v)))
        else:
            out.append("%g" % float(v))
    return "\t".join(out) + "\n"


def dump_measured_spec(kmode, power, fname):
    """``dump_measured_spec`` / ``dump_ps_it`` (IOfunctions.cc:20-34, 37-82): one ``k   P(k)`` line per bin with
    ``k > 0`` and ``P > 0``, C++ default stream formatting (6 significant digits).  ``dump_ps_it`` names the file
    ``<dir>powSpecit<iGibbs>.dat`` (``power_spectrum_filename``)."""
    with open(fname, "w") as f:
        for x, y in zip(np.asarray(kmode).ravel(), np.asarray(power).ravel()):
            if y > 0.0 and x > 0.0:
                f.write("%g   %g\n" % (x, y))


def power_spectrum_filename(directory, iGibbs):
    return os.path.join(directory, "powSpecit%d.dat" % int(iGibbs)) if directory else "powSpecit%d.dat" % int(iGibbs)


def corr_filenames(fname_out, n_bin, auto_nbin=False):
    """The two files of ``tools/2D_corr_fct.cc:301-303`` (before ``write_array``'s extension rule); the ``_Nbin<N>``
    suffix is added when the tool chose the bin count itself (:278-286)."""
    base = fname_out + ("_Nbin%d" % int(n_bin) if auto_nbin else "")
    return base + "_r", base + "_eta"


def dump_corr(fname_out, rmode, corr, auto_nbin=False, n_bin=None):
    """``dump_scalar(rmode, ...)``, ``dump_scalar(corr, ...)`` of the correlation tools: raw ``real_prec`` arrays of
    N_bin (1-D) or N_bin^2 values (2-D, element ``par + N_bin * perp``).  ``n_bin`` names the bin count for the
    ``_Nbin`` suffix; without it the first axis of ``rmode`` is taken, which is right for 1-D arrays and for 2-D arrays
    shaped (N_bin, N_bin), not for a flat N_bin^2 one.  Returns the two paths written."""
    rmode, corr = np.asarray(rmode), np.asarray(corr)
    names = corr_filenames(fname_out, rmode.shape[0] if n_bin is None else n_bin, auto_nbin)
    for name, a in zip(names, (rmode, corr)):
        write_array(name, a)
    return tuple(add_extension_if_missing(n) for n in names)


def interp_filename(fname_in, n_out):
    """``tools/interp_upres.cc:45``: the default output name of the interpolated field."""
    return "%s_interpCIC%d" % (fname_in, int(n_out))


def dump_interp(fname_in, n_out, field):
    """``quick_dump_scalar(result, N1_out, fname_out, 0, false)`` of ``tools/interp_upres.cc``: the raw array under
    ``interp_filename``.  Returns the path written."""
    name = interp_filename(fname_in, n_out)
    write_array(name, np.asarray(field))
    return add_extension_if_missing(name)


def corr_interp_filenames(fname_in, n_out, n_bin, auto_nbin=False):
    """The two files of ``tools/2D_corr_fct_interp.cc:338,397,427-428``: ``<in>_interpCIC<n_out>_corr2D[_Nbin<n>]`` +
    ``_r`` / ``_eta`` (both interpolation modes write under this name)."""
    return corr_filenames(interp_filename(fname_in, n_out) + "_corr2D", n_bin, auto_nbin)


def dump_corr_interp(fname_in, n_out, rmode, corr, auto_nbin=False, n_bin=None):
    """``dump_corr`` under the names of ``corr_interp_filenames``."""
    return dump_corr(interp_filename(fname_in, n_out) + "_corr2D", rmode, corr, auto_nbin, n_bin)


def pow_filename(fname_in):
    """``tools/powspec.cc``: the measured spectrum of a field file goes to ``<in>_pow``."""
    return fname_in + "_pow"


def dump_pow(fname_in, kmode, power):
    """``powspec.cc``'s output through the spectrum writer (``dump_measured_spec``).  Returns the path written."""
    name = pow_filename(fname_in)
    dump_measured_spec(kmode, power, name)
    return name


def pow2d_filenames(fname_in, fname_out=None):
    """The two files of ``tools/2D_powspec.cc:130,162-163`` (before ``write_array``'s extension rule): ``<out>_k`` and
    ``<out>_P``, ``<out>`` defaulting to ``<in>_pow2D``."""
    base = fname_in + "_pow2D" if fname_out is None else fname_out
    return base + "_k", base + "_P"


def dump_pow2D(fname_in, kmode, power, fname_out=None):
    """``dump_scalar(kmode2D, ...)``, ``dump_scalar(power2D, ...)`` of ``2D_powspec.cc``: raw ``real_prec`` arrays of
    N_bin^2 values, element ``par + N_bin * perp``.  Returns the two paths written."""
    names = pow2d_filenames(fname_in, fname_out)
    for name, a in zip(names, (kmode, power)):
        write_array(name, np.asarray(a))
    return tuple(add_extension_if_missing(n) for n in names)


def dump_density(density, fname_out="density"):
    """``quick_dump_scalar(density, N1, fname_out, 0, false)`` of ``tools/density.cc:84``: the raw array of N values under
    ``fname_out`` (the tool's default name, ``density``).  Returns the path written."""
    write_array(fname_out, np.asarray(density))
    return add_extension_if_missing(fname_out)


def poisson_filename(fname_in, N1_out, Nbar):
    """The default output name of ``tools/poisson_upres.cc:88``: ``<in>_poisCIC<N_out>_Nbar<Nbar>``, the two numbers as
    they were typed (pass strings to keep a spelling such as ``8.0``)."""
    fmt = lambda v: v if isinstance(v, str) else "%g" % v
    return "%s_poisCIC%s_Nbar%s" % (fname_in, fmt(N1_out), fmt(Nbar))


def dump_poisson(density, fname_in, N1_out, Nbar, fname_out=None):
    """``quick_dump_scalar(output, N1_out, fname_out, 0, false)`` of ``tools/poisson_upres.cc:154``: the raw array under
    ``fname_out``, by default the tool's ``<in>_poisCIC<N_out>_Nbar<Nbar>``.  Returns the path written."""
    name = fname_out or poisson_filename(fname_in, N1_out, Nbar)
    write_array(name, np.asarray(density))
    return add_extension_if_missing(name)


def ensemble_filenames(directory, name):
    """``<name>_mean`` and ``<name>_std`` under ``directory`` (before ``write_array``'s extension rule)."""
    base = os.path.join(directory, name) if directory else name
    return base + "_mean", base + "_std"


def dump_ensemble(engine, directory, slot, name):
    """The posterior mean and standard deviation of ensemble accumulator ``slot`` (``Engine.ensemble_add``) as raw
    ``real_prec`` arrays of N values, ``<name>_mean`` and ``<name>_std``, like the field dumps they summarise.  Needs two
    samples in the slot.  Returns the two paths written."""
    names = ensemble_filenames(directory, name)
    for path, what in zip(names, ("mean", "std")):
        write_array(path, engine.ensemble_fetch(slot, what))
    return tuple(add_extension_if_missing(n) for n in names)


TWEB_NAMES = ("void", "sheet", "filament", "knot")


def tweb_filenames(directory, name):
    """``<name>_pvoid`` .. ``<name>_pknot`` and ``<name>_tweb.txt`` under ``directory`` (the four before ``write_array``'s
    extension rule)."""
    base = os.path.join(directory, name) if directory else name
    return tuple(base + "_p" + t for t in TWEB_NAMES) + (base + "_tweb.txt",)


def dump_tweb(engine, directory, name):
    """The posterior web-type probabilities of the engine's T-web accumulator (``Engine.tweb_classify`` with
    ``accumulate``) as four raw ``real_prec`` arrays of N values, and one text line with the sample count, the
    smoothing scale and the threshold of the samples.  Needs one sample.  Returns the five paths written."""
    names = tweb_filenames(directory, name)
    for t, path in enumerate(names[:4]):
        write_array(path, engine.tweb_fetch(t, as_probability=True))
    R, lth = engine._tweb_par if engine._tweb_par is not None else (float("nan"), float("nan"))
    with open(names[4], "w") as f:
        f.write("%d %.17g %.17g\n" % (engine.tweb_samples(), R, lth))
    return tuple(add_extension_if_missing(n) for n in names[:4]) + (names[4],)


def dump_bispec(result, directory, name):
    """``Engine.bispectrum``'s dict as the text table ``<name>_bispec.txt`` under ``directory``: a header line, then one
    row per triplet -- s1 s2 s3, the three shells' mean |k|, ntri, B and Q, the reals with 17 digits so that
    ``read_bispec`` returns them bit for bit.  Returns the path."""
    path = (os.path.join(directory, name) if directory else name) + "_bispec.txt"
    km = result["kmean"]
    with open(path, "w") as f:
        f.write("# s1 s2 s3 kmean1 kmean2 kmean3 ntri B Q\n")
        for (s1, s2, s3), nt, b, q in zip(result["triplets"], result["ntri"], result["b"], result["q"]):
            f.write("%d %d %d %.17g %.17g %.17g %.17g %.17g %.17g\n" % (s1, s2, s3, km[s1], km[s2], km[s3], nt, b, q))
    return path


def read_bispec(path):
    """The table ``dump_bispec`` wrote -> dict of ``triplets`` (T, 3) int32, ``kmean`` (T, 3), ``ntri``, ``b``, ``q``."""
    rows = np.loadtxt(path, ndmin=2)
    return dict(triplets=rows[:, :3].astype(np.int32), kmean=rows[:, 3:6].copy(), ntri=rows[:, 6].copy(),
                b=rows[:, 7].copy(), q=rows[:, 8].copy())


def dump_multipoles(result, directory, name):
    """``Engine.measure_multipoles``'s or ``measure_corr_multipoles``'s dict as the text table ``<name>_multipoles.txt``
    under ``directory``: a header line that names the columns, then one row per bin -- k or r, nmode, the means of L_2 and
    L_4, and the three multipoles, the reals with 17 digits so that ``read_multipoles`` returns them bit for bit.
    Returns the path."""
    path = (os.path.join(directory, name) if directory else name) + "_multipoles.txt"
    cols = ("k", "p0", "p2", "p4") if "k" in result else ("r", "xi0", "xi2", "xi4")
    with open(path, "w") as f:
        f.write("# %s nmode leg2 leg4 %s %s %s\n" % cols)
        for row in zip(result[cols[0]], result["nmode"], result["leg2"], result["leg4"], *(result[c] for c in cols[1:])):
            f.write("%.17g %d %.17g %.17g %.17g %.17g %.17g\n" % row)
    return path


def read_multipoles(path):
    """The table ``dump_multipoles`` wrote -> the dict it was given: ``k, nmode, leg2, leg4, p0, p2, p4`` or ``r, ..., xi0,
    xi2, xi4``, nmode as uint64."""
    with open(path) as f:
        names = f.readline().lstrip("#").split()
        rows = [line.split() for line in f if line.strip()]
    out = {}
    for c, name in enumerate(names):
        if name == "nmode":
            out[name] = np.array([int(r[c]) for r in rows], dtype=np.uint64)
        else:
            out[name] = np.array([float(r[c]) for r in rows], dtype=np.float64)
    return out


def dump_deltas(engine, directory, suffix=""):
    """``dump_deltas`` (IOfunctionsGen.cc:136-171) of the resident chain state: deltaLAG, then deltaEUL without
    ``rsd_model``, or deltaRSS (the configured forward model) and deltaEUL (a second Lag2Eul without RSD) with it.
    The forward models run on the device from the resident state (``chain_forward``); only the dumped fields cross to
    the host.  Returns the paths in the order written."""
    def put(name, a):
        path = os.path.join(directory, name + suffix) if directory else name + suffix
        write_array(path, a)
        return add_extension_if_missing(path)

    out = [put("deltaLAG", engine.chain_get_state())]
    if not engine.params.rsd_model:
        engine.chain_forward(0)
        out.append(put("deltaEUL", engine.fetch("deltaX")))
    else:
        engine.chain_forward(1)
        out.append(put("deltaRSS", engine.fetch("deltaX")))
        engine.chain_forward(0)
        out.append(put("deltaEUL", engine.fetch("deltaX")))
    return out
