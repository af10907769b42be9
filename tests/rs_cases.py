"""The cases of the real-space kernel tests: inputs (tests/rs_inputs.py), their longdouble reference (tests/rs_reference.py)
and the bound at C = 1 (tests/rs_bound.py), built once per (kernel, n, type) and shared by the numpy restatement
(tests/test_rs_bounds.py) and the HIP kernels (tests/test_gpu_rs.py).  A case is a dict: name, the input arrays, r (the
reference) and bound.  Every input set at n = 16; the white set and the impulses at the other sizes."""
import functools

import numpy as np

from tests import rs_bound as rb
from tests import rs_inputs as ri
from tests import rs_reference as ref
from tests.kstep_inputs import box, row_stride, types

SMOL = 1.9
HH, F1 = 0.8, ri.TSC_F1


def full(n):
    return n == ri.FULL


@functools.lru_cache(maxsize=2)
def grad_cases(n, prec):
    rdt = types(prec)[0]
    out = []
    for name, phi in ri.phi_sets(n, prec, full(n)):
        r = ref.alpt_grad(phi, n, box(n))
        out.append(dict(name=name, phi=phi, r=r, bound=rb.alpt_grad_bound(r, rdt)))
    return out


@functools.lru_cache(maxsize=2)
def sources_cases(n, prec):
    rdt = types(prec)[0]
    out = []
    for name, phi in ri.phi_sets(n, prec, full(n)):
        if name.startswith("wave"):
            continue  # smooth fields are what the engine-level tests already run
        g3, d1 = ri.sources_inputs(phi, n, prec)
        r = ref.alpt_sources(g3, d1, n, box(n), ri.D1, ri.D2)
        out.append(dict(name=name, g3=g3, d1=d1, r=r, bound=rb.alpt_sources_bound(r, rdt, ri.D2)))
    return out


def table_case(n, prec):
    rdt = types(prec)[0]
    nhp = row_stride(n, rdt, True)
    r = ref.kernel_table(n, nhp, box(n), SMOL)
    return dict(name="table", nhp=nhp, r=r, bound=rb.kernel_table_bound(r, rdt))


def kspace_sets(n, prec):
    return [("white", ri.kspace_white(n, prec)), ("impulses", ri.kspace_impulses(n, prec))]


def gradfft_cases(n, prec):
    rdt = types(prec)[0]
    out = []
    for name, fk in kspace_sets(n, prec):
        r = ref.gradfft_mult(fk, n, box(n), 1.0 / n ** 3)
        out.append(dict(name=name, fk=fk, r=r, bound=rb.gradfft_mult_bound(r, rdt)))
    return out


def conv_cases(n, prec):
    rdt = types(prec)[0]
    F = ri.conv_table(n, prec)
    out = []
    for name, pl in kspace_sets(n, prec):
        r = ref.conv_kernel(pl, F, n, box(n), HH, 1.0 / n ** 3)
        out.append(dict(name=name, pl=pl, F=F, r=r, bound=rb.conv_kernel_bound(r, rdt)))
    return out


def mul3_case(n, prec):
    rdt = types(prec)[0]
    rng = ri.rng_for(n, 41)
    a, b3 = rng.standard_normal(n ** 3).astype(rdt), rng.standard_normal((3, n ** 3)).astype(rdt)
    a[:4] = [0, np.nan, np.inf, -1]
    b3[:, 4:6] = [[0, np.inf]] * 3
    r = ref.mul3(a, b3)
    return dict(name="white", a=a, b3=b3, r=r, bound=rb.mul3_bound(r, rdt))


def findif_cases(n, prec):
    rdt = types(prec)[0]
    out = []
    for code in (0, 1, 2):
        dX, pl = ri.findif_inputs(n, prec, code)
        r = ref.findif_mul(dX, pl, n, box(n), code, ri.LN_RHO_C, ri.LN_DELTA_MIN)
        out.append(dict(name="code%d" % code, code=code, dX=dX, pl=pl, r=r, bound=rb.findif_mul_bound(r, rdt)))
    if full(n):  # the aliased / wrapped arms on the structured sets too
        for name, phi in ri.phi_sets(n, prec, True):
            if name in ("offset", "axes", "impulse_corner"):
                pl = ri.findif_inputs(n, prec, 0)[1]
                r = ref.findif_mul(phi, pl, n, box(n), 0)
                out.append(dict(name="code0_" + name, code=0, dX=phi, pl=pl, r=r, bound=rb.findif_mul_bound(r, rdt)))
    return out


@functools.lru_cache(maxsize=2)
def tsc_cases(n, prec):
    rdt = types(prec)[0]
    geo, sets, conv = ri.tsc_inputs(n, prec, ri.TSC_SETS if full(n) else ("mixed",))
    out = []
    for name, psi in sets:
        for rsd in ((0, 1) if (full(n) or n <= 9) else (1,)):
            r = ref.interp_tsc(psi, conv, geo, rdt, rsd, F1, **ri.TSC_POS)
            out.append(dict(name="%s_rsd%d" % (name, rsd), psi=psi, conv=conv, rsd=rsd, geo=geo, r=r,
                            bound=rb.interp_tsc_bound(r, rdt, rsd, F1)))
    return out
