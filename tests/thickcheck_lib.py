"""Shared statements of the thickness-kernel tests (tests/test_thickness_host.py, tests/test_thickness_gpu.py): the
``thicklib`` fixture - tests/hostcheck/thickcheck.hip, the unit function of K2e compiled for the host with hipcc (skipped if
hipcc is absent) - the fp32 layer values the kernels integrate with the last layer in its half-space role, the numpy
statement fed with a unit's returned rows, and the float64 finite differences of tests/golden/thickness_fd.npz."""
import ctypes
import os

import numpy as np
import pytest

import eigen_ref as E
import hostbuild
from kernel_rows_ref import prep_factors32
from pysurfinv_amd import senskernel

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcheck")
# worst figure of the host-compiled unit function against the numpy statement fed with the same fp32 rows
# (tests/test_thickness_host.py, fraction of the unit's largest |reference| entry; profiles/thickness/parity.txt) and the
# committed bar: 8 x that (the device's logf against numpy's in the attenuation factor, amplified by the jump's
# cancellation), never above the project's 1e-4 for a kernel row
PARITY_MEASURED = {"R": 5.176e-8, "L": 5.132e-8}
PARITY_BAR = {w: min(8.0 * v, 1.0e-4) for w, v in PARITY_MEASURED.items()}
FD = np.load(os.path.join(HERE, "golden", "thickness_fd.npz"))
FD_NAMES = [str(n) for n in FD["names"]]
FD_PERIODS = [float(t) for t in FD["periods"]]


def layers32(model, T, w, nlay=None):
    """eigen_ref.layers32 with the stack's last layer in its half-space role (factors hsf, hsr of prep_stack, fp32 in
    layer_derive's operation order): what layer_at gives for every layer the thickness kernel reads."""
    f32 = np.float32
    m = np.asarray(model, f32)
    n = m.shape[1] if nlay is None else int(nlay)
    lay = E.layers32(m, T, w, nlay)
    fac = prep_factors32(m, 1 if w == "L" else 2, None if nlay is None else [nlay])
    vp, vs, rho, _, qs = (x[n - 1] for x in m)
    lnT = f32(np.log(np.float64(f32(1.0) / f32(T))))
    qsq = qs * lnT / f32(3.1415927)
    qpq = qsq * f32(1.33333333) * (vs * vs) / (vp * vp)
    hsf, hsr = fac["hsf"][0][n - 1], fac["hsr"][0][n - 1]
    b, a, r = vs * (f32(1.0) + qsq) * hsf, vp * (f32(1.0) + qpq) * hsf, rho * hsr
    assert all(x.dtype == f32 for x in (a, b, r))
    lay["a"][n - 1], lay["b"][n - 1], lay["rho"][n - 1] = float(a), float(b), float(r)
    return lay


def reference_unit(model, T, w, c, u, I0, vt, kb, ka, kr, nlay=None):
    """senskernel.thickness_kernels_reference on the fp32 rows of one unit as the library returns them.  vt [4][L] in the
    order (ur, uz, tz, tr); Love: rows 0 and 3 (ut, tq)."""
    vt = np.asarray(vt, np.float64)
    v = vt if w == "R" else vt[[0, 3]]
    return senskernel.thickness_kernels_reference(layers32(model, T, w, nlay), np.asarray(model, np.float32), np.float32(T), np.float32(c),
                                                  np.float32(u), np.float32(I0), v, kb, ka if w == "R" else None, kr, w, nlay=nlay)


def figure(lib, ref):
    """worst |lib - ref| over a unit's row as a fraction of the row's largest |ref|."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(lib, np.float64) - ref).max() / np.abs(ref).max())


def fd_unit(name, w, T):
    """dict(c, u, I0, v, fd_h, fd_vs, fd_vp, fd_rho, lay, model) of one unit of thickness_fd.npz."""
    ip = FD_PERIODS.index(float(T))
    out = {k: FD[f"{name}_{w}_{k}"][ip] for k in ("c", "u", "I0", "v", "fd_h", "fd_vs", "fd_vp", "fd_rho", "lay")}
    out["model"] = FD[f"{name}_model"]
    return out


class ThickHost:
    def __init__(self, so):
        self.H = ctypes.CDLL(so)
        self.H.sd_thickcheck_units.restype = ctypes.c_int

    def units(self, model, per, kind, c, ratio, nlay=None):
        """dict(u, I0 [B, P]; hs [B, P]; vt [B, P, 4, L] (Love: ut, tq in rows 0 and 3); kb, ka, kr, dcdh, dcdz [B, P, L];
        n_nonfinite) of the host-compiled path at the given roots."""
        model = np.ascontiguousarray(model, np.float32)
        model = model[None] if model.ndim == 2 else model
        per = np.ascontiguousarray(per, np.float32)
        B, _, L = model.shape; P = per.size
        c = np.ascontiguousarray(np.asarray(c, np.float32).reshape(B, P))
        ratio = np.ascontiguousarray(np.asarray(ratio, np.float32).reshape(B, P))
        f = lambda *s: np.zeros(s, np.float32)
        o = dict(u=f(B, P), I0=f(B, P), hs=np.zeros((B, P), np.int32), vt=f(B, P, 4, L), kb=f(B, P, L), ka=f(B, P, L), kr=f(B, P, L),
                 dcdh=f(B, P, L), dcdz=f(B, P, L))
        fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        nl = None if nlay is None else np.ascontiguousarray(nlay, np.int32)
        o["n_nonfinite"] = self.H.sd_thickcheck_units(
            B, L, None if nl is None else nl.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), fp(model), P, fp(per), int(kind), fp(c), fp(ratio),
            fp(o["u"]), fp(o["I0"]), o["hs"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)), fp(o["vt"]), fp(o["kb"]), fp(o["ka"]), fp(o["kr"]),
            fp(o["dcdh"]), fp(o["dcdz"]))
        if int(kind) != 2:                                   # (ut, tq) to the rows the eigenfunction entry uses
            o["vt"][:, :, 3] = o["vt"][:, :, 1]
            o["vt"][:, :, 1] = 0
        return o


@pytest.fixture(scope="module")
def thicklib():
    return ThickHost(hostbuild.build(os.path.join(HC, "thickcheck.hip"), os.path.join(HC, "libthickcheck.so")))
