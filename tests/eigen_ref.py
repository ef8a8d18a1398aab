"""Shared statements of the eigenfunction tests (tests/test_eigen_host.py, tests/test_eigen_gpu.py): the reference's
COMMON /rar/ entries of tests/golden/ref_eigen.npz carried to the caller's layer tops, and the layer-by-layer consistency
figure.  Plain numpy, float64; the propagator is pysurfinv_amd.senskernel.eigen_layer_matrix.

The reference stores the MIDDLE of every sublayer (kk = 3: surfa.f:1104-1108, 553-555), the library the TOP of every
caller layer.  The two meet through the exact propagator of the flattened, attenuated layer over half a sublayer - a
distance over which its entries are O(1) - applied in float64 to the reference's fp32 values; the free surface (sea floor)
and the top of the effective half space are entries of both and are compared directly.  (For Rayleigh the half sublayer is bridged with the reference's
own two Runge-Kutta steps, see ref_tops.)"""
import functools
import os

import numpy as np

from pysurfinv_amd import senskernel
from kernel_rows_ref import prep_factors32

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_eigen.npz"))
PERIODS = np.asarray(FIX["periods"], np.float32)
NAMES = [str(n) for n in FIX["names"]]
EPS = 2.0 ** -24
ROWS = {"R": (1, 2, 3, 4), "L": (1, 4)}            # rows of the /rar/ block: ampur, ampuz, stresz, stresr | amp, stress


def units(w):
    """Every solved (case, period) unit of wave type ``w``: dict(name, model [5, L], ip, T, c, u, mmax, ndiv, sums [4], are,
    ratio, rar [5, entries], first [L], hs, nreg, wet)."""
    for name in NAMES:
        m = np.asarray(FIX[f"{name}_model"], np.float32)
        meta, rar, first, hs = (FIX[f"{name}_{w}_{k}"] for k in ("meta", "rar", "first", "hs"))
        for ip, T in enumerate(PERIODS):
            if not meta[ip, 0] > 0:
                continue
            yield dict(name=name, model=m, ip=ip, T=float(T), c=np.float32(meta[ip, 0]), u=np.float32(meta[ip, 1]),
                       mmax=int(meta[ip, 2]), ndiv=max(int(meta[ip, 3]), 1), sums=meta[ip, 4:8], are=meta[ip, 8],
                       ratio=np.float32(meta[ip, 11]), rar=np.asarray(rar[ip], np.float64), first=first[ip],
                       hs=int(hs[ip, 0]), nreg=int(hs[ip, 1]), wet=not (m[1, 0] > 0))


def layers32(model, T, w, nlay=None):
    """The layer values the reference and the kernels actually integrate: the fp32 flattening factors of ``prep_stack``
    (kernel_rows_ref.prep_factors32, bit for bit) and the fp32 attenuation correction of ``layer_derive`` in its operation
    order, as float64 - the dict of senskernel.flattened_layers, regular role.  The float64 formulas of flattened_layers
    differ from these by the fp32 rounding of the flattened thickness, R0 2^-24 = 4e-4 km whatever the layer's own
    thickness, which would dominate the consistency figure of a thin layer."""
    f32 = np.float32
    m = np.asarray(model, f32)
    fac = prep_factors32(m, 1 if w == "L" else 2, None if nlay is None else [nlay])
    vp, vs, rho, _, qs = m
    lnT = f32(np.log(np.float64(f32(1.0) / f32(T))))
    with np.errstate(all="ignore"):
        qsq = qs * lnT / f32(3.1415927)
        qpq = qsq * f32(1.33333333) * (vs * vs) / (vp * vp)
        b = vs * (f32(1.0) + qsq) * fac["dif"][0]
        a = vp * (f32(1.0) + qpq) * fac["dif"][0]
        r = rho * fac["qqq"][0]
    assert a.dtype == f32 and b.dtype == f32 and r.dtype == f32
    return dict(a=a.astype(np.float64), b=b.astype(np.float64), rho=r.astype(np.float64), d=fac["dfl"][0].astype(np.float64))


@functools.lru_cache(maxsize=None)
def _layers(name, ip, w):
    return layers32(FIX[f"{name}_model"], PERIODS[ip], w)


def _mat(un, w, i, frac, rk4_steps=0):
    return senskernel.eigen_layer_matrix(_layers(un["name"], un["ip"], w), i, un["T"], un["c"], w, frac, rk4_steps)


def ref_tops(un, w):
    """The reference's values at the top of every caller layer 0 .. hs, float64 [components][L] (zeros elsewhere), and the
    mask [L] of the layers that have one.  The set entry and the half-space top directly, the others from the layer's
    first sublayer, half a sublayer up.  A cut inside a layer (nreg > 0) leaves that layer's top as any other's."""
    L = un["model"].shape[1]
    rows = ROWS[w]
    tops = np.zeros((len(rows), L)); have = np.zeros(L, bool)
    etop = 1 if un["wet"] else 0
    nd = un["ndiv"]
    for i in range(etop, un["hs"] + 1):
        if i == etop:
            v = un["rar"][rows, 0]
        elif i == un["hs"] and un["nreg"] == 0:
            v = un["rar"][rows, un["mmax"] - 1]
        else:
            # (Rayleigh: the reference's own two Runge-Kutta steps from its knot kk = 3 to its knot kk = 1, the sublayer's
            # top, which it forms and does not store; the exact map differs from them by the step's discretisation error,
            # (lambda h)^5 / 120 each - 2.4e-4 of the shear traction of the thick layers at T = 6 s.  LEIGEN's steps are exact.)
            v = _mat(un, w, i, 0.5 / nd, 2 if w == "R" else 0) @ un["rar"][rows, un["first"][i]]
        tops[:, i] = v; have[i] = True
    if un["wet"]:
        have[0] = True                                 # the sea surface: zero by convention (the reference forms no entry)
    return tops, have


def parity(lib, un, w):
    """Worst |library - reference| over the layer tops, per component, as a fraction of that component's largest absolute
    reference value over the unit; the zero pattern must be identical (-> inf otherwise).  lib [components][L]."""
    tops, have = ref_tops(un, w)
    lib = np.asarray(lib, np.float64)
    if np.any(lib[:, ~have] != 0) or np.any((tops == 0) != (lib == 0)):
        return np.inf
    scale = np.abs(tops).max(axis=1)
    return float((np.abs(lib - tops).max(axis=1) / scale).max())


def _figure(M, vb, vt):
    """|M vb - vt| per component over the fp32 rounding of the stored values carried through M: 2^-24 (|M| |vb| + |vt|)."""
    err = np.abs(M @ vb - vt)
    bound = EPS * (np.abs(M) @ np.abs(vb) + np.abs(vt))
    return float((err / bound).max())


def consistency_lib(lib, un, w):
    """Layer-by-layer consistency of layer-top values lib [components][L]: (worst figure over the interior layers, figure of
    the layer under the SET entry).  The entry at the top of layer i + 1 carried through layer i against the entry at the
    top of layer i."""
    etop = 1 if un["wet"] else 0
    lib = np.asarray(lib, np.float64)
    inner, surf = 0.0, 0.0
    for i in range(etop, un["hs"]):
        f = _figure(_mat(un, w, i, 1.0), lib[:, i + 1], lib[:, i])
        if i == etop:
            surf = f
        else:
            inner = max(inner, f)
    return inner, surf


def consistency_ref(un, w):
    """The same figures of the reference's own fixture values: from the first sublayer of layer i + 1 (the half-space top
    for the last step) up to the first sublayer of layer i - half a sublayer of layer i + 1, then all of layer i but its
    top half sublayer; the set entry from the first sublayer under it."""
    etop = 1 if un["wet"] else 0
    rows = ROWS[w]
    nd = un["ndiv"]
    rar = un["rar"]
    inner = 0.0
    for i in range(etop, un["hs"]):
        if i + 1 == un["hs"] and un["nreg"] == 0:
            M, vb = np.eye(len(rows)), rar[rows, un["mmax"] - 1]
        else:
            M, vb = _mat(un, w, i + 1, 0.5 / nd), rar[rows, un["first"][i + 1]]
        M = _mat(un, w, i, (nd - 0.5) / nd) @ M
        inner = max(inner, _figure(M, vb, rar[rows, un["first"][i]]))
    surf = 0.0
    if un["hs"] > etop:
        surf = _figure(_mat(un, w, etop, 0.5 / nd), rar[rows, un["first"][etop]], rar[rows, 0])
    return inner, surf


def wavenumbers32(c, T):
    """(k, omega) as the kernels hold them: fp32 quotients of the reference's constant (surfa.f:871-874), as float64."""
    two_pi = np.float32(6.2831853072)
    return float(two_pi / (np.float32(c) * np.float32(T))), float(two_pi / np.float32(T))
