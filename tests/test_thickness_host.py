"""Thickness and interface-depth kernels of the phase velocity, without a GPU (include/surfdisp.h section (5g)).

1. The formula itself, float64 only: senskernel.thickness_kernels_reference fed with the exact inputs of
   tests/golden/thickness_fd.npz (tests/golden/make_golden_thickness.py: roots of tests/secular64.py, exact-propagator
   eigenfunctions, central differences) reproduces the central differences of c with respect to every thickness to 1e-6 of
   the unit's largest one; on a flat stack the interface kernels and the free-surface term sum to zero (translation
   invariance) and E is constant through every homogeneous layer.
2. The device function compiled for the host (tests/hostcheck/thickcheck.hip) against the same numpy statement fed with the
   host path's own fp32 rows, on every solved unit of the six stacks of ref_eigen.npz at the reference's roots.
3. The host path end to end (RK4 discretisation, fp32 eigenfunctions and flattening factors) against the float64 central
   differences: A_h = worst |dcdh - fd_h| / max |fd_h| against the same figure A_b of the existing dcdb rows against fd_Vs;
   A_h <= 4 A_b (dcdh sums up to L local terms and carries the chain shares on top of the jump).

Measured (profiles/thickness/parity.txt): 1. worst 2.1e-7 (the differences' own rounding at 6 s), the identity 5e-13;
2. 5.2e-8 both wave types (thickcheck_lib.PARITY_MEASURED); 3. A_h / A_b = 1.16 (Rayleigh), 3.39 (Love)."""
import os

import numpy as np
import pytest

import eigen_ref as E
import thickcheck_lib as TL
from thickcheck_lib import thicklib                        # noqa: F401  (fixture)
from pysurfinv_amd import senskernel



def _generator():
    """tests/golden/make_golden_thickness.py as a module (its float64 root search and eigenfunction), without putting
    tests/golden on sys.path."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_thickness.py")
    spec = importlib.util.spec_from_file_location("make_golden_thickness", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod

PARITY_BAR = TL.PARITY_BAR


@pytest.mark.parametrize("w", ["R", "L"])
@pytest.mark.parametrize("name", TL.FD_NAMES)
def test_formula_against_central_differences(name, w):
    worst = 0.0
    for T in TL.FD_PERIODS:
        f = TL.fd_unit(name, w, T)
        lay = dict(zip(("a", "b", "rho", "d"), f["lay"]))
        dcdh, dcdz, K = senskernel.thickness_kernels_reference(
            lay, f["model"].astype(np.float64), T, f["c"], f["u"], f["I0"], f["v"], f["fd_vs"], f["fd_vp"] if w == "R" else None,
            f["fd_rho"], w)
        err = np.abs(dcdh - f["fd_h"]).max() / np.abs(f["fd_h"]).max()
        r = 6371.0 - np.concatenate([[0.0], np.cumsum(f["model"][3].astype(np.float64))[:-1]])
        chain = np.abs(dcdz - K * 6371.0 / r).max() / np.abs(dcdz).max()
        print(f"{name} {w} T={T:g}: max |dcdh - fd| / max |fd| = {err:.2e} (chain terms up to {chain:.1e} of the largest dcdz)")
        assert dcdz[0] == 0 and dcdh[-1] == 0
        assert np.abs(np.concatenate([[0.0], dcdh[:-1] - dcdh[1:]]) - dcdz).max() <= 1e-12 * np.abs(dcdz).max()
        worst = max(worst, err)
        assert err <= 1.0e-6, (name, w, T, err)
    print(f"{name} {w}: worst {worst:.2e} (bar 1e-6)")


@pytest.mark.parametrize("w", ["R", "L"])
def test_flat_stack_identities(w):
    """A flat five-layer stack (no earth flattening: the layer values are the inputs), T = 16 s: K_0 + sum_j K_j = 0 with K_0 =
    -amp (c^3 / omega^2) [0 - E(v_0; 0)] to 1e-12 of the largest term, and E(v_j; j) = E(v_{j+1}; j) through every layer (to
    1e-10 of the sum of the magnitudes of E's terms: an exact float64 propagator with entries up to e^(kH) < 1e3 and some
    hundred roundings of 2^-53)."""
    G = _generator()
    m = TL.FD["synth_L5_model"].astype(np.float64)
    L = m.shape[1]
    T = 16.0
    lay = dict(a=m[0].copy(), b=m[1].copy(), rho=m[2].copy(), d=np.where(np.arange(L) < L - 1, m[3], 0.0))
    om = G.TWOPI32 / T
    c = G.root_scan(lay, om, w)
    u = G.group_velocity(lay, om, w, c)
    v, I0, resid = G.eigenfunction(lay, T, c, w)
    assert resid < 1e-9
    z = np.zeros(L)
    _, _, K = senskernel.thickness_kernels_reference(lay, m, T, c, u, I0, v, z, None if w == "L" else z, z, w, hs=L - 1)
    k = om / c
    En = lambda vv, i: senskernel.interface_energy(vv, lay["a"][i], lay["b"][i], lay["rho"][i], k, om, w)
    fac = -(1.0 / (2.0 * c * u * I0)) * c ** 3 / om ** 2
    K0 = fac * (0.0 - En(v[:, 0], 0))
    terms = np.concatenate([[K0], K[1:]])
    print(f"{w}: K {terms}, sum {terms.sum():.3e}")
    assert abs(terms.sum()) <= 1e-12 * np.abs(terms).max()
    for i in range(L - 1):
        e_top, e_bot = En(v[:, i], i), En(v[:, i + 1], i)
        mag = sum(abs(senskernel.interface_energy(np.where(np.arange(v.shape[0]) == q, v[:, i], 0.0), lay["a"][i], lay["b"][i], lay["rho"][i], k, om, w))
                  for q in range(v.shape[0]))
        assert abs(e_top - e_bot) <= 1e-10 * mag, (i, e_top, e_bot)
    assert abs(En(v[:, L - 1], L - 1)) <= 1e-10 * abs(En(np.abs(v[:, L - 1]) * [1, 0, 0, 0][:v.shape[0]], L - 1))   # the decaying half-space solution: E = 0


def _host_units(thicklib, w, kind, periods=None):
    """name -> (model, host outputs at the reference's roots, solved mask) for the stacks of ref_eigen.npz."""
    out = {}
    for name in E.NAMES:
        m = np.asarray(E.FIX[f"{name}_model"], np.float32)
        meta = E.FIX[f"{name}_{w}_meta"]
        c = np.where(meta[:, 0] > 0, meta[:, 0], 0.0).astype(np.float32)
        ratio = meta[:, 11].astype(np.float32)
        out[name] = (m, thicklib.units(m, E.PERIODS, kind, c, ratio), c > 0)
    return out


@pytest.mark.parametrize("w,kind", [("R", 2), ("L", 1)])
def test_host_unit_function_against_numpy(thicklib, w, kind):
    worst, n = 0.0, 0
    for name, (m, o, solved) in _host_units(thicklib, w, kind).items():
        assert o["n_nonfinite"] == 0
        for ip, T in enumerate(E.PERIODS):
            if not solved[ip]:
                continue
            assert o["hs"][0, ip] >= 1
            c = np.float32(E.FIX[f"{name}_{w}_meta"][ip, 0])
            dh, dz, K = TL.reference_unit(m, T, w, c, o["u"][0, ip], o["I0"][0, ip], o["vt"][0, ip], o["kb"][0, ip], o["ka"][0, ip], o["kr"][0, ip])
            assert np.array_equal(dh != 0, o["dcdh"][0, ip] != 0) and np.array_equal(dz != 0, o["dcdz"][0, ip] != 0)
            assert o["dcdz"][0, ip, 0] == 0 and o["dcdh"][0, ip, -1] == 0
            f = max(TL.figure(o["dcdh"][0, ip], dh), TL.figure(o["dcdz"][0, ip], dz))
            worst = max(worst, f); n += 1
    print(f"\n{w}: {n} units, host unit function against the numpy statement: worst {worst:.3e} (bar {PARITY_BAR[w]:.3e})")
    assert n == 48
    assert worst <= PARITY_BAR[w]


@pytest.mark.parametrize("w,kind", [("R", 2), ("L", 1)])
def test_host_path_against_fd(thicklib, w, kind):
    """A_h <= 4 A_b at the reference's roots.  Measured: Rayleigh A_h 4.12e-3, A_b 3.54e-3; Love A_h 2.16e-3, A_b 6.37e-4
    (profiles/thickness/parity.txt)."""
    host = _host_units(thicklib, w, kind)
    A_h = A_b = 0.0
    for name in TL.FD_NAMES:
        m, o, solved = host[name]
        for T in TL.FD_PERIODS:
            ip = int(np.flatnonzero(E.PERIODS == np.float32(T))[0])
            assert solved[ip]
            f = TL.fd_unit(name, w, T)
            a_h, a_b = TL.figure(o["dcdh"][0, ip], f["fd_h"]), TL.figure(o["kb"][0, ip], f["fd_vs"])
            print(f"{name} {w} T={T:g}: A_h {a_h:.2e} A_b {a_b:.2e}")
            A_h, A_b = max(A_h, a_h), max(A_b, a_b)
    print(f"{w}: A_h = {A_h:.3e}, A_b = {A_b:.3e}, A_h / A_b = {A_h / A_b:.2f} (bar 4)")
    assert A_h <= 4.0 * A_b


def test_analytic_kernels_refuses_combinations():
    """thickness=True is an entry of its own: refused with group, ellipticity and attenuation before anything runs."""
    for kw in (dict(group=True), dict(ellipticity=True), dict(attenuation=True)):
        with pytest.raises(ValueError, match="thickness=True is an entry of its own"):
            senskernel.analytic_kernels(None, None, wtype="R", thickness=True, **kw)
