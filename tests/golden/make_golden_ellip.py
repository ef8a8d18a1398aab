#!/usr/bin/env python3
"""Central differences of the Rayleigh ellipticity chi (H/V) with respect to every layer's Vs, Vp and rho, in float64
-> tests/golden/ellip_fd.npz.

The project's own float64 checker (tests/secular64.py) and the helpers of make_golden_thickness.py (imported, not copied):
nothing of the reference runs here, nor the library under test.  With D(e) the layer recursion of secular64.ray_step /
ray_close from the start vector e1, e2 or e3 (start = 1, 2, 3; a liquid top layer is passed over for e2 and e3) to the
half-space row, the secular function is D(e1) and chi = D(e3) / (2 D(e2)) at its root - include/surfdisp.h section (5d).

Stacks: the five of thickness_fd.npz (its NAMES, from ref_eigen.npz) at 6, 16, 40 and 100 s, and deepwater_L9 = water_L9
with 5 km of water (h[0] = 5.0) at 6 and 10 s - at these the liquid layer's z = (k d)^2 (c^2 / Vp^2 - 1) is above 1
(1.19 and 1.90), the cosine side of cs_of beyond its series branch, which the 3 km of water_L9 does not reach.  One unit
= one (stack, period), Rayleigh.  Stored per unit (zeros at and below mmax, as in thickness_fd.npz):

    lay, mmax, c   as make_golden_thickness.py: flatten64 on the fp32 inputs widened to float64, cut_index, root_scan,
                   omega = 6.2831853072f / T;
    chi            0.5 D(e3) / D(e2) at that root;
    fd_vs, fd_vp, fd_rho [L]   central differences of chi through the re-found root (root_near on the stepped stack),
                   relative step 1e-5 of the stepped value (one column 2e-4: STEP below), the cut index held fixed; the
                   water layer's own flattening factors are frozen and its entries are zeros (its rows are zero in the
                   library: make_golden_thickness.py);
    part_vs, part_vp, part_rho   the same differences with c held at `c`;
    dchidc         the central difference in c at fixed layers, relative step 1e-6;
    dc_vs, dc_vp, dc_rho   the central differences of the root (thickness_fd.npz's fd_vs, fd_vp, fd_rho of the shared units):
                   fd = part + dchidc dc localises a disagreement;
    fd_err [3]     per column the worst |difference at the step - difference at twice the step| over the layers as a fraction
                   of the column's peak: the fixture's own accuracy;
    zreg [2][3]    the number of solid layers above the half space with z < -1, |z| <= 1, z > 1 for the P row and the S row,
                   z = (k d)^2 (c^2 / v^2 - 1) the argument of cs_of;
    zliq           the same z of the liquid layer, or NaN.

The library does not hold these layer values: its prep stage flattens in fp32, and the flattened thickness of a layer
carries an error of R0 2^-24 = 4e-4 km whatever the layer's own thickness - 1.5e-3 of a 0.25 km layer of eus_L68, and as
much of that layer's share of every kernel row (measured: the rows of the library are 2e-3 .. 4e-3 of the peak from
fd_* on eus_L68 at 6 s and 2e-6 .. 8e-6 from the same differences taken at its own layer values).  So every quantity
above except mmax, zreg and zliq is stored a second time with 32 after its first word (lay32, c32, chi32, dchidc32,
fd32_vs, part32_vs, dc32_vs, fd32_err, ...): the same float64 differences of the same float64 functions, with every
layer value multiplied by the fixed factor that carries it, at the unstepped model, to the fp32 value of the library's
prep stage (thickcheck_lib.layers32, a numpy restatement) - the caller-coordinate derivatives at the kernel's own layers.

Every unit is also solved by the project's CPU oracle (oracle.cport, surfdisp_oracle_forward_dbg) as a P = 1 call; the
fixture is not written unless the oracle solves each of them (deepwater_L9 with 5 km at 6 and 10 s does).

    python tests/golden/make_golden_ellip.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import secular64 as S                                      # noqa: E402
from make_golden_thickness import (NAMES, PERIODS, TWOPI32, cut, cut_index, flatten64, root_near, root_scan)   # noqa: E402

DEEP = "deepwater_L9"
DEEP_H0, DEEP_PERIODS = 5.0, (6.0, 10.0)
DREL, DCREL = 1.0e-5, 1.0e-6
ROWS = (("vs", 1), ("vp", 0), ("rho", 2))
# A column whose differences at 1e-5 are rounding, not truncation: at 6 s synth_L5 is its 40 km top layer over a half space
# it does not feel, chi hardly depends on any density (peak 1.8e-6 per g/cm^3 where chi = 0.68) and the 2e-11 that the root's
# last bit leaves in a difference at 1e-5 is 1e-5 of that peak.  A larger step, still far inside the linear range.
STEP = {("synth_L5", 6.0, "rho"): 2.0e-4}


def models():
    fix = np.load(os.path.join(HERE, "ref_eigen.npz"))
    out = {n: np.asarray(fix[f"{n}_model"], np.float32) for n in NAMES}
    deep = out["water_L9"].copy()
    deep[3, 0] = DEEP_H0
    out[DEEP] = deep
    return out


def units():
    return [(n, T) for n in NAMES for T in PERIODS] + [(DEEP, T) for T in DEEP_PERIODS]


def D(lay, c, om, start):
    """The recursion from e_start to the half-space row."""
    T = 2.0 * np.pi / om                                   # secular64 forms k = 2 pi / (c T)
    a, b, rho, d = lay["a"], lay["b"], lay["rho"], lay["d"]
    last = a.size - 1
    s = tuple(1.0 if q == start - 1 else 0.0 for q in range(5))
    for m in range(last):
        s, _ = S.ray_step(s, c, T, a[m], b[m], d[m], rho[m], rho[m - 1] if m else 0.0, start, m == 0)
    return S.ray_close(s, c, T, a[last], b[last], rho[last], rho[last - 1], start)[0]


def chi_at(lay, c, om):
    return 0.5 * D(lay, c, om, 3) / D(lay, c, om, 2)


def base(m32, T, k32=False):
    """The unit's float64 inputs, omega, cut index, the function model -> cut layer values, and the root.  k32: every
    layer value scaled by the fixed factor that carries it, at the unstepped model, to the fp32 value the library's own
    prep stage holds (thickcheck_lib.layers32) - the same relative derivatives, taken at the kernel's layer values."""
    m0 = np.asarray(m32, np.float32).astype(np.float64)
    om = TWOPI32 / T
    mmax = cut_index(m0, T)
    lay0, f0 = flatten64(m0, T, "R")
    wet = not (m0[1, 0] > 0)
    fac = {k: np.ones(m0.shape[1]) for k in lay0}
    if k32:
        import thickcheck_lib
        l32 = thickcheck_lib.layers32(m32, T, "R")
        for k in fac:
            nz = lay0[k] != 0
            fac[k][nz] = l32[k][nz] / lay0[k][nz]
            assert np.abs(fac[k] - 1.0).max() < 1e-2, (k, fac[k])

    def layers(m):
        lay = flatten64(m, T, "R", f0 if wet else None)[0]
        return cut({k: v * fac[k] for k, v in lay.items()}, mmax)
    lay = layers(m0)
    return m0, om, mmax, lay, layers, wet, root_scan(lay, om, "R")


def column(job):
    """One column (Vs, Vp or rho) of one unit: total, part and dc at the step and at twice the step."""
    name, T, m32, key, row, k32 = job
    m0, om, mmax, lay, layers, wet, c0 = base(m32, T, k32)
    L = m0.shape[1]
    out = np.zeros((2, 3, L))                              # [step | twice the step][total, part, dc][layer]
    for i in range(1 if wet else 0, mmax):
        for q, fac in enumerate((1.0, 2.0)):
            step = fac * STEP.get((name, T, key), DREL) * m0[row, i]
            v = []
            for s in (-1.0, 1.0):
                m = m0.copy()
                m[row, i] += s * step
                ls = layers(m)
                cs = root_near(ls, om, "R", c0)
                v.append((chi_at(ls, cs, om), chi_at(ls, c0, om), cs))
            out[q, :, i] = [(v[1][k] - v[0][k]) / (2.0 * step) for k in range(3)]
    print(f"{name} T={T:g} {key}{'32' if k32 else ''}: done", flush=True)
    return name, T, key, k32, out


def scalars(job):
    """lay, c, chi, dchidc of one unit (k32: lay32, c32, ...), and mmax, zreg, zliq."""
    name, T, m32, k32 = job
    m0, om, mmax, lay, layers, wet, c0 = base(m32, T, k32)
    L = m0.shape[1]
    rec = dict(lay=np.zeros((4, L)), c=c0, chi=chi_at(lay, c0, om))
    rec["lay"][:, :mmax] = np.stack([lay["a"], lay["b"], lay["rho"], lay["d"]])
    dc = DCREL * c0
    rec["dchidc"] = (chi_at(lay, c0 + dc, om) - chi_at(lay, c0 - dc, om)) / (2.0 * dc)
    if k32:
        return name, T, {k + "32": v for k, v in rec.items()}
    rec["mmax"] = np.int32(mmax)
    kd2 = (om / c0 * lay["d"][:mmax - 1]) ** 2
    solid = lay["b"][:mmax - 1] > 0
    zreg = np.zeros((2, 3), np.int32)
    for r, v in enumerate((lay["a"], lay["b"])):
        z = kd2[solid] * (c0 * c0 / v[:mmax - 1][solid] ** 2 - 1.0)
        zreg[r] = [(z < -1).sum(), (np.abs(z) <= 1).sum(), (z > 1).sum()]
    rec["zreg"] = zreg
    rec["zliq"] = kd2[0] * (c0 * c0 / lay["a"][0] ** 2 - 1.0) if wet else np.nan
    print(f"{name} T={T:g}: layers {mmax} c {c0:.9f} chi {rec['chi']:.9f} dchi/dc {rec['dchidc']:.6g} z {zreg.tolist()} zliq {rec['zliq']:.3f}", flush=True)
    return name, T, rec


def oracle_ratio(m32, T):
    """(c, ratio) of the project's CPU oracle, a P = 1 call."""
    from oracle import cport
    O = cport.lib()
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    m = np.ascontiguousarray(m32, np.float32)
    per = np.array([T], np.float32)
    c, u, r = (np.zeros(1, np.float32) for _ in range(3))
    O.surfdisp_oracle_forward_dbg(m.shape[1], 2, fp(m[0]), fp(m[1]), fp(m[2]), fp(m[3]), fp(m[4]), fp(per), 1, fp(c), fp(u), fp(r))
    return float(c[0]), float(r[0])


def main():
    import multiprocessing
    mods = models()
    us = units()
    out = {"names": np.array(list(NAMES) + [DEEP])}
    for n, m in mods.items():
        out[f"{n}_model"] = m
    # the deepest stacks at the longest periods first: they take the longest
    heavy = sorted(us, key=lambda u: -cut_index(mods[u[0]].astype(np.float64), u[1]))
    with multiprocessing.Pool(min(6 * len(us), os.cpu_count() or 1)) as pool:
        sc = pool.map_async(scalars, [(n, T, mods[n], k32) for n, T in us for k32 in (False, True)])
        cols = pool.map_async(column, [(n, T, mods[n], key, row, k32) for n, T in heavy for key, row in ROWS for k32 in (False, True)], chunksize=1)
        sc, cols = sc.get(), cols.get()
    unit = {u: {} for u in us}
    for n, T, rec in sc:
        unit[(n, T)].update(rec)
    for n, T, key, k32, a in cols:
        u, x = unit[(n, T)], "32" if k32 else ""
        u[f"fd{x}_{key}"], u[f"part{x}_{key}"], u[f"dc{x}_{key}"] = a[0]
        u[f"err{x}_{key}"] = np.abs(a[0, 0] - a[1, 0]).max() / np.abs(a[0, 0]).max()
    for (n, T), u in unit.items():
        for x in ("", "32"):
            u[f"fd{x}_err"] = np.array([u.pop(f"err{x}_{key}") for key, _ in ROWS])
        c, r = oracle_ratio(mods[n], T)
        print(f"{n} T={T:g}: fd_err {u['fd_err']} {u['fd32_err']} oracle c {c:.6f} ratio {r:.7f} (chi {u['chi']:.7f}, chi32 {u['chi32']:.7f})")
        if not (c > 0 and np.isfinite(r)):
            raise SystemExit(f"the oracle does not solve {n} at {T:g} s: fixture not written")
    for n in mods:                                         # per stack: its periods, and every quantity with the period first
        per = [T for m, T in us if m == n]
        out[f"{n}_periods"] = np.array(per)
        for k in unit[(n, per[0])]:
            out[f"{n}_{k}"] = np.stack([unit[(n, T)][k] for T in per])
    np.savez_compressed(os.path.join(HERE, "ellip_fd.npz"), **out)


if __name__ == "__main__":
    main()
