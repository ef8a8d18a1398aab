#!/usr/bin/env python3
"""The reference's OWN eigenfunctions, energy integrals and amplitude response -> tests/golden/ref_eigen.npz.

REIGEN / LEIGEN leave the displacements and tractions of every sublayer of the flattened, attenuation-corrected stack in
COMMON /rar/ (dept1, ampur, ampuz, stresz, stresr, mmax; Love: amp in ampur's slot, stress in stresr's: surfa.f:389, 728),
the energy integrals in COMMON /rco1/ (sumi0..sumi3, flagr) and c, cvar, ugr, wvno, ratio, are / ale in COMMON /rco/;
nothing returns them.  This script calls the UNMODIFIED reference (oracle/_ref/libfast_surf_ref.so, built by
oracle/build_ref.sh) with ONE period at a time - the blocks are overwritten at every period - in a fresh-process state and
stores the first ``mmax`` entries next to the inputs.  Data only.  The cases are those of make_golden_partials.py.

Where the entries sit (surfa.f:1104-1108, 1145-1148, 1209-1245; Love 553-555, 499-500, 609-628): entry 0 is SET - the
free surface, or the sea floor under a water layer; the last entry (mmax - 1) is the top of the effective half space;
every entry between is the MIDDLE (kk = 3) of one sublayer, ndiv per caller layer (the water layer is not split and has
no entry of its own).  ``first`` gives, for every caller layer, the index of the entry of its first (top) sublayer - half
a sublayer below the layer's top - or -1; each is cross-checked against dept1 with the float64 flattening formulas.
Runs in the build container only:

    python tests/golden/make_golden_eigen.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from oracle import refso                                   # noqa: E402
from pysurfinv_amd import senskernel                       # noqa: E402
from make_golden_partials import cases, PERIODS            # noqa: E402


# the reference's flattened depths are fp32 differences of R0 ln(R0 / r): absolute rounding ~ R0 2^-24 = 4e-4 km
TOL = lambda z: 2e-5 * z + 1e-3


def commons():
    L = refso.lib()
    rar = np.frombuffer((ctypes.c_float * 5001).in_dll(L, "rar_"), dtype=np.float32)
    mmax = int(np.frombuffer((ctypes.c_int32 * 5001).in_dll(L, "rar_"), dtype=np.int32)[5000])
    rco1 = np.frombuffer((ctypes.c_float * 5).in_dll(L, "rco1_"), dtype=np.float32).copy()
    rco = np.frombuffer((ctypes.c_float * 6).in_dll(L, "rco_"), dtype=np.float32).copy()
    ndiv = int((ctypes.c_int32 * 9).in_dll(L, "c_")[5])
    return rar[:5000].copy().reshape(5, 1000), mmax, rco1, rco, ndiv


def main():
    out = {"periods": PERIODS, "names": np.array([n for n, _ in cases()])}
    ncap = 0
    blocks = {}
    for name, m in cases():
        m = np.ascontiguousarray(m, np.float32)
        L = m.shape[1]
        wet = not (m[1, 0] > 0)
        out[f"{name}_model"] = m
        for kind, w in ((2, "R"), (1, "L")):
            P = len(PERIODS)
            blk = np.zeros((P, 5, 1000), np.float32); meta = np.zeros((P, 12)); first = np.full((P, L), -1, np.int32)
            hsl = np.full((P, 2), -1, np.int32)
            for ip, T in enumerate(PERIODS):
                r = refso.fast_surf(L, kind, m[0], m[1], m[2], m[3], m[4], [T], 1)
                c = r[2][0] if kind == 2 else r[3][0]
                u = r[0][0] if kind == 2 else r[1][0]
                rar, mmax, rco1, rco, ndiv = commons()
                if not c > 0:
                    continue
                assert rco[0] == c and rco[2] == u, (name, w, T, rco, c, u)
                blk[ip, :, :mmax] = rar[:, :mmax]
                meta[ip] = (c, u, mmax, ndiv, rco1[0], rco1[1], rco1[2], rco1[3], rco[5], rco[2], rco[3], rco[4])
                # sublayers above the effective half space: dry, entries 1 .. mmax - 2 (shifted by one); wet, the water slot is
                # entry 0 (overwritten with the sea-floor values) and the solid sublayers are entries 1 .. mmax - 2 as well
                nsub = mmax - 2
                nd = ndiv if ndiv > 1 else 1
                split_water = wet and not (ndiv > 1)             # ndiv = 1: the water layer is an ordinary (skipped) sublayer
                lay = senskernel.flattened_layers(m, T, w)
                ztop = np.cumsum(lay["d"]) - lay["d"]
                if wet and not split_water:
                    hs_layer, nreg_hs = 1 + nsub // nd, nsub % nd
                    idx = lambda i: 1 + (i - 1) * nd if i >= 1 else -1
                elif wet:
                    hs_layer, nreg_hs = mmax - 1, 0              # entries 0 (sea floor), 1 .. : one per layer, no shift
                    idx = lambda i: i if i >= 1 else -1
                else:
                    hs_layer, nreg_hs = nsub // nd, nsub % nd
                    idx = lambda i: 1 + i * nd
                hsl[ip] = (hs_layer, nreg_hs)
                for i in range(hs_layer + (1 if nreg_hs else 0)):
                    j = idx(i)
                    if j < 0:
                        continue
                    first[ip, i] = j
                    want = ztop[i] + lay["d"][i] / nd / 2.0
                    assert abs(rar[0, j] - want) <= TOL(want), (name, w, T, i, j, rar[0, j], want)
                # the last entry holds the VALUES at the top of the effective half space (surfa.f:1145-1148, 499-500); its
                # dept1 is that top only for the true half space - for a dropped stack it is the middle of the sublayer
                # that plays the half space (depth() is formed before the layers are dropped, surfa.f:828-835)
                want = ztop[hs_layer] + nreg_hs * lay["d"][hs_layer] / nd
                if hs_layer < L - 1:
                    want += lay["d"][hs_layer] / nd / 2.0
                assert abs(rar[0, mmax - 1] - want) <= TOL(want), (name, w, T, rar[0, mmax - 1], want)
                ncap = max(ncap, mmax)
            blocks[f"{name}_{w}"] = (blk, meta, first, hsl)
            print(name, w, "c", meta[:, 0].round(4), "mmax", meta[:, 2].astype(int), "ndiv", meta[:, 3].astype(int), "hs", hsl[:, 0], hsl[:, 1])
    for key, (blk, meta, first, hsl) in blocks.items():
        out[f"{key}_rar"] = blk[:, :, :ncap]                  # [P][dept1, ampur | amp, ampuz, stresz, stresr | stress][entry], float32
        out[f"{key}_meta"] = meta                             # [P][c, U, mmax, ndiv, sumi0, sumi1, sumi2, sumi3, are | ale, ugr, wvno, ratio]
        out[f"{key}_first"] = first                           # [P][L] entry of each caller layer's first sublayer, -1: none
        out[f"{key}_hs"] = hsl                                # [P][effective half-space layer, sublayers of it above the cut]
    out["flang"] = np.array(open(os.path.join(os.path.dirname(refso._SO), "BUILD_INFO.txt")).read())
    np.savez_compressed(os.path.join(HERE, "ref_eigen.npz"), **out)


if __name__ == "__main__":
    main()
