"""CPU tests of the eigenfunction instantiations (group_rayleigh<false, true> / group_love<false, true> compiled for the
host, tests/hostcheck/eigencheck.hip) against the reference's own COMMON /rar/, /rco1/, /rco/ blocks
(tests/golden/ref_eigen.npz), at the reference's own c and ratio.

Measured on the fixture, 48 + 48 solved units (profiles/eigen/parity.txt; bars in brackets):
  1. layer tops against the reference, per component, fraction of the component's largest value   R 7.9e-7  L 8.9e-7  [1e-4]
     I0, I1, I2 (Rayleigh), amp against are / ale x sqrt(6.28318) 1e15                             R 5.1e-7  L 9.4e-7  [1e-4]
  2. layer-by-layer consistency figure (error / fp32 rounding carried through the exact propagator), interior layers and
     the layer under the set entry (whose tractions are set to 0, not integrated: the root's residual shows there):
     the reference's own values  R 2.30e4, 1.57e4;  L 2.56e2, 3.38e4   (R: the Runge-Kutta error of 4 steps per layer, ndiv = 1)
     the library's               R 1.61e4, 8.3e3;   L 2.6e1,  3.3e3    [8 x the reference's]
"""
import numpy as np
import pytest

import eigen_ref as E
from eigencheck_lib import eigenlib, finish  # noqa: F401

BAR = 1e-4
AMP_CONST = 1e-15 / np.sqrt(6.28318)              # are = ale = amp x this (surfa.f:1191, 608)


@pytest.fixture(scope="module")
def host(eigenlib):  # noqa: F811
    """Per wave type and case: the host instantiation's layer tops [P, 4, L] (divided by the unit's divisor), the raw stores,
    div, hs, I [P, 3] and u [P], at the reference's c and ratio of every period."""
    out = {}
    for w, kind in (("R", 2), ("L", 1)):
        for name in E.NAMES:
            m = np.asarray(E.FIX[f"{name}_model"], np.float32)
            meta = E.FIX[f"{name}_{w}_meta"]
            u, vals, div, hs, I = eigenlib.group(m, E.PERIODS, kind, meta[:, 0], meta[:, 11])
            out[w, name] = dict(tops=finish(vals, div, hs, kind)[0], vals=vals[0], div=div[0], hs=hs[0], I=I[0], u=u[0])
    return out


def comps(h, ip, w):
    return h["tops"][ip] if w == "R" else h["tops"][ip][[0, 3]]


@pytest.mark.parametrize("w", ["R", "L"])
def test_layer_tops_against_reference(host, w):
    worst, worst_i, n = 0.0, 0.0, 0
    for un in E.units(w):
        h = host[w, un["name"]]
        ip = un["ip"]
        assert h["hs"][ip] == un["hs"], (un["name"], un["T"])
        if w == "L":                                  # (the low-amplitude exclusion would zero an entry: none on these stacks)
            assert np.all(np.abs(comps(h, ip, w)[0][: un["hs"] + 1][1 if un["wet"] else 0:]) >= 1e-20)
        worst = max(worst, E.parity(comps(h, ip, w), un, w))
        lim = 3 if w == "R" else 2                    # Love: I2 is 0 by definition (the reference's sumi2 is another integral)
        ei = np.abs(h["I"][ip][:lim].astype(np.float64) / un["sums"][:lim] - 1).max()
        assert w == "R" or h["I"][ip][2] == 0
        amp = 1.0 / (2.0 * float(un["c"]) * float(h["u"][ip]) * float(h["I"][ip][0]))
        ei = max(ei, abs(amp * AMP_CONST / un["are"] - 1))
        worst_i = max(worst_i, ei)
        n += 1
    print(f"\n{w}: {n} units, layer tops worst {worst:.2e}, integrals and amp worst {worst_i:.2e} (bar {BAR:.0e})")
    assert n >= 40
    assert worst < BAR and worst_i < BAR


@pytest.mark.parametrize("w", ["R", "L"])
def test_layer_by_layer_consistency(host, w):
    ref = np.array([E.consistency_ref(un, w) for un in E.units(w)])
    lib = np.array([E.consistency_lib(comps(host[w, un["name"]], un["ip"], w), un, w) for un in E.units(w)])
    ri, rs = ref.max(axis=0)
    li, ls = lib.max(axis=0)
    print(f"\n{w}: consistency figure, reference interior {ri:.3e} set entry {rs:.3e}; library interior {li:.3e} set entry {ls:.3e} (bar 8 x)")
    assert li <= 8.0 * ri and ls <= 8.0 * rs


@pytest.mark.parametrize("w", ["R", "L"])
def test_identities(host, w):
    for un in E.units(w):
        h = host[w, un["name"]]
        ip = un["ip"]
        t = h["tops"][ip]
        e = 1 if un["wet"] else 0
        if w == "R":
            assert t[0, e] / t[1, e] == un["ratio"] and t[1, e] == 1.0 and t[3, e] == 0.0
            if not un["wet"]:
                assert t[2, 0] == 0.0
            k, om = E.wavenumbers32(un["c"], un["T"])
            I = h["I"][ip].astype(np.float64)
            U = (k * I[1] + I[2]) / (om * I[0])
        else:
            assert t[0, e] == 1.0 and t[3, e] == 0.0 and np.all(t[1] == 0) and np.all(t[2] == 0)
            I = h["I"][ip].astype(np.float64)
            U = I[1] / (float(un["c"]) * I[0])
        if un["wet"]:
            assert np.all(t[:, 0] == 0)
        assert np.all(t[:, un["hs"] + 1:] == 0)
        assert abs(U / float(h["u"][ip]) - 1) <= 4 * E.EPS, (un["name"], un["T"], U, h["u"][ip])


def test_planted_defects(host):
    """Each defect, planted on the library's values, fails test 1 or test 2."""
    def worst(w, plant):
        return max(E.parity(plant(comps(host[w, un["name"]], un["ip"], w).copy(), host[w, un["name"]], un), un, w) for un in E.units(w))

    # the Love scale dropped: the stores as the lane leaves them
    assert worst("L", lambda t, h, un: h["vals"][un["ip"]][[0, 1]] * (np.arange(t.shape[1]) <= un["hs"])) > BAR
    # the entry of layer i stored at i + 1
    shift = lambda t, h, un: np.concatenate([t[:, :1], t[:, :-1]], axis=1)
    assert worst("R", shift) > BAR and worst("L", shift) > BAR
    # tz and tr swapped
    assert worst("R", lambda t, h, un: t[[0, 1, 3, 2]]) > BAR

    # the wet stack's shift ignored: the set entry at the sea surface
    def noshift(t, h, un):
        if un["wet"]:
            t[:, 0] = t[:, 1]
        return t
    assert worst("R", noshift) == np.inf and worst("L", noshift) == np.inf
    # ... and each leaves the unplanted values inside the bar
    assert worst("R", lambda t, h, un: t) < BAR and worst("L", lambda t, h, un: t) < BAR
