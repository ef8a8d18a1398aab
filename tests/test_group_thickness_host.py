"""Thickness kernels of the group velocity, without a GPU (include/surfdisp.h section (5h)).

1. The rule itself, float64 only: senskernel.group_thickness_reference on the float64 thickness rows of
   tests/golden/group_thickness_fd.npz (tests/golden/make_golden_group_thickness.py: dcdh of thickness_kernels_reference at omega
   exp(+-ln((1 + d) / (1 - d)) / 2), layer values frozen at the period) against the central differences of the structural U with
   respect to every thickness: the error is that of the central difference in ln T, so it falls by a factor of four from d = 0.01
   to d = 0.005 - a factor between 3 and 5 on every unit whose d = 0.005 figure stands above the difference quotient's own noise
   (the change of the stored differences under a halved step).  No tolerance is chosen; a wrong sign or factor of either term
   leaves an error that does not fall.
2. What the attenuation correction at the SHIFTED period costs - the device's convention of section (5c): the same rule on the
   float64 rows formed that way, dU/dh against dU/dVs; A_Uh <= FD_RATIO_BAR x A_Ub (group_thickness_lib).
3. The argument rules of the thickness modes with group-velocity data.

Measured (profiles/group_thickness/parity.txt): see the docstrings."""
import numpy as np
import pytest

import group_thickness_lib as GL
import thickcheck_lib as TL
from pysurfinv_amd import _lib, linearized, synth
from pysurfinv_amd.obsdata import DispersionData


def test_fixture_covers_the_units_of_thickness_fd():
    assert GL.NAMES == TL.FD_NAMES and GL.PERIODS == TL.FD_PERIODS and GL.DELTAS == [0.01, 0.005]
    steps = GL.FDG["steps_h"]
    assert steps[1] == 0.5 * steps[0]
    for name in GL.NAMES:
        for w in ("R", "L"):
            for T in GL.PERIODS:
                f, t = GL.fd_rows(name, w, T), TL.fd_unit(name, w, T)
                assert abs(f["c"] - t["c"]) <= 1e-12 * t["c"] and abs(f["u"] - t["u"]) <= 1e-9 * t["u"]      # the same units
                mmax = int(TL.FD[f"{name}_{w}_mmax"][GL.PERIODS.index(T)])
                assert not f["fd_uh"][:, mmax - 1:].any() and f["fd_uh"][:, :2].all()                        # the same layer cut


@pytest.mark.parametrize("w", ["R", "L"])
def test_rule_converges_at_second_order(w):
    """Measured: see profiles/group_thickness/parity.txt (every unit's two figures, their ratio and the noise)."""
    worst_noise_share, n_exempt, ratios = 0.0, 0, []
    for name in GL.NAMES:
        for T in GL.PERIODS:
            f = GL.fd_rows(name, w, T)
            fig = [TL.figure(GL.rule(f, f["rows_h"][di], d), f["fd_uh"][1]) for di, d in enumerate(GL.DELTAS)]
            noise = TL.figure(f["fd_uh"][0], f["fd_uh"][1])
            exempt = fig[1] < noise
            print(f"{name} {w} T={T:g}: figure {fig[0]:.3e} (d = 0.01) {fig[1]:.3e} (d = 0.005) ratio {fig[0] / fig[1]:.3f}; the differences' "
                  f"own half-step change {noise:.1e}{'  (below it: no ratio asked)' if exempt else ''}")
            worst_noise_share = max(worst_noise_share, noise / fig[1])
            if exempt:
                n_exempt += 1
                continue
            ratios.append(fig[0] / fig[1])
            assert 3.0 <= fig[0] / fig[1] <= 5.0, (name, w, T, fig)
    print(f"{w}: ratios {min(ratios):.3f} .. {max(ratios):.3f} on {len(ratios)} units, {n_exempt} below the noise; the half-step change is at most "
          f"{worst_noise_share:.3f} of a d = 0.005 figure")
    assert len(ratios) >= 15                                # (20 units per wave type)


@pytest.mark.parametrize("w", ["R", "L"])
def test_cost_of_the_moving_attenuation_correction(w):
    """A_Uh <= FD_RATIO_BAR x A_Ub on float64 rows with the correction at the shifted period.  The ratio recorded in
    group_thickness_lib.FD_RATIO_MEASURED is the one measured here (to 1 %), so the bar the GPU test uses is this measurement."""
    A_h, A_b, units = GL.moving_figures(w)
    for name, T, a_h, a_b in units:
        print(f"{name} {w} T={T:g}: A_Uh {a_h:.2e} A_Ub {a_b:.2e}")
    ratio = A_h / A_b
    print(f"{w}: float64, correction at the shifted period: A_Uh = {A_h:.3e}, A_Ub = {A_b:.3e}, ratio {ratio:.3f} (bar {GL.FD_RATIO_BAR[w]:.3f})")
    rec = GL.FD_RATIO_MEASURED[w]
    assert rec is not None and abs(rec - ratio) <= 0.01 * ratio
    assert (GL.FD_RATIO_BAR[w] == 4.0) == (ratio <= 4.0)
    assert A_h <= GL.FD_RATIO_BAR[w] * A_b


def test_group_modes_argument_rules_need_no_gpu():
    per = synth.default_periods(6)
    model = synth.synth_models(3, 8, seed=1)
    v = np.full(per.size, 3.5)
    c = DispersionData("R", "c", per, v, 0.01 * v)
    u = DispersionData("R", "U", per, v, 0.01 * v)
    uL = DispersionData("L", "U", per, v, 0.01 * v)
    e = DispersionData("R", "E", per, np.full(per.size, 0.7), np.full(per.size, 0.01))
    T = linearized.interface_mode(model[0, 3], [0, 1, 2], [3, 4])
    # past the mode checks: the next thing that can fail is the device itself
    for data in ([c, u], [u, uL]):
        with pytest.raises(_lib.SurfdispError, match="needs a HIP device"):
            linearized.LinearizedBatch(model, data, modes=T[None], group_modes=True, device="cpu")
    for kw in ({}, dict(group_modes=False)):
        with pytest.raises(ValueError, match="thickness modes need phase-velocity data only: the library has no dU/dh or dchi/dh yet"):
            linearized.LinearizedBatch(model, [c, u], modes=T[None], device="cpu", **kw)
    with pytest.raises(ValueError, match="the library has no dchi/dh"):
        linearized.LinearizedBatch(model, [c, e], modes=T[None], group_modes=True, device="cpu")
    with pytest.raises(ValueError, match="modes"):          # the shape rule comes first, as before
        linearized.LinearizedBatch(model, [c, u], modes=np.zeros((9, 8)), group_modes=True, device="cpu")


def test_reference_is_the_rule_of_the_phase_partials():
    from pysurfinv_amd import senskernel
    rng = np.random.default_rng(3)
    c, u = rng.uniform(3, 4, (5, 1)), rng.uniform(2.5, 3.5, (5, 1))
    hm, hp = rng.normal(size=(5, 9)), rng.normal(size=(5, 9))
    got = senskernel.group_thickness_reference(c, u, hm, hp, GL.dln(0.01))
    assert np.array_equal(got, senskernel.group_from_phase_partials(c, u, hm, hp, GL.dln(0.01)))
    r = u / c
    assert np.allclose(got, r * (2 - r) * 0.5 * (hm + hp) - r * r * (hp - hm) / np.log(1.01 / 0.99), rtol=1e-14, atol=0)
