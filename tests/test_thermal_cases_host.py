"""The thermal-layer case set (tests/thermal_cases.py) on the CPU: every setting takes the native path, the rows
between them reach every branch of surfdisp_thermal_kernel, every row is clear of every decision boundary (so that
the last bits of a device erf / exp cannot flip a decision the float64 statement took), and the rule of
thermseis.cubic_spline_through for rows with fewer than two knots is what its docstring says."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import thermal_cases as tc                                              # noqa: E402
from pysurfinv_amd import thermseis as ts                               # noqa: E402

NAMES = list(tc.CASES)
_REPORT = {}


def report(name):
    if name not in _REPORT:
        p, r, hand = tc.rows(name)
        _REPORT[name] = (tc.decision_report(tc.model(name), p, r), p, hand)
    return _REPORT[name]


def conversion(name):
    return tc.CASES[name]["setting"]["OceanMantleHybrid"]["Conversion"]


@pytest.mark.parametrize("name", NAMES)
def test_settings_are_static_and_native(name):
    mb = tc.model(name)
    assert mb._static_sig is not None
    assert mb._static_sig[-1] + 1 == tc.CASES[name]["npts"]
    assert mb.native_descriptor() is not None
    assert mb._native_thermal is True
    p, r, hand = tc.rows(name)
    assert p.shape[0] <= tc.MAX_ROWS and p.shape[1] == mb.spec.n
    ia = list(mb.spec.names).index(tc.AGE_NAME)
    assert float(p[hand["age_zero"], ia]) == 0.0
    assert float(p[hand["age_below_clamp"], ia]) == 5e-4
    assert float(p[hand["age_max"], ia]) == float(mb.spec.vmax[ia])
    if tc.TP_NAME in mb.spec.names:
        assert float(p[hand["tp_1325"], list(mb.spec.names).index(tc.TP_NAME)]) == 1325.0


def test_layouts_the_case_set_must_hold():
    """The layouts and options the kernel's descriptor distinguishes."""
    sets = {n: c["setting"] for n, c in tc.CASES.items()}
    assert {c["npts"] for c in tc.CASES.values()} == {6, 11, 16, 31, 61}
    assert {conversion(n) for n in NAMES} == {"Ritzwoller", "Yamauchi"}
    assert any(not s["Info"]["lithoAgeQ"] for s in sets.values()) and any(s["Info"]["lithoAgeQ"] for s in sets.values())
    assert any(len(s["OceanMantleHybrid"]["Vs"]) == 7 for s in sets.values())        # + the leading zero: 8 basis slots
    assert any(tc.TP_NAME in tc.model(n).spec.names for n in NAMES)
    for name in ("nowater_ritz", "nowater_yama"):
        mb = tc.model(name)
        assert [lay["kind"] for lay in mb.layers] == ["osed", "ocrust", "hybrid"]
        names = set(mb.spec.names)
        assert {"OceanSediment.H", "OceanSediment.Vs", "OceanCrust.H", "OceanCrust.Vs[0]", "OceanCrust.Vs[1]",
                "OceanMantleHybrid.BottomDepth", tc.AGE_NAME} <= names
        assert tc.TP_NAME not in names and sets[name]["OceanMantleHybrid"]["Tp"] == 1325
        assert sets[name]["Info"]["lithoAgeQ"] is True
        ia = list(mb.spec.names).index(tc.AGE_NAME)
        assert (mb.spec.vmin[ia], mb.spec.vmax[ia]) == (0.0, 180.0)
        assert mb.aux_names == ["topo", "lithoAge", "period"]
        table = np.asarray(tc.CASES[name]["table"], float)
        assert table.shape[0] >= 3
        assert (table[:, 0] < 0).any() and (table[:, 0] == 0).any() and (table[:, 0] > 0).any()
        assert table[:, 1].min() == 10.0 and table[:, 1].max() == 170.0
        _, r, _ = tc.rows(name)
        assert set(r.tolist()) == set(range(table.shape[0]))


def test_case_set_reaches_every_branch():
    """Fails when a case or a hand-set row is taken away so that a branch of the kernel is no longer run."""
    reps = {n: report(n) for n in NAMES}
    knots = set()
    for n, (rep, _, _) in reps.items():
        knots |= set(rep["nknots"].tolist())
        assert (rep["nknots"] == tc.CASES[n]["npts"]).any(), f"{n}: no row keeps every grid point"
    assert {0, 1, 2, 3, 4} <= knots                        # line from non-knots (0, 1), line, parabola, smallest general system
    assert any((rep["melt_index"] < 0).any() for rep, _, _ in reps.values())          # "no depth is hot"
    assert any((rep["melt_index"] >= 0).any() for rep, _, _ in reps.values())
    assert any((rep["z_melt"] <= 0).any() for rep, _, _ in reps.values())             # melting at or above the crust
    for n, (rep, _, hand) in reps.items():
        assert rep["age_clamped"][hand["age_zero"]] and rep["age_clamped"][hand["age_below_clamp"]], n
        assert not rep["age_clamped"][hand["age_max"]], n
    sampled_tp = [n for n in NAMES if tc.TP_NAME in tc.model(n).spec.names]
    assert sampled_tp
    for n in sampled_tp:                                   # Tp == 1325 as a sampled value, among rows where it is not
        rep, _, hand = reps[n]
        assert rep["tp_default"][hand["tp_1325"]] and not rep["tp_default"][: tc.CASES[n]["n"]].any(), n
    assert any(rep["tp_default"].all() for rep, _, _ in reps.values())                # and as the constant
    assert any(rep["q_is_age"].any() for rep, _, _ in reps.values())
    assert any((~rep["q_is_age"]).any() for rep, _, _ in reps.values())
    every = set(range(6))
    for conv in ("Ritzwoller", "Yamauchi"):
        seen = set()
        for n in NAMES:
            if conversion(n) == conv:
                seen |= set(np.unique(reps[n][0]["tn_vs"]).tolist())
        assert seen == every, (conv, seen)
    seen = set()
    for rep, _, _ in reps.values():
        seen |= set(np.unique(rep["tn_qs"]).tolist())
    assert seen == every, seen
    assert any(rep["qs_capped"].any() for rep, _, _ in reps.values())
    assert any((~rep["qs_capped"]).any() for rep, _, _ in reps.values())


@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_clear_of_every_decision_boundary(name):
    """A condition on the case set, not a tolerance on the kernel: no row is exempt; a row that fails means another
    seed.  (2 000 draws per setting: smallest knot margin 1.4e-4 km, smallest melt margin 1.7e-7.)"""
    rep, _, _ = report(name)
    for key, bar in (("m_g", 1e-6), ("m_melt", 1e-9), ("m_knot", 1e-9), ("m_adia", 1e-9)):
        worst = int(np.argmin(rep[key]))
        print(f"{name}: smallest {key} {rep[key][worst]:.3e} (row {worst}, bar {bar:g})")
        assert np.isfinite(rep[key]).all(), key
        assert rep[key][worst] >= bar, (key, worst, rep[key][worst])


def test_fewer_than_two_knots_is_the_line_through_the_first_two_entries():
    """Rows with no kept point, or one: order the grid points as "kept points, then the others in grid order";
    the result is the line through the first two entries of that order, at every grid point."""
    rng = np.random.default_rng(7)
    N = 6
    kept = [None, None, 0, 1, 3, 5]                        # no knot (twice), one knot at the top / inside / at the bottom
    B = len(kept)
    x = np.sort(rng.uniform(0, 3, (B, N)), axis=1)
    x[1] = np.linspace(0.0, 3.1, N)                        # a layer's own grid
    y = 4.4 + 0.1 * rng.normal(size=(B, N))
    keep = np.zeros((B, N), bool)
    want = np.empty((B, N))
    for b, k in enumerate(kept):
        if k is not None:
            keep[b, k] = True
        order = [j for j in range(N) if keep[b, j]] + [j for j in range(N) if not keep[b, j]]
        i0, i1 = order[:2]
        slope = (y[b, i1] - y[b, i0]) / (x[b, i1] - x[b, i0])
        want[b] = y[b, i0] + (x[b] - x[b, i0]) * slope
    got = ts.cubic_spline_through(torch.as_tensor(x), torch.as_tensor(y), torch.as_tensor(keep)).numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], y[0, 0] + (x[0] - x[0, 0]) * ((y[0, 1] - y[0, 0]) / (x[0, 1] - x[0, 0])))


def test_short_knot_rows_of_the_case_set_follow_that_rule():
    """The same statement on the thermal layer itself: the mirror's grid Vs of the no-knot and one-knot rows of the
    3 km layer lies on one line per row, through its first two ordered entries."""
    rep, p, _ = report("bd13_yama")
    mb = tc.model("bd13_yama")
    mb.to_model_torch(p)
    vs = mb.layers[-1]["grid_last"][0].numpy()
    short = np.where(rep["nknots"] < 2)[0]
    assert (rep["nknots"][short] == 0).any() and (rep["nknots"][short] == 1).any()
    t = np.linspace(0.0, 1.0, vs.shape[1])
    for b in short:
        line = np.polyfit(t, vs[b], 1)
        assert np.max(np.abs(np.polyval(line, t) - vs[b])) < 1e-12, b
    full = np.where(rep["nknots"] >= 3)[0]
    assert any(np.max(np.abs(np.polyval(np.polyfit(t, vs[b], 1), t) - vs[b])) > 1e-6 for b in full)
