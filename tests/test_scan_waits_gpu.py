"""The lean scan pass of two-lane Rayleigh teams (surfdisp_kernels.hip, LEAN_BHS in phase_body) tests the scan's upper guard with
the half-space velocity that the evaluation hands back instead of reading the same LDS word again.  No trial velocity, value
or decision of any lane changes: c, u and status must equal, BYTE FOR BYTE, what the parent commit computed.

tests/golden/scan_waits_parent.npz holds those outputs, recorded on the GPU from a build of the parent commit loaded
through SURFDISP_LIB_PATH (scripts/record_scan_waits_parent.py) - never from the code under test.  The cases
(tests/scan_waits_cases.py): 176 stacks (one workgroup of two-lane teams plus a wavefront and a half) at 3, 5, 8, 12.8, 30,
60 and 100 s, as c+U and as phase only: two, three and ten layers, ragged layer counts, a water layer on top, soft
sediments, and a family in which every other stack's scan ends on the upper guard.  Every launch is a pipelined one with the
team forced to two lanes (surfdisp_set_team): by itself the library gives 176 stacks a wavefront each, and that kernel has
no lean pass.  The recording and the run under test both carry the lanes per stack the library reports for the launch."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import scan_waits_cases as swc   # noqa: E402

NAMES = [f + s for f in ("L2", "L3", "L10", "ragged10", "water9", "sediment10", "guard4") for s in ("_cu", "_ph")]
SOLVED = [n for n in NAMES if not n.startswith("guard4")]


@pytest.fixture(scope="module")
def parent():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "scan_waits_parent.npz")))


@pytest.fixture(scope="module")
def here():
    """every case with the library under test, in this process"""
    return swc.run_all()


def test_cases_are_the_recorded_ones(parent):
    assert [c[0] for c in swc.cases()] == NAMES
    assert sorted(parent) == sorted(n + s for n in NAMES for s in ("_c", "_u", "_s", "_team"))
    for n in NAMES:
        assert parent[n + "_c"].shape == (swc.B, len(swc.PERIODS))
        assert parent[n + "_u"].shape == (swc.B, len(swc.PERIODS))
        assert parent[n + "_s"].shape == (swc.B,)
    for n in SOLVED:
        # every unit of these cases is solved: the comparison below is about real roots (and group velocities)
        assert (parent[n + "_s"] == 0).all() and (parent[n + "_c"] > 0).all()
        if n.endswith("_cu") and n != "L2_cu":
            assert (parent[n + "_u"] > 0).all()


def test_two_lane_teams_ran(parent, here):
    """the recording and this run launched two-lane teams - the only root search with a lean pass - in every case, and the
    forcing is gone again"""
    from pysurfinv_amd import _lib
    for n in NAMES:
        assert parent[n + "_team"].tolist() == [swc.TEAM] and here[n + "_team"].tolist() == [swc.TEAM], n
    assert _lib.lib().surfdisp_get_team2(swc.B, 10, len(swc.PERIODS), swc.KIND_RAYLEIGH | swc.PIPELINED) == 64


def test_two_layer_group_velocity_is_the_references(parent):
    """U of a two-layer stack with a 100 km top layer at 3 s is NaN with status 0 for about half of the family - and so it is
    in the reference's own arithmetic (the CPU oracle): the same units, nothing the root search or this change makes.  The
    byte comparison holds those words as well."""
    from oracle import cport
    from pysurfinv_amd import synth
    u = parent["L2_cu_u"]
    _, uo, so = cport.forward_batch(synth.synth_models(swc.B, 2, seed=32), swc.PERIODS, swc.KIND_RAYLEIGH, nthreads=4)
    assert (so == 0).all() and np.array_equal(np.isnan(u), np.isnan(uo))
    assert np.isnan(u[:, 1:]).sum() == 0 and (u[~np.isnan(u)] > 0).all()


@pytest.mark.parametrize("name", ["guard4_cu", "guard4_ph"])
def test_guard_family_fails_and_solves(parent, name):
    """at least 8 stacks whose scan ends on the upper guard (a failed period: status != 0, c = 0 from there on) and at
    least 8 that solve every period - in the recorded parent outputs and on the CPU oracle the seed was chosen with"""
    from oracle import cport
    st, c = parent[name + "_s"], parent[name + "_c"]
    failed, solved = st != 0, (st == 0) & (c > 0).all(axis=1)
    print(f"{name}: {int(failed.sum())} stacks fail, {int(solved.sum())} solve every period")
    assert failed.sum() >= 8 and solved.sum() >= 8
    assert ((c[failed] > 0).sum(axis=1) < len(swc.PERIODS)).all()
    co, _, so = cport.forward_batch(swc.guard_models(), swc.PERIODS, swc.KIND_RAYLEIGH, nthreads=4)
    assert (so != 0).sum() >= 8 and ((so == 0) & (co > 0).all(axis=1)).sum() >= 8
    assert np.array_equal(so != 0, failed)


def _differs(a, b):
    return a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_bytes_equal_the_parent_build(parent, here, name):
    bad = [s for s in ("_c", "_u", "_s") if _differs(here[name + s], parent[name + s])]
    if bad:
        for s in bad:
            d = here[name + s] != parent[name + s]
            print(f"{name}{s}: {int(d.sum())} of {d.size} words differ, per period {d.sum(axis=0) if d.ndim == 2 else ''}")
    assert not bad, f"{name}: {bad} differ from the parent build's bytes"
