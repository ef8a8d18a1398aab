"""The double lean pass of two-lane Rayleigh teams (LEAN2 in phase_body, surfdisp_kernels.hip): a lane evaluates two grid
points one after the other and the team decides once over its four points.  No trial velocity, value or decision changes,
so c, u, status and the number of stacks handed to the exact fallback must equal, BIT FOR BIT, what the same library gives
with the lean pass switched off (SURFDISP_LEANSCAN=0: every pass takes the general body, one grid point per lane).  The
knob is read once per process: the reference leg runs in a child process of its own, the default build in this one.

Cases: tests/scan_double_cases.py (176 stacks, two-lane teams forced, pipelined launches, c+U and phase only)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import scan_double_cases as sdc   # noqa: E402
import scan_waits_cases as swc    # noqa: E402

NAMES = [f + s for f in ("L10", "mm20", "guard4", "L2", "L3", "ragged10", "water9", "sediment10", "single", "thick200")
         for s in ("_cu", "_ph")]
CHILD = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import numpy as np; import scan_double_cases as sdc; "
         "np.savez(sys.argv[3], **sdc.run_all())")


@pytest.fixture(scope="module")
def here():
    """every case with the default build, in this process"""
    return sdc.run_all()


@pytest.fixture(scope="module")
def general(tmp_path_factory):
    """every case with the lean pass switched off, in a fresh process"""
    path = str(tmp_path_factory.mktemp("scan_double") / "general.npz")
    env = dict(os.environ, SURFDISP_LEANSCAN="0")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, HERE, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def oracle_l10():
    """c of the L10 family at the cases' periods from the CPU oracle"""
    from oracle import cport
    model = dict((n, m) for n, m, _ in swc.families())["L10"]
    c, _, st = cport.forward_batch(model, swc.PERIODS, swc.KIND_RAYLEIGH, nthreads=4)
    assert (st == 0).all() and (c > 0).all()
    return model, c


def _grid(c1, npts):
    """the scan's grid from c1: repeated fp32 additions of dc (calcul.f:157,161)"""
    g = np.empty((npts,) + c1.shape, np.float32)
    g[0] = c1
    for i in range(1, npts):
        g[i] = g[i - 1] + sdc.DC
    return g


def test_crossing_falls_on_each_of_the_four_points(oracle_l10):
    """Period k >= 1 starts its scan at 0.9 c(k-1) (calcul.f:143) and a wavefront's teams start it together, on round A of a
    double pass: grid point i is the team's point i mod 4 (lane 0 A, lane 1 A, lane 0 B, lane 1 B).  From the oracle's roots,
    each of the four positions takes the crossing in at least 10 % of ALL (stack, period) pairs (the first period's pairs,
    whose start comes from the model, are counted in the total only)."""
    _, c = oracle_l10
    c1 = (np.float32(0.9) * c[:, :-1].astype(np.float32)).astype(np.float32)
    root = c[:, 1:].astype(np.float32)
    g = _grid(c1, 400)
    up = root > c1                                             # (a root below the start is no crossing of this kind)
    assert (g[-1] > root).all()
    idx = (g > root[None]).argmax(axis=0)                      # first grid point above the root
    share = [float(((idx % 4 == p) & up).sum()) / c.size for p in range(4)]
    print("share of (stack, period) pairs with the crossing at point 0..3:", share)
    assert min(share) >= 0.10, share


def test_mm_changes_between_a_lanes_two_points(oracle_l10):
    """mm20: at 8, 12.8 and 17.7 s layer dropping (surfa.f:94-105: the first layer at which the thickness of the layers faster
    than the trial passes 4 c T) moves within two grid steps somewhere along the scan of most stacks - estimated here from
    the model's own Vs and thicknesses along the grid below the period's root."""
    from oracle import cport
    model, _ = oracle_l10
    c, _, st = cport.forward_batch(model, sdc.MM_PERIODS, swc.KIND_RAYLEIGH, nthreads=4)
    assert (st == 0).all()
    vs, h = model[:, 1, :].astype(np.float32), model[:, 3, :].astype(np.float32)
    n = vs.shape[1]
    pairs = 0
    for k in range(1, len(sdc.MM_PERIODS)):
        g = _grid((np.float32(0.9) * c[:, k - 1]).astype(np.float32), 80)                    # [80, B]
        s = np.cumsum(np.where(g[:, :, None] < vs[None], h[None], np.float32(0)), axis=2)    # [80, B, L]
        cnt = (s <= (4.0 * g * sdc.MM_PERIODS[k])[:, :, None]).sum(axis=2)
        mm = np.maximum(np.where(cnt < n, cnt + 1, n), 2)
        below = g[2:] <= c[None, :, k]
        pairs += int(((mm[2:] != mm[:-2]) & below).any(axis=0).sum())
    print("(stack, period) pairs whose mm changes between grid points i and i + 2:", pairs)
    assert pairs >= sdc.B // 4


def test_two_lane_teams_ran_and_cases_solve(here, general):
    assert sorted(here) == sorted(general) == sorted(n + s for n in NAMES for s in ("_c", "_u", "_s", "_fb", "_team"))
    for n in NAMES:
        assert here[n + "_team"].tolist() == [sdc.TEAM] and general[n + "_team"].tolist() == [sdc.TEAM], n
    for n in NAMES:
        if n.startswith(("guard4", "thick200")):
            continue
        assert (general[n + "_s"] == 0).all() and (general[n + "_c"] > 0).all(), n
    for n in ("guard4_cu", "guard4_ph"):
        failed = general[n + "_s"] != 0
        assert failed.sum() >= 8 and (~failed).sum() >= 8, n


@pytest.mark.parametrize("name", ["thick200_cu", "thick200_ph"])
def test_fallback_count_equals_the_general_bodys(here, general, name):
    print(f"{name}: {int(here[name + '_fb'][0])} stacks through the exact fallback, general body {int(general[name + '_fb'][0])}")
    assert general[name + "_fb"][0] > 0
    assert here[name + "_fb"][0] == general[name + "_fb"][0]


def _differs(a, b):
    return a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_bytes_equal_the_general_body(here, general, name):
    bad = [s for s in ("_c", "_u", "_s", "_fb") if _differs(here[name + s], general[name + s])]
    for s in bad:
        d = here[name + s] != general[name + s]
        print(f"{name}{s}: {int(d.sum())} of {d.size} words differ, per period {d.sum(axis=0) if d.ndim == 2 else ''}")
    assert not bad, f"{name}: {bad} differ from the general pass body's bytes"
