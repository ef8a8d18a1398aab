"""The forward solve's trims (surfdisp_kernels.hip: the wave-uniform skip of layer_coef's sinh series, the group kernel's no-drop
shortcut, the Rayleigh group kernel's layer stash) remove work whose result is thrown away and change no arithmetic: c, u and
status must equal, BYTE FOR BYTE, what the commit before them computed.

tests/golden/forward_trims_parent.npz holds those outputs, recorded on the GPU from a build of the parent commit loaded
through SURFDISP_LIB_PATH (scripts/record_forward_trims.py) - never from the code under test.  The cases
(tests/forward_trims_cases.py): 192 stacks (one and a half workgroups of two-lane teams) at the periods 8, 12.8, 30, 60, 95
and 100 s - units that drop layers and units that cannot, |x| on both sides of 1/4 in layer_coef; Rayleigh c+U with
four-lane teams and, pipelined, with two-lane lean teams; Love c+U; ten layers (the stash is on, except in the pipelined
launches) and 11 / 14 layers (it is off); soft sediments; a water layer on top; ragged layer counts.

Each case is run twice: in this process with the library's defaults, and in a fresh child process with
SURFDISP_GROUP_STASH=0 (the knobs are read once per process), which sends the ten-layer launches through the recompute
path too.  Both must give the parent's bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import forward_trims_cases as ftc   # noqa: E402

NAMES = ["L10_R", "L10_Rp", "L10_Love", "L11_Rp", "L14_R", "sediment10_R", "water9_Rp", "water9_Love", "ragged10_Rp",
         "ragged14_R"]


@pytest.fixture(scope="module")
def parent():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "forward_trims_parent.npz")))


@pytest.fixture(scope="module")
def here():
    """every case with the library's defaults, in this process"""
    return ftc.run_all()


@pytest.fixture(scope="module")
def no_stash(tmp_path_factory):
    """every case in a fresh child process with SURFDISP_GROUP_STASH=0"""
    path = str(tmp_path_factory.mktemp("trims") / "no_stash.npz")
    env = dict(os.environ)
    env["SURFDISP_GROUP_STASH"] = "0"
    env.pop("SURFDISP_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "record_forward_trims.py"), path], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(path))


def test_cases_are_the_recorded_ones(parent):
    assert [c[0] for c in ftc.cases()] == NAMES
    assert sorted(parent) == sorted(n + s for n in NAMES for s in ("_c", "_u", "_s"))
    for n in NAMES:
        # every unit of every case is solved: the comparison below is about real roots and group velocities
        assert (parent[n + "_s"] == 0).all() and (parent[n + "_c"] > 0).all() and (parent[n + "_u"] > 0).all()
        assert parent[n + "_c"].shape == (ftc.B, len(ftc.PERIODS))


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


@pytest.mark.parametrize("name", NAMES)
def test_bytes_equal_the_parent_build_without_the_stash(parent, no_stash, name):
    bad = [s for s in ("_c", "_u", "_s") if _differs(no_stash[name + s], parent[name + s])]
    assert not bad, f"{name} with SURFDISP_GROUP_STASH=0: {bad} differ from the parent build's bytes"
