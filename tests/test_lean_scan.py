"""The root search's lean scan pass (pure scan passes of the default scan, two-lane teams: see LEAN in surfdisp_kernels.hip)
against the general pass body it stands in for.  Both must give the same c, U and status BIT FOR BIT: the lean body reorganises the
control flow of a scan pass and changes no arithmetic.  SURFDISP_LEANSCAN=0 sends every pass through the general body;
the knobs are read once per process, so each configuration runs in a child process of its own.

Shapes: a bench-shaped batch (ten layers, 20 periods, two-lane teams, pipelined launch), soft sediments, water on top,
ragged layer counts, Rayleigh c+U, Rayleigh phase only and Love, every team size from 1 to 64 lanes, lock step on and
off (SURFDISP_LOCKSTEP=0).  The other team sizes run the general body under both settings and pin the knob's plumbing."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from pysurfinv_amd import _lib, forward, synth

L = _lib.lib()
dev = torch.device("cuda:0")
per = torch.from_numpy(synth.default_periods(20)).to(dev)
rng = np.random.default_rng(7)
ragged = synth.synth_models(1024, 16, seed=4)
fams = {
    "sediment": (synth.sediment_models(1024, 12, seed=1), None),
    "water": (synth.sediment_models(1024, 12, seed=2, water=True), None),
    "ocean": (synth.water_models(512), None),
    "ragged": (ragged, rng.integers(2, 17, 1024).astype(np.int32)),
}
out = {}

def run(tag, model, nlay, kind, team, pipelined):
    L.surfdisp_set_team(team)
    m = torch.from_numpy(model).to(dev)
    nl = torch.from_numpy(nlay).to(dev) if nlay is not None else None
    plan = forward.BatchPlan(m.shape[0], m.shape[2], per.numel(), device=dev)
    c, u, st = plan.run(m, per, kind=kind, nlay=nl, pipelined=pipelined)
    torch.cuda.synchronize()
    out[tag + "_c"] = c.cpu().numpy().copy()
    out[tag + "_u"] = u.cpu().numpy().copy()
    out[tag + "_s"] = st.cpu().numpy().copy()

bench = synth.synth_models(16384, 10, seed=3)
run("bench_R", bench, None, 2, 2, True)
run("bench_R_default_team", bench, None, 2, 0, False)
run("bench_L", bench, None, 1, 2, True)
for name, (model, nlay) in fams.items():
    for team in (1, 2, 4, 8, 16, 32, 64):
        for kind in (2, 1, 2 | 0x10):
            run(f"{name}_{kind}_{team}", model, nlay, kind, team, team == 2)
L.surfdisp_set_team(0)
np.savez(sys.argv[2], **out)
"""


def _child(tmp_path, tag, env_extra):
    path = str(tmp_path / f"{tag}.npz")
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(path))


@pytest.mark.parametrize("lockstep", ["1", "0"])
def test_lean_scan_bit_identical(tmp_path, lockstep):
    lean = _child(tmp_path, "lean", {"SURFDISP_LEANSCAN": "1", "SURFDISP_LOCKSTEP": lockstep})
    gen = _child(tmp_path, "general", {"SURFDISP_LEANSCAN": "0", "SURFDISP_LOCKSTEP": lockstep})
    assert lean.keys() == gen.keys()
    assert (lean["bench_R_s"] == 0).all() and (lean["bench_R_c"] > 0).all()
    bad = []
    for k in sorted(lean):
        a, b = lean[k], gen[k]
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append(k)
    assert not bad, f"lean and general scan passes differ in {bad}"
