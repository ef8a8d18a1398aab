"""The cases of tests/test_scan_waits_gpu.py, shared with scripts/record_scan_waits_parent.py (which records the same cases
from a build of the parent commit into tests/golden/scan_waits_parent.npz).

B = 176 stacks: one workgroup of two-lane teams (128 stacks) plus a wavefront and a half.  Periods 3 ... 100 s: the short
ones drop layers of the 200 km stacks, 30 s and longer cannot.  Every case runs as a pipelined launch with the team FORCED
to two lanes (surfdisp_set_team(2): left to itself the library gives a batch this small a whole wavefront per stack, whose
kernel has no lean pass), as c+U and as phase only: the lean scan pass and its guard are what the cases are about.

  L2 / L3 / L10   synth_models; two layers make the layer before the half space layer 0, three take the layer loop's exits
  ragged10        layer counts 2 ... 10: the teams of one wavefront have different half spaces
  water9          liquid top layer; after dropping, water is the layer before the half space
  sediment10      NEVILL and general-body passes between the lean ones
  guard4          a slow half space under every other stack: the scan of those runs into the upper guard (calcul.f:166)"""
import numpy as np

B = 176
PERIODS = np.array([3.0, 5.0, 8.0, 12.8, 30.0, 60.0, 100.0], dtype=np.float32)
KIND_RAYLEIGH, PHASE_ONLY, PIPELINED = 2, 0x10, 0x40
TEAM = 2
GUARD_SEED = 31
NAMES = ["L2", "L3", "L10", "ragged10", "water9", "sediment10", "guard4"]


def guard_models(seed=GUARD_SEED):
    """Four layers; every other stack gets a half space slower than its lid (Vs 2.0-2.8 km/s under 3.0-4.6): no
    fundamental-mode root below the half-space velocity at the longer periods, the scan ends on the upper guard."""
    from pysurfinv_amd import synth
    rng = np.random.default_rng(seed)
    m = synth.synth_models(B, 4, seed=seed + 1, total_thickness=60.0)
    slow = np.arange(B) % 2 == 1
    vs = rng.uniform(2.0, 2.8, B).astype(np.float32)
    m[slow, 1, 3] = vs[slow]
    m[slow, 0, 3] = 1.76 * vs[slow]
    m[slow, 2, 3] = 0.541 + 0.3601 * m[slow, 0, 3]
    return m


def families():
    """[(name, model [B,5,L], nlay or None)]; seeded, the same in every process."""
    from pysurfinv_amd import synth
    rng = np.random.default_rng(30)
    nl = rng.integers(2, 11, B).astype(np.int32)
    return [("L2", synth.synth_models(B, 2, seed=32), None),
            ("L3", synth.synth_models(B, 3, seed=33), None),
            ("L10", synth.synth_models(B, 10, seed=34), None),
            ("ragged10", synth.synth_models(B, 10, seed=35), nl),
            ("water9", synth.water_models(B, seed=36), None),
            ("sediment10", synth.sediment_models(B, 10, seed=37), None),
            ("guard4", guard_models(), None)]


def cases():
    """[(name, model, nlay, kind)]: every family as c+U (_cu) and as phase only (_ph)."""
    out = []
    for name, model, nlay in families():
        out.append((name + "_cu", model, nlay, KIND_RAYLEIGH))
        out.append((name + "_ph", model, nlay, KIND_RAYLEIGH | PHASE_ONLY))
    return out


def run_all(device="cuda:0"):
    """{name_c / name_u / name_s: array, name_team: lanes per stack of the launch}: every case's c, u and status from the
    library this process loaded, with the team forced to TEAM lanes (process-wide setting: put back to 0 on the way out)."""
    import torch
    from pysurfinv_amd import _lib, forward
    L = _lib.lib()
    dev = torch.device(device)
    per = torch.from_numpy(PERIODS).to(dev)
    out = {}
    assert L.surfdisp_set_team(TEAM) == 0
    try:
        for name, model, nlay, kind in cases():
            m = torch.from_numpy(model).to(dev)
            nl = torch.from_numpy(nlay).to(dev) if nlay is not None else None
            plan = forward.BatchPlan(m.shape[0], m.shape[2], per.numel(), device=dev)
            team = int(L.surfdisp_get_team2(int(m.shape[0]), int(m.shape[2]), int(per.numel()), kind | PIPELINED))
            assert team == TEAM, (name, team)
            c, u, st = plan.run(m, per, kind=kind, nlay=nl, pipelined=True)
            torch.cuda.synchronize()
            out[name + "_c"] = c.cpu().numpy().copy()
            out[name + "_u"] = u.cpu().numpy().copy()
            out[name + "_s"] = st.cpu().numpy().copy()
            out[name + "_team"] = np.array([team], dtype=np.int32)
    finally:
        L.surfdisp_set_team(0)
    return out
