"""The cases of tests/test_scan_double_gpu.py: the double lean pass of two-lane Rayleigh teams (LEAN2 in phase_body,
surfdisp_kernels.hip) against the general pass body.  A plain module, so that the reference leg can run the same cases in a
child process of its own (SURFDISP_LEANSCAN is read once per process).

176 stacks as in tests/scan_waits_cases.py (imported: its families, its guard family, its periods), every launch pipelined
with the team forced to two lanes, every case as c+U and as phase only:

  L10          ten 20 km layers at 3 ... 100 s: the crossing falls on each of the team's four points
  mm20         the same stacks at 8, 12.8 and 17.7 s: layer dropping changes mm between a lane's two points
  guard4       every other stack's scan ends on the upper guard
  L2, L3       two and three layers
  ragged10     layer counts 2 ... 10
  water9       a water layer on top
  sediment10   soft sediments
  single       one period
  thick200     four layers of 200 km at 3, 8 and 30 s: stacks go to the exact fallback kernel"""
import numpy as np

import scan_waits_cases as swc

B, TEAM = swc.B, swc.TEAM
MM_PERIODS = np.array([8.0, 12.8, 17.7], dtype=np.float32)
SINGLE_PERIOD = np.array([12.8], dtype=np.float32)
THICK_PERIODS = np.array([3.0, 8.0, 30.0], dtype=np.float32)
DC = np.float32(0.01)                  # the scan's grid step (init.f:25)


def thick_models():
    from pysurfinv_amd import synth
    return synth.synth_models(B, 4, seed=41, total_thickness=800.0)


def families():
    """[(name, model [B,5,L], nlay or None, periods)]; seeded, the same in every process."""
    fam = {name: (model, nlay) for name, model, nlay in swc.families()}
    out = [("L10", *fam["L10"], swc.PERIODS), ("mm20", *fam["L10"], MM_PERIODS), ("guard4", *fam["guard4"], swc.PERIODS)]
    out += [(n, *fam[n], swc.PERIODS) for n in ("L2", "L3", "ragged10", "water9", "sediment10")]
    out += [("single", *fam["L10"], SINGLE_PERIOD), ("thick200", thick_models(), None, THICK_PERIODS)]
    return out


def names():
    return [f[0] + s for f in families() for s in ("_cu", "_ph")]


def run_all(device="cuda:0"):
    """{name_c / name_u / name_s: array, name_fb: stacks through the exact fallback, name_team: lanes per stack}: every case
    with the library this process loaded and the team forced to TEAM lanes (put back to 0 on the way out)."""
    import torch
    from pysurfinv_amd import _lib, forward
    L = _lib.lib()
    dev = torch.device(device)
    out = {}
    assert L.surfdisp_set_team(TEAM) == 0
    try:
        for name, model, nlay, periods in families():
            per = torch.from_numpy(periods).to(dev)
            m = torch.from_numpy(model).to(dev)
            nl = torch.from_numpy(nlay).to(dev) if nlay is not None else None
            for tag, kind in (("_cu", swc.KIND_RAYLEIGH), ("_ph", swc.KIND_RAYLEIGH | swc.PHASE_ONLY)):
                plan = forward.BatchPlan(m.shape[0], m.shape[2], per.numel(), device=dev)
                team = int(L.surfdisp_get_team2(int(m.shape[0]), int(m.shape[2]), int(per.numel()), kind | swc.PIPELINED))
                c, u, st = plan.run(m, per, kind=kind, nlay=nl, pipelined=True)
                torch.cuda.synchronize()
                out[name + tag + "_c"] = c.cpu().numpy().copy()
                out[name + tag + "_u"] = u.cpu().numpy().copy()
                out[name + tag + "_s"] = st.cpu().numpy().copy()
                out[name + tag + "_fb"] = np.array([plan.fallback_count()], dtype=np.int32)
                out[name + tag + "_team"] = np.array([team], dtype=np.int32)
    finally:
        L.surfdisp_set_team(0)
    return out
