"""The cases of tests/test_forward_trims_gpu.py, shared with scripts/record_forward_trims.py (which records the same cases
from a build of the parent commit into tests/golden/forward_trims_parent.npz).

B = 192 stacks: one and a half workgroups of two-lane teams.  Periods on both sides of the group kernel's layer dropping
(8 and 12.8 s drop layers of the 200 km stacks, 30 s and longer do not) and of |x| = 1/4 in layer_coef's sinh (the series is
taken at 95 and 100 s only).  Ten layers is the deepest stack whose group-velocity launch keeps the fit's layer values
for the integral sweep (a launch that is not pipelined: L10_R, sediment10_R); 11 and 14 layers recompute them."""
import numpy as np

B = 192
PERIODS = np.array([8.0, 12.8, 30.0, 60.0, 95.0, 100.0], dtype=np.float32)
KIND_LOVE, KIND_RAYLEIGH = 1, 2


def cases():
    """[(name, model [B,5,L], nlay or None, kind, pipelined)]; seeded, the same in every process."""
    from pysurfinv_amd import synth
    rng = np.random.default_rng(20)
    m10 = synth.synth_models(B, 10, seed=21)
    m11 = synth.synth_models(B, 11, seed=22)
    m14 = synth.synth_models(B, 14, seed=23)
    sed = synth.sediment_models(B, 10, seed=24)
    wat = synth.water_models(B, seed=25)
    rag10 = synth.synth_models(B, 10, seed=26)
    nl10 = rng.integers(2, 11, B).astype(np.int32)
    rag14 = synth.synth_models(B, 14, seed=27)
    nl14 = rng.integers(2, 15, B).astype(np.int32)
    R, Lv = KIND_RAYLEIGH, KIND_LOVE
    # _R: four-lane teams; _Rp: pipelined launch, two-lane lean teams
    return [("L10_R", m10, None, R, False), ("L10_Rp", m10, None, R, True), ("L10_Love", m10, None, Lv, False),
            ("L11_Rp", m11, None, R, True), ("L14_R", m14, None, R, False),
            ("sediment10_R", sed, None, R, False),
            ("water9_Rp", wat, None, R, True), ("water9_Love", wat, None, Lv, False),
            ("ragged10_Rp", rag10, nl10, R, True), ("ragged14_R", rag14, nl14, R, False)]


def run_all(device="cuda:0"):
    """{name_c / name_u / name_s: array}: every case's c, u and status from the library this process loaded."""
    import torch
    from pysurfinv_amd import forward
    dev = torch.device(device)
    per = torch.from_numpy(PERIODS).to(dev)
    out = {}
    for name, model, nlay, kind, pipelined in cases():
        m = torch.from_numpy(model).to(dev)
        nl = torch.from_numpy(nlay).to(dev) if nlay is not None else None
        plan = forward.BatchPlan(m.shape[0], m.shape[2], per.numel(), device=dev)
        c, u, st = plan.run(m, per, kind=kind, nlay=nl, pipelined=pipelined)
        torch.cuda.synchronize()
        out[name + "_c"] = c.cpu().numpy().copy()
        out[name + "_u"] = u.cpu().numpy().copy()
        out[name + "_s"] = st.cpu().numpy().copy()
    return out
