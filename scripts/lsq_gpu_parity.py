#!/usr/bin/env python3
"""GPU: raw results of the Python layers of the linearised inversion, to compare two revisions of pysurfinv_amd/linearized.py on
the same library build word for word.

    lsq_gpu_parity.py save OUT.npz [ROOT]   ROOT: the tree whose pysurfinv_amd is imported (default: this one); load the same
                                            library into both with SURFDISP_LIB_PATH
    lsq_gpu_parity.py compare A.npz B.npz   exit status 1 when a key, a dtype, a shape or a byte differs

16 stacks x 12 layers, 8 periods, without modes (Rc + RU + Lc) and with K = 2 (Rc + Lc): every tensor of LsqPlan.step and
LsqPlan.resolution, every history array of LinearizedBatch.run(4) and every tensor of LinearizedBatch.resolution()."""
import os
import sys

import numpy as np

B, L, P = 16, 12, 8


def flat(prefix, out, into):
    for k, v in (out.items() if isinstance(out, dict) else enumerate(out)):
        if isinstance(v, (dict, list)):
            flat(f"{prefix}/{k}", v, into)
        elif v is not None:
            into[f"{prefix}/{k}"] = v.detach().cpu().numpy().copy()


def save(path, root):
    sys.path.insert(0, root)
    import torch
    from pysurfinv_amd import forward, linearized, synth
    from pysurfinv_amd.obsdata import DispersionData
    true = synth.synth_models(B, L, seed=5)
    per = synth.default_periods(P)
    dm, dp = torch.from_numpy(true).cuda(), torch.from_numpy(per).cuda()
    plan = forward.BatchPlan(B, L, P)
    cR, uR = (x.cpu().numpy().astype(np.float64) for x in plan.run(dm, dp, kind=2)[:2])
    cL = plan.run(dm, dp, kind=1)[0].cpu().numpy().astype(np.float64)
    obs = {("R", "c"): cR, ("R", "U"): uR, ("L", "c"): cL}
    start = true.copy()
    start[:, 1, :] *= (1.0 + 0.03 * np.cos(np.pi * np.linspace(0.0, 1.0, L)))[None, :].astype(np.float32)
    h = start[0, 3].astype(np.float64)
    T = np.stack([linearized.interface_mode(h, range(0, 3), range(3, 6)), linearized.thickness_mode(h, [0, 1])])
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    out = {}
    for tag, sets, modes in (("vs", (("R", "c"), ("R", "U"), ("L", "c")), None), ("K2", (("R", "c"), ("L", "c")), T)):
        data = [DispersionData(w, q, per, obs[w, q], 0.005 * np.abs(obs[w, q])) for w, q in sets]
        kw = {} if modes is None else dict(modes=t(modes), mode_scale=t(np.array([1e-4, 1e-3])), mode_prior=t(np.array([0.0, 0.01])),
                                           mode_y=t(np.full((B, 2), 0.25)))
        lp = linearized.LsqPlan(B, L, data)
        for name in ("step", "resolution"):
            flat(f"{tag}/plan.{name}", getattr(lp, name)(t(start), t(np.full(B, 2.0)), alpha=0.05, **kw), out)
        mk = {} if modes is None else dict(modes=modes, mode_scale=[1e-4, 1e-3], mode_prior=[0.0, 0.01])
        inv = linearized.LinearizedBatch(start, data, alpha=0.05, **mk)
        flat(f"{tag}/batch.run", inv.run(4, keep_models=True), out)
        flat(f"{tag}/batch.resolution", inv.resolution(), out)
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes, linearized.py of {root}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    diff = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            diff.append(k)
    print(f"{pa} against {pb}: {len(a.files)} arrays, " + ("equal word for word" if not diff else f"DIFFERENT in {diff}"))
    return 1 if diff else 0


if __name__ == "__main__":
    if sys.argv[1] == "save":
        save(sys.argv[2], os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
