#!/usr/bin/env python3
"""GPU: cost of the analytic Rayleigh ellipticity kernels (surfdisp_forward_ellip_kernels_device) for 16 384 x L64 x P20
stacks, against the phase-velocity kernels alone (run_kernels) and the group-velocity kernels (run_group_kernels).  Whole
calls between torch events on the launch stream.  Also reports n_nonfinite (solved units with NaN rows) of the batch.
Writes the report to the file named by the first argument too, if given."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pysurfinv_amd import forward, synth  # noqa: E402

B, L, P = int(os.environ.get("TG_B", 16384)), int(os.environ.get("TG_L", 64)), 20
m = torch.from_numpy(synth.synth_models(B, L, seed=1, noise=0.02, total_thickness=300.0)).cuda()
per = torch.from_numpy(synth.default_periods(P)).cuda()
plan = forward.BatchPlan(B, L, P)


def timed(fn, n=5):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


lines = [f"{B} x L{L} x P{P}, Rayleigh"]
print(lines[0], flush=True)
t_k = timed(lambda: plan.run_kernels(m, per, kind=2))
# (n_failed / n_nonfinite are read back after each call: that synchronisation is inside the timed region, as a caller would have it)
t_g = timed(lambda: plan.run_group_kernels(m, per, kind=2))
t_e = timed(lambda: plan.run_ellip_kernels(m, per, kind=2))
out = plan.run_ellip_kernels(m, per, kind=2)
solved = int((out[0] > 0).sum().item())
lines.append(f"run_kernels {t_k:.3f} ms  run_group_kernels {t_g:.3f} ms (+{t_g - t_k:.3f})  "
             f"run_ellip_kernels {t_e:.3f} ms (+{t_e - t_k:.3f})  n_nonfinite {out[10]} of {solved} solved units")
lines.append(f"workspace: run_ellip_kernels {plan.workspace('ellip')[1] / 2**20:.0f} MiB, run_group_kernels {plan.workspace('group')[1] / 2**20:.0f} MiB")
print("\n".join(lines[1:]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
