#!/usr/bin/env python3
"""GPU: cost of the analytic group-velocity kernels (surfdisp_forward_group_kernels_device) for 16 384 x L64 x P20 stacks,
Rayleigh and Love, against the phase-velocity kernels alone (run_kernels) and against the finite-difference route for the
same kernels (sens_kernel_pert_batch: 2L+1 full solves per stack, the U of the perturbed batch).  Whole calls between torch
events on the launch stream.  The FD route perturbs Vs only; a route for all columns (Vs, Vp, rho) costs three times that.
Also reports n_failed (solved units whose shifted root failed) of the batch."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pysurfinv_amd import forward, senskernel, synth  # noqa: E402

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


print(f"{B} x L{L} x P{P}", flush=True)
for kind, w in ((2, "R"), (1, "L")):
    t_k = timed(lambda: plan.run_kernels(m, per, kind=kind))
    # (n_failed is read back after each call: that synchronisation is inside the timed region, as a caller would have it)
    t_g = timed(lambda: plan.run_group_kernels(m, per, kind=kind))
    out = plan.run_group_kernels(m, per, kind=kind)
    solved = int((out[0] > 0).sum().item())
    t_fd = timed(lambda: senskernel.sens_kernel_pert_batch(m, per, wtype=w), n=1)
    print(f"{w}: run_kernels {t_k:.3f} ms  run_group_kernels {t_g:.3f} ms (+{t_g - t_k:.3f})  "
          f"FD route (Vs only, {2 * L + 1} solves per stack) {t_fd:.1f} ms  n_failed {out[9]} of {solved} solved units",
          flush=True)
