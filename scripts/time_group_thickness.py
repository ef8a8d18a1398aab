#!/usr/bin/env python3
"""GPU: cost of the group-thickness entry (surfdisp_forward_group_thickness_kernels_device) for 16 384 x L64 x P20 stacks,
Rayleigh and Love, against run_group_kernels alone (the parent's code path, unchanged) and against what a caller had to launch
for the same numbers before it: run_group_kernels followed by three run_thickness_kernels calls - at T and, one team per unit
(SURFDISP_INDEPENDENT: the freshly built stack the shifted passes have), at T (1 - d) and T (1 + d); the combination on the host
comes on top of that route and is not timed.  The same route with three plain thickness calls is shown beside it.  Whole calls
between torch events on the launch stream; the variants take turns for GT_ROUNDS rounds of GT_N calls and the median round is
reported with the spread.  Also compares the outputs the new entry shares with the three existing entries bit for bit at this
size and prints the traffic floor of the combine kernel (its own time comes from a kernel trace of this script in a run of its
own).  Writes the report to the file named by the first argument too, if given."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pysurfinv_amd import _lib, forward, synth  # noqa: E402

B, L, P = int(os.environ.get("GT_B", 16384)), int(os.environ.get("GT_L", 64)), 20
ROUNDS, N = int(os.environ.get("GT_ROUNDS", 7)), int(os.environ.get("GT_N", 3))
D = 0.01
m = torch.from_numpy(synth.synth_models(B, L, seed=1, noise=0.02, total_thickness=300.0)).cuda()
per_h = synth.default_periods(P)
per = torch.from_numpy(per_h).cuda()
per_m, per_p = (torch.from_numpy(per_h * f).cuda() for f in (np.float32(1) - np.float32(D), np.float32(1) + np.float32(D)))
plan = forward.BatchPlan(B, L, P)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N


def three_calls(kind, flag):
    plan.run_group_kernels(m, per, kind=kind, dlnT_frac=D, count=False)
    plan.run_thickness_kernels(m, per, kind=kind, count=False)
    plan.run_thickness_kernels(m, per_m, kind=kind | flag, count=False)
    plan.run_thickness_kernels(m, per_p, kind=kind | flag, count=False)


lines = [f"{B} x L{L} x P{P}, dlnT_frac {D}; whole calls, median of {ROUNDS} alternating rounds of {N} calls (min .. max)"]
print(lines[0], flush=True)
same = lambda a, b: (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))
for kind, name in ((2, "Rayleigh"), (1, "Love")):
    variants = (("run_group_kernels", lambda: plan.run_group_kernels(m, per, kind=kind, dlnT_frac=D, count=False)),
                ("run_group_thickness_kernels", lambda: plan.run_group_thickness_kernels(m, per, kind=kind, dlnT_frac=D, count=False)),
                ("run_group_thickness, dudh only", lambda: plan.run_group_thickness_kernels(m, per, kind=kind, dlnT_frac=D, want_vp=False,
                                                                                           want_rho=False, want_dcdz=False, want_dudz=False, count=False)),
                ("group + 3 thickness (shifted: INDEPENDENT)", lambda: three_calls(kind, _lib.INDEPENDENT)),
                ("group + 3 thickness (all plain)", lambda: three_calls(kind, 0)))
    ref_g = [t.clone() if hasattr(t, "clone") else t for t in plan.run_group_kernels(m, per, kind=kind, dlnT_frac=D)]
    ref_t = [t.clone() if hasattr(t, "clone") else t for t in plan.run_thickness_kernels(m, per, kind=kind)]
    out = plan.run_group_thickness_kernels(m, per, kind=kind, dlnT_frac=D)
    equal = all(same(a, b) for a, b in zip(ref_g[:9], out[:9])) and same(ref_t[6], out[9]) and same(ref_t[7], out[10])
    solved = out[0] > 0
    nan_units = int(torch.isnan(out[11]).any(dim=2).sum())
    for _, fn in variants:                                  # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    t = {n: [] for n, _ in variants}
    for _ in range(ROUNDS):
        for n, fn in variants:
            t[n].append(timed(fn))
    med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
    base = med["run_group_kernels"]
    for n, _ in variants:
        extra = "" if n == "run_group_kernels" else f"  (+{med[n] - base:.3f} ms, {100 * (med[n] / base - 1):.1f} %)"
        lines.append(f"{name:8s} {n:44s} {med[n]:.3f} ms  ({min(t[n]):.3f} .. {max(t[n]):.3f}){extra}")
    unit = B * P * L * 4 / 1e6
    lines.append(f"{name:8s} c .. dudr bit-identical to run_group_kernels, dcdh, dcdz to run_thickness_kernels: {equal};  solved units "
                 f"{int(solved.sum())}, n_failed {out[13]}, n_nonfinite {out[14]}, units with NaN rows {nan_units};  combine kernel's floor: 4 row "
                 f"planes + dcdh read once ({5 * unit:.0f} MB, the shifted entry of dcdh from cache) + 2 row arrays written ({2 * unit:.0f} MB)")
    print("\n".join(lines[-6:]), flush=True)
lines.append(f"workspace: run_group_thickness_kernels {plan.workspace('group_thickness')[1] / 2**20:.0f} MiB, run_group_kernels "
             f"{plan.workspace('group')[1] / 2**20:.0f} MiB, run_thickness_kernels {plan.workspace('thickness')[1] / 2**20:.0f} MiB")
print(lines[-1], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
