#!/usr/bin/env python3
"""GPU: cost of the apparent-attenuation entry (surfdisp_forward_atten_device) for 16 384 x L64 x P20 stacks, Rayleigh and
Love, with the dqdq rows and without, against the phase-velocity kernels entry alone (surfdisp_forward_kernels_device:
the parent's code path, unchanged).  Whole calls between torch events on the launch stream; the three variants take turns
for TA_ROUNDS rounds of TA_N calls and the median round is reported with the spread.  Also compares the two entries' common
outputs bit for bit at this size.  Writes the report to the file named by the first argument too, if given."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pysurfinv_amd import forward, synth  # noqa: E402

B, L, P = int(os.environ.get("TA_B", 16384)), int(os.environ.get("TA_L", 64)), 20
ROUNDS, N = int(os.environ.get("TA_ROUNDS", 7)), int(os.environ.get("TA_N", 5))
m = torch.from_numpy(synth.synth_models(B, L, seed=1, noise=0.02, total_thickness=300.0)).cuda()
per = torch.from_numpy(synth.default_periods(P)).cuda()
plan = forward.BatchPlan(B, L, P)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N


lines = [f"{B} x L{L} x P{P}; whole calls, median of {ROUNDS} alternating rounds of {N} calls (min .. max)"]
print(lines[0], flush=True)
for kind, name in ((2, "Rayleigh"), (1, "Love")):
    variants = (("run_kernels", lambda: plan.run_kernels(m, per, kind=kind)),
                ("run_atten", lambda: plan.run_atten(m, per, kind=kind)),
                ("run_atten, no dqdq", lambda: plan.run_atten(m, per, kind=kind, want_kernel=False)))
    ref = [t.clone() if t is not None else None for t in plan.run_kernels(m, per, kind=kind)]
    out = plan.run_atten(m, per, kind=kind)
    same = all((a is None and b is None) or torch.equal(a, b) for a, b in zip(ref, out[:6]))
    qinv = out[6]
    solved = out[0] > 0
    for _, fn in variants:                                  # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    t = {n: [] for n, _ in variants}
    for _ in range(ROUNDS):
        for n, fn in variants:
            t[n].append(timed(fn))
    med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
    base = med["run_kernels"]
    for n, _ in variants:
        extra = "" if n == "run_kernels" else f"  (+{med[n] - base:.3f} ms, {100 * (med[n] / base - 1):.1f} %)"
        lines.append(f"{name:8s} {n:20s} {med[n]:.3f} ms  ({min(t[n]):.3f} .. {max(t[n]):.3f}){extra}")
    lines.append(f"{name:8s} common outputs bit-identical to run_kernels: {same};  solved units {int(solved.sum())}, "
                 f"1/Q in [{float(qinv[solved].min()):.3e}, {float(qinv[solved].max()):.3e}]")
    print("\n".join(lines[-4:]), flush=True)
lines.append(f"workspace: run_atten {plan.workspace('atten')[1] / 2**20:.0f} MiB = run_kernels {plan.workspace('kernels')[1] / 2**20:.0f} MiB")
print(lines[-1], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
