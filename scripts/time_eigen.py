#!/usr/bin/env python3
"""GPU: cost of the eigenfunction entry (surfdisp_forward_eigen_device) for 16 384 x L64 x P20 stacks, Rayleigh and Love,
with all outputs and with ur alone, against the forward entry (surfdisp_forward_batch_device: the parent's code path,
unchanged).  Whole calls between torch events on the launch stream; the three variants take turns for TE_ROUNDS rounds of
TE_N calls and the median round is reported with the spread.  Also compares c, u, status of the two entries bit for bit at
this size and prints the transposition kernel's traffic floor (its own time comes from a kernel trace of this script in a
run of its own).  Writes the report to the file named by the first argument too, if given."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pysurfinv_amd import _lib, forward, synth  # noqa: E402

B, L, P = int(os.environ.get("TE_B", 16384)), int(os.environ.get("TE_L", 64)), 20
ROUNDS, N = int(os.environ.get("TE_ROUNDS", 7)), int(os.environ.get("TE_N", 5))
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
    variants = (("run", lambda: plan.run(m, per, kind=kind)),
                ("run_eigen", lambda: plan.run_eigen(m, per, kind=kind)),
                ("run_eigen, ur only", lambda: plan.run_eigen(m, per, kind=kind, want_uz=False, want_tz=False, want_tr=False,
                                                              want_energy=False)))
    ref = [t.clone() for t in plan.run(m, per, kind=kind)]
    out = plan.run_eigen(m, per, kind=kind)
    same = all(torch.equal(a, b) for a, b in zip(ref, out[:3]))
    solved = out[0] > 0
    deep = (out[3] != 0).sum(dim=2)[solved].float().mean()
    for _, fn in variants:                                  # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    t = {n: [] for n, _ in variants}
    for _ in range(ROUNDS):
        for n, fn in variants:
            t[n].append(timed(fn))
    med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
    base = med["run"]
    for n, _ in variants:
        extra = "" if n == "run" else f"  (+{med[n] - base:.3f} ms, {100 * (med[n] / base - 1):.1f} %)"
        lines.append(f"{name:8s} {n:20s} {med[n]:.3f} ms  ({min(t[n]):.3f} .. {max(t[n]):.3f}){extra}")
    planes = 4 if kind == 2 else 2
    unit = B * P * L * 4 / 1e6
    lines.append(f"{name:8s} c, u, status bit-identical to run: {same};  solved units {int(solved.sum())}, mean layers per unit "
                 f"{float(deep):.1f} of {L};  transposition floor: {planes} planes written + read at most ({2 * planes * unit:.0f} MB) "
                 f"+ 4 row arrays written ({4 * unit:.0f} MB)")
    print("\n".join(lines[-4:]), flush=True)
lines.append(f"workspace: run_eigen {plan.workspace('eigen')[1] / 2**20:.0f} MiB, run {plan.workspace('forward')[1] / 2**20:.0f} MiB, "
             f"run_kernels {_lib.lib().surfdisp_kernels_workspace_bytes(B, L, P) / 2**20:.0f} MiB")
print(lines[-1], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
