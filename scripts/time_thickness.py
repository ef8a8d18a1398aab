#!/usr/bin/env python3
"""GPU: cost of the thickness-kernel entry (surfdisp_forward_thickness_kernels_device) for 16 384 x L64 x P20 stacks, Rayleigh
and Love, against what a caller had to launch for the same inputs before it - run_kernels followed by run_eigen (two root
searches) - and against run_kernels alone (the parent's code path, unchanged).  Whole calls between torch events on the
launch stream; the variants take turns for TT_ROUNDS rounds of TT_N calls and the median round is reported with the spread.
Also compares c, u, status and the partials of the new entry with run_kernels bit for bit at this size and prints the
traffic floor of the thickness kernel (its own time comes from a kernel trace of this script in a run of its own).  Writes
the report to the file named by the first argument too, if given."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pysurfinv_amd import forward, synth  # noqa: E402

B, L, P = int(os.environ.get("TT_B", 16384)), int(os.environ.get("TT_L", 64)), 20
ROUNDS, N = int(os.environ.get("TT_ROUNDS", 7)), int(os.environ.get("TT_N", 5))
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


def both(kind):
    plan.run_kernels(m, per, kind=kind)
    plan.run_eigen(m, per, kind=kind)


lines = [f"{B} x L{L} x P{P}; whole calls, median of {ROUNDS} alternating rounds of {N} calls (min .. max)"]
print(lines[0], flush=True)
for kind, name in ((2, "Rayleigh"), (1, "Love")):
    variants = (("run_kernels", lambda: plan.run_kernels(m, per, kind=kind)),
                ("run_thickness_kernels", lambda: plan.run_thickness_kernels(m, per, kind=kind, count=False)),
                ("run_thickness, dcdh only", lambda: plan.run_thickness_kernels(m, per, kind=kind, want_vp=False, want_rho=False,
                                                                                want_dcdz=False, count=False)),
                ("run_kernels + run_eigen", lambda: both(kind)))
    ref = [None if t is None else t.clone() for t in plan.run_kernels(m, per, kind=kind)]
    out = plan.run_thickness_kernels(m, per, kind=kind)
    same = all((a is None and b is None) or torch.equal(a, b) for a, b in zip(ref, out[:6]))
    solved = out[0] > 0
    deep = (out[6] != 0).sum(dim=2)[solved].float().mean()
    finite = bool(torch.isfinite(out[6]).all()) and bool(torch.isfinite(out[7]).all())
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
        lines.append(f"{name:8s} {n:26s} {med[n]:.3f} ms  ({min(t[n]):.3f} .. {max(t[n]):.3f}){extra}")
    eplanes, kplanes = (4, 3) if kind == 2 else (2, 2)
    unit = B * P * L * 4 / 1e6
    lines.append(f"{name:8s} c, u, status, dcdb, dcda, dcdr bit-identical to run_kernels: {same};  solved units {int(solved.sum())}, "
                 f"n_nonfinite {out[8]}, all finite {finite}, mean non-zero dcdh entries per unit {float(deep):.1f} of {L};  thickness kernel's "
                 f"floor: {eplanes} + {kplanes} planes read once ({(eplanes + kplanes) * unit:.0f} MB) + 2 row arrays written ({2 * unit:.0f} MB)")
    print("\n".join(lines[-5:]), flush=True)
lines.append(f"workspace: run_thickness_kernels {plan.workspace('thickness')[1] / 2**20:.0f} MiB, run_kernels {plan.workspace('kernels')[1] / 2**20:.0f} MiB, "
             f"run_eigen {plan.workspace('eigen')[1] / 2**20:.0f} MiB, run {plan.workspace('forward')[1] / 2**20:.0f} MiB")
print(lines[-1], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
