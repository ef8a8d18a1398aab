#!/usr/bin/env python3
"""GPU box: ms per lock step of a sampler with a prior, ``PriorRules(redraw="rounds")`` (masked redraw rounds: about 15 small
launches per lock step) against ``redraw="kernel"`` (the redraw loop inside the propose kernel: one launch), same build, same
process, alternating:

  * 25 600 chains x MCMC_SETTING (96 layers, 19 periods), the plain lock step in the sampler's default two chain groups;
  * 100 chains with PriorRules(vs_max=4.9) at spec_depth 1, 3 and 4 (the rounds mode draws no tree: its figures at depth > 1
    are those of a sampler WITHOUT a prior, given for scale).

Timed with device events around the lock steps after a warm-up of every shape; the best and the median of REPS windows.
Then the propose stage ALONE on an otherwise idle chip, 50 calls between two events: the one call of the kernel mode against
the propose call plus the 8 x 2 launches of the rounds - what the stage costs when no other group's root search shares the chip.
A last line times 25 600 chains as ONE chain group (``groups=1``), where nothing overlaps the propose stage."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pysurfinv_amd import settings
from pysurfinv_amd.mcmc import MetropolisBatch, PriorRules

REPS = int(os.environ.get("REPS", "5"))
dev = torch.device("cuda:0")
mb, c_obs, unc = settings.synthetic_observations(1, dev)


def sampler(mode, d=1):
    rules = PriorRules(mb, vs_max=4.9, redraw=mode) if (mode == "kernel" or d == 1) else None      # (the rounds draw no tree)
    return MetropolisBatch(mb.spec, mb.to_model, settings.MCMC_PERIODS, c_obs[0], unc[0], device=dev, seed=3, isgood=rules)


def window(mc, C, nsteps, d, groups=None):
    """(ms per lock step, accept rate of the last one) of ``nsteps`` lock steps between two device events - ``run()``'s own
    loop (``fused_step`` on the chain groups, or ``fused_tree_step``) without its start models: those come from a torch loop."""
    N = mb.spec.n
    p = mc._start(C, False, None).contiguous().clone()
    row = torch.zeros((C, d, 3 + N), dtype=torch.float64, device=dev)
    cg = mc.chain_groups(C, groups) if d == 1 else None
    stride = d * (3 + N)
    if cg is not None:                                                 # the states' own misfits, in the buffers that advance them
        cg.fork(); cg.step(p, row=row, row_stride=stride, first=True); cg.join()
    else:
        mc.fused_step(p, row=row, row_stride=stride, first=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    if cg is not None:
        cg.fork()
    for _ in range(nsteps):
        if d > 1:
            mc.fused_tree_step(p, d, d, row=row, row_stride=stride, step_stride=3 + N)
        elif cg is not None:
            cg.step(p, row=row, row_stride=stride)
        else:
            mc.fused_step(p, row=row, row_stride=stride)
    if cg is not None:
        cg.join()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / nsteps, float(row[:, :, 2].mean())


print(f"device: {torch.cuda.get_device_name(0)}; windows per figure: {REPS}", flush=True)
for what, C, nsteps, d, groups in (("25 600 chains, plain lock step (two chain groups)", 25600, 40, 1, None),
                                   ("100 chains, spec_depth 1", 100, 600, 1, None),
                                   ("100 chains, spec_depth 3", 100, 600, 3, None),
                                   ("100 chains, spec_depth 4", 100, 600, 4, None),
                                   ("25 600 chains, plain lock step, ONE chain group", 25600, 40, 1, 1)):
    mcs = {mode: sampler(mode, d) for mode in ("rounds", "kernel")}
    for mc in mcs.values():
        window(mc, C, max(nsteps // 10, 4), d, groups)                 # warm-up: plans, buffers, code objects
    ms = {mode: [] for mode in mcs}
    acc = {}
    for _ in range(REPS):
        for mode, mc in mcs.items():                                   # alternating
            t, acc[mode] = window(mc, C, nsteps, d, groups)
            ms[mode].append(t)
    print(what)
    for mode in mcs:
        note = "  (no rules at this depth)" if mode == "rounds" and d > 1 else ""
        print(f"    redraw={mode:7s}: best {min(ms[mode]):7.3f}  median {float(np.median(ms[mode])):7.3f} ms per lock step; "
              f"accept rate {acc[mode]:.3f}; exhausted {mcs[mode].prior_exhausted()}{note}", flush=True)


# ---- the propose stage alone
print("the propose stage alone (idle chip, one stream), us per call")
N = mb.spec.n
for C, d in ((25600, 1), (12800, 1), (100, 1), (100, 4)):
    line = []
    for mode in ("rounds", "kernel"):
        mc = sampler(mode, d)
        q = mc.proposer.reset(5 * C)
        p = q[PriorRules(mb, vs_max=4.9)(q)][:C].contiguous()          # good start states
        st = mc._fused_buffers(C)
        out = torch.empty((C, (1 << d) - 1, N), dtype=torch.float64, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def stage(counter):                                            # the sampler's own propose stage (rounds at depth > 1: the tree entry alone)
            mc.proposal().draw(stream, p, out.view(C, N) if d == 1 else out, d, counter, st, mc._chain0)
        for i in range(5):
            stage(1 + i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(50):
            stage(10 + i)
        e1.record()
        torch.cuda.synchronize()
        line.append(f"redraw={mode} {e0.elapsed_time(e1) / 50 * 1e3:7.1f}")
        if mode == "kernel":
            t = mc.last_prior_tries().cpu().view(torch.int16).float()
            line.append(f"(mean retries {float(t.mean()):.2f}, most {int(t.max())})")
    print(f"    {C:6d} chains, depth {d}: " + "   ".join(line) + ("  (rounds: no rules at this depth)" if d > 1 else ""), flush=True)
