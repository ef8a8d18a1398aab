#!/usr/bin/env python3
"""GPU box: what U data, a Love solve and the Rayleigh ellipticity add to a Metropolis lock step (MetropolisBatch(data=...),
pysurfinv_amd.obsdata).

For the data sets {Rc}, {Rc, RU}, {Rc, RU, Lc, LU}, {Rc, RE} and {Rc, RU, Lc, LU, RE} (all on the 19 periods of MCMC_PERIODS,
per-chain synthetic observations of the 96-layer continental model; RE: the signed ellipticity of the Rayleigh solve, which
then also runs the ellipticity passes) and, as the baseline, the (periods, c_obs, uncer) sampler: ms per lock
step of MetropolisBatch.run on its default path, and the joint accept kernel's time (HIP events around repeated launches
on the last lock step's predictions, all chains in one launch, alone on the chip) as a share of the lock step.

    python scripts/time_joint_mcmc.py [--chains 25600,100] [--steps 40]

Each configuration runs in a fresh process of its own (see ``one``).

Shapes: 25 600 chains (the mcmc leg's shape: two chain groups, one lock step = one Metropolis step) and 100 chains (the
default speculative path: depth 4, four Metropolis steps per lock step)."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pysurfinv_amd import _lib, settings
from pysurfinv_amd.brownian import TorchProposer
from pysurfinv_amd.forward import BatchPlan
from pysurfinv_amd.layers_batch import Model1DBatch
from pysurfinv_amd.mcmc import MetropolisBatch
from pysurfinv_amd.obsdata import DispersionData


def observations(mb, n_points, dev, seed=100):
    """Rc, RU, RE, Lc, LU [n_points, P] of 'true' models (prior draws shrunk towards the start model), 1 % / 2 % errors
    (RE: 2 % of |chi|)."""
    per = torch.as_tensor(np.asarray(settings.MCMC_PERIODS, np.float32), device=dev)
    v0 = torch.as_tensor(mb.spec.v0, dtype=torch.float64, device=dev)[None, :]
    truth = torch.cat([v0, v0 + 0.3 * (TorchProposer(mb.spec, dev, seed=seed).reset(n_points) - v0)])
    model, nlay = mb.to_model(truth)
    out = {}
    for w, kind in (("R", _lib.KIND_RAYLEIGH), ("L", _lib.KIND_LOVE)):
        plan = BatchPlan(model.shape[0], model.shape[2], per.numel(), device=dev)
        c, u, st, e = (t.clone() for t in plan.run(model.contiguous(), per, kind=kind, nlay=nlay, want_ratio=True))
        bad = (st != 0)[:, None] | (c < 0.01) | ~(u >= 0.01) | ~torch.isfinite(e)
        for q, a in (("c", c), ("U", u)) + ((("E", e),) if w == "R" else ()):
            a = torch.where(bad.any(dim=1, keepdim=True), a[:1].expand_as(a), a)[1:].double().cpu().numpy()
            out[w + q] = (a, (0.01 if q == "c" else 0.02) * np.abs(a))
    return out


def accept_ms(mc, C, depth, reps=50):
    """ms of one accept launch over all C chains on the predictions of C * (2^depth - 1) start models (the joint kernel,
    or for a (periods, c_obs, uncer) sampler the Rayleigh-phase one; state, chi-squares and rows on copies)."""
    st = mc._fused_buffers(C)
    M = (1 << depth) - 1 if depth > 1 else 1
    q = torch.as_tensor(mc.spec.v0, dtype=torch.float64, device=mc.device)[None, :].repeat(C * M, 1).contiguous()
    pred = mc._solve_raw(q)
    p = torch.zeros((C, mc.spec.n), dtype=torch.float64, device=mc.device)
    row = torch.zeros((C, max(depth, 1), 3 + mc.spec.n), dtype=torch.float64, device=mc.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(mc.device).cuda_stream)
    rowp = ctypes.c_void_p(row.data_ptr())
    go = lambda: mc._accept(stream, pred, st, q, p, rowp, row.stride(0), 1, True, depth=max(depth, 1), nsteps=max(depth, 1),
                            step_stride=3 + mc.spec.n)
    go(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        go()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def lock_step_ms(mc, C, steps, depth, trials=3):
    """ms per lock step of run(): the difference of two runs (setup and first row cancel), the least of ``trials``."""
    per_lock = max(depth, 1)
    n1, n2 = 1 + per_lock * 4, 1 + per_lock * (4 + steps)
    mc.run(C, n1); torch.cuda.synchronize()
    best = float("inf")
    for _ in range(trials):
        ts = []
        for n in (n1, n2):
            t0 = time.perf_counter()
            mc.run(C, n); torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        best = min(best, (ts[1] - ts[0]) / steps * 1e3)
    return best


CONFIGS = (("(periods, c_obs, uncer) sampler", None), ("data={Rc}", ("Rc",)), ("data={Rc, RU}", ("Rc", "RU")),
           ("data={Rc, RU, Lc, LU}", ("Rc", "RU", "Lc", "LU")), ("data={Rc, RE}", ("Rc", "RE")),
           ("data={Rc, RU, Lc, LU, RE}", ("Rc", "RU", "Lc", "LU", "RE")))


def one(C, which, steps):
    """One configuration, measured in a process of its own: every configuration then creates its streams (chain groups, the
    Love solve's stream) in the same order, and the streams land on the same hardware queues (two chain groups that share
    one queue do not overlap: a first-run artefact of 2 ms per lock step at 25 600 chains when measured in one process)."""
    dev = torch.device("cuda:0")
    mb = Model1DBatch(settings.MCMC_SETTING, device=dev)
    T = np.asarray(settings.MCMC_PERIODS, np.float64)
    per_point = 50 if C >= 5000 else C
    obs = observations(mb, C // per_point, dev)
    rep = lambda a: np.repeat(a, per_point, axis=0)
    name, keys = CONFIGS[which]
    if keys is None:
        mc = MetropolisBatch(mb.spec, mb.to_model, T, rep(obs["Rc"][0]), rep(obs["Rc"][1]), device=dev, seed=3)
    else:
        mc = MetropolisBatch(mb.spec, mb.to_model, device=dev, seed=3,
                             data=[DispersionData(k[0], k[1], T, rep(obs[k][0]), rep(obs[k][1])) for k in keys])
    depth = mc.auto_spec_depth(C)
    if which == 0:
        groups = mc.chain_groups(C)
        L = mb.to_model(torch.as_tensor(mb.spec.v0, device=dev)[None, :])[0].shape[2]
        print(f"\n{C} chains ({C // per_point} points x {per_point}), {L} layers, {T.size} periods: default path = "
              f"{'speculative depth %d' % depth if depth > 1 else 'one step per lock step'}, "
              f"{groups.G if groups is not None else 1} chain group(s); {torch.cuda.get_device_name(dev)}", flush=True)
    ms = lock_step_ms(mc, C, steps, depth)
    acc = accept_ms(mc, C, depth)
    kern = "its accept kernel" if keys is None else "joint accept kernel"
    print(f"  {name:34s}: {ms:7.3f} ms per lock step; {kern:19s} {acc * 1e3:6.1f} us = {100 * acc / ms:5.2f} % of the lock step",
          flush=True)


def main():
    import subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="25600,100")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:
        C, which = (int(x) for x in args.one.split(","))
        return one(C, which, args.steps)
    for C in (int(x) for x in args.chains.split(",")):
        for which in range(len(CONFIGS)):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{C},{which}", "--steps", str(args.steps)],
                           check=True, timeout=600)


if __name__ == "__main__":
    main()
