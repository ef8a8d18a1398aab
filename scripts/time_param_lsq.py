#!/usr/bin/env python3
"""Time the parameter Jacobian and the parameter-space step beside the kernel entry they follow, at a grid share:
B points x settings.MCMC_SETTING (L 96, 13 unknowns, 19 periods of Rayleigh phase velocity).

    python scripts/time_param_lsq.py [B=25600] [rounds=7]

Whole calls between two events on the current stream, median of the rounds (min .. max); the parts take turns inside a round."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pysurfinv_amd import _lib, paramlsq, settings
from pysurfinv_amd.brownian import TorchProposer
from pysurfinv_amd.layers_batch import Model1DBatch
from pysurfinv_amd.obsdata import DispersionData


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 25600
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = "cuda:0"
    mb = Model1DBatch(settings.MCMC_SETTING, device=dev)
    Nu = mb.spec.n
    pr = TorchProposer(mb.spec, dev, seed=1)
    v0 = torch.as_tensor(mb.spec.v0, dtype=torch.float64, device=dev)[None, :]
    p = (v0 + 0.3 * (pr.reset(B) - v0)).contiguous()
    per = np.asarray(settings.MCMC_PERIODS, np.float64)
    c0, _ = mb.forward(v0, periods=settings.MCMC_PERIODS)
    obs = np.tile(c0.double().cpu().numpy(), (B, 1))
    plan = paramlsq.ParamLsqPlan(mb, B, [DispersionData("R", "c", per, obs, 0.01 * obs)])
    lam = torch.ones(B, dtype=torch.float64, device=dev)
    scale = torch.as_tensor(mb.spec.step, dtype=torch.float64, device=dev)
    parts = {
        "to_model (surfdisp_params_to_model_device)": lambda: mb.to_model(p)[0],
        "LsqPlan.kernels(thickness=True) (section (5g))": lambda: plan.lsq.kernels(model, thickness=True),
        "Model1DBatch.jacobian (new)": lambda: mb.jacobian(p),
        "ParamLsqPlan.step: all of the above + the step kernel": lambda: plan.step(p, lam, scale),
        "... with cov, sigma, logdet": lambda: plan.step(p, lam, scale, want_cov=True),
    }
    model = mb.to_model(p)[0]
    for fn in parts.values():                                  # warm-up: workspaces, buffers
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in parts}
    for _ in range(rounds):
        for k, fn in parts.items():
            t[k].append(timed(fn)[0])
    st = plan.step(p, lam, scale, want_cov=True)
    flags = np.bincount(st["flag"].cpu().numpy(), minlength=3)
    print(f"{B} x MCMC_SETTING (L {plan.L}, {Nu} unknowns, {per.size} periods, cR); whole calls, median of {rounds} rounds (min .. max)")
    med = {}
    for k, v in t.items():
        med[k] = float(np.median(v))
        print(f"{k:58s} {med[k]:9.3f} ms  ({min(v):.3f} .. {max(v):.3f})")
    ks = list(parts)
    extra = med[ks[3]] - med[ks[0]] - med[ks[1]] - med[ks[2]]
    print(f"step kernel alone (the whole step minus its three parts)   {extra:9.3f} ms;  inverse and log det on top "
          f"{med[ks[4]] - med[ks[3]]:.3f} ms")
    print(f"jac: {st['jac'].numel() * 8 / 2**20:.0f} MiB written once, read once per staged tile of 16 rows;  flags 0/1/2: {flags.tolist()};  "
          f"rows used {int(st['used'].min())} .. {int(st['used'].max())} of {per.size}")
    print(f"library sources {_lib.source_hash()}")


if __name__ == "__main__":
    main()
