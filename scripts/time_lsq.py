#!/usr/bin/env python3
"""GPU: cost of the damped least-squares step (surfdisp_lsq_step_device) and of a whole iteration of
pysurfinv_amd.linearized.LinearizedBatch for 16 384 x L64 stacks at 20 periods: cR + uR + cL (N = 60 rows) and the same with
chi added (N = 80).  HIP events on the launch stream around n calls after a warm-up call; the step kernel alone is timed on
the partial arrays of one kernels call (LsqPlan.kernels), so its time holds no forward solve.  The arithmetic of the step is
about N n^2 / 2 + n^3 / 6 fp64 FMAs per stack (n = 64 free layers).  The resolution kernel (surfdisp_lsq_resolution_device) is
timed the same way on the same arrays, with both matrices, with one and with none written: N n^2 / 2 + n^3 / 2 FMAs and 8 n^2
bytes per matrix and stack."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pysurfinv_amd import _lib, forward, linearized, synth  # noqa: E402
from pysurfinv_amd.obsdata import DispersionData  # noqa: E402

B, L, P = int(os.environ.get("TL_B", 16384)), int(os.environ.get("TL_L", 64)), 20
true = synth.synth_models(B, L, seed=1, noise=0.02, total_thickness=300.0)
per = synth.default_periods(P)
dm, dp = torch.from_numpy(true).cuda(), torch.from_numpy(per).cuda()
plan = forward.BatchPlan(B, L, P)
cR, uR, st, eR = (x.cpu().numpy().astype(np.float64) for x in plan.run(dm, dp, kind=2, want_ratio=True))
cL = plan.run(dm, dp, kind=1)[0].cpu().numpy().astype(np.float64)
del plan
obs = {("R", "c"): cR, ("R", "U"): uR, ("L", "c"): cL, ("R", "E"): eR}
z = np.linspace(0.0, 1.0, L)
start = true.copy()
start[:, 1, :] *= (1.0 + 0.03 * np.cos(np.pi * z))[None, :].astype(np.float32)


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


print(f"{B} x L{L} x P{P}, n = {L} free layers", flush=True)
for sets in ((("R", "c"), ("R", "U"), ("L", "c")), (("R", "c"), ("R", "U"), ("L", "c"), ("R", "E"))):
    data = [DispersionData(w, q, per, obs[w, q], 0.005 * np.abs(obs[w, q])) for w, q in sets]
    inv = linearized.LinearizedBatch(start, data, alpha=0.05)
    lp, jd = inv.plan, inv.plan.joint
    N = jd.Ptot
    t_kern = timed(lambda: lp.kernels(inv.model))
    pred, part = lp.kernels(inv.model)
    arrs = [pred["cR"], pred["uR"], pred["cL"], pred["uL"], pred["eR"]]
    predp = (ctypes.c_void_p * 5)(*[a.data_ptr() if a is not None else None for a in arrs])
    strides = (ctypes.c_long * 5)(*[a.stride(0) if a is not None else 0 for a in arrs])
    partp = (ctypes.c_void_p * 15)(*[a.data_ptr() if a is not None else None for a in part])
    nper = (ctypes.c_int * 2)(P, P)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def step_only():
        _lib.check(_lib.lib().surfdisp_lsq_step_device(
            stream, B, L, None, p(inv.model), p(inv.free8), 1, inv.nfree_max, partp, predp, strides, nper, N, p(jd.cols),
            p(jd.weights), p(lp.obs), p(lp.uncer), p(lp.mask8), 1, None, None, 0, inv.alpha, None, 0, p(inv.lam), p(lp.delta),
            p(lp.stats), p(lp.info)))

    res_buf = dict(cov=torch.zeros(B, inv.nfree_max, inv.nfree_max, dtype=torch.float64, device="cuda"),
                   res=torch.zeros(B, inv.nfree_max, inv.nfree_max, dtype=torch.float64, device="cuda"),
                   per_layer=torch.zeros(3, B, L, dtype=torch.float64, device="cuda"),
                   stats=torch.zeros(B, 2, dtype=torch.float64, device="cuda"), info=torch.zeros(B, 3, dtype=torch.int32, device="cuda"))

    def resolution_only(cov=True, res=True):
        _lib.check(_lib.lib().surfdisp_lsq_resolution_device(
            stream, B, L, None, p(inv.model), p(inv.free8), 1, inv.nfree_max, partp, predp, strides, nper, N, p(jd.cols),
            p(jd.weights), p(lp.obs), p(lp.uncer), p(lp.mask8), 1, None, None, 0, inv.alpha, None, 0, p(inv.lam),
            p(res_buf["cov"] if cov else None), p(res_buf["res"] if res else None), p(res_buf["per_layer"][0]),
            p(res_buf["per_layer"][1]), p(res_buf["per_layer"][2]), p(res_buf["stats"]), p(res_buf["info"])))

    lam_res = float(inv.lam[0])
    t_step = timed(step_only, n=10)
    t_res = [timed(lambda: resolution_only(*w), n=10) for w in ((True, True), (True, False), (False, True), (False, False))]
    rflags = np.bincount(res_buf["info"][:, 2].cpu().numpy(), minlength=4)
    rd = res_buf["per_layer"][2].cpu().numpy()
    t_fwd = timed(lambda: lp.chi_square(inv.model))
    t_iter = timed(lambda: inv.run(1), n=4)
    flags = np.bincount(lp.info[:, 2].cpu().numpy(), minlength=4)
    rms = inv.rms.cpu().numpy()
    print(f"{'+'.join(w + q for w, q in sets)} (N = {N}): step kernel {t_step:.3f} ms  kernel entries {t_kern:.3f} ms  "
          f"trial solve + misfit {t_fwd:.3f} ms  whole iteration {t_iter:.3f} ms   flags 0/1/2/3 of the last step {flags.tolist()}  "
          f"median rms after 5 iterations {np.median(rms):.3f}", flush=True)
    print(f"    resolution kernel at the start model, lam {lam_res:g}: cov + res {t_res[0]:.3f} ms ({t_res[0] / t_step:.2f} x the step kernel)  "
          f"cov only {t_res[1]:.3f} ms  res only {t_res[2]:.3f} ms  neither matrix {t_res[3]:.3f} ms   flags 0/1/2/3 {rflags.tolist()}  "
          f"rdiag median {np.median(rd):.3f} min {rd.min():.3f}", flush=True)
    del res_buf
