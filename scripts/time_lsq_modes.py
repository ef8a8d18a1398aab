#!/usr/bin/env python3
"""GPU: cost of thickness modes in the least-squares step and the resolution kernel (include/surfdisp.h section (6h)) for
16 384 x L64 stacks at 20 periods, Rayleigh + Love phase velocities (N = 40 rows), n = 64 free layers.  HIP events on the launch
stream around n calls after a warm-up call (as scripts/time_lsq.py).  Timed: the step and the resolution kernel alone through
the entries of (6d) / (6e), through the mode entries with K = 0 and with K = 2 on the arrays of one kernels call; the kernels
call with and without the thickness kernels (the extra launches of run_thickness_kernels); LsqPlan.step as a whole with and
without modes.  With a library that lacks the mode entries (SURFDISP_LIB_PATH = a build of the parent commit) only the old
entries are timed: run both libraries alternately in one session to see the run-to-run noise."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pysurfinv_amd import _lib, forward, linearized, synth  # noqa: E402
from pysurfinv_amd.obsdata import DispersionData  # noqa: E402

B, L, P, K = int(os.environ.get("TL_B", 16384)), int(os.environ.get("TL_L", 64)), 20, 2
have_modes = hasattr(_lib.lib(), "surfdisp_lsq_step_modes_device")
true = synth.synth_models(B, L, seed=1, noise=0.02, total_thickness=300.0)
per = synth.default_periods(P)
dm, dp = torch.from_numpy(true).cuda(), torch.from_numpy(per).cuda()
plan = forward.BatchPlan(B, L, P)
cR = plan.run(dm, dp, kind=2)[0].cpu().numpy().astype(np.float64)
cL = plan.run(dm, dp, kind=1)[0].cpu().numpy().astype(np.float64)
del plan
start = true.copy()
start[:, 1, :] *= (1.0 + 0.03 * np.cos(np.pi * np.linspace(0.0, 1.0, L)))[None, :].astype(np.float32)
data = [DispersionData(w, "c", per, v, 0.005 * np.abs(v)) for w, v in (("R", cR), ("L", cL))]


def timed(fn, n=10):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


inv = linearized.LinearizedBatch(start, data, alpha=0.05)
lp, jd = inv.plan, inv.plan.joint
N, nmax = jd.Ptot, inv.nfree_max
h = start[0, 3].astype(np.float64)
T = np.stack([linearized.interface_mode(h, range(0, L // 4), range(L // 4, L // 2)), linearized.thickness_mode(h, range(0, 4))])
z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device="cuda")
Td, ms = torch.as_tensor(T).cuda(), torch.full((K,), 1e-4, dtype=torch.float64, device="cuda")
p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
out = dict(delta_y=z(B, K), cov=z(B, nmax + K, nmax + K), res=z(B, nmax + K, nmax + K), per_layer=z(3, B, L), per_mode=z(3, B, K),
           stats=z(B, 3), info=z(B, 3, dt=torch.int32))

t_kern = timed(lambda: lp.kernels(inv.model, want_vp=False, want_rho=False), n=5)
if have_modes:
    t_kern_h = timed(lambda: lp.kernels(inv.model, want_vp=False, want_rho=False, thickness=True), n=5)
    pred, part, part_h = lp.kernels(inv.model, want_vp=False, want_rho=False, thickness=True)
    parthp = (ctypes.c_void_p * 5)(*[a.data_ptr() if a is not None else None for a in part_h])
else:
    pred, part = lp.kernels(inv.model, want_vp=False, want_rho=False)
arrs = [pred["cR"], pred["uR"], pred["cL"], pred["uL"], pred["eR"]]
predp = (ctypes.c_void_p * 5)(*[a.data_ptr() if a is not None else None for a in arrs])
strides = (ctypes.c_long * 5)(*[a.stride(0) if a is not None else 0 for a in arrs])
partp = (ctypes.c_void_p * 15)(*[a.data_ptr() if a is not None else None for a in part])
nper = (ctypes.c_int * 2)(P, P)
head = (stream, B, L, None, p(inv.model), p(inv.free8), 1, nmax, partp, predp, strides, nper, N, p(jd.cols), p(jd.weights), p(lp.obs),
        p(lp.uncer), p(lp.mask8), 1, None, None, 0, inv.alpha, None, 0, p(inv.lam))
pl, pm = out["per_layer"], out["per_mode"]
C = _lib.lib()


def modes_in(k):
    return (k, p(Td) if k else None, 0, parthp if k else None, p(ms) if k else None, None, None)


step_old = lambda: _lib.check(C.surfdisp_lsq_step_device(*head, p(lp.delta), p(out["stats"]), p(out["info"])))
res_old = lambda: _lib.check(C.surfdisp_lsq_resolution_device(*head, p(out["cov"]), p(out["res"]), p(pl[0]), p(pl[1]), p(pl[2]),
                                                             p(out["stats"]), p(out["info"])))
step_new = lambda k: _lib.check(C.surfdisp_lsq_step_modes_device(*head, *modes_in(k), p(lp.delta), p(out["delta_y"]), p(out["stats"]),
                                                                 p(out["info"])))
res_new = lambda k: _lib.check(C.surfdisp_lsq_resolution_modes_device(*head, *modes_in(k), p(out["cov"]), p(out["res"]), p(pl[0]), p(pl[1]),
                                                                     p(pl[2]), p(pm[0]), p(pm[1]), p(pm[2]), p(out["stats"]), p(out["info"])))
kw = dict(free=inv.free8, nfree_max=nmax, alpha=inv.alpha)
tag = "with the mode entries" if have_modes else "WITHOUT the mode entries (a build of the parent commit)"
print(f"{B} x L{L} x P{P}, Rc + Lc (N = {N}), n = {nmax} free layers; library {tag}", flush=True)
print(f"old entries:           step kernel {timed(step_old):.3f} ms  resolution kernel (cov + res) {timed(res_old):.3f} ms  "
      f"kernels call (run_kernels x 2) {t_kern:.3f} ms  LsqPlan.step {timed(lambda: lp.step(inv.model, inv.lam, **kw), n=5):.3f} ms", flush=True)
if have_modes:
    for k in (0, K):
        ts, tr = timed(lambda: step_new(k)), timed(lambda: res_new(k))
        fl = np.bincount(out["info"][:, 2].cpu().numpy(), minlength=4).tolist()
        print(f"mode entries, K = {k}:   step kernel {ts:.3f} ms  resolution kernel (cov + res) {tr:.3f} ms   flags 0/1/2/3 {fl}", flush=True)
    t_step_m = timed(lambda: lp.step(inv.model, inv.lam, modes=Td, mode_scale=ms, **kw), n=5)
    print(f"with K = {K} modes:      kernels call (run_thickness_kernels x 2) {t_kern_h:.3f} ms (+{t_kern_h - t_kern:.3f} ms for the thickness "
          f"kernels)  LsqPlan.step {t_step_m:.3f} ms", flush=True)
