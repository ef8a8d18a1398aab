#!/usr/bin/env python3
"""GPU: cost of posterior.posterior_predictive on a REAL sampler track - TP_POINTS points x TP_CHAINS chains x TP_CHAINL rows (64 x 8 x
250) of the continental setting of the tests with the driver fixture's observations (scaled a little from point to point), sampled
here by MetropolisBatch.run_points - against the baseline: forward-solving ALL final rows through the sampler's `misfit`, which is
what the package could do before (the gather of MetropolisBatch.summarise_points restated line by line, then `misfit` in slices
of the same max_batch).  Reported: the share of distinct source rows among the final rows, the whole call (host synchronisation
included, wall clock around a device synchronise; median of TP_ROUNDS alternating rounds after a warm-up of both), the two device
entries alone between device events, and the largest difference of the two routes' means.
Writes the report to the file named by the first argument too, if given."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from settings import CONT  # noqa: E402
from pysurfinv_amd import posterior  # noqa: E402
from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402
from pysurfinv_amd.mcmc import MetropolisBatch  # noqa: E402

NP, CH, CL = (int(os.environ.get(k, v)) for k, v in (("TP_POINTS", 64), ("TP_CHAINS", 8), ("TP_CHAINL", 250)))
ROUNDS, MAXB = int(os.environ.get("TP_ROUNDS", 5)), int(os.environ.get("TP_MAX_BATCH", 65536))
G = np.load(os.path.join(ROOT, "tests", "golden", "ref_driver.npz"))
dev = torch.device("cuda:0")
mb = Model1DBatch(CONT, device=dev)
per = G["trace/periods"]
c_pts = np.tile(G["trace/c_obs"], (NP, 1)) * (1 + 0.002 * (np.arange(NP) % 7)[:, None])
u_pts = np.tile(G["trace/uncer"], (NP, 1))
run = MetropolisBatch(mb.spec, mb.to_model, per, np.repeat(c_pts, CH, axis=0), np.repeat(u_pts, CH, axis=0), device=dev, seed=7)
track = run.run_points(NP, CH, CL, on_device=True).reshape(NP, CH * CL, -1).contiguous()
torch.cuda.synchronize()
R, N = track.shape[1], mb.spec.n
mc = MetropolisBatch(mb.spec, mb.to_model, per, c_pts, u_pts, device=dev, seed=7)      # point p reads observation row p


def all_final_rows():
    """The baseline: every final row's parameters (MetropolisBatch.summarise_points' gather), solved by `misfit`."""
    acc = track[:, :, 2] > 0.5
    idx = torch.arange(R, device=dev)[None, :].expand(NP, R)
    last = torch.cummax(torch.where(acc, idx, torch.zeros_like(idx)), dim=1).values
    mis = torch.nan_to_num(track[:, :, 0], nan=float("inf"))
    mn = mis.min(dim=1).values
    final = mis < torch.maximum(2.0 * mn, mn + 0.5)[:, None]
    pt, row = torch.nonzero(final, as_tuple=True)
    par = track[pt, last[pt, row], 3:]
    pred = torch.empty((par.shape[0], len(per)), dtype=torch.float64, device=dev)
    for a in range(0, par.shape[0], MAXB):
        pred[a:a + MAXB] = mc.misfit(par[a:a + MAXB].contiguous(), rows=pt[a:a + MAXB], return_c=True)[3]
    mean = torch.zeros((NP, len(per)), dtype=torch.float64, device=dev).index_add_(0, pt, pred) / final.sum(dim=1)[:, None]
    return mean, int(par.shape[0])


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn, n=20):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


predictive = lambda: posterior.posterior_predictive(mc, track, max_batch=MAXB)
out = predictive()
mean_all, n_rows = all_final_rows()                                       # (warm-up of both, and the comparison)
torch.cuda.synchronize()
t = {"posterior_predictive": [], "all final rows through misfit": []}
for _ in range(ROUNDS):
    t["posterior_predictive"].append(wall(predictive)[0])
    t["all final rows through misfit"].append(wall(all_final_rows)[0])
n_final, n_src = int(out["n_final"].sum()), int(out["n_sources"].sum())
acc_rate = float((track[:, :, 2] > 0.5).double().mean())
src = posterior.posterior_sources(track)
nz = torch.nonzero(src["weight"])
w = src["weight"][nz[:, 0], nz[:, 1]].contiguous()
offsets = torch.zeros(NP + 1, dtype=torch.int32, device=dev); offsets[1:] = torch.cumsum(src["n_sources"], 0)
pred32 = torch.rand((nz.shape[0], len(per)), dtype=torch.float32, device=dev) + 3.0
lines = [f"{NP} points x {CH} chains x {CL} rows of a sampled track (CONT, {len(per)} periods, N = {N}); accept rate {100 * acc_rate:.1f} %",
         f"final rows {n_final} of {NP * R} ({100 * n_final / (NP * R):.1f} %); distinct source rows {n_src} = {100 * n_src / max(n_final, 1):.1f} % of the "
         f"final rows; failed {int(out['n_failed'].sum())}; baseline solved {n_rows} rows",
         f"whole calls (wall clock around a device synchronise), median of {ROUNDS} alternating rounds (min .. max), max_batch {MAXB}"]
med = {}
for n, v in t.items():
    med[n] = sorted(v)[len(v) // 2]
    lines.append(f"{n:34s} {med[n]:9.3f} ms  ({min(v):.3f} .. {max(v):.3f})")
lines.append(f"ratio baseline / posterior_predictive: {med['all final rows through misfit'] / med['posterior_predictive']:.2f}")
lines.append(f"surfdisp_posterior_sources_device alone (device events, 20 calls): {events(lambda: posterior.posterior_sources(track)):.3f} ms")
lines.append(f"surfdisp_posterior_predictive_device alone on {nz.shape[0]} rows x {len(per)} columns: "
             f"{events(lambda: posterior.predictive_statistics(pred32, None, w, offsets)):.3f} ms; with a 100-bin histogram: "
             f"{events(lambda: posterior.predictive_statistics(pred32, None, w, offsets, hist=(np.full(len(per), 2.0), np.full(len(per), 5.0), 100))):.3f} ms")
lines.append(f"pred_mean against the mean over all final rows: max |diff| = {float((out['pred_mean'] - mean_all).abs().max()):.2e} "
             f"(the two batches may run with different teams: 1e-6 is the solver's spread between team sizes)")
lines.append(f"misfit_dev (largest |recomputed - recorded| misfit of a source row): max over points {float(out['misfit_dev'].max()):.2e}; "
             f"largest |fit| of a column: {float(out['fit'].abs().max()):.2f} sigma")
print("\n".join(lines), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
