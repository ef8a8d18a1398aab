#!/usr/bin/env python3
"""GPU: cost of the posterior-profile entry (surfdisp_posterior_profile_device, pysurfinv_amd.posterior.posterior_profiles) on a
track of the grid workload's shape - one GPU's share, TP_POINTS x TP_CHAINS chains x TP_CHAINL rows (256 x 100 x 1 000), the
96-layer MCMC_SETTING, TP_DEPTHS (64) depths - against the parent's only device route to a comparable quantity: the gather and
sum of MetropolisBatch.summarise_points up to avg_par (the final rows' mean parameters), restated here line by line.
Whole calls between torch events on the launch stream after a warm-up of every variant; the variants take turns for TP_ROUNDS
rounds of TP_N calls (60: the shortest window, the parent's route, is then about 0.3 s), the median round is reported with the
spread.  Bytes touched = two reads of the track (selection, then
profile) + the outputs and per-slab partials; the floor stated beside it is two reads of the track at the achievable HBM rate
(6.3 TB/s).  The track is synthetic (parameters uniform in the prior box, misfits and accept flags drawn so that about half
of the rows are final): both routes' cost depends on the shape and the final fraction, not on the values.
Writes the report to the file named by the first argument too, if given."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pysurfinv_amd import posterior, settings  # noqa: E402
from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402

NP, CH, CL, D = (int(os.environ.get(k, v)) for k, v in (("TP_POINTS", 256), ("TP_CHAINS", 100), ("TP_CHAINL", 1000), ("TP_DEPTHS", 64)))
ROUNDS, NCALL = int(os.environ.get("TP_ROUNDS", 5)), int(os.environ.get("TP_N", 60))
HBM = 6.3e12
dev = torch.device("cuda:0")
mb = Model1DBatch(settings.MCMC_SETTING, device=dev)
N, R = mb.spec.n, CH * CL
g = torch.Generator(device=dev); g.manual_seed(1)
lo = torch.as_tensor(np.asarray(mb.spec.vmin, float), device=dev)
hi = torch.as_tensor(np.asarray(mb.spec.vmax, float), device=dev)
track = torch.empty((NP, R, 3 + N), dtype=torch.float64, device=dev)
for p in range(NP):                                         # point by point: no second copy of the track's size
    track[p, :, 3:] = lo + (hi - lo) * torch.rand((R, N), dtype=torch.float64, device=dev, generator=g)
    track[p, :, 0] = 0.6 + 2.0 * torch.rand(R, dtype=torch.float64, device=dev, generator=g) ** 2
    track[p, :, 1] = torch.exp(-track[p, :, 0])
    track[p, :, 2] = (torch.rand(R, dtype=torch.float64, device=dev, generator=g) < 0.35).to(torch.float64)
track[:, ::CL, 2] = 1.0
zd = np.linspace(0.5, 190.0, D)
HIST = (1.0, 5.5, 450)


def parent_gather_and_sum():
    """MetropolisBatch.summarise_points, its lines up to avg_par."""
    npnt = track.shape[0]
    acc = track[:, :, 2] > 0.5
    idx = torch.arange(R, device=dev)[None, :].expand(npnt, R)
    last = torch.cummax(torch.where(acc, idx, torch.zeros_like(idx)), dim=1).values
    paras = torch.gather(track[:, :, 3:], 1, last[:, :, None].expand(npnt, R, N))
    mis = torch.nan_to_num(track[:, :, 0], nan=float("inf"))
    imin = mis.argmin(dim=1)
    ar = torch.arange(npnt, device=dev)
    min_mis = mis[ar, imin]
    thres = torch.maximum(2.0 * min_mis, min_mis + 0.5)
    final = mis < thres[:, None]
    nfin = final.sum(dim=1)
    return (paras * final[:, :, None]).sum(dim=1) / nfin.clamp(min=1)[:, None], nfin


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(NCALL):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / NCALL


variants = (("posterior_profiles, histogram", lambda: posterior.posterior_profiles(mb, track, zd, hist=HIST, quantiles=())),
            ("posterior_profiles, no histogram", lambda: posterior.posterior_profiles(mb, track, zd)),
            ("parent: gather + sum to avg_par", parent_gather_and_sum))
out = posterior.posterior_profiles(mb, track, zd, hist=HIST)
avg, nfin = parent_gather_and_sum()
torch.cuda.synchronize()
track_bytes = track.numel() * 8
slabs = -(-R // posterior.SLAB_ROWS)
touched = 2 * track_bytes + 2 * NP * slabs * (D + N) * 40 + NP * (5 * D + 2 * N + 4) * 8
lines = [f"{NP} points x {CH} chains x {CL} rows, N = {N} parameters (track {track_bytes / 2**30:.2f} GiB), {D} depths; "
         f"final rows {int(out['n_final'].sum())} of {NP * R} ({100 * float(out['n_final'].sum()) / (NP * R):.1f} %)",
         f"whole calls, median of {ROUNDS} alternating rounds of {NCALL} calls (min .. max)",
         f"pmean against the parent's avg_par: max |diff| = {float((out['pmean'] - avg).abs().max()):.2e}; n_final equal: "
         f"{bool(torch.equal(out['n_final'], nfin))}"]
for _, fn in variants:
    fn()
torch.cuda.synchronize()
t = {n: [] for n, _ in variants}
for _ in range(ROUNDS):
    for n, fn in variants:
        t[n].append(timed(fn))
med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
for n, _ in variants:
    lines.append(f"{n:34s} {med[n]:9.3f} ms  ({min(t[n]):.3f} .. {max(t[n]):.3f})")
floor = 2 * track_bytes / HBM * 1e3
for n in ("posterior_profiles, histogram", "posterior_profiles, no histogram"):
    lines.append(f"{n:34s} bytes touched {touched / 1e9:.2f} GB / time = {touched / med[n] / 1e9:.2f} TB/s; floor (two reads of the "
                 f"track at 6.3 TB/s) {floor:.3f} ms = {100 * floor / med[n]:.0f} % of the call")
a, b = med["posterior_profiles, no histogram"], med["parent: gather + sum to avg_par"]
lines.append(f"condition (entry without histogram <= parent's gather and sum): {a:.3f} ms vs {b:.3f} ms: {'met' if a <= b else 'NOT met'}")
print("\n".join(lines), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
