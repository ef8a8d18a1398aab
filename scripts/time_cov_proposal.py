#!/usr/bin/env python3
"""GPU box: what the covariance-shaped proposal (``MetropolisBatch.set_proposal``, surfdisp_mcmc_propose_cov_device) costs per lock
step and what it buys per step, into profiles/cov_proposal/.

    python scripts/time_cov_proposal.py              # both steps below, each a child process under its own time limit, chained:
                                                     # the second starts only if the first ended well
    python scripts/time_cov_proposal.py timing       # -> time_cov_proposal.txt
    python scripts/time_cov_proposal.py efficiency   # -> efficiency.txt

timing: ms per lock step of all chains, device events around the lock steps after a warm-up of every shape, the best and the median
of REPS windows, the variants alternating in one process: 25 600 chains x MCMC_SETTING (96 layers, 19 periods) in two chain groups
and in one, 100 chains at the automatic depth (4); without a prior and with PriorRules(vs_max=4.9); the reference's proposal (the
kernels of the parent commit: their listings are unchanged, profiles/cov_proposal/isa_identity.txt) against a factor per point (50
chains per point; 4 diag(step) R with a random correlation factor R, so that the rules refuse as often as in profiles/prior_redraw/).

efficiency: the 16 synthetic points of the least-squares tests (``settings.synthetic_observations``), 32 chains x 2000 steps each
under PriorRules, the default proposal and start (chain 0 at v0, the others at prior draws) against ``ParamLsqBatch.run(8)`` ->
``proposal_factor()`` -> ``set_proposal`` -> ``run_points(start=)``: accept rate; per parameter the integrated autocorrelation time of
the chains' states over their second half (Sokal's window, c = 5; the median over the 512 chains) and the effective samples per 1000
steps; the steps until a chain's misfit first falls below its point's threshold max(2 min, min + 0.5) (min: the point's smallest
misfit over both runs)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "cov_proposal")
LIMITS = {"timing": 420, "efficiency": 300}            # seconds per step


def sokal_tau(x, c=5.0):
    """Integrated autocorrelation time of the series x [T] with Sokal's automatic window: tau(M) = 1 + 2 sum_{t=1..M} rho_t at the
    smallest M with M >= c tau(M).  A constant series: inf (the chain never moved)."""
    import numpy as np
    x = np.asarray(x, np.float64) - np.mean(x)
    T = x.size
    if not np.any(x):
        return float("inf")
    f = np.fft.rfft(x, 2 * T)
    acf = np.fft.irfft(f * np.conj(f))[:T]
    rho = acf / acf[0]
    tau = 1.0 + 2.0 * np.cumsum(rho[1:])
    ok = np.arange(1, T) >= c * tau
    return float(tau[np.argmax(ok)] if ok.any() else tau[-1])


def timing(out):
    import numpy as np
    import torch
    from pysurfinv_amd import settings
    from pysurfinv_amd.mcmc import MetropolisBatch, PriorRules
    REPS = int(os.environ.get("REPS", "5"))
    dev = torch.device("cuda:0")
    mb, c_obs, unc = settings.synthetic_observations(1, dev)
    N = mb.spec.n
    CPP = 50

    def factors(F):
        rng = np.random.default_rng(1)
        fac = []
        for _ in range(F):
            a = rng.normal(size=(N, N))
            c = a @ a.T / N + 0.2 * np.eye(N)
            d = np.sqrt(np.diag(c))
            fac.append(4.0 * mb.spec.step[:, None] * np.linalg.cholesky(c / np.outer(d, d)))
        return torch.as_tensor(np.stack(fac), device=dev)

    def sampler(rules, cov, C):
        isgood = None if rules is None else PriorRules(mb, vs_max=4.9, redraw=rules)
        mc = MetropolisBatch(mb.spec, mb.to_model, settings.MCMC_PERIODS, c_obs[0], unc[0], device=dev, seed=3, isgood=isgood)
        if cov:
            mc.set_proposal(factors((C + CPP - 1) // CPP), CPP)
        return mc

    def window(mc, C, nsteps, d, groups):
        p = mc._start(C, False, None).contiguous().clone()
        row = torch.zeros((C, d, 3 + N), dtype=torch.float64, device=dev)
        cg = mc.chain_groups(C, groups) if d == 1 else None
        stride = d * (3 + N)
        if cg is not None:
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

    variants = (("no prior, reference proposal", None, False), ("no prior, factor", None, True),
                ("PriorRules rounds, reference proposal", "rounds", False), ("PriorRules kernel, reference proposal", "kernel", False),
                ("PriorRules, factor", "rounds", True))
    print(f"device: {torch.cuda.get_device_name(0)}; windows per figure: {REPS}; ms per lock step of all chains", file=out, flush=True)
    for what, C, nsteps, groups in (("25 600 chains, two chain groups", 25600, 40, None), ("25 600 chains, ONE chain group", 25600, 40, 1),
                                    ("100 chains at the automatic depth", 100, 600, None)):
        mcs = {name: sampler(rules, cov, C) for name, rules, cov in variants}
        depth = {name: (mc.auto_spec_depth(C) if groups is None else 1) for name, mc in mcs.items()}
        for name, mc in mcs.items():
            window(mc, C, max(nsteps // 10, 4), depth[name], groups)
        ms, acc = {name: [] for name in mcs}, {}
        for _ in range(REPS):
            for name, mc in mcs.items():
                t, acc[name] = window(mc, C, nsteps, depth[name], groups)
                ms[name].append(t)
        print(what, file=out)
        for name, mc in mcs.items():
            print(f"    {name:40s} depth {depth[name]}: best {min(ms[name]):7.3f}  median {float(np.median(ms[name])):7.3f}; "
                  f"per Metropolis step {float(np.median(ms[name])) / depth[name]:7.3f}; accept rate {acc[name]:.3f}; exhausted {mc.prior_exhausted()}",
                  file=out, flush=True)


def efficiency(out):
    import numpy as np
    import torch
    from pysurfinv_amd import settings
    from pysurfinv_amd.mcmc import MetropolisBatch, PriorRules
    from pysurfinv_amd.obsdata import DispersionData
    from pysurfinv_amd.paramlsq import ParamLsqBatch
    dev = torch.device("cuda:0")
    NP, CPP, T = 16, 32, 2000
    mb, c_obs, unc = settings.synthetic_observations(NP, dev)
    N = mb.spec.n
    rules = PriorRules(mb)
    tracks, secs = {}, {}
    for name in ("default", "laplace"):
        mc = MetropolisBatch(mb.spec, mb.to_model, settings.MCMC_PERIODS, np.repeat(c_obs, CPP, axis=0), np.repeat(unc, CPP, axis=0),
                             device=dev, seed=3, isgood=rules)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        start = None
        if name == "laplace":
            inv = ParamLsqBatch(mb, [DispersionData("R", "c", settings.MCMC_PERIODS, c_obs, unc)], rules=rules)
            start = inv.run(8)["params"].contiguous()
            pf = inv.proposal_factor()
            mc.set_proposal(pf["factor"], CPP)
        tr = mc.run_points(NP, CPP, T, on_device=True, start=start)
        e1.record()
        torch.cuda.synchronize()
        tracks[name], secs[name] = tr.cpu().numpy(), e0.elapsed_time(e1) / 1e3
        extra = f"; fit rms median {float(inv.rms.median()):.4f}, factor fallbacks {int(pf['flag'].sum())}" if name == "laplace" else ""
        print(f"{name}: {NP} points x {CPP} chains x {T} steps in {secs[name]:.2f} s (fit and factor included), spec_depth "
              f"{mc.auto_spec_depth(NP * CPP)}, exhausted {mc.prior_exhausted()}{extra}", file=out, flush=True)
    pmin = np.minimum(*[tracks[k][..., 0].reshape(NP, -1).min(axis=1) for k in tracks])
    thres = np.maximum(2 * pmin, pmin + 0.5)
    names = [f"p{j}" for j in range(N)]
    print(f"{'':10s}{'accept':>8s}{'steps to thres (median / 90 % / never)':>42s}", file=out)
    taus = {}
    for name, tr in tracks.items():
        acc = tr[:, :, 1:, 2].mean()
        below = tr[..., 0] < thres[:, None, None]
        first = np.where(below.any(axis=2), below.argmax(axis=2), T).ravel()
        st = tr[..., 3:].copy()                                         # the chains' states: a rejected row keeps the last accepted one
        a = tr[..., 2] > 0.5
        idx = np.maximum.accumulate(np.where(a, np.arange(T)[None, None, :], 0), axis=2)
        st = np.take_along_axis(st, idx[..., None], axis=2)[:, :, T // 2:]
        taus[name] = np.array([[sokal_tau(st[i, k, :, j]) for j in range(N)] for i in range(NP) for k in range(CPP)])
        print(f"{name:10s}{acc:8.3f}{np.median(first):18.0f} /{np.percentile(first, 90):8.0f} /{int((first == T).sum()):6d} of {first.size}", file=out)
    print("integrated autocorrelation time (median over chains; second half of every chain) and effective samples per 1000 steps", file=out)
    print(f"{'parameter':>10s}{'tau default':>14s}{'tau laplace':>14s}{'ESS/1000 default':>18s}{'ESS/1000 laplace':>18s}", file=out)
    for j, nm in enumerate(names):
        td, tl = np.median(taus["default"][:, j]), np.median(taus["laplace"][:, j])
        print(f"{nm:>10s}{td:14.1f}{tl:14.1f}{1000 / td:18.1f}{1000 / tl:18.1f}", file=out)
    td, tl = np.median(taus["default"]), np.median(taus["laplace"])
    print(f"{'all':>10s}{td:14.1f}{tl:14.1f}{1000 / td:18.1f}{1000 / tl:18.1f}", file=out, flush=True)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    if len(sys.argv) > 1:
        step = sys.argv[1]
        with open(os.path.join(OUT, {"timing": "time_cov_proposal.txt", "efficiency": "efficiency.txt"}[step]), "w") as fh:
            {"timing": timing, "efficiency": efficiency}[step](fh)
        sys.exit(0)
    for step, limit in LIMITS.items():                                 # chained: a step that fails, faults or hangs ends the script
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step]).returncode
        print(f"{step}: exit status {rc}", flush=True)
        if rc != 0:
            sys.exit(rc)
