#!/usr/bin/env python3
"""GPU box: what the adaptive proposal (``MetropolisBatch.set_adaptive``, surfdisp_mcmc_adapt_device) buys per step and what it costs
per lock step, into profiles/adaptive_proposal/.

    python scripts/time_adaptive_proposal.py              # both steps below, each a child process under its own time limit, chained:
                                                          # the second starts only if the first ended well
    python scripts/time_adaptive_proposal.py efficiency   # -> efficiency.txt
    python scripts/time_adaptive_proposal.py timing       # -> time_adaptive_proposal.txt

efficiency: the data set of profiles/cov_proposal/efficiency.txt - the 16 synthetic points of the least-squares tests (MCMC_SETTING),
32 chains x 2000 steps each under PriorRules, seed 3 - with the default proposal, the Laplace factor and the adaptive proposal, and a
thermal data set of the same size (C5_SETTING, no rules: the Laplace route refuses it) with the default proposal and the adaptive
one.  The adaptive runs: the defaults of ``set_adaptive`` and one option changed at a time (every, start, forget, ridge).  Per run:
the accept rate and, per parameter, the integrated autocorrelation time of the chains' states (Sokal's window, c = 5; the median
over the 512 chains) over the rows from ``until`` = 1000 on - the same rows for every proposal: before them an adaptive chain is
no sample -, the effective samples per 1000 steps, and the steps until a chain's misfit first falls below its point's threshold
max(2 min, min + 0.5) (min: the point's smallest misfit over the runs of the data set).

timing: ms per lock step of 25 600 chains x MCMC_SETTING (96 layers, 19 periods) in two chain groups, 50 chains per point:
the reference's proposal, a fixed factor per point, and the adaptive proposal with an update every 10 steps (every update refactors:
min_weight = the chains of a point), under PriorRules(vs_max=4.9) and without a prior, device events around windows of 40 lock steps, the
variants alternating on ONE sampler per prior (the same two group streams for all of them: with a sampler per variant the figures
depended on which sampler of the process a variant was); 'factor rejoin' is the fixed factor with the chain groups joining and
forking at the adaptive variant's instants, so that the join and the update can be told apart; 'adaptive small' keeps the scale at
exp(-3): the windows start from prior draws, whose pooled covariance is the prior's, so the adaptive variant's first factors propose
far wider than a converged run's and the propose kernel redraws more often (the redraws per proposal are printed).  With PARENT_LIB=<a
build of the parent commit's library> the first two variants are also measured with that library, in child processes that
alternate with this tree's (``SURFDISP_LIB_PATH``): the parent commit's step, in the same session.  The update's own kernels
(adapt + factor, 512 points) are timed alone; the cost of an instant - join, update, fork - is ``every`` times the difference
between the adaptive and the fixed-factor step.  (The adaptive variant's accept rate in these short windows is that of chains
40 steps from their prior draws whose proposal has just been scaled: it says nothing about a run.)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "adaptive_proposal")
LIMITS = {"efficiency": 420, "timing": 420}            # seconds per step
CHILD_LIMIT = 150                                      # one timing child


def efficiency(out):
    import numpy as np
    import torch
    from time_cov_proposal import sokal_tau
    from pysurfinv_amd import settings
    from pysurfinv_amd.mcmc import ADAPT_DEFAULTS, MetropolisBatch, PriorRules
    from pysurfinv_amd.obsdata import DispersionData
    from pysurfinv_amd.paramlsq import ParamLsqBatch
    dev = torch.device("cuda:0")
    NP, CPP, T = 16, 32, 2000
    UNTIL = T // 2
    tuned = [("adaptive", {})] + [(f"adaptive {k}={v}", {k: v}) for k, v in
                                  (("every", 5), ("every", 25), ("start", 100), ("forget", 0.98), ("forget", 0.9), ("ridge", 1e-2),
                                   ("ridge", 1e-4), ("target_accept", -1.0))]
    print(f"device: {torch.cuda.get_device_name(0)}; {NP} points x {CPP} chains x {T} steps, seed 3; set_adaptive's defaults: {ADAPT_DEFAULTS}; "
          f"until = {UNTIL}: tau, ESS and the accept rate over the rows {UNTIL} .. {T - 1} of every run", file=out, flush=True)
    for label, setting, with_rules in (("MCMC_SETTING under PriorRules", settings.MCMC_SETTING, True),
                                       ("C5_SETTING (thermal mantle), no rules", settings.C5_SETTING, False)):
        mb, c_obs, unc = settings.synthetic_observations(NP, dev, setting=setting)
        N = mb.spec.n
        rules = PriorRules(mb) if with_rules else None
        runs = [("default", None)] + ([("laplace", None)] if with_rules else []) + tuned
        tracks, info = {}, {}
        for name, opts in runs:
            mc = MetropolisBatch(mb.spec, mb.to_model, settings.MCMC_PERIODS, np.repeat(c_obs, CPP, axis=0), np.repeat(unc, CPP, axis=0),
                                 device=dev, seed=3, isgood=rules)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            start, extra = None, ""
            if name == "laplace":
                inv = ParamLsqBatch(mb, [DispersionData("R", "c", settings.MCMC_PERIODS, c_obs, unc)], rules=rules)
                start = inv.run(8)["params"].contiguous()
                mc.set_proposal(inv.proposal_factor()["factor"], CPP)
            elif opts is not None:
                mc.set_adaptive(CPP, **opts)
            tr = mc.run_points(NP, CPP, T, on_device=True, start=start)
            e1.record()
            torch.cuda.synchronize()
            if opts is not None:
                ad = mc.adaptation()
                extra = (f"; updates {int(ad['n_updates'].max())}, fallbacks {int(ad['fallbacks'].sum())}, scale median "
                         f"{float(ad['scale'].median()):.3f} (min {float(ad['scale'].min()):.3f}, max {float(ad['scale'].max()):.3f})")
            tracks[name] = tr.cpu().numpy()
            info[name] = f"{e0.elapsed_time(e1) / 1e3:.2f} s, exhausted {mc.prior_exhausted()}{extra}"
        pmin = np.min([tracks[k][..., 0].reshape(NP, -1).min(axis=1) for k in tracks], axis=0)
        thres = np.maximum(2 * pmin, pmin + 0.5)
        print(f"\n== {label}: {N} parameters", file=out)
        print(f"{'':28s}{'accept':>8s}{'tau':>8s}{'ESS/1000':>10s}{'tau worst par':>15s}   steps to thres (median / 90 % / never)", file=out)
        for name, tr in tracks.items():
            acc = tr[:, :, UNTIL:, 2].mean()
            below = tr[..., 0] < thres[:, None, None]
            first = np.where(below.any(axis=2), below.argmax(axis=2), T).ravel()
            a = tr[..., 2] > 0.5
            idx = np.maximum.accumulate(np.where(a, np.arange(T)[None, None, :], 0), axis=2)
            st = np.take_along_axis(tr[..., 3:], idx[..., None], axis=2)[:, :, UNTIL:]     # a rejected row keeps the last accepted state
            tau = np.array([[sokal_tau(st[i, k, :, j]) for j in range(N)] for i in range(NP) for k in range(CPP)])
            med, worst = float(np.median(tau)), float(np.median(tau, axis=0).max())
            print(f"{name:28s}{acc:8.3f}{med:8.1f}{1000 / med:10.1f}{worst:15.1f}   {np.median(first):6.0f} /{np.percentile(first, 90):6.0f} /"
                  f"{int((first == T).sum()):5d} of {first.size}   [{info[name]}]", file=out, flush=True)


def _timing_child():
    """One process: the variants of this library, alternating windows; one JSON line."""
    import numpy as np
    import torch
    from pysurfinv_amd import _lib, settings
    from pysurfinv_amd.mcmc import MetropolisBatch, PriorRules, fused_schedule
    REPS = int(os.environ.get("REPS", "4"))
    dev = torch.device("cuda:0")
    mb, c_obs, unc = settings.synthetic_observations(1, dev)
    N = mb.spec.n
    C, CPP, NSTEPS, EVERY = 25600, 50, 40, 10
    has_adapt = hasattr(_lib.lib(), "surfdisp_mcmc_adapt_device")

    def factors():
        rng = np.random.default_rng(1)
        fac = []
        for _ in range(C // CPP):
            a = rng.normal(size=(N, N))
            c = a @ a.T / N + 0.2 * np.eye(N)
            d = np.sqrt(np.diag(c))
            fac.append(mb.spec.step[:, None] * np.linalg.cholesky(c / np.outer(d, d)))
        return torch.as_tensor(np.stack(fac), device=dev)

    def set_mode(mc, kind, fac):
        """ONE sampler per prior takes every variant in turn, so that all of them run on the same two group streams."""
        mc.set_proposal(None)                           # (turns adaptation off too)
        if kind.startswith("factor"):
            mc.set_proposal(fac, CPP)
        elif kind.startswith("adaptive"):
            bounds = (-3.0, -3.0) if kind.endswith("small") else (-3.0, 3.0)
            mc.set_adaptive(CPP, every=EVERY, start=1, until=NSTEPS + 1, min_weight=CPP, log_scale_bounds=bounds)

    def window(mc, nsteps, rejoin=False):
        """run()'s own loop (``_walk`` over ``fused_schedule``, two chain groups) with events around the rows 1 .. nsteps; rejoin:
        the rows walked in pieces that end at the adaptive variant's instants, so that the groups join and fork there without an
        update between."""
        p = mc._start(C, False, None).contiguous().clone()
        track = torch.zeros((C, nsteps + 1, 3 + N), dtype=torch.float64, device=dev)
        ad = mc._adaptation
        if ad is not None:
            ad.begin(C, nsteps + 1, mc._given, mc.isgood)
        cg = mc.chain_groups(C, 2)
        mc._last_groups = cg                            # (last_prior_tries reads the groups' buffers)
        calls = list(fused_schedule(nsteps + 1, 1))
        ends = [i + 1 for i in range(1, nsteps + 1) if (i - 1) % EVERY == 0] if rejoin else []
        pieces = [calls[a:b] for a, b in zip([1] + ends, ends + [nsteps + 1]) if a < b]
        mc._walk(p, track, cg, 1, calls[:1])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for piece in pieces:
            mc._walk(p, track, cg, 1, piece)
        e1.record()
        torch.cuda.synchronize()
        if ad is not None:
            ad.end()
        return e0.elapsed_time(e1) / nsteps, float(track[:, 1:, 2].mean())

    kinds = ["plain", "factor", "factor rejoin"] + (["adaptive", "adaptive small"] if has_adapt else [])
    ms, acc, tries = {}, {}, {}
    fac = factors()
    for prior in ("PriorRules", "no prior"):
        isgood = PriorRules(mb, vs_max=4.9) if prior == "PriorRules" else None
        mc = MetropolisBatch(mb.spec, mb.to_model, settings.MCMC_PERIODS, c_obs[0], unc[0], device=dev, seed=3, isgood=isgood)
        for k in kinds:
            set_mode(mc, k, fac)
            window(mc, 10, rejoin=k.endswith("rejoin"))
            ms[f"{prior}, {k}"] = []
        for _ in range(REPS):
            for k in kinds:
                set_mode(mc, k, fac)
                t, acc[f"{prior}, {k}"] = window(mc, NSTEPS, rejoin=k.endswith("rejoin"))
                ms[f"{prior}, {k}"].append(t)
                lt = mc.last_prior_tries() if k != "plain" else None
                tries[f"{prior}, {k}"] = None if lt is None else float(lt.view(torch.int16).float().mean())
    res = dict(lib=os.path.basename(_lib.LIB_PATH), ms=ms, accept=acc, tries=tries)
    if has_adapt:                                       # the update's own kernels, alone on the stream
        set_mode(mc, "adaptive", fac)
        p = mc._start(C, False, None).contiguous().clone()
        track = torch.zeros((C, 12, 3 + N), dtype=torch.float64, device=dev)
        ad = mc._adaptation
        ad.begin(C, 24, mc._given, mc.isgood)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ad.update(p, track, 12 * (3 + N), 3 + N, 10)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            ad.prev = 0
            ad.update(p, track, 12 * (3 + N), 3 + N, 10)
        e1.record()
        torch.cuda.synchronize()
        ad.end()
        res["update_kernels_ms"] = e0.elapsed_time(e1) / 20
    print("RESULT " + json.dumps(res), flush=True)


def timing(out):
    import numpy as np
    parent = os.environ.get("PARENT_LIB")
    rounds = int(os.environ.get("ROUNDS", "2"))
    libs = [("this tree", None)] + ([("parent commit", parent)] if parent else [])
    got = {name: [] for name, _ in libs}
    for _ in range(rounds):
        for name, path in libs:                        # alternating; a child that fails, faults or hangs ends the script
            env = dict(os.environ)
            if path:
                env["SURFDISP_LIB_PATH"] = path
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "timing-child"],
                               env=env, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
                sys.exit(r.returncode)
            got[name].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    print("25 600 chains x MCMC_SETTING, two chain groups, 50 chains per point, under PriorRules(vs_max=4.9) and without a prior; "
          "'factor rejoin': the fixed factor with the groups joining and forking every 10 steps, no update; ms per lock step of all chains over windows of "
          "40 lock steps; per library the processes alternate, per process the variants alternate", file=out)
    med = {}
    for name, _ in libs:
        for kind in got[name][0]["ms"]:
            v = np.array([x for g in got[name] for x in g["ms"][kind]])
            per = [float(np.median(g["ms"][kind])) for g in got[name]]
            med[name, kind] = float(np.median(v))
            print(f"    {name:14s} {kind:26s} best {v.min():7.3f}  median {np.median(v):7.3f}  worst {v.max():7.3f}   per process "
                  f"{' '.join(f'{x:.3f}' for x in per)}   accept rate {got[name][-1]['accept'][kind]:.3f}"
                  + ("" if got[name][-1]["tries"][kind] is None else f", redraws per proposal in the last step {got[name][-1]['tries'][kind]:.2f}"),
                  file=out, flush=True)
    uk = [g["update_kernels_ms"] for g in got["this tree"] if "update_kernels_ms" in g]
    if uk:
        print(f"    the update's kernels alone (adapt + factor, 512 points): {float(np.median(uk)):.4f} ms per instant", file=out)
        for prior in ("PriorRules", "no prior"):
            f, r, a, sm = (med["this tree", f"{prior}, {k}"] for k in ("factor", "factor rejoin", "adaptive", "adaptive small"))
            print(f"    {prior}: per instant (10 x the difference per lock step): join and fork alone {10 * (r - f):+.3f} ms, the update between them "
                  f"{10 * (sm - r):+.3f} ms, together {10 * (sm - f):+.3f} ms = {sm - f:+.4f} ms per lock step at every = 10; the wide proposals of "
                  f"chains 40 steps from their prior draws (redraws, rougher models) {a - sm:+.4f} ms per lock step more", file=out, flush=True)
        if parent:
            f, sm = med["parent commit", "PriorRules, factor"], med["this tree", "PriorRules, adaptive small"]
            print(f"    against the parent commit's fixed-factor step under PriorRules: {sm:.3f} against {f:.3f} ms, {sm - f:+.4f} ms per lock step "
                  f"({100 * (sm - f) / f:+.1f} %)", file=out, flush=True)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    if len(sys.argv) > 1:
        step = sys.argv[1]
        if step == "timing-child":
            _timing_child()
            sys.exit(0)
        with open(os.path.join(OUT, {"timing": "time_adaptive_proposal.txt", "efficiency": "efficiency.txt"}[step]), "w") as fh:
            {"timing": timing, "efficiency": efficiency}[step](fh)
        sys.exit(0)
    for step, limit in LIMITS.items():                                 # chained: a step that fails, faults or hangs ends the script
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step]).returncode
        print(f"{step}: exit status {rc}", flush=True)
        if rc != 0:
            sys.exit(rc)
