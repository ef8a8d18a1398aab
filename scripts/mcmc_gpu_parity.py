#!/usr/bin/env python3
"""GPU: raw results of the Python layer of the Metropolis sampler, to compare two revisions of pysurfinv_amd/mcmc.py (and what it
imports) on the same library build byte for byte.

    mcmc_gpu_parity.py save OUT.npz [ROOT]   ROOT: the tree whose pysurfinv_amd is imported (default: this one); load the same
                                             library into both with SURFDISP_LIB_PATH
    mcmc_gpu_parity.py compare A.npz B.npz   one line per case; exit status 1 when a key, a dtype, a shape or a byte differs

Every case: a seeded sampler of 8 or 16 chains x 16 rows on the continental model of ``settings.synthetic_observations`` (one case on
the thermal model, three with joint data on the tests' continental model), through the public methods only.  After every run the
track, ``_counter``, ``n_forward``, ``prior_exhausted()``, ``last_prior_tries()`` and ``adaptation()`` (where there is one) are kept.
The cases: no rules (depths 1, 2, 4; two groups; two runs in a row; ``run(start=)``; ``run_points`` with a [points, N] start;
``independent=True``), ``PriorRules`` in rounds mode (depth 1, two groups) and with ``redraw="kernel"`` (depths 1 and 3, two groups,
caps tight enough that nodes exhaust), ``set_proposal`` ([N, N] and [points, N, N] factors, with and without rules, depths 1 and 3,
two groups, then off), ``set_adaptive(4, every=3, start=2, until=11, min_weight=4)`` (depths 1 and 3, two groups, after a
``set_proposal`` factor, the thermal model, then off), joint data (Rc + RU + Lc at depths 1 and 2, with an ellipticity set at depth
2) and ``local_rows`` with per-chain observations (depths 1 and 2)."""
import os
import sys

import numpy as np

CHAINL, CPP = 16, 4
ADAPT = dict(every=3, start=2, until=11, min_weight=4)


def save(path, root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    import torch
    from pysurfinv_amd import settings
    from pysurfinv_amd.forward import BatchPlan
    from pysurfinv_amd.layers_batch import Model1DBatch
    from pysurfinv_amd.mcmc import MetropolisBatch, PriorRules
    from pysurfinv_amd.obsdata import DispersionData
    dev = torch.device("cuda:0")
    out = {}

    def keep(tag, mc, tr):
        torch.cuda.synchronize()
        out[f"{tag}/track"] = (tr if isinstance(tr, np.ndarray) else tr.cpu().numpy()).copy()
        out[f"{tag}/counter_n_forward_exhausted"] = np.array([mc._counter, mc.n_forward, mc.prior_exhausted()], np.int64)
        t = mc.last_prior_tries()
        if t is not None:
            out[f"{tag}/tries"] = t.cpu().view(torch.int16).numpy().copy()
        ad = mc.adaptation()
        for k, v in ({} if ad is None else ad).items():
            out[f"{tag}/adaptation/{k}"] = v.cpu().numpy().copy()

    mb, c_obs, unc = settings.synthetic_observations(4, dev)
    N = mb.spec.n
    rep = lambda a, C: np.repeat(a, C // a.shape[0], axis=0)

    def sampler(C, isgood=None, seed=3, model=mb, obs=(c_obs, unc), **kw):
        return MetropolisBatch(model.spec, model.to_model, settings.MCMC_PERIODS, rep(obs[0], C), rep(obs[1], C), device=dev, seed=seed,
                               isgood=isgood, **kw)

    def ways(tag, make, C=16, depths=(1, 3), **kw):
        """One fresh sampler per way of stepping: the depths, then two chain groups."""
        for name, how in [(f"d{d}", dict(spec_depth=d)) for d in depths] + [("g2", dict(groups=2, spec_depth=1))]:
            mc = make()
            keep(f"{tag}/{name}", mc, mc.run(C, CHAINL, **how, **kw))

    # ---- no rules
    ways("plain", lambda: sampler(16), depths=(1, 2, 4))
    mc = sampler(8)
    keep("plain/again/1", mc, mc.run(8, CHAINL))
    keep("plain/again/2", mc, mc.run(8, CHAINL, spec_depth=1))
    starts = sampler(16, seed=9).reset(16).contiguous()
    mc = sampler(16)
    keep("plain/start", mc, mc.run(16, CHAINL, start=starts))
    mc = sampler(16)
    keep("plain/run_points_start", mc, mc.run_points(4, CPP, CHAINL, start=starts[:4].contiguous()))
    mc = sampler(16, independent=True)
    keep("plain/independent", mc, mc.run(16, CHAINL))
    # ---- PriorRules
    ways("rounds", lambda: sampler(16, PriorRules(mb, vs_max=4.9)), depths=(1,), init_first=False)
    ways("kernel", lambda: sampler(16, PriorRules(mb, vs_max=4.9, redraw="kernel")), init_first=False)
    good = sampler(64, PriorRules(mb, vs_max=4.9), seed=9).reset(16).contiguous()          # states the cap 4.9 accepts ...
    mc = sampler(16, PriorRules(mb, vs_max=0.5, redraw="kernel", gauss_tries=3, uniform_tries=4))    # ... under a cap nothing passes
    for i in range(3):
        mc.fused_step(good, first=(i == 0))
    keep("kernel/exhausting", mc, good)
    # ---- set_proposal
    rng = np.random.default_rng(1)

    def factors(F):
        fac = []
        for _ in range(F):
            a = rng.normal(size=(N, N))
            c = a @ a.T / N + 0.2 * np.eye(N)
            d = np.sqrt(np.diag(c))
            fac.append(mb.spec.step[:, None] * np.linalg.cholesky(c / np.outer(d, d)))
        return torch.as_tensor(np.stack(fac), device=dev)

    one, per_point = factors(1)[0].contiguous(), factors(4)
    for rtag, rules in (("norules", lambda: None), ("rules", lambda: PriorRules(mb, vs_max=4.9))):
        for ftag, args in (("NN", (one,)), ("FNN", (per_point, CPP))):
            def make():
                mc = sampler(16, rules())
                mc.set_proposal(*args)
                return mc
            ways(f"factor/{rtag}/{ftag}", make, init_first=False)
    mc = sampler(16, PriorRules(mb, vs_max=4.9))
    mc.set_proposal(per_point, CPP)
    keep("factor/off/with", mc, mc.run(16, CHAINL, init_first=False))
    mc.set_proposal(None)
    keep("factor/off/after", mc, mc.run(16, CHAINL, init_first=False))
    # ---- set_adaptive
    for name, how in (("d1", dict(spec_depth=1)), ("d3", dict(spec_depth=3)), ("g2", dict(groups=2, spec_depth=1))):
        mc = sampler(16, PriorRules(mb, vs_max=4.9))
        mc.set_adaptive(CPP, **ADAPT)
        keep(f"adaptive/{name}", mc, mc.run_points(4, CPP, CHAINL, **how))
    mc = sampler(16)
    mc.set_proposal(per_point, CPP)
    mc.set_adaptive(CPP, **ADAPT)
    keep("adaptive/after_factor", mc, mc.run_points(4, CPP, CHAINL))
    mc.set_adaptive(None)
    keep("adaptive/off/factor_again", mc, mc.run_points(4, CPP, CHAINL))
    mc.set_proposal(None)
    keep("adaptive/off/plain_again", mc, mc.run_points(4, CPP, CHAINL))
    tmb, t_obs, t_unc = settings.synthetic_observations(2, dev, setting=settings.C5_SETTING)
    mc = sampler(8, model=tmb, obs=(t_obs, t_unc))
    mc.set_adaptive(CPP, **ADAPT)
    keep("adaptive/thermal", mc, mc.run_points(2, CPP, CHAINL))
    # ---- joint data: the curves of a slightly faster start model, per-chain rows, a few masked entries
    from settings import CONT
    jmb = Model1DBatch(CONT, device=dev)
    model, nlay = jmb.to_model(torch.as_tensor(jmb.spec.v0, device=dev)[None, :] * 1.01)
    jr = np.random.default_rng(0)

    def curve(w, q, T, unc_abs, k):
        plan = BatchPlan(1, model.shape[2], len(T), device=dev)
        res = plan.run(model.contiguous(), torch.as_tensor(np.asarray(T, np.float32), device=dev), kind=1 if w == "L" else 2, nlay=nlay,
                       want_ratio=(q == "E"))
        val = res[{"c": 0, "U": 1, "E": 3}[q]][0].double().cpu().numpy()
        val = np.tile(val, (8, 1)) * (1 + 0.01 * jr.standard_normal((8, 1)))
        val[::5 + k, k % len(T)] = np.nan
        return DispersionData(w, q, T, val, np.full((8, len(T)), unc_abs), weight=1.0 + 0.25 * k)

    three = [curve("R", "c", np.arange(8.0, 40.0, 4.0), 0.02, 0), curve("R", "U", np.array([6.0, 10.0, 16.0, 30.0]), 0.04, 1),
             curve("L", "c", np.array([10.0, 20.0, 30.0, 40.0]), 0.03, 2)]
    for name, data, d in (("RcRULc/d1", three, 1), ("RcRULc/d2", three, 2),
                          ("RcRULcRE/d2", three + [curve("R", "E", np.array([8.0, 14.0, 20.0, 30.0]), 0.02, 3)], 2)):
        mc = MetropolisBatch(jmb.spec, jmb.to_model, device=dev, seed=4, data=data)
        keep(f"joint/{name}", mc, mc.run(8, CHAINL, spec_depth=d))
    # ---- local_rows: a per-point topography, per-chain observations
    setting = dict(settings.MCMC_SETTING, Info=dict(settings.MCMC_SETTING["Info"], topo=0.0))
    lmb = Model1DBatch(setting, device=dev, local_keys=["topo"]).set_local_info(np.array([[-1.0], [0.8], [2.5], [0.3]]))
    for d in (1, 2):
        mc = sampler(16, model=lmb, local_rows=np.repeat(np.arange(4), CPP))
        keep(f"local_rows/d{d}", mc, mc.run(16, CHAINL, spec_depth=d, init_first=False))
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes, pysurfinv_amd of {root}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    cases = {}
    for k in sorted(set(a.files) | set(b.files)):
        same = k in a.files and k in b.files and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        cases.setdefault(k.rsplit("/", 2 if "/adaptation/" in k else 1)[0], []).append((k, same))
    diff = []
    for case, keys in cases.items():
        bad = [k for k, same in keys if not same]
        diff += bad
        print(f"    {case:32s} {len(keys):3d} arrays  " + ("equal" if not bad else f"DIFFERENT: {bad}"))
    print(f"{pa} against {pb}: {len(cases)} cases, " + ("equal byte for byte" if not diff else f"DIFFERENT in {len(diff)} arrays"))
    return 1 if diff else 0


if __name__ == "__main__":
    if sys.argv[1] == "save":
        save(sys.argv[2], os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
