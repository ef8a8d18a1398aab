"""Covariance-shaped proposals (csrc/surfdisp_mcmc_cov.hip: surfdisp_mcmc_propose_cov_device, surfdisp_mcmc_cov_factor_device;
``MetropolisBatch.set_proposal``, ``run(start=)``, ``ParamLsqBatch.proposal_factor``, ``run_grid(proposal="laplace")``) - what needs
no device: the host statement (tests/mcmc_cov_replay.py) against the replays it is built on, its statistics, the numpy statement of
the factor, the interface's refusals, the entries' argument checks (invalid calls only: nothing launches), and the share of
doubtful cases in the configurations tests/test_mcmc_cov_gpu.py compares on the device.

Configurations without a model ("box cases"): a box around a centre, one random SPD covariance per factor, states scattered
around the centre.
  wide    the box 24 sigma wide, states within 2 sigma of the centre, caps 1000 / 10000: nothing is redrawn but by accident.
  tight   the box 2.8 sigma wide (of the widest factor: narrower ones leave it less often), states within 0.3 sigma, G = 6, U = 3:
          a third of the first candidates leave the box, `tries` takes every value 0 .. G, and one case in ten reaches the uniform
          phase (whose first draw is good: without rules a uniform draw always is).
With rules: MCMC_SETTING under PriorRules(vs_max = 4.5), the start states of tests/test_prior_redraw.py, factors 4 diag(step) R with
a random unit lower-triangular-ish R per point (the "tight" configuration of that file with correlated steps)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mcmc_replay as R                              # noqa: E402
import mcmc_prior_replay as PR                       # noqa: E402
import mcmc_cov_replay as CR                         # noqa: E402
from test_mcmc_replay import SEEDS, _bits            # noqa: E402
from test_prior_redraw import CHAIN0_BIG, _cpu_model, _starts   # noqa: E402

from pysurfinv_amd import mcmc, settings             # noqa: E402
from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402
from pysurfinv_amd.mcmc import MetropolisBatch, PriorRules, cov_factor_reference   # noqa: E402
from pysurfinv_amd.proposal import Factor, KernelRedraw, ReferenceSteps, rules_args   # noqa: E402

# the stand-alone configurations of the entry, no rules: name -> (N, C, depth, chains_per_factor)
CONFIGS = {"a": (1, 3, 1, 1), "b": (13, 67, 1, 8), "c": (13, 67, 4, 8), "d": (64, 5, 2, 2)}
WIDE = dict(half=12.0, spread=2.0, G=1000, U=10000)
TIGHT = dict(half=1.4, spread=0.3, G=6, U=3)
RULES = dict(kw=dict(vs_max=4.5), step=4.0, G=1000, U=10000, C=67, cpf=8)


def random_spd(rng, N):
    """A random SPD matrix with correlations: A A^T / N + 0.2 I, scaled."""
    a = rng.normal(size=(N, N))
    return (a @ a.T / N + 0.2 * np.eye(N)) * rng.uniform(0.5, 2.0) ** 2


def box_case(N, C, cpf, chain0, seed, half, spread):
    """(p [C, N], vmin, vmax, factor [nF, N, N], factor0) of a configuration without a model: the factors the chains chain0 ..
    chain0 + C - 1 read (factor0: the index of the first in the whole sampler's list), Cholesky factors of random SPD matrices."""
    rng = np.random.default_rng(seed)
    f0 = chain0 // cpf
    nF = (chain0 + C - 1) // cpf - f0 + 1
    cov = np.stack([random_spd(rng, N) for _ in range(nF)])
    L = np.linalg.cholesky(cov)
    sig = np.sqrt(np.einsum("fii->fi", cov))
    f = np.array([(chain0 + c) // cpf - f0 for c in range(C)])
    centre = 3.0 * rng.normal(size=N)
    p = centre + spread * sig[f] * rng.uniform(-1, 1, (C, N))
    w = half * sig.max(axis=0)
    return p, centre - w, centre + w, L, f0


@functools.lru_cache(maxsize=None)
def rules_case(chain0):
    """(p, spec, factor [nF, 13, 13], factor0, rules on the CPU model) of the configuration with PriorRules."""
    m = _cpu_model()
    spec = m.spec
    C, cpf, N = RULES["C"], RULES["cpf"], spec.n
    rng = np.random.default_rng(29)
    f0 = chain0 // cpf
    nF = (chain0 + C - 1) // cpf - f0 + 1
    fac = []
    for _ in range(nF):
        c = random_spd(rng, N)
        d = np.sqrt(np.diag(c))
        fac.append(RULES["step"] * spec.step[:, None] * np.linalg.cholesky(c / np.outer(d, d)))   # unit-variance rows x 4 step
    p = np.array(_starts(4.5, C))
    return p, spec, np.stack(fac), f0, PriorRules(m, **RULES["kw"])


def replay_box(name, chain0, cfg, seed=SEEDS[1], counter=2 ** 32 + 3, given=None, depth=None):
    N, C, d, cpf = CONFIGS[name]
    d = d if depth is None else depth
    p, lo, hi, L, f0 = box_case(N, C, cpf, chain0, 100 + N, cfg["half"], cfg["spread"])
    return (p, lo, hi, L, f0, cpf, d), CR.propose_cov(p, lo, hi, L, cpf, None, seed, counter, d, cfg["G"], cfg["U"], chain0, given, f0)


# ------------------------------------------------------------------------------------------------------ the host statement
def test_diagonal_factor_is_the_plain_proposal_and_the_uniform_phase_is_the_prior_replays():
    """Retry 0 of node 0 with L = diag(step), in a box nothing leaves: mcmc_replay's plain proposal (its first candidate, cos) within
    the tolerance; G = 0: every row is mcmc_prior_replay's uniform candidate bit for bit."""
    spec = _cpu_model().spec
    N, C = spec.n, 9
    rng = np.random.default_rng(3)
    p = spec.vmin + (spec.vmax - spec.vmin) * rng.uniform(0.3, 0.7, (C, N))
    lo, hi = spec.vmin - 100.0, spec.vmax + 100.0
    for chain0 in (0, CHAIN0_BIG):
        out, tries, margin, tol, slack = CR.propose_cov(p, lo, hi, np.diag(spec.step)[None], 1 << 62, None, SEEDS[1], 2 ** 32 + 3, 1, 1000, 10000, chain0)
        ref, rm, rt, uni = R.propose(p, lo, hi, spec.step, SEEDS[1], 2 ** 32 + 3, False, chain0)
        assert (tries == 0).all() and not uni.any() and (margin > 1).all() and np.isinf(slack).all()
        assert (np.abs(out[:, 0] - ref) <= tol[:, 0]).all() and (tol[:, 0] <= 2.5 * rt).all()
        out, tries, *_ = CR.propose_cov(p, spec.vmin, spec.vmax, np.diag(spec.step)[None], 1 << 62, None, SEEDS[0], 7, 2, 0, 5, chain0)
        for k in range(3):
            want = PR.candidate(p if k != 1 else out[:, 0], spec.vmin, spec.vmax, spec.step, SEEDS[0], 7, k, 0, 0, PR.retry_index(C, N, chain0, 0))[0]
            assert np.array_equal(_bits(out[:, k]), _bits(want)) and (tries[:, k] == 0).all()
    # a retry moves the stream index, not the tag: retry 1 of node 0 is another draw
    u0, u1 = CR.uniforms(SEEDS[0], 5, 0, 0, C, N, 0), CR.uniforms(SEEDS[0], 5, 0, 1, C, N, 0)
    assert (u0[0] != u1[0]).all()


def test_statistics_of_the_statement():
    """4096 draws from one state at the centre of a box 40 sigma wide, N = 13, a random SPD Sigma: every mean within
    6 sqrt(Sigma_ii / n), every sample covariance entry within 6 sqrt((Sigma_ii Sigma_jj + Sigma_ij^2) / n) of Sigma_ij."""
    n, N = 4096, 13
    rng = np.random.default_rng(17)
    cov = random_spd(rng, N)
    L = np.linalg.cholesky(cov)
    sig = np.sqrt(np.diag(cov))
    x = np.tile(3.0 * rng.normal(size=N), (n, 1))
    u1, u2 = CR.uniforms(SEEDS[0], 9, 0, 0, n, N, 0)
    v, inside, m, tol = CR.gaussian_candidates(x, x[0] - 20 * sig, x[0] + 20 * sig, np.broadcast_to(L, (n, N, N)), u1, u2, exact=False)
    assert inside.all()
    d = v - x
    assert (np.abs(d.mean(axis=0)) <= 6 * np.sqrt(np.diag(cov) / n)).all()
    S = d.T @ d / n
    assert (np.abs(S - cov) <= 6 * np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / n)).all()


def test_exact_row_agrees_with_the_double_sum():
    """The high-precision value and the plain double sum of one candidate differ by far less than the tolerance (mostly rounding of
    the double sum), on the widest row (N = 64)."""
    p, lo, hi, L, f0 = box_case(64, 2, 2, 0, 5, 12.0, 2.0)
    u1, u2 = CR.uniforms(SEEDS[0], 3, 0, 0, 2, 64, 0)
    z = CR.normals(u1, u2)
    for b in range(2):
        ex = CR.exact_row(p[b], L[0], u1[b], u2[b])
        terms = np.tril(L[0]) * z[b][None, :]
        tol = CR.tol_factor(64) * CR.EPS * (np.abs(p[b]) + np.abs(terms).sum(axis=1))
        assert (np.abs(ex - (p[b] + terms.sum(axis=1))) <= tol / 3).all()


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("chain0", [0, CHAIN0_BIG])
def test_doubtful_cases_of_the_wide_configurations(name, chain0):
    _, (out, tries, margin, tol, slack) = replay_box(name, chain0, WIDE)
    assert int(CR.doubtful(margin, slack).sum()) == 0                  # 1e-13 per decision: none is expected
    assert tries.max() < WIDE["G"] and (tries == 0).mean() > 0.9


@pytest.mark.parametrize("depth", [1, 4])
def test_doubtful_cases_and_spread_of_the_tight_configuration(depth):
    (p, lo, hi, L, f0, cpf, d), (out, tries, margin, tol, slack) = replay_box("c", 0, TIGHT, seed=SEEDS[depth > 1], counter=11, depth=depth)
    G, U = TIGHT["G"], TIGHT["U"]
    assert int(CR.doubtful(margin, slack).sum()) == 0
    hist = np.bincount(tries.ravel(), minlength=G + U + 1)
    print(f"tight depth {depth}: tries histogram {hist.tolist()}")
    assert (hist[:G] > 0).all()                                        # spread over the Gaussian phase
    assert hist[G] > 0 and tries.max() == G                            # the uniform phase is reached; its first draw is good
    assert ((out > lo) & (out < hi)).all()


@pytest.mark.parametrize("depth", [1, 4])
def test_doubtful_cases_with_rules(depth):
    p, spec, L, f0, rules = rules_case(0)
    out, tries, margin, tol, slack = CR.propose_cov(p, spec.vmin, spec.vmax, L, RULES["cpf"], rules, SEEDS[depth > 1], 11, depth,
                                                    RULES["G"], RULES["U"], 0, None, f0)
    n = int(CR.doubtful(margin, slack).sum())
    print(f"rules depth {depth}: {n} of {tries.size} doubtful, mean retries {tries.mean():.2f}, most {tries.max()}")
    assert n <= CR.MAX_EXCLUDED * tries.size
    assert rules(torch.as_tensor(out.reshape(-1, spec.n))).all() and (tries >= 1).mean() > 0.2 and tries.max() < RULES["G"]


# ------------------------------------------------------------------------------------------------------ the factor
def test_cov_factor_reference():
    rng = np.random.default_rng(41)
    for N in (1, 13, 64):
        cov = np.stack([random_spd(rng, N) for _ in range(5)])
        fixed = [2, 7] if N > 8 else []
        cov[1][fixed, :] = 0.0
        cov[1][:, fixed] = 0.0
        scale = 2.38 / np.sqrt(N)
        fb = rng.uniform(0.01, 0.1, N)
        L, flag = cov_factor_reference(cov, scale, fb)
        assert not flag.any() and not np.triu(L, 1).any()
        for p in range(5):
            free = np.flatnonzero(np.diag(cov[p]) != 0)
            ref = scale * np.linalg.cholesky(cov[p][np.ix_(free, free)])
            assert np.allclose(L[p][np.ix_(free, free)], ref, rtol=1e-12, atol=1e-15 * np.abs(ref).max())
        assert not L[1][fixed, :].any() and not L[1][:, fixed].any()   # a fixed parameter: zero row and column
    # the fallback: an indefinite matrix, a NaN, an infinite pivot, a NaN scale - and a good neighbour keeps its factor
    cov = np.stack([random_spd(rng, 13) for _ in range(5)])
    cov[0][3, 3] = -1.0
    cov[1][5, 2] = cov[1][2, 5] = np.nan
    cov[2] = np.ones((13, 13))                                         # rank one: the second pivot is 0
    cov[3][0, 0] = np.inf
    fb = rng.uniform(0.01, 0.1, 13)
    L, flag = cov_factor_reference(cov, 1.0, fb)
    assert flag.tolist() == [1, 1, 1, 1, 0]
    for p in range(4):
        assert np.array_equal(L[p], np.diag(fb))
    assert np.allclose(L[4], np.linalg.cholesky(cov[4]), rtol=1e-12)
    assert cov_factor_reference(cov[4:], np.nan, fb)[1].tolist() == [1]


# ------------------------------------------------------------------------------------------------------ the interface
def _cpu_sampler(isgood=None, **kw):
    m = _cpu_model()
    P = len(settings.MCMC_PERIODS)
    return MetropolisBatch(m.spec, m.to_model, settings.MCMC_PERIODS, np.full(P, 3.5), np.full(P, 0.05), device="cpu", isgood=isgood, **kw)


def test_set_proposal_shapes_and_refusals():
    mc = _cpu_sampler()
    N = mc.spec.n
    eye = torch.eye(N, dtype=torch.float64)
    assert mc._given is None and not mc.proposal().redraws_in_kernel
    mc.set_proposal(None)                                              # always allowed: the reference's proposal
    for bad in (eye.float(), eye[:, :5], torch.zeros(2, 3, N, N, dtype=torch.float64), torch.zeros(4, N + 1, N + 1, dtype=torch.float64),
                np.eye(N)):
        with pytest.raises(ValueError, match="float64 tensor"):
            mc.set_proposal(bad)
    with pytest.raises(ValueError, match="chains_per_point"):
        mc.set_proposal(eye, 0)
    with pytest.raises(ValueError, match="fused"):                     # no HIP device: no fused path
        mc.set_proposal(eye)
    with pytest.raises(ValueError, match="callback"):
        _cpu_sampler(isgood=lambda p: torch.ones(p.shape[0], dtype=torch.bool)).set_proposal(eye)
    rules = PriorRules(_cpu_model())
    with pytest.raises(ValueError, match="local_rows"):
        _cpu_sampler(isgood=rules, local_rows=np.zeros(4, np.int64)).set_proposal(eye)
    assert mc._given is None
    # the switches, asked without a device
    mc2 = _cpu_sampler(isgood=rules)
    mc2._given = Factor(mc2.proposer, rules, mc2._exh, torch.zeros(1, N, N, dtype=torch.float64), 1)
    assert mc2.proposal().redraws_in_kernel and type(mc2.proposal()) is Factor
    assert mc2.auto_spec_depth(100) == 4 and mc2.auto_spec_depth(5000) == 1    # like redraw="kernel"
    mc2._given = None
    assert mc2.auto_spec_depth(100) == 1


def test_proposal_in_force():
    """Class and deepest tree of the proposal in force for every way of setting one; the off switches return to the earlier answer."""
    m = _cpu_model()
    N = m.spec.n
    ft = torch.zeros(3, N, N, dtype=torch.float64)
    rounds, kernel = PriorRules(m), PriorRules(m, redraw="kernel")
    for isgood, cls, deepest in ((None, ReferenceSteps, 4), (rounds, ReferenceSteps, 1), (kernel, KernelRedraw, 4)):
        mc = _cpu_sampler(isgood=isgood)
        first = mc.proposal()
        assert type(first) is cls and first.max_depth == deepest and first.redraws_in_kernel == (cls is KernelRedraw)
        assert first.isgood is isgood and mc.proposal() is first
        mc._given = Factor(mc.proposer, isgood, mc._exh, ft, 4)            # (set_proposal itself needs a device)
        pr = mc.proposal()
        assert pr is mc._given and pr.max_depth == 4 and pr.redraws_in_kernel and pr.isgood is isgood and (pr.F, pr.cpf) == (3, 4)
        mc.set_proposal(None)
        assert mc.proposal() is first
        mc.set_adaptive(None)
        assert mc.proposal() is first
    # isgood is assignable after construction: the proposal follows it
    mc = _cpu_sampler()
    assert mc.proposal().max_depth == 4 and mc.auto_spec_depth(100) == 4
    mc.isgood = rounds
    assert type(mc.proposal()) is ReferenceSteps and mc.proposal().max_depth == 1 and mc.auto_spec_depth(100) == 1
    mc.isgood = kernel
    assert type(mc.proposal()) is KernelRedraw and mc.proposal().isgood is kernel and mc.auto_spec_depth(100) == 4
    with pytest.raises(ValueError, match="spec_depth"):
        _cpu_sampler(isgood=rounds)._check_depth(2)
    with pytest.raises(ValueError, match="at most 4"):
        _cpu_sampler()._check_depth(5)


def test_rules_descriptor_is_marshalled_once():
    """proposal.rules_args: the tensors of native_descriptor() / device_flags() by identity, vs_max = -1.0 for None.  The model of
    this file has no per-point constants (K = 0): no aux columns."""
    m = _cpu_model()
    assert m.n_aux == 0
    p = torch.as_tensor(np.array(_starts(4.5, 5)))
    idesc, fdesc, L = m.native_descriptor()
    for vs_max in (None, 4.5):
        rules = PriorRules(m, vs_max=vs_max)
        K, Lout, aux, i2, f2, flags, cap = rules_args(rules, p)
        assert (K, Lout, aux) == (0, int(L), None) and i2 is idesc and f2 is fdesc and flags is rules.device_flags()
        assert cap == (-1.0 if vs_max is None else 4.5) and isinstance(cap, float)


def test_run_start_refusals():
    rules = PriorRules(_cpu_model(), vs_max=4.5)
    mc = _cpu_sampler(isgood=rules, forward=lambda *a: pytest.fail("nothing may be evaluated"))
    spec = mc.spec
    good = torch.as_tensor(np.array(_starts(4.5, 4)))
    for bad in (good[:3], good.float(), good.numpy(), good[:, :5]):
        with pytest.raises(ValueError, match="start"):
            mc.run(4, 3, start=bad)
    out = good.clone(); out[2, 1] = spec.vmax[1]                       # on the wall: the box is open
    with pytest.raises(ValueError, match="outside the open prior box"):
        mc.run(4, 3, start=out)
    broken = torch.as_tensor(np.array(_starts(4.9, 64)))
    broken = broken[~rules(broken)][:4]
    assert broken.shape[0] == 4
    with pytest.raises(ValueError, match="break the prior's rules"):
        mc.run(4, 3, start=broken)
    with pytest.raises(ValueError, match="start"):
        mc.run_points(2, 2, 3, start=good[:3])
    with pytest.raises(ValueError, match="outside the open prior box"):
        mc.run_points(2, 2, 3, start=out[2:4])                         # [n_points, N]: chain 0 of point 0 would start on the wall
    with pytest.raises(ValueError, match="break the prior's rules"):
        mc.run_points(2, 2, 3, start=broken.reshape(2, 2, -1))


def test_laplace_proposal_refuses_a_thermal_model():
    from pysurfinv_amd import grid
    from pysurfinv_amd.point import Point
    mb = Model1DBatch(settings.C5_SETTING, device="cpu")
    P = len(settings.MCMC_PERIODS)
    obs = np.full((3, P), 3.8)
    with pytest.raises(ValueError, match="thermal"):
        grid.run_grid(mb, np.arange(3.0), np.zeros(3), settings.MCMC_PERIODS, obs, 0.01 * obs, 2, 3, device="cpu", proposal="laplace",
                      forward=lambda *a: pytest.fail("nothing may be evaluated"))
    with pytest.raises(ValueError, match="proposal"):
        grid.run_grid(mb, np.arange(3.0), np.zeros(3), settings.MCMC_PERIODS, obs, 0.01 * obs, 2, 3, device="cpu", proposal="bogus")
    pt = Point(settings.C5_SETTING, periods=settings.MCMC_PERIODS, vels=[3.8] * P, uncers=[0.04] * P, device="cpu")
    with pytest.raises(ValueError, match="thermal"):
        pt.MCinvMP(outdir="unused", runN=4, chainL=2, proposal="laplace")
    with pytest.raises(ValueError, match="proposal"):
        pt.MCinvMP(outdir="unused", runN=4, chainL=2, proposal="bogus")


# ------------------------------------------------------------------------------------------------------ the entries' argument checks
def _cov_args(**over):
    """The arguments of one call of the propose entry on host dummies (never dereferenced: every call below is rejected on the host)."""
    buf = (ctypes.c_double * 8)()
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    a = dict(stream=None, C=4, N=13, K=0, L=96, depth=2, p=ptr, aux=None, vmin=ptr, vmax=ptr, factor_t=ptr, cpf=2, F=2, idesc=ptr, fdesc=ptr,
             flags=ptr, vs_max=ctypes.c_double(4.5), G=1000, U=10000, seed=1, counter=1, chain0=0, out=ptr, tries=ptr, exhausted=ptr)
    a.update(over)
    a["_keep"] = buf
    return a


def test_entries_reject_bad_arguments_before_any_device_call():
    from pysurfinv_amd import _lib
    L = _lib.lib()
    order = ("stream", "C", "N", "K", "L", "depth", "p", "aux", "vmin", "vmax", "factor_t", "cpf", "F", "idesc", "fdesc", "flags", "vs_max",
             "G", "U", "seed", "counter", "chain0", "out", "tries", "exhausted")
    some = _cov_args()["p"]
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "surfdisp.h")).read()
    assert "#define SURFDISP_MCMC_COV_N_MAX 64\n" in hdr and mcmc.COV_MAX_N == 64
    norules = dict(flags=None, idesc=None, fdesc=None, K=0, L=0)
    bad = [dict(depth=0), dict(depth=5), dict(C=0), dict(N=0), dict(N=65), dict(K=-1), dict(L=0), dict(L=_lib.NLAY_MAX + 1),
           dict(G=0, U=0), dict(G=16384, U=1), dict(G=1, U=16384), dict(G=-1, U=5), dict(G=5, U=-1),
           dict(N=16, C=1, chain0=2 ** 44 - 1, cpf=2 ** 44, F=1), dict(chain0=-1),
           dict(cpf=0), dict(cpf=-3), dict(F=0), dict(C=4, cpf=2, F=1), dict(C=5, cpf=2, F=2), dict(chain0=4, cpf=2, F=2),
           dict(K=2, aux=None), dict(K=250, aux=some), dict(idesc=None), dict(fdesc=None),
           dict(out=None), dict(p=None), dict(vmin=None), dict(vmax=None), dict(factor_t=None), dict(exhausted=None),
           # without flags there are no rules: every descriptor argument must be absent
           dict(norules, L=96), dict(norules, K=1), dict(norules, idesc=some), dict(norules, fdesc=some), dict(norules, aux=some),
           dict(norules, N=65), dict(norules, F=1)]
    for over in bad:
        a = _cov_args(**over)
        rc = L.surfdisp_mcmc_propose_cov_device(*[a[k] for k in order])
        assert rc == _lib.ERR_INVALID, (over, rc)
        assert b"surfdisp_mcmc_propose_cov_device" in L.surfdisp_last_error(), over
    for over in (dict(P=0), dict(N=0), dict(N=65), dict(cov=None), dict(fb=None), dict(factor_t=None), dict(flag=None)):
        a = dict(P=3, N=13, cov=some, fb=some, factor_t=some, flag=some)
        a.update(over)
        rc = L.surfdisp_mcmc_cov_factor_device(None, a["P"], a["N"], a["cov"], ctypes.c_double(1.0), a["fb"], a["factor_t"], a["flag"])
        assert rc == _lib.ERR_INVALID, (over, rc)
        assert b"surfdisp_mcmc_cov_factor_device" in L.surfdisp_last_error(), over
