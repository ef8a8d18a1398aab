"""The prior's redraw loop inside the propose kernel (csrc/surfdisp_mcmc_prior.hip, surfdisp_mcmc_propose_prior_device;
``PriorRules(redraw="kernel")``) against an exact host replay (tests/mcmc_prior_replay.py, built on tests/mcmc_replay.py).

CPU: the ``PriorRules`` interface, the counter layout of the retry index, the replay's own semantics, the entry's argument
checks (invalid calls only: nothing launches), ``Point.MCinvMP`` raising on an exhausted prior.
GPU: with rules that accept everything the entry writes the bits of the plain and the tree entries; with a tight prior every
(chain, node) takes the replay's retry and value; the uniform phase; exhaustion (reported, not looped on); chain groups; the
sampler end to end against the torch loop.

Model: MCMC_SETTING (N = 13 scalars, K = 0, L = 96 output layers: more than one pass of the 64 lanes over the layers).  Start
states: uniform prior draws that satisfy the rules.
  tight          vs_max = 4.5, step x 4, G = 1000, U = 10000: about 58 % of the first Gaussian tries are good, a mean of one
                 retry, the worst chain of 3 000 needed 25 - the loop is exercised 40 x below its caps.
  uniform phase  vs_max = 4.9, step x 4, G = 1, U = 64: 22 % of the chains reach the uniform draws, 40 % of which are good, so a
                 node exhausts its 64 with probability 0.6^64 = 6e-15.
Marginal entries - a compared scalar within the replay's bounds margin (margin < 1) or a rule inequality within 1e-9
(mcmc_prior_replay.SLACK_BAND) - are left out of value and decision comparisons and counted: at most 0.5 % in any test."""
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
from test_mcmc_replay import SEEDS, _bits, _dev, _ptr, _states   # noqa: E402

from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402
from pysurfinv_amd.mcmc import MetropolisBatch, PriorRules   # noqa: E402
from pysurfinv_amd.settings import MCMC_PERIODS, MCMC_SETTING   # noqa: E402

ACCEPT_ALL = dict(monotone_groups=(), positive_jumps=False, vs_max=None)
TIGHT = dict(kw=dict(vs_max=4.5), step=4.0, G=1000, U=10000)
UNIFORM = dict(kw=dict(vs_max=4.9), step=4.0, G=1, U=64)
CHAIN0_BIG = 2 ** 33 // 13 + 3                                          # element indices beyond 2^32
MAX_EXCLUDED = 0.005


@functools.lru_cache(maxsize=None)
def _cpu_model():
    return Model1DBatch(MCMC_SETTING)


@functools.lru_cache(maxsize=None)
def _starts(vs_max, C):
    """C good start states of the rules with this cap: computed once, shared, never written to."""
    m = _cpu_model()
    p = PR.good_starts(PriorRules(m, vs_max=vs_max), m.spec, C, seed=7)
    p.setflags(write=False)
    return p


# =================================================================================================================== CPU
def test_prior_rules_interface():
    m = _cpu_model()
    r = PriorRules(m)
    assert r.redraw == "rounds" and (r.gauss_tries, r.uniform_tries) == (1000, 10000) and (r.rounds, r.reset_rounds) == (5, 2)
    k = PriorRules(m, redraw="kernel", gauss_tries=3, uniform_tries=4)
    assert k.redraw == "kernel" and (k.gauss_tries, k.uniform_tries) == (3, 4)
    with pytest.raises(ValueError):
        PriorRules(m, redraw="bogus")
    for g, u in ((0, 0), (16384, 1), (1, 16384), (-1, 5), (5, -1)):
        with pytest.raises(ValueError):
            PriorRules(m, gauss_tries=g, uniform_tries=u)
    assert PriorRules(m, gauss_tries=0, uniform_tries=16384).uniform_tries == 16384
    assert PriorRules(m, gauss_tries=1, uniform_tries=0).gauss_tries == 1
    # the sampler's switches: no device needed to ask
    P = len(MCMC_PERIODS)
    mc = MetropolisBatch(m.spec, m.to_model, MCMC_PERIODS, np.full(P, 3.5), np.full(P, 0.05), device="cpu", isgood=k)
    assert mc.proposal().redraws_in_kernel and mc.proposal().isgood is k and mc.prior_exhausted() == 0
    mc.isgood = r
    assert not mc.proposal().redraws_in_kernel and mc.proposal().isgood is r


def test_retry_counter_layout():
    """(word 1 tag, high half of word 3) of every draw of the new kernel - nodes 0..14, Gaussian tries 0..499 and the uniform
    word, retry r in {0, 1, 999, 1000, 10999, 16383} - for the extreme stream indices below 2^48: pairwise distinct, distinct
    from the masked-redraw nodes 64..98 and the accept words (whose word 3 carries no retry), and (gidx, r) is recovered from
    words 2, 3.  At r = 0 they are mcmc_replay's tag_try / tag_fallback on the unshifted index."""
    retries = (0, 1, 999, 1000, 10999, 16383)
    tags = [R.tag_try(k, t) for k in range(15) for t in range(R.MAX_CALLS)] + [R.tag_fallback(k) for k in range(15)]
    assert len(set(tags)) == 15 * 501
    other = [R.tag_try(k, t) for k in range(64, 99) for t in range(R.MAX_CALLS)] + [R.tag_fallback(k) for k in range(64, 99)] \
        + [R.tag_accept(s) for s in range(4)]
    assert not set(tags) & set(other)                                  # word 1 alone separates the kernel from those streams
    for gidx in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 48 - 1):
        seen = set()
        for r in retries:
            idx = gidx + (r << 48)
            assert idx < 2 ** 62                                       # a positive long
            w2, w3 = idx & 0xffffffff, idx >> 32
            assert (w3 >> 16, ((w3 & 0xffff) << 32) | w2) == (r, gidx)     # bits 16..29 of word 3: the retry, nothing else
            seen |= {(t, w3) for t in tags}
        assert len(seen) == len(retries) * len(tags)
        assert not {(t, gidx >> 32) for t in other} & seen
    C, N, chain0 = 3, 13, CHAIN0_BIG
    assert np.array_equal(PR.retry_index(C, N, chain0, 0), R._grid(C, N, chain0))
    assert np.array_equal(PR.retry_index(C, N, chain0, 5) - R._grid(C, N, chain0), np.full((C, N), 5 << 48, np.uint64))
    with pytest.raises(AssertionError):
        PR.retry_index(1, 16, 2 ** 44 - 1, 0)                          # (chain0 + C) N = 2^48
    # one draw, spelled out: retry 0 of the replay's candidate is mcmc_replay.propose's draw
    m = _cpu_model()
    p = _states(np.random.default_rng(5), C, m.spec)
    a = PR.candidate(p, m.spec.vmin, m.spec.vmax, m.spec.step, SEEDS[1], 9, 3, 0, 1000, PR.retry_index(C, N, chain0, 0))[0]
    b = R.propose(p, m.spec.vmin, m.spec.vmax, m.spec.step, SEEDS[1], 9, False, chain0, node=3)[0]
    c = PR.candidate(p, m.spec.vmin, m.spec.vmax, m.spec.step, SEEDS[1], 9, 3, 1, 1000, PR.retry_index(C, N, chain0, 1))[0]
    assert np.array_equal(_bits(a), _bits(b)) and (a != c).all()


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_replay_with_rules_that_accept_everything_is_the_tree_replay(depth):
    m = _cpu_model()
    spec = m.spec
    p = _states(np.random.default_rng(3), 9, spec)
    rules = PriorRules(m, **ACCEPT_ALL)
    out, tries, margin, tol, slack = PR.propose_prior(p, None, spec.vmin, spec.vmax, spec.step, rules, SEEDS[1], 2 ** 32 + 3, depth, 1000, 10000, 977)
    ref, rm, rt, _ = R.propose_tree(p, spec.vmin, spec.vmax, spec.step, SEEDS[1], 2 ** 32 + 3, depth, 977)
    assert np.array_equal(_bits(out), _bits(ref)) and (tries == 0).all()
    assert np.array_equal(margin, rm.min(axis=2)) and np.array_equal(tol, rt) and np.isinf(slack).all()


def test_replay_in_the_tight_configuration():
    """C = 200, depth 2: every row satisfies the rules; a row found at retry 0 is propose_tree's row (drawn from the same state);
    the caps are far away; the loop is exercised."""
    m = _cpu_model()
    spec = m.spec
    rules = PriorRules(m, **TIGHT["kw"])
    p = np.array(_starts(4.5, 200))
    assert rules(torch.as_tensor(p)).all()
    step = spec.step * TIGHT["step"]
    out, tries, margin, tol, slack = PR.propose_prior(p, None, spec.vmin, spec.vmax, step, rules, SEEDS[0], 5, 2, TIGHT["G"], TIGHT["U"])
    assert rules(torch.as_tensor(out.reshape(-1, spec.n))).all()
    assert tries.max() < 1000 and 0.2 < (tries >= 1).mean() < 0.8
    ref = R.propose_tree(p, spec.vmin, spec.vmax, step, SEEDS[0], 5, 2, given=out)[0]
    first = tries == 0
    assert first.sum() > 100 and np.array_equal(_bits(out[first]), _bits(ref[first]))
    assert not np.array_equal(out[~first], ref[~first])
    n_marg = int(PR.marginal(margin, slack).sum())
    print(f"tight replay: mean retries {tries.mean():.2f}, worst {tries.max()}, {n_marg} of {tries.size} marginal, smallest slack {slack.min():.2e}")
    assert n_marg <= MAX_EXCLUDED * tries.size


def _entry_args(**over):
    """The arguments of one call of the entry on host dummies (never dereferenced: the calls below are all rejected on the host)."""
    buf = (ctypes.c_double * 8)()
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    a = dict(stream=None, C=4, N=13, K=0, L=96, depth=2, p=ptr, aux=None, vmin=ptr, vmax=ptr, step=ptr, idesc=ptr, fdesc=ptr, flags=ptr,
             vs_max=ctypes.c_double(4.5), G=1000, U=10000, seed=1, counter=1, chain0=0, out=ptr, tries=ptr, exhausted=ptr)
    a.update(over)
    a["_keep"] = buf
    return a


def test_entry_rejects_bad_arguments_before_any_device_call():
    from pysurfinv_amd import _lib
    L = _lib.lib()
    order = ("stream", "C", "N", "K", "L", "depth", "p", "aux", "vmin", "vmax", "step", "idesc", "fdesc", "flags", "vs_max", "G", "U",
             "seed", "counter", "chain0", "out", "tries", "exhausted")
    some = _entry_args()["p"]
    ROW = 256                                                           # SURFDISP_MCMC_PRIOR_ROW_MAX of include/surfdisp.h
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "surfdisp.h")).read()
    assert f"#define SURFDISP_MCMC_PRIOR_ROW_MAX {ROW}\n" in hdr and "#define SURFDISP_MCMC_PRIOR_TRIES_MAX 16384\n" in hdr
    bad = [dict(depth=0), dict(depth=5), dict(G=0, U=0), dict(G=16384, U=1), dict(G=1, U=16384), dict(G=-1, U=5), dict(G=5, U=-1),
           dict(N=16, C=1, chain0=2 ** 44 - 1), dict(chain0=-1), dict(N=13, K=ROW + 1 - 13, aux=some), dict(N=ROW + 1),
           dict(K=2, aux=None), dict(out=None), dict(p=None), dict(exhausted=None), dict(flags=None), dict(C=0), dict(N=0), dict(K=-1),
           dict(L=0), dict(L=_lib.NLAY_MAX + 1)]
    for over in bad:
        a = _entry_args(**over)
        rc = L.surfdisp_mcmc_propose_prior_device(*[a[k] for k in order])
        assert rc == _lib.ERR_INVALID, (over, rc)
        assert b"surfdisp_mcmc_propose_prior_device" in L.surfdisp_last_error(), over


def test_point_raises_when_the_prior_was_exhausted(monkeypatch, tmp_path):
    """``Point.MCinvMP`` reads ``prior_exhausted()`` after the run and raises as the reference does (models.py:219); nothing is
    written.  (The sampler is stubbed: a prior no model passes cannot produce start states either, so the real run never starts.)"""
    from pysurfinv_amd.point import Point
    N = _cpu_model().spec.n
    monkeypatch.setattr(MetropolisBatch, "run", lambda self, C, chainL, **kw: torch.zeros((C, chainL, 3 + N), dtype=torch.float64))
    pt = Point(MCMC_SETTING, periods=MCMC_PERIODS, vels=[3.5] * len(MCMC_PERIODS), uncers=[0.05] * len(MCMC_PERIODS), device="cpu")
    monkeypatch.setattr(MetropolisBatch, "prior_exhausted", lambda self: 5)
    with pytest.raises(RuntimeError, match="good model"):
        pt.MCinvMP(outdir=str(tmp_path / "mc"), runN=4, chainL=2)
    assert not (tmp_path / "mc").exists()
    monkeypatch.setattr(MetropolisBatch, "prior_exhausted", lambda self: 0)
    assert pt.MCinvMP(outdir=str(tmp_path / "mc"), runN=4, chainL=2).shape == (4, 3 + N)


# =================================================================================================================== GPU
@functools.lru_cache(maxsize=None)
def _gpu_model():
    return Model1DBatch(MCMC_SETTING, device=torch.device("cuda:0"))


def _call_prior(p, rules_kw, step, seed, counter, depth, G, U, chain0, exhausted=None, mb=None, aux=None):
    """One call of the entry on the states p (numpy [C, N]) -> (out [C, M, N], tries [C, M], the exhausted counter after it).
    mb: the model on the device (default: MCMC_SETTING's); aux: its per-chain constants, numpy [C, K]."""
    from pysurfinv_amd import _lib
    mb = _gpu_model() if mb is None else mb
    rules = PriorRules(mb, **rules_kw)
    idesc, fdesc, L = mb.native_descriptor()
    C, N = p.shape
    M = (1 << depth) - 1
    dp, lo, hi, st = _dev(p), _dev(mb.spec.vmin), _dev(mb.spec.vmax), _dev(step)
    K = 0 if aux is None else int(aux.shape[1])
    daux = None if aux is None else _dev(np.ascontiguousarray(aux, np.float64))
    out = torch.full((C, M, N), float("nan"), dtype=torch.float64, device="cuda:0")
    tries = torch.full((C, M), -1, dtype=torch.int16, device="cuda:0").view(torch.uint16)       # (65535: never a valid count)
    exh = torch.zeros(1, dtype=torch.int32, device="cuda:0") if exhausted is None else exhausted
    _lib.check(_lib.lib().surfdisp_mcmc_propose_prior_device(
        None, C, N, K, int(L), depth, _ptr(dp), _ptr(daux), _ptr(lo), _ptr(hi), _ptr(st), _ptr(idesc), _ptr(fdesc), _ptr(rules.device_flags()),
        ctypes.c_double(-1.0 if rules.vs_max is None else rules.vs_max), G, U, seed, counter, chain0, _ptr(out), _ptr(tries), _ptr(exh)))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tries.cpu().view(torch.int16).numpy().view(np.uint16).astype(np.int64), int(exh.item())


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 5, 67])
def test_accept_all_rules_give_the_plain_and_the_tree_entries_bits(C):
    from pysurfinv_amd import _lib
    mb = _gpu_model()
    spec, N = mb.spec, mb.spec.n
    p = _states(np.random.default_rng(3), C, spec)
    dp, lo, hi, st = _dev(p), _dev(spec.vmin), _dev(spec.vmax), _dev(spec.step)
    L = _lib.lib()
    for depth in (1, 2, 3, 4):
        M = (1 << depth) - 1
        for chain0 in (0, CHAIN0_BIG):
            for seed in SEEDS:
                counter = 2 ** 32 + 3 if seed == SEEDS[1] else 7
                out, tries, exh = _call_prior(p, ACCEPT_ALL, spec.step, seed, counter, depth, 1000, 10000, chain0)
                tree = torch.full((C, M, N), float("nan"), dtype=torch.float64, device="cuda:0")
                _lib.check(L.surfdisp_mcmc_propose_tree_device(None, C, N, depth, _ptr(dp), _ptr(lo), _ptr(hi), _ptr(st), seed, counter,
                                                               _ptr(tree), chain0))
                torch.cuda.synchronize()
                what = (C, depth, chain0, seed)
                assert np.array_equal(_bits(out), _bits(tree.cpu().numpy())), what
                assert (tries == 0).all() and exh == 0, what
                if depth == 1:
                    one = torch.full((C, N), float("nan"), dtype=torch.float64, device="cuda:0")
                    _lib.check(L.surfdisp_mcmc_propose_device(None, C, N, _ptr(dp), _ptr(lo), _ptr(hi), _ptr(st), seed, counter, 0, _ptr(one), chain0))
                    torch.cuda.synchronize()
                    assert np.array_equal(_bits(out[:, 0]), _bits(one.cpu().numpy())), what


def _against_replay(cfg, vs_max, C, depth, chain0, seed, counter, min_retried, what, model=None):
    """One device call in configuration `cfg` against the replay on the device's own tree: tries and values of every non-marginal
    (chain, node).  The replay's tries is its FIRST good retry, so equal tries say that every earlier retry is bad in the replay and
    the chosen one good.  Returns (dev out, dev tries, replay out, replay tol, keep).
    model: None (MCMC_SETTING, start states good under the cap `vs_max`), or (the model on the CPU, the same on the device, the
    local-info row of each chain or None); the start states are then good under the rules of `cfg` themselves."""
    if model is None:
        m, mb, rows, aux = _cpu_model(), None, None, None
        p = np.array(_starts(vs_max, C))
    else:
        m, mb, rows = model
        aux = None if rows is None else m._aux.numpy()[np.asarray(rows)]
        p = PR.good_starts(PriorRules(m, **cfg["kw"]), m.spec, C, seed=7, rows=rows)
    spec = m.spec
    step = spec.step * cfg["step"]
    out, tries, exh = _call_prior(p, cfg["kw"], step, seed, counter, depth, cfg["G"], cfg["U"], chain0, mb=mb, aux=aux)
    rules = PriorRules(m, **cfg["kw"])
    ref, rtries, margin, tol, slack = PR.propose_prior(p, aux, spec.vmin, spec.vmax, step, rules, seed, counter, depth, cfg["G"], cfg["U"],
                                                       chain0, given=out, rows=rows)
    keep = ~PR.marginal(margin, slack)
    excluded = int((~keep).sum())
    err = np.abs(out - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    worst = float(rel[keep].max())
    retried = float((tries >= 1).mean())
    print(f"{what}: worst difference {worst:.4f} of the bound, {excluded} of {keep.size} (chain, node) excluded as marginal, "
          f"{retried:.3f} retried, most tries {tries.max()}, smallest slack {slack.min():.2e}, exhausted {exh}")
    assert exh == 0, what
    assert excluded <= MAX_EXCLUDED * keep.size, what
    assert np.array_equal(tries[keep], rtries[keep]), what
    assert worst <= 1.0, what
    M = out.shape[1]
    assert bool(rules(torch.as_tensor(out.reshape(-1, spec.n)), rows=None if rows is None else np.repeat(np.asarray(rows), M)).all()), what
    assert retried >= min_retried, what
    return out, tries, ref, tol, keep


@pytest.mark.gpu
@pytest.mark.parametrize("depth,chain0", [(1, 0), (1, CHAIN0_BIG), (4, 0), (4, CHAIN0_BIG)])
def test_retry_loop_is_the_replay_in_the_tight_configuration(depth, chain0):
    out, tries, *_ = _against_replay(TIGHT, 4.5, 67, depth, chain0, SEEDS[depth > 1], 2 ** 32 + 3 if chain0 else 11, 0.20,
                                     f"tight depth {depth} chain0 {chain0}")
    assert tries.max() < TIGHT["G"]                                    # the Gaussian phase alone: the caps are far away
    spec = _cpu_model().spec
    assert ((out > spec.vmin) & (out < spec.vmax)).all()


@pytest.mark.gpu
def test_uniform_phase_is_the_replay():
    out, tries, ref, tol, keep = _against_replay(UNIFORM, 4.9, 67, 2, CHAIN0_BIG, SEEDS[1], 13, 0.05, "uniform phase depth 2")
    spec = _cpu_model().spec
    uni = tries >= 1                                                   # G = 1: every retry is a uniform draw
    ut = np.broadcast_to(R.uniform_tolerance(spec.vmin, spec.vmax), out.shape)
    assert np.array_equal(tol[uni], ut[uni])
    sel = uni & keep
    assert (np.abs(out - ref)[sel] <= ut[sel]).all()
    assert tries.max() < 1 + UNIFORM["U"]


@pytest.mark.gpu
def test_exhaustion_is_reported_and_not_looped_on():
    """vs_max = 0.5: no model passes.  Every node stops at G + U = 7 tries, proposes the state it drew from bit for bit - so every
    node of a chain's tree is the chain's state - and the counter grows by C x nodes; a second call adds to it."""
    C, depth = 5, 2
    spec = _cpu_model().spec
    p = np.array(_starts(4.9, C))
    exh = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    out, tries, n = _call_prior(p, dict(vs_max=0.5), spec.step, SEEDS[0], 3, depth, 3, 4, 0, exhausted=exh)
    assert (tries == 7).all() and n == 5 * 3
    assert np.array_equal(_bits(out), _bits(np.repeat(p[:, None, :], 3, axis=1)))
    assert _call_prior(p, dict(vs_max=0.5), spec.step, SEEDS[0], 4, 1, 3, 4, 0, exhausted=exh)[2] == 5 * 3 + 5
    # the sampler: three lock steps from good states under a prior that then rejects everything
    from pysurfinv_amd.settings import synthetic_observations
    dev = torch.device("cuda:0")
    mb, c_obs, unc = synthetic_observations(1, dev, seed=100)
    rules = PriorRules(mb, vs_max=0.5, redraw="kernel", gauss_tries=3, uniform_tries=4)
    mc = MetropolisBatch(mb.spec, mb.to_model, MCMC_PERIODS, c_obs[0], unc[0], device=dev, seed=3, isgood=rules)
    assert mc.fused_available() and mc.prior_exhausted() == 0
    state = _dev(p).clone()
    for i in range(3):
        mc.fused_step(state, first=(i == 0))
    assert mc.prior_exhausted() == 2 * C                               # (the first step evaluates the states: no proposal)
    assert (mc.last_prior_tries().cpu().view(torch.int16).numpy() == 7).all()
    assert np.array_equal(_bits(state.cpu().numpy()), _bits(p))


@pytest.mark.gpu
def test_chain_groups_draw_what_one_call_draws():
    spec = _cpu_model().spec
    p = np.array(_starts(4.5, 67))
    step = spec.step * TIGHT["step"]
    for chain0 in (0, CHAIN0_BIG):
        one = _call_prior(p, TIGHT["kw"], step, SEEDS[1], 21, 1, TIGHT["G"], TIGHT["U"], chain0)
        a = _call_prior(p[:33], TIGHT["kw"], step, SEEDS[1], 21, 1, TIGHT["G"], TIGHT["U"], chain0)
        b = _call_prior(p[33:], TIGHT["kw"], step, SEEDS[1], 21, 1, TIGHT["G"], TIGHT["U"], chain0 + 33)
        assert np.array_equal(_bits(one[0]), _bits(np.concatenate([a[0], b[0]])))
        assert np.array_equal(one[1], np.concatenate([a[1], b[1]])) and (one[1] >= 1).mean() > 0.2


# ------------------------------------------------------------------------------------------------------------ the sampler
def _no_accepted_duplicate(tr):
    """No accepted row of the track proposes the state the chain was in (the rounds mode's "own state" fallback would)."""
    state = tr[:, 0, 3:]
    for i in range(1, tr.shape[1]):
        prop, acc = tr[:, i, 3:], tr[:, i, 2] > 0.5
        if bool((acc & (prop == state).all(dim=1)).any()):
            return False
        state = torch.where(acc[:, None], prop, state)
    return True


@functools.lru_cache(maxsize=None)
def _sampler_case():
    from pysurfinv_amd.settings import synthetic_observations
    dev = torch.device("cuda:0")
    mb, c_obs, unc = synthetic_observations(1, dev, seed=100)
    make = lambda rules: MetropolisBatch(mb.spec, mb.to_model, MCMC_PERIODS, c_obs[0], unc[0], device=dev, seed=3, isgood=rules)
    tr = make(PriorRules(mb, vs_max=4.9)).run(512, 40, init_first=False, fused=False)          # the torch loop: the reference's redraw
    torch.cuda.synchronize()
    return mb, make, (float(tr[:, 1:, 2].mean()), float(tr[:, -1, 0].median()))


@pytest.mark.gpu
def test_sampler_switches():
    mb, make, _ = _sampler_case()
    mc = make(PriorRules(mb, vs_max=4.9, redraw="kernel"))
    assert mc.fused_available() and mc.auto_spec_depth(100) == 4 and mc.auto_spec_depth(5000) == 1
    assert make(PriorRules(mb, vs_max=4.9)).auto_spec_depth(100) == 1
    assert mc.last_prior_tries() is None


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 3])
def test_sampler_with_the_kernel_redraw_against_the_torch_loop(d):
    """run(512, 40) at spec_depth 1 and 3: every recorded row satisfies the rules (at every node of the tree), nothing exhausted,
    and acceptance rate and final median misfit are the torch loop's within the bars tests/test_prior.py uses at this size."""
    mb, make, ref = _sampler_case()
    rules = PriorRules(mb, vs_max=4.9, redraw="kernel")
    mc = make(rules)
    tr = mc.run(512, 40, init_first=False, spec_depth=d)
    torch.cuda.synchronize()
    assert bool(rules(tr[:, :, 3:].reshape(-1, mb.spec.n)).all())
    assert mc.prior_exhausted() == 0
    t = mc.last_prior_tries()
    assert t.shape == (512, (1 << d) - 1) and t.dtype == torch.uint16
    got = (float(tr[:, 1:, 2].mean()), float(tr[:, -1, 0].median()))
    print(f"spec_depth {d}: acceptance {got[0]:.4f} (torch loop {ref[0]:.4f}), final median misfit {got[1]:.4f} ({ref[1]:.4f})")
    assert abs(got[0] - ref[0]) < 0.03, (got, ref)
    assert abs(got[1] / ref[1] - 1) < 0.15, (got, ref)
    assert _no_accepted_duplicate(tr)


@pytest.mark.gpu
def test_sampler_with_the_kernel_redraw_in_chain_groups():
    mb, make, _ = _sampler_case()
    rules = PriorRules(mb, vs_max=4.9, redraw="kernel")
    mc = make(rules)
    tr = mc.run(4096, 6, init_first=False)                             # two chain groups from 4 096 chains on
    torch.cuda.synchronize()
    assert mc._last_groups is not None and len(mc._last_groups.children) == 2
    assert bool(rules(tr[:, :, 3:].reshape(-1, mb.spec.n)).all())
    assert float((tr[:, 1:, 3:] != tr[:, :-1, 3:]).any(dim=2).float().mean()) > 0.9
    assert mc.prior_exhausted() == 0 and mc.last_prior_tries().shape == (4096, 1)
    assert _no_accepted_duplicate(tr)


@pytest.mark.gpu
def test_explicit_depth_with_the_redraw_rounds_is_refused():
    """The redraw rounds cannot follow a tree: run(spec_depth=3) under PriorRules in its default mode raises before anything is
    launched or counted (it used to take the tree kernels without any prior); the default depth runs, and every row obeys the rules."""
    mb, make, _ = _sampler_case()
    rules = PriorRules(mb, vs_max=4.9)
    mc = make(rules)
    before = (mc.n_forward, mc._counter)
    with pytest.raises(ValueError, match='spec_depth.*redraw="kernel"'):
        mc.run(16, 6, spec_depth=3)
    assert (mc.n_forward, mc._counter) == before
    tr = mc.run(16, 6)
    torch.cuda.synchronize()
    assert tr.shape == (16, 6, 3 + mb.spec.n) and mc._counter == 6
    assert bool(rules(tr[:, :, 3:].reshape(-1, mb.spec.n)).all())
