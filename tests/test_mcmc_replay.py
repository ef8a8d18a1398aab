"""The Metropolis kernels (csrc/surfdisp_mcmc.hip) against an exact host replay of their random streams (tests/mcmc_replay.py).

CPU tests: the Philox known answers, u53, the injectivity of the counter layout, and the DISTRIBUTION of the restatement
(Kolmogorov-Smirnov against the truncated normal, acceptance frequencies against exp(-d / 2), correlations), thresholds at
the 1e-6 quantile of the null distribution.  GPU tests: every proposal and every accept decision of the C entries against the
replay - values within 16 eps (|x| + s rad) (2 ulp for uniform draws), decisions, walked nodes and states exactly.  Together:
the kernel equals the restatement, and the restatement has the distribution the sampler claims.

What the replay found: on every draw compared, the kernels are the replay.  One deviation from the kernel's own comment is
known and NOT fixed here: u53 returns exactly 1.0 for the one bit pattern v = 2^53 - 1 (v + 0.5 rounds to even in double),
against its "never 0 nor 1" - log u1 = 0, a uniform draw on vmax, an accept draw above every threshold below 1.  The
restatement states the specification (that value is kept at the largest double below 1), so kernel and replay differ on
that pattern alone: probability 2^-53 per draw, no recorded trace is affected, no test here can meet it.  The fix is one
fmin in u53; it waits for the next change of the kernel sources, because the committed counter profiles are tagged with
the sources' hash (tests/test_host.py) and a source change needs a new counter pass of every bench leg.  The figure
1 - 2^-54 for the all-ones word is the exact value and no double; the test asks for the largest double below 1 and for
(v + 1/2) / 2^53 within half a spacing.

Mutations of the RESTATEMENT tried on the CPU and what rejected them (not kept as a harness):
  acceptance test without the / 2     test_accept_rule_frequency (d = 0.5, 2, 6: 183, 215 and 97 sigma off)
  M0 and M1 swapped, nine rounds       test_philox_known_answers (all three vectors)
  sincospi(u2) for sincospi(2 u2)      test_proposal_distribution (KS 0.021, 0.065, 0.034 in mid-box, one step and 0.1 step from the
                                       bound, against a threshold of 0.0060) and test_box_muller_candidates_are_uncorrelated
  u53 one bit short (>> 12)            test_u53_extremes_and_spacing
The device-only ones (the second candidate reusing cs, a node drawn from its sibling's state, the accept draw indexed by
the local chain, two draws on one counter word) change values or decisions of the GPU comparisons below, which run with
chain0 != 0, indices beyond 2^32 and every node of the trees.

Measured on an MI355X: the worst difference of a Gaussian proposal is 0.062 of the bound (about one eps of |x| + s rad, against
the threefold margin of the derivation), of a uniform draw 0.5 of its bound (one ulp); 0 elements and 0 chains excluded as
marginal in every test (the smallest |u - threshold| met was 1.2e-4)."""
import ctypes
import inspect
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from settings import CONT                            # noqa: E402
import mcmc_replay as R                              # noqa: E402

N_STAT = 200000
KS_BAR = math.sqrt(-math.log(5e-7) / (2 * N_STAT))                    # P(D > bar) = 1e-6 (two-sided, asymptotic)
SEEDS = (11, (0x9E3779B9 << 32) | 0x7F4A7C15)                          # the second: a nonzero high word


# =================================================================================================================== CPU
def test_philox_known_answers():
    """The Random123 known-answer vectors of Philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = " ".join(format(int(v), "08x") for v in R.philox4x32_10(ctr, key))
        assert got == want, (ctr, key)
    # vectorised: a batch of counters gives each counter's own answer
    batch = R.philox4x32_10(np.array([k[0] for k in kat[:1]] * 3 + [kat[1][0]], np.uint64), (0, 0))
    assert batch.shape == (4, 4) and (batch[0] == batch[2]).all() and not (batch[0] == batch[3]).all()


def test_u53_extremes_and_spacing():
    """All-zero bits: 2^-54.  All-one bits: the exact (2^53 - 1/2) / 2^53 = 1 - 2^-54 is no double and rounds to 1.0; u53 gives
    the largest double below 1.  Never 0, never 1; every value within half a spacing of the exact one; 2^-53 apart in the
    lower half, 2^-52 (v + 1/2 rounds to even) in the upper."""
    from fractions import Fraction
    ones = 0xffffffff
    assert R.u53(0, 0) == 2.0 ** -54
    top = float(R.u53(ones, ones))
    assert top < 1.0 and top == np.nextafter(1.0, 0.0)
    word = lambda v: ((v << 11) >> 32, (v << 11) & ones)               # the two words whose top 53 bits are v
    vs = [0, 1, 2, 3, 12345, 2 ** 52 - 2, 2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1, 2 ** 52 + 2, 2 ** 53 - 4, 2 ** 53 - 3, 2 ** 53 - 2, 2 ** 53 - 1]
    for v in vs:
        a, b = word(v)
        u = float(R.u53(a, b))
        assert 0.0 < u < 1.0
        assert abs(Fraction(u) - Fraction(2 * v + 1, 2 ** 54)) <= Fraction(1, 2 ** 54), v
        assert float(R.u53(a, b | 0x7ff)) == u                         # the low 11 bits do not count
    lower = R.u53(*np.array([word(v) for v in range(1000, 1010)], np.uint64).T)
    assert (np.diff(lower) == 2.0 ** -53).all()
    upper = np.unique(R.u53(*np.array([word(v) for v in range(2 ** 52 + 1000, 2 ** 52 + 1020)], np.uint64).T))
    assert (np.diff(upper) == 2.0 ** -52).all() and upper.size in (10, 11)


def test_counter_layout_is_injective():
    """Word 1 of every draw the kernels can make under one call counter: Gaussian tries 0..499 of the tree nodes 0..14 and of
    the masked-redraw nodes 64 + attempt (every attempt PriorRules can request, also with rounds = 32), each node's uniform
    fallback, the accept words of the steps 0..3 - all distinct, so the streams are separate although propose indexes words
    2, 3 by element and accept by chain.

    The limit, from the bit layout: the tags live in bits 8..29, and the counter's high word is XORed onto them.  Under ONE
    counter that XOR is a bijection, so the draws stay distinct for any counter; ACROSS counters with the same low word the
    pair (high word, tag) is recovered from word 1 only while the high word stays in the bits no tag uses, 0..7: counters
    below 2^40.  Counter 2^40 + L, node 0, try 0 is counter L, node 0, try 1.  MetropolisBatch counts one per lock step from 0
    and refuses a counter of 2^40 (COUNTER_LIMIT); a run cannot get there anyway - its track of 2^40 rows of at least four
    doubles for one chain alone is 32 TiB."""
    from pysurfinv_amd.mcmc import MetropolisBatch, PriorRules
    attempts = 0
    for rules in (PriorRules(None), PriorRules(None, rounds=32)):
        attempts = max(attempts, rules.rounds + rules.reset_rounds + 1)
    assert attempts == 35
    nodes = list(range(15)) + [64 + a for a in range(attempts)]
    tags = [R.tag_try(k, t) for k in nodes for t in range(R.MAX_CALLS)] + [R.tag_fallback(k) for k in nodes] + [R.tag_accept(s) for s in range(4)]
    assert len(tags) == len(nodes) * 501 + 4 and len(set(tags)) == len(tags)
    for counter in (1, 2 ** 32 - 1):                                   # "a fixed 64-bit counter below 2^32": word 1 is the tag itself
        assert {(counter >> 32) ^ t for t in tags} == set(tags)
    used = 0
    for t in tags:
        used |= t
    assert used & ~0x3fffff00 == 0                                     # bits 8..29
    limit = MetropolisBatch.COUNTER_LIMIT
    assert limit == 1 << 40
    # below the limit (counter, tag) -> (word 0, word 1) is injective: the high word fills bits 0..7 only
    assert all(((hi ^ t) & 0xff, (hi ^ t) & ~0xff) == (hi, t) for hi in (0, 1, 0xff) for t in tags[::97])
    # ... and at the limit it stops
    assert ((limit + 5) >> 32) ^ R.tag_try(0, 0) == (5 >> 32) ^ R.tag_try(0, 1) and (limit + 5) & 0xffffffff == 5
    # the sampler cannot get there: its entry point for every fused call refuses the counter before anything is launched
    mc = object.__new__(MetropolisBatch)
    mc._counter = limit - 1
    with pytest.raises(OverflowError):
        mc._fused_call(1, None, 0, None)
    with pytest.raises(OverflowError):
        mc._fused_call(1, None, 0, limit)
    src = inspect.getsource(MetropolisBatch)
    assert src.count("self._counter = 0") == 1 and "_fused_call(C, row, row_offset, counter)" in src
    rows_bytes = limit * 4 * 8
    assert rows_bytes == 32 * 2 ** 40 and rows_bytes > 288e9           # the track of such a run against the card's 288 GB


def _ks(sample, cdf):
    x = np.sort(sample)
    F = cdf(x)
    n = x.size
    return max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n))


def _truncnorm_cdf(v, x, lo, hi, s):
    try:
        from scipy.stats import truncnorm
        return truncnorm.cdf(v, (lo - x) / s, (hi - x) / s, loc=x, scale=s)
    except ImportError:
        import torch
        Phi = lambda z: 0.5 * (1 + torch.erf(torch.as_tensor(z, dtype=torch.float64) / math.sqrt(2))).numpy()
        a, b = Phi((lo - x) / s), Phi((hi - x) / s)
        return (Phi((v - x) / s) - a) / (b - a)


BOX = (0.0, 4.0, 1.0)                                                  # lo, hi, step of the distribution tests


@pytest.mark.parametrize("x", [2.0, 1.0, 0.1], ids=["mid", "one_step", "tenth_step"])
def test_proposal_distribution(x):
    """2e5 bounded steps of the restatement from a state in mid-box, one step and 0.1 step from a bound: Kolmogorov-Smirnov
    distance to the truncated normal below the 1e-6 quantile of its null distribution (0.0060).  Measured here: 0.0027, 0.0024,
    0.0023."""
    lo, hi, s = BOX
    full = np.full(N_STAT, 1.0)
    v, _, _, uni = R.draw_bounded(x * full, lo * full, hi * full, s * full, SEEDS[0], 3, 0, np.arange(N_STAT), exact=False)
    assert not uni.any() and ((v > lo) & (v < hi)).all()
    d = _ks(v, lambda t: _truncnorm_cdf(t, x, lo, hi, s))
    print(f"KS distance at x = {x}: {d:.5f} (bar {KS_BAR:.5f})")
    assert d < KS_BAR


def test_box_muller_candidates_are_uncorrelated():
    """The cos and the sin candidate of one Philox call: correlation within 5 sigma of 0 over all 2e5 first tries, and over
    the draws where BOTH are observed - the cos candidate fell outside the box of a state 0.1 step (and one step) from the
    bound; both standard normal (KS).  Measured over the second candidates: -0.15 and +0.41 sigma."""
    lo, hi, s = BOX
    z0, z1 = R.normal_pair(SEEDS[0], 3, 0, 0, np.arange(N_STAT))
    corr = lambda a, b: float(np.corrcoef(a, b)[0, 1])
    assert abs(corr(z0, z1)) < 5 / math.sqrt(N_STAT)
    Phi = lambda t: _truncnorm_cdf(t, 0.0, -40.0, 40.0, 1.0)
    assert _ks(z0, Phi) < KS_BAR and _ks(z1, Phi) < KS_BAR
    for x in (0.1, 1.0):
        out = ~((x + s * z0 > lo) & (x + s * z0 < hi))
        n = int(out.sum())
        assert n > 20000
        c = corr(z0[out], z1[out])
        print(f"x = {x}: {n} second candidates, correlation {c * math.sqrt(n):+.2f} sigma")
        assert abs(c) < 5 / math.sqrt(n)
        assert abs(z1[out].mean()) < 5 / math.sqrt(n)                  # ... and the second is centred whatever the first did


@pytest.mark.parametrize("d", [0.0, 0.5, 2.0, 6.0])
def test_accept_rule_frequency(d):
    """At chi - chi0 = d the restatement accepts exp(-d / 2) of 2e5 chains, within 5 sigma of the binomial (d = 0: all).
    Measured: 1.15, 0.83 and 0.04 sigma."""
    C = N_STAT
    chi0 = np.full(C, 3.0)
    chi = chi0[:, None] + d
    w = R.accept_walk(chi, chi, chi, np.ones((C, 1, 1)), np.zeros((C, 1)), chi0, SEEDS[0], 5, chain0=0)
    f, p = w["rows"][:, 0, 2].mean(), math.exp(-d / 2)
    sigma = math.sqrt(p * (1 - p) / C)
    print(f"d = {d}: accepted {f:.5f}, exp(-d/2) = {p:.5f}, {abs(f - p) / sigma if sigma else 0:.2f} sigma")
    assert abs(f - p) <= 5 * sigma
    assert np.array_equal(w["rows"][:, 0, 2] > 0.5, w["p0"][:, 0] == 1.0)


def test_accept_draw_is_uncorrelated_with_the_proposal():
    """N = 1: element index and chain index coincide, so the proposal and the accept draw of a chain differ in word 1 alone.
    The accept uniform against the same chain's first Gaussian candidates, the fallback uniform and the next step's accept
    draw: every correlation within 5 sigma of 0; the accept uniform is uniform (KS).  The restatement passes with room."""
    g = np.arange(N_STAT)
    u = R.accept_uniform(SEEDS[0], 3, 0, g)
    assert _ks(u, lambda t: t) < KS_BAR
    z0, z1 = R.normal_pair(SEEDS[0], 3, 0, 0, g)
    r = R._words(SEEDS[0], 3, R.tag_fallback(0), g)
    others = [z0, z1, R.u53(r[:, 0], r[:, 1]), R.accept_uniform(SEEDS[0], 3, 1, g), R.accept_uniform(SEEDS[0], 4, 0, g)]
    for o in others:
        assert abs(float(np.corrcoef(u, o)[0, 1])) < 5 / math.sqrt(N_STAT)
        assert abs(float(np.corrcoef(u, np.abs(o - np.median(o)))[0, 1])) < 5 / math.sqrt(N_STAT)


# =================================================================================================================== GPU
def _spec():
    from pysurfinv_amd.layers_batch import Model1DBatch
    return Model1DBatch(CONT, device="cpu").spec


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype)), device="cuda:0")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_values(dev, ref, margin, tol, what):
    """|dev - ref| <= tol wherever the replay's margin is at least 1; at most 1e-4 of the elements excluded.  Prints and returns
    (worst difference in units of the bound, excluded)."""
    keep = margin >= 1.0
    excluded = int((~keep).sum())
    err = np.abs(dev - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    worst = float(rel[keep].max()) if keep.any() else 0.0
    print(f"{what}: worst difference {worst:.4f} of the bound, {excluded} of {keep.size} excluded as marginal")
    assert excluded <= 1e-4 * keep.size, what
    assert worst <= 1.0, what
    return worst, excluded


def _call_propose(p, lo, hi, st, seed, counter, reset, chain0):
    import torch
    from pysurfinv_amd import _lib
    out = torch.full_like(p, float("nan"))
    _lib.check(_lib.lib().surfdisp_mcmc_propose_device(None, p.shape[0], p.shape[1], _ptr(p), _ptr(lo), _ptr(hi), _ptr(st), seed, counter,
                                                       reset, _ptr(out), chain0))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _states(rng, C, spec):
    """States all over the box of CONT, every 5th chain within a few steps of a bound."""
    p = spec.vmin + (spec.vmax - spec.vmin) * rng.random((C, spec.n))
    p[::5] = (spec.vmin + spec.step * rng.random((C, spec.n)) * 0.5)[::5]
    p[2::5] = (spec.vmax - spec.step * rng.random((C, spec.n)) * 0.5)[2::5]
    return np.clip(p, spec.vmin, spec.vmax)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS, ids=["seed_lo", "seed_hi"])
def test_plain_propose_is_the_replay(seed):
    """surfdisp_mcmc_propose_device, C = 1031 (C N no multiple of 256), N = 13, CONT's bounds and steps: reset 0 and 1, chain0
    0 and 2^31 + 5 (element indices beyond 2^32), counters 1 and 2^32 + 3, a seed with and without a high word."""
    spec = _spec()
    C, N = 1031, spec.n
    assert N == 13 and (C * N) % 256 != 0
    rng = np.random.default_rng(1)
    p = _states(rng, C, spec)
    dp, lo, hi, st = _dev(p), _dev(spec.vmin), _dev(spec.vmax), _dev(spec.step)
    seen = []
    for reset in (0, 1):
        for chain0 in (0, 2 ** 31 + 5):
            for counter in (1, 2 ** 32 + 3):
                dev = _call_propose(dp, lo, hi, st, seed, counter, reset, chain0)
                ref, margin, tol, uni = R.propose(p, spec.vmin, spec.vmax, spec.step, seed, counter, bool(reset), chain0)
                assert uni.all() == bool(reset) and (reset or not uni.any())
                assert ((dev > spec.vmin) & (dev < spec.vmax)).all() or reset
                _check_values(dev, ref, margin, tol, f"propose reset={reset} chain0={chain0} counter={counter}")
                seen.append(dev)
    for i in range(len(seen)):
        for j in range(i):
            assert (seen[i] != seen[j]).mean() > 0.99                  # every (reset, chain0, counter): another stream


@pytest.mark.gpu
def test_edge_boxes_are_the_replay():
    """C = 257, N = 6, one column each: bounds 50 steps away; the state 0.1 step inside lo; the state ON lo (even chains) and
    two steps outside the box (odd chains: only redraws can succeed); a box 1e-4 step wide (nearly every element exhausts its
    1000 candidates and takes the uniform word); step 0 inside the box (the state itself); lo == hi (the uniform word: lo)."""
    C = 257
    lo = np.array([5.0, 2.0, 1.0, 4.0, 7.0, 3.5])
    hi = np.array([15.0, 6.0, 3.0, 4.0001, 8.0, 3.5])
    st = np.array([0.1, 0.5, 0.25, 1.0, 0.0, 0.2])
    rng = np.random.default_rng(2)
    p = np.tile([10.0, 2.05, 1.0, 4.00005, 7.3, 3.5], (C, 1))
    p[:, 0] += rng.standard_normal(C)
    p[1::2, 2] = 0.5
    p[:, 3] = 4.0 + 1e-4 * rng.random(C)
    dev = _call_propose(_dev(p), _dev(lo), _dev(hi), _dev(st), SEEDS[1], 9, 0, 3)
    ref, margin, tol, uni = R.propose(p, lo, hi, st, SEEDS[1], 9, False, 3)
    assert not uni[:, :3].any() and 0.8 < uni[:, 3].mean() < 1.0 and not uni[:, 4].any() and uni[:, 5].all()
    margin[:, 5] = np.inf                                              # lo == hi: no candidate can succeed, nothing to branch on
    _check_values(dev, ref, margin, tol, "edge boxes")
    assert ((dev[:, :5] > lo[:5]) & (dev[:, :5] < hi[:5])).all()
    assert np.array_equal(_bits(dev[:, 4]), _bits(p[:, 4])) and (dev[:, 5] == 3.5).all()
    assert np.abs(dev[:, 0] - p[:, 0]).std() > 0.04 and (dev[:, 2] > 1.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_tree_is_the_replay(depth):
    """surfdisp_mcmc_propose_tree_device, C = 130, N = 13: every node against the replay's draw from the state of ITS branch -
    on the device's own proposals as the children's states (bit-equal input, the plain bound) and as the replay's own tree
    (the bounds of a branch add up).  Depth 1 through the tree entry is the plain entry bit for bit."""
    import torch
    from pysurfinv_amd import _lib
    spec = _spec()
    C, N, M = 130, spec.n, (1 << depth) - 1
    p = _states(np.random.default_rng(3), C, spec)
    dp, lo, hi, st = _dev(p), _dev(spec.vmin), _dev(spec.vmax), _dev(spec.step)
    seed, counter, chain0 = SEEDS[1], 2 ** 32 + 3, 977
    L = _lib.lib()
    out = torch.full((C, M, N), float("nan"), dtype=torch.float64, device="cuda:0")
    _lib.check(L.surfdisp_mcmc_propose_tree_device(None, C, N, depth, _ptr(dp), _ptr(lo), _ptr(hi), _ptr(st), seed, counter, _ptr(out), chain0))
    one = torch.full((C, N), float("nan"), dtype=torch.float64, device="cuda:0")
    _lib.check(L.surfdisp_mcmc_propose_tree_device(None, C, N, 1, _ptr(dp), _ptr(lo), _ptr(hi), _ptr(st), seed, counter, _ptr(one), chain0))
    torch.cuda.synchronize()
    plain = _call_propose(dp, lo, hi, st, seed, counter, 0, chain0)
    assert np.array_equal(_bits(one.cpu().numpy()), _bits(plain))
    dev = out.cpu().numpy()
    assert np.array_equal(_bits(dev[:, 0]), _bits(plain))              # the root is the plain proposal too
    assert ((dev > spec.vmin) & (dev < spec.vmax)).all()
    ref, margin, tol, _ = R.propose_tree(p, spec.vmin, spec.vmax, spec.step, seed, counter, depth, chain0, given=dev)
    _check_values(dev, ref, margin, tol, f"tree depth {depth}, children from the device's states")
    ref, margin, tol, _ = R.propose_tree(p, spec.vmin, spec.vmax, spec.step, seed, counter, depth, chain0)
    _check_values(dev, ref, margin, tol, f"tree depth {depth}, the replay's own tree")


@pytest.mark.gpu
def test_masked_redraw_is_the_replay():
    """surfdisp_mcmc_propose_masked_device: modes 0, 1, 2 x attempts 0 and 6, tag 3 on every 3rd chain (other chains carry 0, 2
    or 4), `out` prefilled with a sentinel that the untagged rows keep bit for bit."""
    import torch
    from pysurfinv_amd import _lib
    spec = _spec()
    C, N = 257, spec.n
    p = _states(np.random.default_rng(4), C, spec)
    tags = np.array([3 if c % 3 == 0 else (0, 2, 4)[c % 3 if c % 2 else 0] for c in range(C)], np.uint8)
    dp, lo, hi, st, dt = _dev(p), _dev(spec.vmin), _dev(spec.vmax), _dev(spec.step), _dev(tags)
    seed, counter, chain0 = SEEDS[0], 2 ** 32 + 3, 2 ** 31 + 5
    sentinel = np.full((C, N), -777.25)
    seen = {}
    for mode in (0, 1, 2):
        for attempt in (0, 6):
            out = _dev(sentinel)
            _lib.check(_lib.lib().surfdisp_mcmc_propose_masked_device(None, C, N, _ptr(dp), _ptr(lo), _ptr(hi), _ptr(st), seed, counter,
                                                                      attempt, mode, _ptr(dt), 3, _ptr(out), chain0))
            torch.cuda.synchronize()
            dev = out.cpu().numpy()
            ref, margin, tol = R.propose_masked(p, spec.vmin, spec.vmax, spec.step, seed, counter, attempt, mode, tags, 3, sentinel, chain0)
            assert np.array_equal(_bits(dev[tags != 3]), _bits(sentinel[tags != 3]))
            if mode == 2:
                assert np.array_equal(_bits(dev), _bits(ref))
            _check_values(dev, ref, margin, tol, f"masked mode {mode} attempt {attempt}")
            seen[mode, attempt] = dev[tags == 3]
    assert (seen[0, 0] != seen[0, 6]).mean() > 0.99 and (seen[1, 0] != seen[1, 6]).mean() > 0.99
    plain = _call_propose(dp, lo, hi, st, seed, counter, 0, chain0)
    assert (seen[0, 0] != plain[tags == 3]).mean() > 0.99             # a redraw is not the step's first proposal again


# ------------------------------------------------------------------------------------------------------------ accept
P_ACC, N_ACC, C_ACC = 7, 4, 1031


def _accept_arrays(depth, per_chain, seed=5):
    """Hand-made fp32 predictions [C M, P], observations and states for which chi - chi0 spreads over about [-5, 12], with the
    planted cases: chi-squares on both sides of the clamp at 50, failed stacks (status, c < 0.01 - in a masked-out period too),
    states that had already failed (chi0 = 88888), masked periods."""
    rng = np.random.default_rng(seed)
    C, P, M = C_ACC, P_ACC, (1 << depth) - 1
    S = C * M
    obs = 3.0 + 0.1 * np.arange(P) + (0.02 * rng.standard_normal((C, P)) if per_chain else 0.0)
    unc = np.full(obs.shape, 0.05) * (1 + 0.3 * rng.random(obs.shape))
    mask = np.ones(obs.shape, np.uint8)
    if per_chain:
        mask[rng.random(obs.shape) < 0.15] = 0
        mask[:, 0] = 1
    else:
        mask[4] = 0
    target = rng.uniform(1.0, 14.0, S)
    high = rng.random(S) < 0.05
    target[high] = rng.choice([49.9, 49.9999, 50.0001, 52.0, 60.0, 200.0], int(high.sum()))
    ob = lambda a: np.repeat(a, M, axis=0) if per_chain else np.broadcast_to(a, (S, P))
    e = rng.standard_normal((S, P)) * ob(mask)
    e *= np.sqrt(target / (e * e).sum(axis=1))[:, None]
    c = (ob(obs) + ob(unc) * e).astype(np.float32)
    status = np.zeros(S, np.int32)
    status[rng.random(S) < 0.03] = 2
    low = np.flatnonzero(rng.random(S) < 0.03)
    c[low, rng.integers(0, P, low.size)] = 0.005
    c[np.setdiff1d(np.arange(S), low)[:3], 4] = 0.0                    # (period 4: masked out with shared observations)
    chi0 = rng.uniform(2.0, 7.0, C)
    hot = rng.random(C) < 0.05
    chi0[hot] = rng.uniform(48.0, 56.0, int(hot.sum()))
    chi0[rng.random(C) < 0.05] = R.FAILED
    q = rng.standard_normal((C, M, N_ACC))
    p0 = rng.standard_normal((C, N_ACC))
    obs = np.where(mask != 0, obs, np.nan)                             # a masked-out observation is never read
    return dict(c=c, status=status, obs=obs, unc=unc, mask=mask, chi0=chi0, q=q, p0=p0, M=M)


def _check_accept(dev_rows, dev_p0, dev_chi0, w, what, steps_all=True):
    """rows / state / chi-square of a device call against the replay `w`; steps whose accept draw lies within 1e-9 of its
    threshold, and the later steps of that chain, are excluded (at most 1e-4 of the chains)."""
    C, ns = w["dist"].shape
    valid = np.minimum.accumulate(w["dist"], axis=1) >= 1e-9
    bad = int((~valid.all(axis=1)).sum())
    print(f"{what}: {bad} of {C} chains excluded as marginal; smallest |u - threshold| {w['dist'].min():.3e}")
    assert bad <= 1e-4 * C, what
    ref = w["rows"]
    if dev_rows is not None:
        assert np.array_equal(dev_rows[:, :, 2][valid], ref[:, :, 2][valid]), what          # the decision
        assert np.array_equal(_bits(dev_rows[:, :, 3:])[valid], _bits(ref[:, :, 3:])[valid]), what   # the node the replay walks
        assert np.abs(dev_rows[:, :, 0] - ref[:, :, 0])[valid].max() < 1e-9, what
        assert np.abs(dev_rows[:, :, 1] - ref[:, :, 1])[valid].max() < 1e-12, what
    ok = valid.all(axis=1)
    assert np.array_equal(_bits(dev_p0[ok]), _bits(w["p0"][ok])), what
    assert np.abs(dev_chi0 - w["chi0"])[ok].max() < 1e-9, what


def _walk_covers(w, first=False):
    """The planted spread does its work: at every step chains are accepted outright, accepted on the draw and rejected."""
    acc, drew = w["rows"][:, :, 2] > 0.5, np.isfinite(w["dist"])
    for s in range(acc.shape[1]):
        if first:
            assert acc[:, s].all()
        else:
            assert (acc[:, s] & ~drew[:, s]).sum() > 20 and (acc[:, s] & drew[:, s]).sum() > 20 and (~acc[:, s]).sum() > 20, s
    for s in range(1, acc.shape[1]):                                   # both children of every walked node
        assert np.unique(w["node"][:, s]).size == 2 ** s


def _run_accept(depth, nsteps, per_chain, first, chain0, with_row, counter, seed):
    import torch
    from pysurfinv_amd import _lib
    A = _accept_arrays(depth, per_chain)
    C, P, N, M = C_ACC, P_ACC, N_ACC, A["M"]
    ob = (lambda a: np.repeat(a, M, axis=0)) if per_chain else (lambda a: a)
    mis, chi, L = (a.reshape(C, M) for a in R.rayleigh_misfit(A["c"], A["status"], ob(A["obs"]), ob(A["unc"]), ob(A["mask"])))
    assert (mis == R.FAILED).mean() > 0.03 and ((chi > 49) & (chi < 51)).sum() > 10
    w = R.accept_walk(mis, chi, L, A["q"], A["p0"], A["chi0"], seed, counter, bool(first), depth, nsteps, chain0)
    failed0 = A["chi0"] == R.FAILED
    m0 = mis[:, 0]
    assert (failed0 & (m0 == R.FAILED)).sum() >= 1 and (failed0 & (m0 < R.FAILED)).sum() >= 10
    if not first:
        assert w["rows"][failed0, 0, 2].all()                          # out of a failed state every proposal is taken
        d = chi[:, 0] - A["chi0"]
        assert np.percentile(d[~failed0 & (m0 < R.FAILED)], 2) < -4 and np.percentile(d[~failed0 & (m0 < R.FAILED)], 90) > 8
    _walk_covers(w, first)
    dc, dst, dq = _dev(A["c"]), _dev(A["status"]), _dev(A["q"])
    dobs, dunc, dmask = _dev(A["obs"]), _dev(A["unc"]), _dev(A["mask"])
    p0, chi0 = _dev(A["p0"]), _dev(A["chi0"])
    stride = 3 + N
    row = torch.zeros((C, nsteps, stride), dtype=torch.float64, device="cuda:0") if with_row else None
    Lb = _lib.lib()
    if depth == 1:
        _lib.check(Lb.surfdisp_mcmc_accept_device(None, C, N, P, _ptr(dc), _ptr(dst), _ptr(dobs), _ptr(dunc), _ptr(dmask), int(per_chain),
                                                  _ptr(dq), _ptr(p0), _ptr(chi0), _ptr(row), nsteps * stride, seed, counter, int(first), chain0))
    else:
        _lib.check(Lb.surfdisp_mcmc_accept_tree_device(None, C, N, P, depth, nsteps, _ptr(dc), _ptr(dst), _ptr(dobs), _ptr(dunc), _ptr(dmask),
                                                       int(per_chain), _ptr(dq), _ptr(p0), _ptr(chi0), _ptr(row), nsteps * stride, stride,
                                                       seed, counter, chain0))
    torch.cuda.synchronize()
    what = f"accept depth {depth} nsteps {nsteps} per_chain {per_chain} first {first} chain0 {chain0} row {with_row}"
    _check_accept(row.cpu().numpy() if with_row else None, p0.cpu().numpy(), chi0.cpu().numpy(), w, what)


@pytest.mark.gpu
@pytest.mark.parametrize("per_chain,first,chain0,with_row", [(0, 0, 0, 1), (1, 0, 2 ** 32 + 7, 1), (1, 1, 0, 1), (0, 1, 2 ** 32 + 7, 1),
                                                             (0, 0, 2 ** 32 + 7, 0), (1, 0, 0, 0)])
def test_accept_entry_is_the_replay(per_chain, first, chain0, with_row):
    """surfdisp_mcmc_accept_device, C = 1031, P = 7: decision, row, state and chi-square of every chain; shared and per-chain
    observations, first = 1, chain0 beyond 2^32, row = NULL."""
    _run_accept(1, 1, per_chain, first, chain0, with_row, 2 ** 32 + 3 if per_chain else 1, SEEDS[per_chain])


@pytest.mark.gpu
@pytest.mark.parametrize("depth,nsteps", [(2, 1), (2, 2), (3, 1), (3, 3), (4, 1), (4, 4)])
def test_accept_tree_entry_is_the_replay(depth, nsteps):
    """surfdisp_mcmc_accept_tree_device at depth 2..4, nsteps 1 and depth: every step's decision, the walked node's parameters
    bit for bit, the final state; per-chain observations at odd depth, chain0 beyond 2^32 at even depth, once without rows."""
    _run_accept(depth, nsteps, depth % 2, 0, (2 ** 32 + 7) if depth % 2 == 0 else 0, not (depth == 4 and nsteps == 1),
                2 ** 32 + 3 if depth == 3 else depth, SEEDS[nsteps > 1])


@pytest.mark.gpu
def test_accept_tree_joint5_entry_is_the_replay():
    """surfdisp_mcmc_accept_tree_joint5_device at depth 3 (it shares accept_walk): the hand-made arrays, `Entry` and the numpy
    joint misfit of test_ellip_mcmc.py - all six sources - with the replay's tree walk."""
    import torch
    from test_ellip_mcmc import Entry, _hand_made, _np_joint5, _observe
    C, N, PR, PL, depth = 1031, 3, 6, 4, 3
    M = (1 << depth) - 1
    rng = np.random.default_rng(6)
    src, st = _hand_made(rng, C, PR, PL)
    eR = (0.6 + rng.random((C, PR))).astype(np.float32)
    eR[:, 2] *= -1.0
    eR[12, 0] = np.nan
    src = src + [eR]
    cols = np.array([[0, 0], [0, 2], [4, 0], [1, 1], [5, 4], [2, 1], [4, 2], [3, 2], [5, 2], [3, 0], [2, 3], [1, 2]], np.int32)
    wt = np.array([1, 1, 1.5, 2, 0.75, 0.5, 1.5, 3, 0.75, 3, 0.5, 2], np.float64)
    obs, unc, mask = _observe(rng, src, cols, C, per_chain_noise=0.008)
    big = [np.repeat(a, M, axis=0) * (1 + 0.004 * rng.standard_normal((C * M, 1))).astype(np.float32) for a in src]
    stb = [np.repeat(s, M) for s in st]
    rep = lambda a: np.repeat(a, M, axis=0)
    ref = _np_joint5(big, stb, (PR, PL), cols, wt, rep(obs), rep(unc), rep(mask))
    mis, chi, L = (ref[:, k].reshape(C, M) for k in (0, 1, 2))
    chi0 = np.where(chi[:, 0] < R.FAILED, chi[:, 0], np.median(chi[:, 0])) + rng.uniform(-5.0, 6.0, C)
    chi0[::50] = R.FAILED
    e = Entry(big, (PR, PR, PL, PL, PR), (PR, PL), stb, cols, wt, obs, unc, mask, N, M)
    counter = 2 ** 32 + 3
    rc, row, p0, chi_d = e(True, depth, 0, torch.as_tensor(chi0, device="cuda:0"), counter=counter)
    assert rc == 0
    q = e.q.cpu().numpy().reshape(C, M, N)
    w = R.accept_walk(mis, chi, L, q, np.zeros((C, N)), chi0, 5, counter, False, depth, depth, 0)
    _walk_covers(w)
    # (Entry starts every state at zero: a chain that never accepts keeps it)
    _check_accept(row.cpu().numpy(), p0.cpu().numpy(), chi_d.cpu().numpy(), w, "joint5 tree depth 3")
