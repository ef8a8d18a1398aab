"""A host replay of surfdisp_mcmc_propose_prior_device (csrc/surfdisp_mcmc_prior.hip), written from the entry's comment in
include/surfdisp.h as a SPECIFICATION - a helper of tests/test_prior_redraw.py like mcmc_replay.py, which it is built on.

Per chain and tree node k = 0, 1, ..., 2^depth - 2 (node 0 draws from the chain's state, child 2k + 1 from the final proposal of
k, child 2k + 2 from the state of k) and whole-proposal retry r = 0 .. G + U - 1:

    candidate[n] = mcmc_replay.draw_bounded(state[n], ..., node k, stream index gidx + (r << 48), reset = r >= G)
    good         = the torch PriorRules on the CPU in float64

the first good candidate is the node's proposal and r its `tries`; none: the state itself, tries = G + U.

Counter layout: word 1 of a draw is mcmc_replay's (tag_try / tag_fallback of node k); the retry r sits in bits 16..29 of word 3
(the stream index's bits 48..61), which (chain0 + C) N < 2^48 keeps free.  r = 0 is the draw of the plain and the tree entries.

Doubt.  `margin` is mcmc_replay's: the smallest distance of a compared candidate scalar from a bound, in units of its tolerance
(< 1: the device may have branched differently).  `slack` is the smallest absolute difference between the two sides of any rule
inequality tested on a candidate, up to and including the chosen one: a device Vs differs from the torch one by rounding (about
1e-15), so below 1e-9 - a million ulp of a Vs near 4 - the decision is left out of a comparison, far above what the prior
kernel's test against the torch rules (tests/test_prior.py, zero mismatches on 5 000 draws) leaves room for.
"""
import numpy as np
import torch

import mcmc_replay as R

SLACK_BAND = 1e-9
EPS_MONO = float(np.finfo(float).eps)                                 # monoIncrease, models.py:8


def rule_margins(rules, params, rows=None):
    """(good bool [B], slack float [B]) of the PriorRules on the rows of `params` (numpy [B, N]; `rows`: the local-info row of each,
    for a model with per-point constants): good is the torch
    ``PriorRules.__call__`` on the CPU in float64; slack the smallest |lhs - rhs| over every inequality the rules test
    (models.py:302-320: jumps between groups, the cap at every grid point, diff >= eps inside a monotone group), restated here
    on the same grid points and checked to give the same verdict."""
    m = rules.model
    t = torch.from_numpy(np.array(params, dtype=np.float64))          # (a copy: the caller's rows may be read-only)
    good = rules(t, rows=rows).numpy()
    (z, vs, *_), grp, ngrid = m.seis_prop_grids(t, rows=rows, ref_layer=False)
    nm = np.asarray([m.GROUP_NAMES[int(q)] for q in grp[0].tolist() if int(q) >= 0])
    vs = vs[:, :nm.size].numpy()
    slack = np.full(vs.shape[0], np.inf)
    ok = np.ones(vs.shape[0], bool)
    if rules.positive_jumps:
        for i in np.where(nm[1:] != nm[:-1])[0]:
            d = vs[:, i + 1] - vs[:, i]
            ok &= ~(vs[:, i + 1] < vs[:, i])
            slack = np.minimum(slack, np.abs(d))
    if rules.vs_max is not None:
        ok &= ~(vs > rules.vs_max).any(axis=1)
        slack = np.minimum(slack, np.abs(vs - rules.vs_max).min(axis=1))
    for g in rules.monotone_groups:
        sel = np.where(nm == g)[0]
        if sel.size > 1:
            d = np.diff(vs[:, sel], axis=1)
            ok &= (d >= EPS_MONO).all(axis=1)
            slack = np.minimum(slack, np.abs(d - EPS_MONO).min(axis=1))
    assert np.array_equal(ok, good), "the restated inequalities disagree with PriorRules.__call__"
    return good, slack


def retry_index(C, N, chain0, r):
    """Stream index [C, N] of whole-proposal retry r: gidx + (r << 48), gidx = (chain0 + c) N + n (Python integers, then uint64)."""
    assert 0 <= r < 16384 and (chain0 + C) * N < 2 ** 48
    return R._grid(C, N, chain0) + np.uint64(r << 48)


def candidate(x, vmin, vmax, step, seed, counter, node, r, G, gidx, exact=True):
    """The candidate rows of retry r of node `node` drawn from the states x [B, N] -> (value, margin, tol, uniform), each [B, N]
    (mcmc_replay.draw_bounded).  gidx [B, N]: the rows of ``retry_index(C, N, chain0, r)`` that belong to the rows of x."""
    B, N = x.shape
    b = lambda a: np.broadcast_to(np.asarray(a, np.float64), (B, N))
    return R.draw_bounded(x, b(vmin), b(vmax), b(step), seed, counter, node, gidx, reset=r >= G, exact=exact)


def propose_prior(p, aux, vmin, vmax, step, rules, seed, counter, depth, G, U, chain0=0, given=None, rows=None):
    """surfdisp_mcmc_propose_prior_device on the host: p [C, N] -> (out [C, M, N], tries [C, M], margin [C, M], tol [C, M, N],
    slack [C, M]), M = 2^depth - 1.  aux: None (K = 0), or the per-chain constants [C, K] the device call is given - then `rows` [C]
    names the row of the model's local-information table each chain reads, aux must be those rows of the table, and the rules are
    evaluated with rows=; the draws do not depend on aux.
    given: the device's `out`, whose rows serve as the children's states, so that every node is compared on bit-equal input;
    None: the replay's own tree, and a child inherits the doubt (margin, slack) and the error bound of the state it starts from.
    margin / slack: the smallest over every candidate the node compared, up to and including the chosen one (see the module's
    text); tol: the bound on |device - out| of the chosen candidate (the state's own bound where the node is exhausted and
    proposes its state: 0 on the device's tree)."""
    if aux is not None and np.size(aux):
        rows = np.asarray(rows, np.int64)
        assert np.array_equal(np.asarray(aux, np.float64), rules.model._aux.cpu().numpy()[rows]), "aux is not the table's rows"
    else:
        rows = None
    p = np.ascontiguousarray(p, np.float64)
    C, N = p.shape
    M = (1 << depth) - 1
    cap = G + U
    assert G >= 0 and U >= 0 and 1 <= cap <= 16384
    out, tol = np.zeros((C, M, N)), np.zeros((C, M, N))
    tries = np.full((C, M), cap, np.int64)
    margin, slack = np.full((C, M), np.inf), np.full((C, M), np.inf)
    S = {0: (p, np.full(C, np.inf), np.full(C, np.inf), np.zeros((C, N)))}      # state of node k: value, margin, slack, error bound
    for k in range(M):
        x, xm, xs, xt = S[k]
        act = np.arange(C)
        mg, sl = xm.copy(), xs.copy()
        out[:, k], tol[:, k] = x, xt                                   # (kept where every retry is bad)
        for r in range(cap):
            if act.size == 0:
                break
            v, m, t, u = candidate(x[act], vmin, vmax, step, seed, counter, k, r, G, retry_index(C, N, chain0, r)[act])
            good, s = rule_margins(rules, v, None if rows is None else rows[act])
            mg[act] = np.minimum(mg[act], m.min(axis=1))
            sl[act] = np.minimum(sl[act], s)
            hit = act[good]
            out[hit, k], tries[hit, k] = v[good], r
            tol[hit, k] = t[good] + np.where(u[good], 0.0, xt[hit])
            act = act[~good]
        margin[:, k], slack[:, k] = mg, sl
        if 2 * k + 2 < M:
            if given is None:
                S[2 * k + 1] = (out[:, k].copy(), mg, sl, tol[:, k].copy())
            else:
                S[2 * k + 1] = (np.ascontiguousarray(given[:, k], np.float64), np.full(C, np.inf), np.full(C, np.inf), np.zeros((C, N)))
            S[2 * k + 2] = S[k]
    return out, tries, margin, tol, slack


def marginal(margin, slack):
    """bool [C, M]: the (chain, node) entries left out of value and decision comparisons."""
    return (margin < 1.0) | (slack < SLACK_BAND)


def good_starts(rules, spec, C, seed, rows=None):
    """C uniform prior draws that satisfy `rules` (the first C good ones of a seeded numpy stream).  rows [C]: the local-info row of
    each chain; chain c then takes the first unused draw that is good at ITS row."""
    rng = np.random.default_rng(seed)
    if rows is None:
        keep = []
        for _ in range(200):
            q = spec.vmin + (spec.vmax - spec.vmin) * rng.random((max(4 * C, 256), spec.n))
            g, _ = rule_margins(rules, q)
            keep.extend(q[g])
            if len(keep) >= C:
                return np.ascontiguousarray(np.array(keep[:C]))
        raise RuntimeError("good_starts: the prior accepts too few uniform draws")
    rows = np.asarray(rows, np.int64)
    out, todo = np.zeros((C, spec.n)), np.arange(C)
    for _ in range(200):
        q = spec.vmin + (spec.vmax - spec.vmin) * rng.random((todo.size, spec.n))
        g, _ = rule_margins(rules, q, rows[todo])
        out[todo[g]] = q[g]
        todo = todo[~g]
        if todo.size == 0:
            return np.ascontiguousarray(out)
    raise RuntimeError("good_starts: the prior accepts too few uniform draws")
