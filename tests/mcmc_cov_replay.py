"""A host replay of surfdisp_mcmc_propose_cov_device (csrc/surfdisp_mcmc_cov.hip), written from the entry's comment in
include/surfdisp.h as a SPECIFICATION - a helper of tests/test_mcmc_cov_host.py and tests/test_mcmc_cov_gpu.py, built on
mcmc_prior_replay.py as that is built on mcmc_replay.py.

Per chain c and tree node k = 0, 1, ..., 2^depth - 2 (node 0 draws from the chain's state, child 2k + 1 from the final proposal of k,
child 2k + 2 from the state of k) and whole-proposal retry r = 0 .. G + U - 1:

    r <  G   z_n = sqrt(-2 log u1) cospi(2 u2) of ONE Philox call: word 1 = mcmc_replay.tag_try(k, 0), stream index
             gidx + (r << 48), gidx = (chain0 + c) N + n (mcmc_prior_replay.retry_index);
             cand_n = x_n + sum_{j <= n} L[n][j] z_j, L = factor[(chain0 + c) // chains_per_factor]
    r >= G   mcmc_prior_replay.candidate(..., r >= G): the uniform draw
    good     every scalar strictly inside (vmin_n, vmax_n) and, with rules, the torch PriorRules on the CPU in float64

the first good candidate is the node's proposal and r its `tries`; none: the state itself, tries = G + U.

Floating point.  The value that is COMPARED comes from mpmath at 50 digits - z and the sum in high precision, rounded to double
once (numpy.longdouble where mpmath is missing).  Tolerance of candidate scalar n, with S_n = |x_n| + sum_j |L[n][j] z_j| and
eps = 2^-52, derived as mcmc_replay derives its 16 eps:
  * z_j: -2 log u1 errs by 1 eps relative (log: 1 ulp), its root by 0.5 + (0.5 .. 1) (sqrt correctly rounded, or 1 ulp), cospi
    2, their product 0.5: at most 4 eps |z_j|; the product with L[n][j] 0.5 more (none when it is fused): 4.5 eps |L[n][j] z_j|
    per term, 4.5 eps S_n together;
  * the n + 2 terms (x_n and n + 1 products) take n + 1 additions, in any association, with or without FMA; each result is at
    most S_n in magnitude and is rounded by at most half an eps of it: 0.5 (n + 1) eps S_n;
  * the compared value is itself rounded once: 0.5 eps S_n.
Together (0.5 n + 5.5) eps S_n; with the threefold margin of mcmc_replay, TOL_n = 1.5 (n + 11) eps S_n.  (For n = 0 that is
16.5 eps (|x| + |L z|), mcmc_replay's 16 plus the rounding of the compared value.  The form 3 (n + 5) eps S_n counts a whole eps
per addition and none for the compared value; this bound is the tighter one from n = 3 on.)  A uniform draw: mcmc_replay's
uniform_tolerance.

Doubt.  A candidate's in / out decision is certain when one scalar lies outside the box by more than its tolerance, or all lie
inside by more than theirs; `margin` is the smallest distance that decided, in tolerances, over every candidate of the node up
to and including the chosen one (< 1: the device may have decided differently; a candidate within mcmc_replay.SCREEN tolerances
of a wall is decided on the high-precision value).  `slack` is mcmc_prior_replay's for the rules.  A doubtful (chain, node) is
left out of a comparison together with everything below it in the tree (`doubtful`).
"""
import numpy as np

import mcmc_replay as R
import mcmc_prior_replay as PR

mpmath = R.mpmath
EPS = R.EPS
SCREEN = R.SCREEN
SLACK_BAND = PR.SLACK_BAND
MAX_EXCLUDED = 0.01                                                    # of the (chain, node) cases of one comparison


def tol_factor(N):
    """[N]: TOL_n / (eps S_n) = 1.5 (n + 11) (the module's text)."""
    return 1.5 * (np.arange(N) + 11.0)


def uniforms(seed, counter, node, r, C, N, chain0):
    """(u1, u2) [C, N] of retry r of node `node`: one Philox call per (chain, scalar), the tag of Gaussian try 0."""
    w = R._words(seed, counter, R.tag_try(node, 0), PR.retry_index(C, N, chain0, r))
    return R.u53(w[..., 0], w[..., 1]), R.u53(w[..., 2], w[..., 3])


def normals(u1, u2):
    """z = sqrt(-2 log u1) cospi(2 u2) in plain double (the angle reduced exactly)."""
    rad, cs, _ = R.box_muller(u1, u2)
    return rad * cs


def exact_row(x, L, u1, u2):
    """The candidate row x + L z [N] with z and the sums in high precision, rounded to double once."""
    N = x.size
    if mpmath is not None:
        mp = mpmath.mp
        z = [mp.sqrt(-2 * mp.log(mp.mpf(float(a)))) * mp.cospi(2 * mp.mpf(float(b))) for a, b in zip(u1, u2)]
        return np.array([float(mp.mpf(float(x[n])) + mp.fsum(mp.mpf(float(L[n, j])) * z[j] for j in range(n + 1))) for n in range(N)])
    ld = np.longdouble
    k, r = R._octant(np.asarray(u2, np.float64))
    a = ld(np.pi) * r.astype(ld) + ld(1.2246467991473532e-16) * r.astype(ld)          # pi to 106 bits
    cs, _ = R._rotate(k, np.cos(a), np.sin(a))
    z = np.sqrt(ld(-2) * np.log(np.asarray(u1, np.float64).astype(ld))) * cs
    return np.array([float(ld(x[n]) + (np.tril(L)[n].astype(ld) * z).sum()) for n in range(N)])


def _decide(v, lo, hi, tol):
    """(inside bool [B], margin [B]) of the rows v [B, N]: see the module's text."""
    d = np.minimum(v - lo, hi - v)                                     # > 0 inside
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(tol > 0, np.abs(d) / tol, np.where(d == 0, 0.0, np.inf))
    inside = ((v < hi) & (v > lo)).all(axis=1)
    out_by = np.where(d < 0, m, 0.0).max(axis=1)                       # the scalar furthest outside decides an "out"
    return inside, np.where(out_by >= 1.0, out_by, m.min(axis=1))


def gaussian_candidates(x, lo, hi, Ls, u1, u2, exact=True, xtol=0.0):
    """The rows x + L z of one retry, x [B, N] (known to within xtol), Ls [B, N, N] -> (value [B, N], inside [B], margin [B], tol [B, N]).  Plain double
    where the decision is certain by SCREEN tolerances, the high-precision value otherwise; `exact`: which rows get the
    high-precision value whatever their distance (True: those inside; a bool [B])."""
    B, N = x.shape
    z = normals(u1, u2)
    terms = np.tril(Ls) * z[:, None, :]
    v = x + terms.sum(axis=2)
    tol = tol_factor(N) * EPS * (np.abs(x) + np.abs(terms).sum(axis=2)) + xtol
    inside, m = _decide(v, lo, hi, tol)
    want = (m < SCREEN) | (inside & exact)
    for b in np.flatnonzero(want):
        v[b] = exact_row(x[b], Ls[b], u1[b], u2[b])
    if want.any():
        inside, m = _decide(v, lo, hi, tol)
    return v, inside, m, tol


def propose_cov(p, vmin, vmax, factor, chains_per_factor, rules, seed, counter, depth, G, U, chain0=0, given=None, factor0=0):
    """surfdisp_mcmc_propose_cov_device on the host: p [C, N], factor [F, N, N] (lower triangular; NOT transposed) -> (out [C, M,
    N], tries [C, M], margin [C, M], tol [C, M, N], slack [C, M]), M = 2^depth - 1.  factor0: the index, in the whole sampler's list
    of factors, of factor[0] (a call far into the list - chain0 - is handed the factors it reads only).  rules: a PriorRules on a CPU model, or None (the
    box alone).  given: the device's `out`, whose rows serve as the children's states, so that every node is compared on bit-equal
    input; None: the replay's own tree, and a child inherits the doubt and the error bound of the state it starts from.  tol: the
    bound on |device - out| of the chosen candidate (the state's own where the node is exhausted: 0 on the device's tree)."""
    p = np.ascontiguousarray(p, np.float64)
    C, N = p.shape
    M = (1 << depth) - 1
    cap = G + U
    assert G >= 0 and U >= 0 and 1 <= cap <= 16384 and 1 <= N <= 64
    factor = np.asarray(factor, np.float64).reshape(-1, N, N)
    f = np.array([(chain0 + c) // chains_per_factor - factor0 for c in range(C)])
    assert f.min() >= 0 and f.max() < factor.shape[0]
    Ls = factor[f]
    lo, hi = (np.broadcast_to(np.asarray(a, np.float64), (N,)) for a in (vmin, vmax))
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
            if r < G:
                u1, u2 = uniforms(seed, counter, k, r, C, N, chain0)
                v, inside, m, t = gaussian_candidates(x[act], lo, hi, Ls[act], u1[act], u2[act], xtol=xt[act])
            else:
                v, _, t, _ = PR.candidate(x[act], lo, hi, np.zeros(N), seed, counter, k, r, G, PR.retry_index(C, N, chain0, r)[act])
                inside, m = _decide(v, lo, hi, t)
            good, s = inside.copy(), np.full(act.size, np.inf)
            if rules is not None and inside.any():
                good[inside], s[inside] = PR.rule_margins(rules, v[inside])
            mg[act] = np.minimum(mg[act], m)
            sl[act] = np.minimum(sl[act], s)
            hit = act[good]
            out[hit, k], tries[hit, k], tol[hit, k] = v[good], r, t[good]
            act = act[~good]
        margin[:, k], slack[:, k] = mg, sl
        if 2 * k + 2 < M:
            if given is None:
                S[2 * k + 1] = (out[:, k].copy(), mg, sl, tol[:, k].copy())
            else:
                S[2 * k + 1] = (np.ascontiguousarray(given[:, k], np.float64), np.full(C, np.inf), np.full(C, np.inf), np.zeros((C, N)))
            S[2 * k + 2] = S[k]
    return out, tries, margin, tol, slack


def doubtful(margin, slack):
    """bool [C, M]: the (chain, node) cases left out of a comparison - a decision within a tolerance of a wall or within SLACK_BAND
    of a rule's threshold, and every node below such a one in the tree."""
    d = (margin < 1.0) | (slack < SLACK_BAND)
    for k in range(d.shape[1]):
        for ch in (2 * k + 1, 2 * k + 2):
            if ch < d.shape[1]:
                d[:, ch] |= d[:, k]
    return d
