"""A host replay of the sampler kernels' random streams (csrc/surfdisp_mcmc.hip), written from the kernels' comments and the C
ABI of include/surfdisp.h as a SPECIFICATION, in vectorised numpy - a helper of tests/test_mcmc_replay.py like secular64.py,
not a test.

The streams are counter based (Philox4x32-10, Salmon et al. 2011: "reproducible for a given (seed, counter), independent of
the launch geometry"), so the host can restate them exactly: the integers bit for bit, the floating-point values up to the
rounding of the device's log / sqrt / sincospi.

Counter layout (the four 32-bit words of one Philox call; key = (seed low, seed high)):

    word 0   counter, low 32 bits                        the caller's call counter (one per lock step)
    word 1   counter, high 32 bits, XOR the stream tag   (below)
    word 2   index, low 32 bits                          propose: (chain0 + c) * N + n;  accept: chain0 + c
    word 3   index, high 32 bits

    tag of word 1            bits
    Gaussian try t of node k (k << 20) ^ (t << 8)         t = 0..499 in bits 8..16, k in bits 20..26: tree nodes 0..14, masked
                                                          redraw number a: node 64 + a
    uniform fallback, node k (k << 20) ^ 0x00ffff00       bits 8..19 all set (a try never sets 17..19), bits 20..23 inverted
    accept draw of step s    0x00aaaa00 ^ (s << 28)       bits 17 and 19 set, 18 clear: neither a try nor a fallback

Propose indexes words 2, 3 by element and accept by chain; those ranges overlap, so word 1 alone separates the streams.

Floating point.  The device evaluates x + s * sqrt(-2 log u1) * cospi(2 u2) (then sinpi) in double.  Here the value that is
COMPARED comes from mpmath at 50 digits, rounded to double once (numpy.longdouble, after an exact reduction of 2 u2 to an
octant, where mpmath is missing).  The in / out decision of a candidate is taken in plain double where it is certain - the
candidate lies more than SCREEN tolerances from both bounds - and in high precision otherwise; mpmath is therefore paid for
the accepted candidates and the near-bound ones only, and a box too narrow to hit costs 1000 cheap candidates.

Tolerance of a proposal value: |dev - ref| <= 16 eps (|x| + s rad), eps = 2^-52.  The published HIP math tables give double
log 1 ulp, sincospi 2 ulp, and sqrt correctly rounded (1 ulp in some editions; the installed ROCm tree carries no accuracy
table to check against, so both are carried): -2 log u1 errs by 1 eps relative, its root by 0.5 + (0.5 .. 1), times cospi
(2) and two products (0.5 each) is at most 4.5 eps of s rad, plus half an ulp of the sum: <= 5 eps (|x| + s rad) with or
without FMA contraction.  16 is a threefold margin over that.  A uniform draw lo + (hi - lo) u: 2 ulp of max(|lo|, |hi|).
"""
import numpy as np

try:
    import mpmath
    mpmath.mp.dps = 50
except ImportError:                                                    # numpy.longdouble serves (64-bit mantissa on x86)
    mpmath = None

M32 = np.uint64(0xFFFFFFFF)
EPS = 2.0 ** -52
TOL_ULPS = 16.0                                                        # the bound of a Gaussian proposal, in eps (|x| + s rad)
SCREEN = 64.0                                                          # a candidate further than this many tolerances from both bounds is decided in double
MAX_CALLS = 500                                                        # Philox calls of the bounded step, two candidates each
TAG_FALLBACK = 0x00ffff00
TAG_ACCEPT = 0x00aaaa00
U_MAX = 1.0 - 2.0 ** -53                                               # the largest double below 1


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------- integers
def philox4x32_10(ctr, key, rounds=10, m0=0xD2511F53, m1=0xCD9E8D57):
    """Philox4x32 with 10 rounds: ctr [..., 4] and key (k0, k1), 32-bit values held in uint64 arrays -> [..., 4]."""
    ctr = _u64(ctr) & M32
    x, y, z, w = (ctr[..., i] for i in range(4))
    k0, k1 = _u64(key[0]) & M32, _u64(key[1]) & M32
    m0, m1 = np.uint64(m0), np.uint64(m1)
    for _ in range(rounds):
        p0, p1 = m0 * x, m1 * z                                        # 32 x 32 -> 64 bits, exact
        x, y, z, w = (p1 >> np.uint64(32)) ^ y ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ w ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(np.broadcast_arrays(x, y, z, w), axis=-1)


def u53(a, b):
    """Uniform in (0, 1) from the top 53 bits v of (a << 32 | b): (v + 1/2) / 2^53 rounded to double, never 0 nor 1.
    (v + 1/2 is exact below 2^52 - the values are 2^-53 apart from 2^-54 on - and rounds to an even integer above, 2^-52
    apart; v = 2^53 - 1 alone would round to 1.0 and is kept at the largest double below 1 - the kernel's u53 does not do
    that yet and returns 1.0 there, see tests/test_mcmc_replay.py.)"""
    v = ((_u64(a) << np.uint64(32)) | _u64(b)) >> np.uint64(11)
    return np.minimum((v.astype(np.float64) + 0.5) * 2.0 ** -53, U_MAX)


def tag_try(node, t):
    return (int(node) << 20) ^ (int(t) << 8)


def tag_fallback(node):
    return (int(node) << 20) ^ TAG_FALLBACK


def tag_accept(s):
    return TAG_ACCEPT ^ (int(s) << 28)


def _words(seed, counter, tag, index):
    """One Philox call per entry of `index` (uint64 array): the four output words."""
    index = _u64(index)
    ctr = np.empty(index.shape + (4,), np.uint64)
    ctr[..., 0] = np.uint64(counter & 0xFFFFFFFF)
    ctr[..., 1] = _u64((counter >> 32) & 0xFFFFFFFF) ^ _u64(tag)
    ctr[..., 2] = index & M32
    ctr[..., 3] = index >> np.uint64(32)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def accept_uniform(seed, counter, s, global_chain):
    """The accept draw of step s of a call for the chains `global_chain` (chain0 + c)."""
    r = _words(seed, counter, tag_accept(s), global_chain)
    return u53(r[..., 0], r[..., 1])


# ------------------------------------------------------------------------------------------------------- the bounded step
def _octant(u2):
    """2 u2 = k / 2 + r exactly (u2 a dyadic in (0, 1)): the quadrant k and r in [-1/4, 1/4]."""
    v = 2.0 * u2
    k = np.rint(2.0 * v)
    return k.astype(np.int64) & 3, v - 0.5 * k


def _rotate(k, c, s):
    """(cospi, sinpi) of k / 2 + r from those of r."""
    cs = np.where(k == 0, c, np.where(k == 1, -s, np.where(k == 2, -c, s)))
    sn = np.where(k == 0, s, np.where(k == 1, c, np.where(k == 2, -s, -c)))
    return cs, sn


def box_muller(u1, u2, two_u2=True):
    """(rad, cos, sin) of one Philox call in plain double: rad = sqrt(-2 log u1), the angle 2 pi u2 reduced exactly."""
    rad = np.sqrt(-2.0 * np.log(u1))
    k, r = _octant(u2 if two_u2 else 0.5 * u2)
    cs, sn = _rotate(k, np.cos(np.pi * r), np.sin(np.pi * r))
    return rad, cs, sn


def normal_pair(seed, counter, node, t, gidx):
    """The two standard normals (cos first, then sin) of try t of node `node` for the elements gidx, in plain double."""
    r = _words(seed, counter, tag_try(node, t), gidx)
    rad, cs, sn = box_muller(u53(r[..., 0], r[..., 1]), u53(r[..., 2], r[..., 3]))
    return rad * cs, rad * sn


def _exact_candidate(x, s, u1, u2, which):
    """x + s sqrt(-2 log u1) cospi(2 u2) (which = 0) or sinpi (1) in high precision, rounded to double once."""
    if mpmath is not None:
        mp = mpmath.mp
        rad = mp.sqrt(-2 * mp.log(mp.mpf(float(u1))))
        ang = 2 * mp.mpf(float(u2))
        return float(mp.mpf(float(x)) + mp.mpf(float(s)) * rad * (mp.sinpi(ang) if which else mp.cospi(ang)))
    ld = np.longdouble
    k, r = _octant(np.float64(u2))
    a = ld(np.pi) * ld(r) + ld(1.2246467991473532e-16) * ld(r)         # pi to 106 bits
    cs, sn = _rotate(k, np.cos(a), np.sin(a))
    rad = np.sqrt(ld(-2) * np.log(ld(u1)))
    return float(ld(x) + ld(s) * rad * (sn if which else cs))


def value_tolerance(x, s, rad):
    return TOL_ULPS * EPS * (np.abs(x) + np.abs(s) * rad)


def uniform_tolerance(lo, hi):
    return 2.0 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)))


def draw_bounded(x, lo, hi, s, seed, counter, node, gidx, reset=False, exact=True):
    """The bounded Gaussian step around x: candidates x + s z, cos first, then sin, of up to 500 Philox calls until one lies
    in the open interval (lo, hi); then, or at once with `reset`, the uniform word: lo + (hi - lo) u.

    x, lo, hi, s, gidx: arrays of one shape.  Returns (value, margin, tol, uniform):
    margin   the smallest distance, over every candidate tested up to and including the accepted one, between a candidate
             and either bound, in units of that candidate's tolerance - below 1 the device may legitimately have branched
             differently; inf for `reset`
    tol      the bound on |device - value|
    uniform  True where the value is the uniform draw
    exact=False: everything in plain double (the distribution tests, which need no last bit)."""
    shape = np.shape(x)
    x, lo, hi, s = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), shape)).ravel() for a in (x, lo, hi, s))
    gidx = np.ascontiguousarray(np.broadcast_to(_u64(gidx), shape)).ravel()
    n = x.size
    val = np.full(n, np.nan)
    margin = np.full(n, np.inf)
    tol = np.zeros(n)
    uniform = np.zeros(n, bool)
    act = np.arange(n) if not reset else np.arange(0)
    for t in range(MAX_CALLS):
        if act.size == 0:
            break
        r = _words(seed, counter, tag_try(node, t), gidx[act])
        u1, u2 = u53(r[:, 0], r[:, 1]), u53(r[:, 2], r[:, 3])
        rad, cs, sn = box_muller(u1, u2)
        tl = value_tolerance(x[act], s[act], rad)
        done = np.zeros(act.size, bool)
        for which, trig in ((0, cs), (1, sn)):
            todo = np.flatnonzero(~done)
            i = act[todo]
            nv = x[i] + s[i] * rad[todo] * trig[todo]
            d = np.minimum(nv - lo[i], hi[i] - nv)                     # > 0 inside
            if exact:
                near = np.flatnonzero(~(np.abs(d) > SCREEN * tl[todo]))
                for j in near:
                    nv[j] = _exact_candidate(x[i[j]], s[i[j]], u1[todo[j]], u2[todo[j]], which)
                d = np.minimum(nv - lo[i], hi[i] - nv)
            ok = (nv < hi[i]) & (nv > lo[i])
            with np.errstate(divide="ignore", invalid="ignore"):
                m = np.where(tl[todo] > 0, np.abs(d) / tl[todo], np.where(d == 0, 0.0, np.inf))
            margin[i] = np.minimum(margin[i], m)
            hit = todo[ok]
            if exact:
                for j in np.flatnonzero(ok):
                    nv[j] = _exact_candidate(x[i[j]], s[i[j]], u1[todo[j]], u2[todo[j]], which)
            val[act[hit]] = nv[ok]
            tol[act[hit]] = tl[hit]
            done[hit] = True
        act = act[~done]
    rest = np.flatnonzero(np.isnan(val))
    if rest.size:
        r = _words(seed, counter, tag_fallback(node), gidx[rest])
        ld = np.longdouble
        u = u53(r[:, 0], r[:, 1])
        val[rest] = (ld(lo[rest]) + (ld(hi[rest]) - ld(lo[rest])) * ld(u)).astype(np.float64)
        tol[rest] = uniform_tolerance(lo[rest], hi[rest])
        uniform[rest] = True
    return val.reshape(shape), margin.reshape(shape), tol.reshape(shape), uniform.reshape(shape)


def _grid(C, N, chain0):
    """gidx [C, N] of a call on C chains from chain0 on (Python integers: chain0 * N may pass 2^32)."""
    return _u64([[(chain0 + c) * N + n for n in range(N)] for c in range(C)])


def propose(p, vmin, vmax, step, seed, counter, reset=False, chain0=0, node=0, exact=True):
    """surfdisp_mcmc_propose_device: one proposal per chain, p [C, N] -> (out, margin, tol, uniform), each [C, N]."""
    C, N = p.shape
    b = lambda a: np.broadcast_to(np.asarray(a, np.float64), (C, N))
    return draw_bounded(p, b(vmin), b(vmax), b(step), seed, counter, node, _grid(C, N, chain0), reset, exact)


def propose_tree(p, vmin, vmax, step, seed, counter, depth, chain0=0, given=None):
    """surfdisp_mcmc_propose_tree_device: [C][2^depth - 1][N]; node k is drawn from the state of its branch - node 0 from p,
    child 2k + 1 ("accepted") from the proposal of k, child 2k + 2 ("rejected") from the state of k.
    given: a tree (the device's) whose proposals serve as the children's states, so that every node is compared on bit-equal
    input; None: the tree is the replay's own, and margin / tol accumulate along a branch (a child inherits the doubt and
    the error of the state it starts from).  Returns (out, margin, tol, uniform)."""
    C, N = p.shape
    M = (1 << depth) - 1
    out, margin, tol, uni = (np.zeros((C, M, N), t) for t in (np.float64, np.float64, np.float64, bool))
    S = {0: (p, np.full((C, N), np.inf), np.zeros((C, N)))}           # state of node k: value, margin, error bound
    for k in range(M):
        x, xm, xt = S[k]
        v, m, t, u = propose(x, vmin, vmax, step, seed, counter, False, chain0, node=k)
        out[:, k], margin[:, k], tol[:, k], uni[:, k] = v, np.minimum(m, xm), t + np.where(u, 0.0, xt), u
        if 2 * k + 2 < M:
            S[2 * k + 1] = (v, margin[:, k], tol[:, k]) if given is None else (given[:, k], np.full((C, N), np.inf), np.zeros((C, N)))
            S[2 * k + 2] = S[k]
    return out, margin, tol, uni


def propose_masked(p, vmin, vmax, step, seed, counter, attempt, mode, tags, tag, out, chain0=0):
    """surfdisp_mcmc_propose_masked_device: the chains with tags[c] == tag draw again as node 64 + attempt (mode 0 the
    bounded step, 1 the uniform draw, 2 the chain's state itself); the other rows of `out` stay.  -> (out, margin, tol)."""
    out = np.array(out, np.float64)
    margin, tol = np.full(out.shape, np.inf), np.zeros(out.shape)
    sel = np.asarray(tags) == tag
    if mode == 2:
        out[sel] = p[sel]
    else:
        v, m, t, _ = propose(p, vmin, vmax, step, seed, counter, mode == 1, chain0, node=64 + attempt)
        out[sel], margin[sel], tol[sel] = v[sel], m[sel], t[sel]
    return out, margin, tol


# ---------------------------------------------------------------------------------------------------------------- accept
FAILED = 88888.0


def rayleigh_misfit(c, status, c_obs, uncer, mask):
    """(misfit, chi-square, L) of the Rayleigh phase entries in float64 from the fp32 predictions c [S, P]: chi2 the sum of
    ((obs - pred) / uncer)^2 over the masked-in periods, misfit sqrt(chi2 / count), chi2 := sqrt(50 chi2) from 50 on,
    L = exp(-chi2 / 2); (88888, 88888, 0) for a stack whose status is not 0 or with a prediction below 0.01 at ANY period.
    c_obs, uncer, mask: [P] or [S, P] (the row of the stack's chain)."""
    v = np.asarray(c, np.float32).astype(np.float64)
    m = np.broadcast_to(np.asarray(mask) != 0, v.shape)
    failed = (v < 0.01).any(axis=1)
    if status is not None:
        failed |= np.asarray(status) != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (np.asarray(c_obs, np.float64) - v) / np.asarray(uncer, np.float64)
        chi = np.where(m, r * r, 0.0).sum(axis=1)
        mis = np.sqrt(chi / m.sum(axis=1))
        chi = np.where(chi < 50.0, chi, np.sqrt(50.0 * chi))
        L = np.exp(-0.5 * chi)
    return np.where(failed, FAILED, mis), np.where(failed, FAILED, chi), np.where(failed, 0.0, L)


def accept_walk(mis, chi, L, q, p0, chi0, seed, counter, first=False, depth=1, nsteps=1, chain0=0, halve=True):
    """The Metropolis test(s) of one call: mis, chi, L [C, M] of the M = 2^depth - 1 stacks of every chain (M = 1: the plain
    entry), q [C, M, N] their parameters, p0 [C, N] and chi0 [C] the states.  Per step: the proposal of the node the chain
    stands on is accepted if `first`, if chi < chi0, or if u > 1 - exp(-(chi - chi0) / 2) with the step's accept draw u; then
    child 2k + 1 (accepted) or 2k + 2.  Returns a dict: rows [C, nsteps, 3 + N] = (misfit, L, accepted, proposal), p0, chi0
    after the call, node [C, nsteps] the nodes walked, dist [C, nsteps] = |u - threshold| (inf where no draw decided)."""
    C, M, N = q.shape
    assert M == (1 << depth) - 1 and 1 <= nsteps <= depth
    p0, chi0 = np.array(p0, np.float64), np.array(chi0, np.float64)
    rows = np.zeros((C, nsteps, 3 + N))
    nodes, dist = np.zeros((C, nsteps), np.int64), np.full((C, nsteps), np.inf)
    node = np.zeros(C, np.int64)
    ar = np.arange(C)
    gc = _u64([chain0 + c for c in range(C)])
    for s in range(nsteps):
        m1, c1, l1, q1 = mis[ar, node], chi[ar, node], L[ar, node], q[ar, node]
        u = accept_uniform(seed, counter, s, gc)
        with np.errstate(over="ignore", invalid="ignore"):
            thr = 1.0 - np.exp(-(c1 - chi0) / (2.0 if halve else 1.0))
        better = c1 < chi0
        acc = np.full(C, True) if first else better | (u > thr)
        if not first:
            dist[:, s] = np.where(better, np.inf, np.abs(u - thr))
        rows[:, s, 0], rows[:, s, 1], rows[:, s, 2], rows[:, s, 3:] = m1, l1, acc, q1
        nodes[:, s] = node
        p0[acc], chi0[acc] = q1[acc], c1[acc]
        node = np.where(acc, 2 * node + 1, 2 * node + 2)
    return dict(rows=rows, p0=p0, chi0=chi0, node=nodes, dist=dist)
