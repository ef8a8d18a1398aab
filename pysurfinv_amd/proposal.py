"""What draws the proposals of a fused lock step of ``mcmc.MetropolisBatch``, and what adapts them.

A proposal is one object.  ``MetropolisBatch.proposal()`` returns the one in force; its ``draw`` launches the propose stage of a
lock step - a plain step and the speculative tree alike - and it states what the sampler has to know about it: ``max_depth``, the
deepest tree it can draw, and ``redraws_in_kernel``, whether its kernel redraws until the candidate is good, writes the retry
indices (``tries``) and counts the nodes that found none (``ExhaustedCounter``).

* ``ReferenceSteps``: the reference's independent steps ``spec.step`` (``surfdisp_mcmc_propose_device`` / ``_tree_device``), then the
  masked redraw rounds of a ``PriorRules(redraw="rounds")`` - which know no tree;
* ``KernelRedraw``: ``PriorRules(redraw="kernel")``, the reference's redraw loop inside ``surfdisp_mcmc_propose_prior_device``;
* ``Factor``: ``x + F z`` with a lower-triangular factor per grid point (``set_proposal``, and the working factors of an adaptive
  run), through ``surfdisp_mcmc_propose_cov_device``, with or without rules.

``Adaptation`` is ``set_adaptive``: the validated options and the state of a run.  The numpy statements of the factor and the
adaptation kernels (``cov_factor_reference``, ``adapt_reference``) live here too; ``mcmc`` re-exports every public name."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

MAX_DEPTH = 4              # the deepest speculative tree of the propose and accept kernels (SD_MCMC_MAX_DEPTH)
COV_MAX_N = 64             # scalars per chain of the covariance-shaped proposal: one lane each (SURFDISP_MCMC_COV_N_MAX)
COV_TRIES = (1000, 10000)  # whole-proposal Gaussian / uniform redraws of a factor without PriorRules (the reference's caps)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def cov_factor_reference(cov, scale, fallback_step):
    """``surfdisp_mcmc_cov_factor_device`` in numpy float64: cov [P, N, N] (symmetric; zero rows and columns at fixed parameters) ->
    (L [P, N, N] lower triangular with L L^T = scale^2 cov over the rows whose diagonal is not zero and zero rows and columns
    elsewhere, flag [P]).  Right-looking Cholesky, the kernel's order of operations; a pivot that is not positive and finite: flag 1
    and L = diag(fallback_step)."""
    cov = np.asarray(cov, np.float64)
    P, N, _ = cov.shape
    fb = np.asarray(fallback_step, np.float64)
    out, flag = np.zeros((P, N, N)), np.zeros(P, np.int32)
    for p in range(P):
        live = np.flatnonzero(np.diagonal(cov[p]) != 0.0)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            A = (float(scale) * float(scale)) * np.triu(cov[p]).T          # the kernel reads cov[k][n], k <= n, as A[n][k]
            Lp, bad = np.zeros((N, N)), False
            for a, j in enumerate(live):
                d = A[j, j]
                if not (d > 0.0 and np.isfinite(d)):
                    bad = True
                    break
                s = np.sqrt(d)
                below = live[a + 1:]
                l = A[below, j] / s
                Lp[j, j], Lp[below, j] = s, l
                for b, n in enumerate(below):
                    ks = below[:b + 1]
                    A[n, ks] -= l[b] * l[:b + 1]
        out[p], flag[p] = (np.diag(fb), 1) if bad else (Lp, 0)
    return out, flag


def cov_factor(cov, scale, fallback_step):
    """The proposal factors of P covariances on the device (``surfdisp_mcmc_cov_factor_device``: one launch, no host
    synchronisation): cov float64 [P, N, N] on a HIP device, ``scale`` a float, ``fallback_step`` [N] -> dict(factor [P, N, N] lower
    triangular - a view of the kernel's transposed layout, what ``MetropolisBatch.set_proposal`` takes -, flag [P] int32: 1 where the
    matrix could not be factored and the point got diag(fallback_step))."""
    import torch
    if cov.dtype != torch.float64 or cov.ndim != 3 or cov.shape[1] != cov.shape[2] or not 1 <= cov.shape[1] <= COV_MAX_N:
        raise ValueError(f"cov_factor: float64 [P, N, N] with 1 <= N <= {COV_MAX_N} expected, got {cov.dtype} {tuple(cov.shape)}")
    if cov.device.type != "cuda":
        raise _lib.SurfdispError("cov_factor needs a HIP device")
    P, N, _ = cov.shape
    cov = cov.contiguous()
    fb = torch.as_tensor(np.asarray(fallback_step, np.float64) if not torch.is_tensor(fallback_step) else fallback_step,
                         dtype=torch.float64, device=cov.device).contiguous()
    if tuple(fb.shape) != (N,):
        raise ValueError(f"cov_factor: fallback_step ({N},) expected, got {tuple(fb.shape)}")
    factor_t = torch.empty_like(cov)
    flag = torch.empty(P, dtype=torch.int32, device=cov.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cov.device).cuda_stream)
    with torch.cuda.device(cov.device):
        _lib.check(_lib.lib().surfdisp_mcmc_cov_factor_device(stream, P, N, _ptr(cov), ctypes.c_double(float(scale)), _ptr(fb),
                                                              _ptr(factor_t), _ptr(flag)))
    return dict(factor=factor_t.transpose(1, 2), flag=flag)


ADAPT_HEAD = 8             # doubles before the mean in a point's adaptation block (SURFDISP_MCMC_ADAPT_HEAD)
ADAPT_DEFAULTS = dict(every=10, start=20, until=None, forget=1.0, target_accept=0.25, gain=1.0, decay=0.6, min_weight=None, ridge=1e-3,
                      log_scale_bounds=(-3.0, 3.0))


def adapt_state_len(N):
    """Doubles per point of the adaptation state (include/surfdisp.h: [W, ls, k, fallbacks, wrote-cov, 0, 0, 0 | mean [N] | S [N][N]])."""
    return ADAPT_HEAD + N + N * N


def adapt_state_views(state, N):
    """dict of views into a state array / tensor [F, adapt_state_len(N)]: weight, log_scale, n_updates, fallbacks, ready [F],
    mean [F, N], scatter [F, N, N] (its upper triangle is the scatter)."""
    F = state.shape[0]
    return dict(weight=state[:, 0], log_scale=state[:, 1], n_updates=state[:, 2], fallbacks=state[:, 3], ready=state[:, 4],
                mean=state[:, ADAPT_HEAD:ADAPT_HEAD + N], scatter=state[:, ADAPT_HEAD + N:].reshape(F, N, N))


def adapt_reference(state, x, flags, step, forget=1.0, target_accept=0.25, gain=1.0, decay=0.6, min_weight=None, ridge=1e-3,
                    log_scale_bounds=(-3.0, 3.0), cov=None):
    """``surfdisp_mcmc_adapt_device`` in numpy float64, in the kernel's order of operations: ``state`` [F, adapt_state_len(N)] (None:
    the fresh state, zeros), ``x`` [F, cpp, N] the chains' states, ``flags`` [F, cpp, R] the accept flags of the window's R rows
    (None or R = 0: an empty window), ``step`` [N] -> (state', cov): cov [F, N, N] with the points that reached ``min_weight``
    (default 4 N) written and the others as in ``cov=`` (zeros without), or None when no point did."""
    x = np.asarray(x, np.float64)
    F, cpp, N = x.shape
    step = np.asarray(step, np.float64)
    min_weight = 4.0 * N if min_weight is None else float(min_weight)
    st = np.zeros((F, adapt_state_len(N))) if state is None else np.array(state, np.float64)
    v = adapt_state_views(st, N)
    up = np.triu(np.ones((N, N), bool))
    W = v["weight"] * float(forget)
    S = v["scatter"] * float(forget)
    mean = v["mean"].copy()
    for j in range(cpp):                                               # one Welford step per chain, ascending
        W = W + 1.0
        d = x[:, j] - mean
        mean = mean + d / W[:, None]
        e = x[:, j] - mean
        S = S + np.where(up, d[:, :, None] * e[:, None, :], 0.0)
    ls, k = v["log_scale"].copy(), v["n_updates"].copy()
    R = 0 if flags is None else np.asarray(flags).shape[2]
    if target_accept >= 0.0 and R > 0:
        cnt = (np.asarray(flags, np.float64) > 0.5).sum(axis=(1, 2))   # integers: exact, order-free
        a = cnt.astype(np.float64) / float(cpp * R)
        k = k + 1.0
        g = float(gain) * np.power(k, -float(decay))
        inc = g * (a - float(target_accept))
        ls = np.minimum(np.maximum(ls + inc, float(log_scale_bounds[0])), float(log_scale_bounds[1]))
    ready = W >= min_weight
    v["weight"][:], v["log_scale"][:], v["n_updates"][:], v["ready"][:] = W, ls, k, ready
    v["mean"][:], v["scatter"][:] = mean, S
    if not ready.any():
        return st, None
    out = np.zeros((F, N, N)) if cov is None else np.array(cov, np.float64)
    out[ready] = adapt_cov_formula(S[ready], W[ready], ls[ready], step, ridge)
    return st, out


def adapt_cov_formula(S, W, ls, step, ridge):
    """Step 4 of ``surfdisp_mcmc_adapt_device``: cov [F, N, N] = exp(2 ls) (2.38^2 / N_live) (S / W + ridge diag(step^2)), symmetric from the
    upper triangle of S [F, N, N]; a scalar whose diagonal is zero: a zero row and column, and not counted in N_live."""
    S, W, ls, step = (np.asarray(a, np.float64) for a in (S, W, ls, step))
    F, N, _ = S.shape
    Su = np.triu(S)
    B = (Su + np.transpose(np.triu(S, 1), (0, 2, 1))) / W[:, None, None]
    i = np.arange(N)
    B[:, i, i] = B[:, i, i] + (float(ridge) * step) * step
    live = B[:, i, i] != 0.0
    nlive = live.sum(axis=1)
    with np.errstate(divide="ignore"):
        c = np.where(nlive > 0, np.exp(2.0 * ls) * ((2.38 * 2.38) / nlive.astype(np.float64)), 0.0)
    return np.where(live[:, :, None] & live[:, None, :], c[:, None, None] * B, 0.0)


# ---------------------------------------------------------------------------------------------------------------- the proposals
def rules_args(rules, p):
    """What the prior and the redrawing propose entries take of a ``PriorRules`` for the states ``p`` [C, N]: (K, L, aux, idesc,
    fdesc, flags, vs_max) - the model's constants per chain, K columns ``aux`` [C, K] (None: K = 0), its native descriptor with L
    output layers, the rules' flags per output layer, and the Vs cap (-1.0: none)."""
    mb = rules.model
    idesc, fdesc, L = mb.native_descriptor()
    aux = mb._full(p)[:, p.shape[1]:].contiguous() if mb.n_aux else None
    return int(mb.n_aux), int(L), aux, idesc, fdesc, rules.device_flags(), -1.0 if rules.vs_max is None else rules.vs_max


def _tries(st, p, depth):
    """The retry indices of a redrawing propose kernel, uint16 [C, 2^depth - 1], in the fused buffers ``st`` (what
    ``MetropolisBatch.last_prior_tries`` returns)."""
    import torch
    shape = (p.shape[0], (1 << int(depth)) - 1)
    tries = st.get("tries")
    if tries is None or tries.shape != shape:
        tries = st["tries"] = torch.zeros(shape, dtype=torch.int16, device=p.device).view(torch.uint16)
    return tries


class ExhaustedCounter:
    """The device int the redrawing propose kernels count exhausted nodes in: one per sampler, shared by its chain groups and by
    every proposal the sampler is given; made and zeroed at its first use."""

    def __init__(self, device):
        self.device, self._t = device, None

    def tensor(self):
        if self._t is None:
            import torch
            self._t = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._t

    def count(self):
        """Synchronises once (not at all before the first use)."""
        return 0 if self._t is None else int(self._t.item())


class ReferenceSteps:
    """The reference's proposal: every scalar moves by its own bounded Gaussian step ``spec.step``.  With an ``isgood`` - a
    ``PriorRules(redraw="rounds")`` - the redraw loop of ``MCinv.perturb`` / ``reset`` (models.py:192-219) follows as masked rounds,
    on the device and without a host synchronisation: the prior kernel marks the chains whose proposal breaks a rule, the masked
    propose kernel draws those again - ``rounds`` Gaussian rounds, ``reset_rounds`` uniform ones, then the chain's own state.  The
    rounds redraw one proposal per chain: they cannot follow a tree."""

    redraws_in_kernel = False

    def __init__(self, proposer, isgood=None):
        self.proposer, self.isgood = proposer, isgood

    @property
    def max_depth(self):
        return MAX_DEPTH if self.isgood is None else 1

    def draw(self, stream, p, out, depth, counter, st, chain0):
        """The proposals ``out`` of the states ``p`` [C, N]: [C, N] a plain step, [C, 2^depth - 1, N] the tree."""
        C, N = p.shape
        L, pr = _lib.lib(), self.proposer
        if out.ndim == 2:
            _lib.check(L.surfdisp_mcmc_propose_device(stream, C, N, _ptr(p), _ptr(pr.vmin), _ptr(pr.vmax), _ptr(pr.step),
                                                      pr.seed_int, counter, 0, _ptr(out), chain0))
        else:
            _lib.check(L.surfdisp_mcmc_propose_tree_device(stream, C, N, int(depth), _ptr(p), _ptr(pr.vmin), _ptr(pr.vmax),
                                                           _ptr(pr.step), pr.seed_int, counter, _ptr(out), chain0))
        if self.isgood is not None:
            self._rounds(stream, p, out.view(C, N), counter, st, chain0)

    def _rounds(self, stream, p, p1, counter, st, chain0):
        """One tag per chain, rising from round to round (cleared once per step)."""
        import torch
        rules, pr = self.isgood, self.proposer
        C, N = p1.shape
        K, Lout, aux, idesc, fdesc, flags, vs_max = rules_args(rules, p)
        if st.get("tags") is None or st["tags"].numel() != C:
            st["tags"] = torch.zeros(C, dtype=torch.uint8, device=p.device)
        tags = st["tags"]
        L = _lib.lib()
        total = rules.rounds + rules.reset_rounds + 1
        tags.zero_()                                               # once per step: the rounds use rising tags 1, 2, ...
        for r in range(total):
            q = p1 if aux is None else torch.cat([p1, aux], dim=1)
            # round r: chains redrawn in round r - 1 carry tag r (all chains in round 0); the ones that break a rule get r + 1 ...
            _lib.check(L.surfdisp_prior_device(stream, C, N + K, Lout, _ptr(q), _ptr(idesc), _ptr(fdesc), _ptr(flags),
                                               ctypes.c_double(vs_max), r if r > 0 else -1, r + 1, _ptr(tags)))
            # ... and draw again: Gaussian rounds, then uniform prior draws, last the chain's own state
            mode = 0 if r < rules.rounds else (1 if r < rules.rounds + rules.reset_rounds else 2)
            _lib.check(L.surfdisp_mcmc_propose_masked_device(stream, C, N, _ptr(p), _ptr(pr.vmin), _ptr(pr.vmax), _ptr(pr.step),
                                                             pr.seed_int, counter, r, mode, _ptr(tags), r + 1, _ptr(p1), chain0))


class KernelRedraw:
    """``PriorRules(redraw="kernel")``: every row of the proposal tree is redrawn inside the kernel until the rules hold
    (``surfdisp_mcmc_propose_prior_device``: one launch) - ``gauss_tries`` whole-proposal Gaussian redraws, then ``uniform_tries``
    uniform ones; a node that exhausts both proposes the state it drew from and is counted."""

    redraws_in_kernel = True
    max_depth = MAX_DEPTH

    def __init__(self, proposer, isgood, exhausted):
        self.proposer, self.isgood, self.exhausted = proposer, isgood, exhausted

    def draw(self, stream, p, out, depth, counter, st, chain0):
        C, N = p.shape
        rules, pr = self.isgood, self.proposer
        K, L, aux, idesc, fdesc, flags, vs_max = rules_args(rules, p)
        _lib.check(_lib.lib().surfdisp_mcmc_propose_prior_device(
            stream, C, N, K, L, int(depth), _ptr(p), _ptr(aux), _ptr(pr.vmin), _ptr(pr.vmax), _ptr(pr.step),
            _ptr(idesc), _ptr(fdesc), _ptr(flags), ctypes.c_double(vs_max), rules.gauss_tries, rules.uniform_tries,
            pr.seed_int, counter, chain0, _ptr(out), _ptr(_tries(st, p, depth)), _ptr(self.exhausted.tensor())))


class Factor:
    """``x + F z`` (z standard normal): ``factor_t`` [F, N, N] float64 in the kernel's layout, factor_t[f][k][n] = L_f[n][k], chain
    c of the whole sampler taking factor ``c // cpf``.  Every row of the proposal tree is redrawn inside the kernel until it lies
    in the open prior box and the rules of ``isgood`` (a ``PriorRules`` in either redraw mode, or None) hold
    (``surfdisp_mcmc_propose_cov_device``: one launch), within the rules' caps or ``COV_TRIES``."""

    redraws_in_kernel = True
    max_depth = MAX_DEPTH

    def __init__(self, proposer, isgood, exhausted, factor_t, cpf):
        self.proposer, self.isgood, self.exhausted = proposer, isgood, exhausted
        self.factor_t, self.cpf, self.F = factor_t, int(cpf), int(factor_t.shape[0])

    def draw(self, stream, p, out, depth, counter, st, chain0):
        C, N = p.shape
        rules, pr = self.isgood, self.proposer
        if rules is not None:
            K, L, aux, idesc, fdesc, flags, vs_max = rules_args(rules, p)
            caps = (rules.gauss_tries, rules.uniform_tries)
        else:
            (K, L, aux, idesc, fdesc, flags, vs_max), caps = (0, 0, None, None, None, None, -1.0), COV_TRIES
        _lib.check(_lib.lib().surfdisp_mcmc_propose_cov_device(
            stream, C, N, K, L, int(depth), _ptr(p), _ptr(aux), _ptr(pr.vmin), _ptr(pr.vmax), _ptr(self.factor_t), self.cpf, self.F,
            _ptr(idesc), _ptr(fdesc), _ptr(flags), ctypes.c_double(vs_max), *caps, pr.seed_int, counter, chain0, _ptr(out),
            _ptr(_tries(st, p, depth)), _ptr(self.exhausted.tensor())))


def fused_schedule(chainL, depth):
    """The calls of a fused run of ``chainL`` rows at speculative depth ``depth``, as (first_row, nsteps, is_first): row 0 alone -
    the start models themselves, evaluated and accepted -, then ``depth`` rows per call (the last call: what is left).  Call
    number n, counted from 1, takes the Philox counter ``base + n``."""
    i = 0
    while i < chainL:
        ns = 1 if i == 0 else min(max(int(depth), 1), chainL - i)
        yield i, ns, i == 0
        i += ns


# ---------------------------------------------------------------------------------------------------------------- adaptation
class Adaptation:
    """``MetropolisBatch.set_adaptive``: the validated options (``cpp`` chains per point, ``every``, ``start``, ``until``, ``forget``,
    ``target_accept``, ``gain``, ``decay``, ``min_weight``, ``ridge``, ``ls_min``, ``ls_max``) and the state of a run - ``state`` [F,
    adapt_state_len(N)], ``cov`` [F, N, N] and ``flag`` [F] on the device, the working factors ``factor_t`` the chains propose
    with (``working``: the ``Factor`` around them while the run lasts, None otherwise), ``stop`` (the resolved ``until``), the
    weight followed on the host, the row of the previous update and the number of refactorings."""

    def __init__(self, proposer, N, exhausted, chains_per_point, every=10, start=20, until=None, forget=1.0, target_accept=0.25,
                 gain=1.0, decay=0.6, min_weight=None, ridge=1e-3, log_scale_bounds=(-3.0, 3.0)):
        if N > COV_MAX_N:
            raise ValueError(f"set_adaptive: {N} random-walk parameters, the kernel takes at most {COV_MAX_N}")
        if int(chains_per_point) < 1:
            raise ValueError("set_adaptive: chains_per_point >= 1 expected")
        if int(every) < 1 or int(start) < 0:
            raise ValueError("set_adaptive: every >= 1 and start >= 0 expected")
        if until is not None and int(until) <= int(start):
            raise ValueError("set_adaptive: until > start expected (None: half of the chain)")
        lo, hi = (float(b) for b in log_scale_bounds)
        if not (0.0 < float(forget) <= 1.0) or not float(ridge) >= 0.0 or not lo <= hi or not float(target_accept) <= 1.0:
            raise ValueError("set_adaptive: 0 < forget <= 1, ridge >= 0, log_scale_bounds (lo <= hi) and target_accept <= 1 expected")
        mw = 4.0 * N if min_weight is None else float(min_weight)
        if not mw >= 1.0:
            raise ValueError("set_adaptive: min_weight >= 1 expected")
        self.proposer, self.N, self.exhausted = proposer, int(N), exhausted
        self.cpp, self.every, self.start, self.until = int(chains_per_point), int(every), int(start), None if until is None else int(until)
        self.forget, self.target_accept, self.gain, self.decay = float(forget), float(target_accept), float(gain), float(decay)
        self.min_weight, self.ridge, self.ls_min, self.ls_max = mw, float(ridge), lo, hi
        self.state = self.cov = self.flag = self.factor_t = self.working = None
        self.stop, self.weight, self.prev, self.refactors = self.until, 0.0, None, 0

    def begin(self, C, chainL, given, isgood):
        """The fresh adaptation of a run of C chains x chainL rows: state, covariance and flag buffers, and the working factors - a
        copy of ``given``'s (the ``Factor`` of ``set_proposal``), or diag(spec.step) - which are the proposal in force until ``end``."""
        import torch
        N, dev = self.N, self.exhausted.device
        if C % self.cpp:
            raise ValueError(f"run: {C} chains are no whole number of points of {self.cpp} chains (set_adaptive)")
        F = C // self.cpp
        if given is None:
            ft = torch.diag(self.proposer.step.to(torch.float64)).expand(F, N, N).contiguous()
        elif given.F == 1:
            ft = given.factor_t.expand(F, N, N).contiguous()
        elif given.F == F and given.cpf == self.cpp:
            ft = given.factor_t.clone()
        else:
            raise ValueError(f"run: set_proposal gave {given.F} factors for {given.cpf} chains each, set_adaptive expects "
                             f"{F} points of {self.cpp} chains")
        self.state = torch.zeros((F, adapt_state_len(N)), dtype=torch.float64, device=dev)
        self.cov = torch.zeros((F, N, N), dtype=torch.float64, device=dev)
        self.flag = torch.zeros(F, dtype=torch.int32, device=dev)
        self.factor_t = ft
        self.stop = chainL // 2 if self.until is None else self.until
        self.weight, self.prev, self.refactors = 0.0, None, 0
        self.working = Factor(self.proposer, isgood, self.exhausted, ft, self.cpp)

    def end(self):
        """The run is over: the working factors are no longer in force (``report`` still shows them)."""
        self.working = None

    def due(self, lo, hi):
        """Whether an update instant lies among the steps lo .. hi - 1."""
        a, b = max(lo, self.start), min(hi, self.stop)
        if a >= b:
            return False
        first = a + (-(a - self.start)) % self.every               # the first instant >= a
        return first < b

    def update(self, p, track, chain_stride, row_stride, i):
        """The update after step i (the current stream; every group joined): the window is the rows since the previous update - at
        the first one max(1, i - every + 1) .. i, so that row 0, accepted by construction, never counts -, then the factors of all
        points once their weight - the same on every point, followed on the host - has reached ``min_weight``."""
        import torch
        N, F, dev = self.N, self.state.shape[0], self.state.device
        lo = max(1, i - self.every + 1) if self.prev is None else self.prev + 1
        self.prev = i
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        step = self.proposer.step
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().surfdisp_mcmc_adapt_device(
                stream, F, self.cpp, N, _ptr(p), _ptr(track), int(chain_stride), int(row_stride), int(lo), int(i) + 1, _ptr(step),
                self.forget, self.target_accept, self.gain, self.decay, self.ls_min, self.ls_max, self.min_weight, self.ridge,
                _ptr(self.state), _ptr(self.cov)))
            w = self.weight * self.forget                          # the kernel's own arithmetic: W is this number on every point
            for _ in range(self.cpp):
                w += 1.0
            self.weight = w
            if w >= self.min_weight:
                _lib.check(_lib.lib().surfdisp_mcmc_cov_factor_device(stream, F, N, _ptr(self.cov), ctypes.c_double(1.0), _ptr(step),
                                                                      _ptr(self.factor_t), _ptr(self.flag)))
                self.state[:, 3] += self.flag
                self.refactors += 1

    def report(self):
        """``MetropolisBatch.adaptation()``: the adaptation of the last run, device tensors (None before the first)."""
        import torch
        if self.state is None:
            return None
        v = adapt_state_views(self.state, self.N)
        S = torch.triu(v["scatter"])
        S = S + torch.triu(S, 1).transpose(1, 2)
        return dict(weight=v["weight"], mean=v["mean"], cov=S / v["weight"][:, None, None], scale=torch.exp(v["log_scale"]),
                    n_updates=v["n_updates"].to(torch.int64), fallbacks=v["fallbacks"].to(torch.int64),
                    factor=self.factor_t.transpose(1, 2))
