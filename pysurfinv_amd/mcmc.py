"""Batched, device-resident Metropolis sampler: the GPU counterpart of ``Point.misfit`` /
``Point.MCinv`` / ``Point.MCinvMP`` (``/root/reference/point.py:15-125``).

The reference advances one chain per process, one forward solve per step.  Here C chains (of one or
many grid points) advance in lock step: every step is ONE batched forward solve of C stacks through
``libsurfdisp_hip`` (root-search kernel only - the misfit uses Rayleigh phase velocity,
``point.py:11,18``), with proposals, misfit and the accept rule evaluated by torch ops on the device.
With ``data=`` (``pysurfinv_amd.obsdata``) the misfit is the joint one of Rayleigh and / or Love, phase and / or group
velocity curves: one solve per wave type with data, the group-velocity kernel only where U data exist.

Semantics kept from the reference:
* proposal: every random-walk scalar moves by a bounded Gaussian step (``brownian.py:20-27``), the
  whole proposal is redrawn while ``isgood`` rejects it (<= 1000 times, then uniform ``reset``,
  ``models.py:192-219``);
* misfit: ``chi2 = sum(((cO-cP)/uncer)**2)``, ``misfit = sqrt(chi2/N)``, ``chi2 := sqrt(50*chi2)``
  when ``chi2 >= 50``, ``L = exp(-chi2/2)``; a failed forward solve gives ``(88888, 88888, 0)``
  (``point.py:20-31``);
* accept: ``chi1 < chi0`` or ``random() > 1 - exp(-(chi1-chi0)/2)`` (``point.py:34-37``);
* a chain starts from the initial model (first chain when ``init``) or from a uniform prior draw
  (``point.py:47-57``); ``mcTrack`` rows are ``[misfit, L, accepted, *params]`` of the PROPOSED
  model (``models.py:254-256``, ``point.py:58,73-76``); output ``.npz`` keys ``mcTrack, setting,
  obs, invMeta`` (``point.py:82-85``) so ``PostPoint`` / ``Model3D.loadInvDir`` can read it.
Opt-in, beyond the reference: ``set_proposal`` replaces the independent steps by ``x + F z`` with a lower-triangular factor per grid
point (e.g. ``paramlsq.ParamLsqBatch.proposal_factor``), ``run(start=)`` starts chains at given rows (e.g. the fitted ones);
``set_adaptive`` makes that factor inside the run from the pooled states of a point's chains (adaptive Metropolis with a
Robbins-Monro scale, for any model the sampler runs; the rows before ``until`` are adaptation, no valid samples).
RNG: CPython's Mersenne Twister cannot be reproduced on the device; the production path uses a
torch Philox generator (statistical parity), and ``PythonRandomProposer`` replays the reference's
exact stream for one chain (trace parity, ``tests/test_mcmc.py``).
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import numpy as np

from . import _lib
from .brownian import ParamSpec, TorchProposer

FAIL = 88888.0                                                  # point.py:21

# the accept entries of libsurfdisp_hip: (data kind, tree walk) -> symbol (include/surfdisp.h)
_ACCEPT_ENTRIES = {
    ("c", False): "surfdisp_mcmc_accept_device", ("c", True): "surfdisp_mcmc_accept_tree_device",
    ("joint", False): "surfdisp_mcmc_accept_joint_device", ("joint", True): "surfdisp_mcmc_accept_tree_joint_device",
    ("joint5", False): "surfdisp_mcmc_accept_joint5_device", ("joint5", True): "surfdisp_mcmc_accept_tree_joint5_device",
}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _accept_rule(torch, chi0, chi1, u):
    """bool[C]: ``chi1 < chi0`` or ``u > 1 - exp(-(chi1 - chi0) / 2)`` (point.py:34-37).  Pure tensor code: no host
    synchronisation, so it can be captured in a HIP graph."""
    better = chi1 < chi0
    return better | (~better & (u > 1.0 - torch.exp(-(chi1 - chi0) / 2.0)))


def _put_row(track, i, mis, L, acc, p):
    """mcTrack row ``i`` of every chain: [misfit, L, accepted, *params] of the proposed model (models.py:254-256)."""
    track[:, i, 0] = mis; track[:, i, 1] = L; track[:, i, 2] = acc; track[:, i, 3:] = p


# (the proposals, the adaptation and their numpy statements live in .proposal; every public name is re-exported here)
from .proposal import (ADAPT_DEFAULTS, ADAPT_HEAD, COV_MAX_N, COV_TRIES, MAX_DEPTH, Adaptation, ExhaustedCounter, Factor,    # noqa: F401
                       KernelRedraw, ReferenceSteps, adapt_cov_formula, adapt_reference, adapt_state_len, adapt_state_views,
                       cov_factor, cov_factor_reference, fused_schedule, rules_args)


class PriorRules:
    """The GENERIC prior predicates the reference's model classes build ``isgood`` from (models.py:294-320), in a form the
    device can evaluate (csrc/surfdisp_layers.hip::surfdisp_prior_kernel) - pass it as ``MetropolisBatch(isgood=...)`` and
    the lock step stays on the device (fused kernels, chain groups, HIP graphs):

    * ``monotone_groups``: Vs must increase with depth over the grid points of these layer groups ("sediment", "crust", ...:
      ``monoIncrease``, models.py:8-9, 315-320);
    * ``positive_jumps``: Vs must not drop across a boundary between two groups (models.py:302-307);
    * ``vs_max``: every grid point's Vs at most this (models.py:309-313; None: no cap).

    The reference redraws the WHOLE proposal until the predicate holds (``MCinv.perturb``: 1000 tries, then ``reset``'s uniform
    draws, models.py:192-219).  On the device the same loop runs as MASKED redraw rounds without a host synchronisation:
    ``rounds`` Gaussian rounds (only the chains whose proposal broke a rule draw again), then ``reset_rounds`` rounds of uniform
    prior draws, and a chain that is still without a good proposal proposes its own state (a wasted step: with a prior that
    accepts half of the Gaussian draws, 1 chain in 60 reaches the uniform rounds and fewer than 1 in 1e3 the wasted step).  Called with a parameter tensor it evaluates
    the same rules in torch on ``Model1DBatch.seis_prop_grids`` (the torch lock step; the tests compare the two).
    ``redraw="kernel"`` runs the reference's own loop instead, inside one kernel per lock step (``surfdisp_mcmc_propose_prior_device``):
    ``gauss_tries`` whole-proposal Gaussian redraws, then ``uniform_tries`` uniform ones, at every node of the speculative tree too;
    a chain that exhausts both proposes its own state and is counted (``MetropolisBatch.prior_exhausted``)."""

    MAX_TRIES = 16384               # gauss_tries + uniform_tries: the retry index has 14 bits of the random streams' index

    def __init__(self, model, monotone_groups=("sediment", "crust"), positive_jumps=True, vs_max=None, rounds=5, reset_rounds=2,
                 redraw="rounds", gauss_tries=1000, uniform_tries=10000):
        self.model = model
        self.monotone_groups = tuple(monotone_groups)
        self.positive_jumps = bool(positive_jumps)
        self.vs_max = None if vs_max is None else float(vs_max)
        self.rounds, self.reset_rounds = int(rounds), int(reset_rounds)
        if redraw not in ("rounds", "kernel"):
            raise ValueError("PriorRules: redraw must be 'rounds' or 'kernel'")
        self.redraw = redraw
        self.gauss_tries, self.uniform_tries = int(gauss_tries), int(uniform_tries)
        if self.gauss_tries < 0 or self.uniform_tries < 0 or not 1 <= self.gauss_tries + self.uniform_tries <= self.MAX_TRIES:
            raise ValueError(f"PriorRules: gauss_tries >= 0, uniform_tries >= 0 and 1 <= their sum <= {self.MAX_TRIES}")
        self._flags = None

    def __call__(self, params, rows=None):
        return self.model.prior_good(params, self, rows=rows)

    def device_flags(self):
        """int32 [L] flags for the prior kernel, or None (no native descriptor / thermal layer: the torch loop serves)."""
        if self._flags is None:
            self._flags = self.model.prior_flags(self)
        return self._flags


class ChainGroups:
    """The chains of a ``MetropolisBatch`` as contiguous groups, each advancing on its own stream (``chain_groups``).
    ``fork()`` once (the group streams wait for the current stream), ``step()`` per lock step, ``join()`` once (the current
    stream waits for every group): between the two nothing synchronises the groups with each other."""

    def __init__(self, mc, C, G):
        import copy
        torch = mc.torch
        self.mc, self.C, self.G = mc, int(C), int(G)
        self.bounds = [self.C * g // self.G for g in range(self.G + 1)]
        self.streams = [torch.cuda.Stream(device=mc.device) for _ in range(self.G)]
        self.children, self._obs = [], None
        for g in range(self.G):
            ch = copy.copy(mc)                                  # shares spec, proposer (bounds, steps, seed), periods, to_model
            ch._fresh_state()                                   # (its own plans, fused buffers, counters, Love stream)
            ch._pipelined = True                                # the library sizes its teams for both groups' stacks
            self.children.append(ch)
        self._refresh()

    def _refresh(self):
        """The children's slices of the parent's observations / local rows and its run-time switches, taken at construction and
        afresh at every fork: a parent whose observations or ``local_rows`` were replaced, or whose ``independent`` / ``fast_scan`` changed after
        a first grouped run, must not advance on the first run's copies."""
        mc = self.mc
        obs = (mc.c_obs, mc.uncer, mc.mask)
        sliced = self._obs is not None and all(a is b for a, b in zip(obs, self._obs))     # the children hold slices of these already
        self._obs = obs
        pr = mc.proposal()                                      # one object for all groups, its factors indexed by the chain's
        if pr.redraws_in_kernel:                                # index in the whole sampler, and one counter, zeroed before the fork
            pr.exhausted.tensor()
        for g, ch in enumerate(self.children):
            lo, hi = self.bounds[g], self.bounds[g + 1]
            if mc.c_obs.ndim == 2 and mc.c_obs.shape[0] != self.C:
                raise ValueError(f"{self.C} chains against {mc.c_obs.shape[0]} rows of observations")
            if not sliced:                                      # (new tensors: _fused_buffers then makes the child's buffers anew)
                ch.c_obs, ch.uncer, ch.mask = (a[lo:hi] for a in obs) if mc.c_obs.ndim == 2 else obs
            ch.local_rows = None if mc.local_rows is None else mc.local_rows[lo:hi]
            ch.independent, ch.fast_scan, ch.isgood = mc.independent, mc.fast_scan, mc.isgood
            ch.joint, ch.periods = mc.joint, mc.periods
            ch._chain0 = mc._chain0 + lo
            ch._shared = pr

    def fork(self):
        self._refresh()
        cur = self.mc.torch.cuda.current_stream(self.mc.device)
        for s in self.streams:
            s.wait_stream(cur)
        self.children[0].event_ring, self.children[0]._ev_i = self.mc.event_ring, self.mc._ev_i    # bench.py's measurement hook

    def step(self, p, row=None, row_stride=0, row_offset=0, first=False, counter=None):
        """One Metropolis step of every chain: state ``p`` [C, N] in place, rows as ``MetropolisBatch.fused_step``."""
        torch = self.mc.torch
        if counter is None:
            self.mc._counter += 1
            counter = self.mc._counter
        for g, ch in enumerate(self.children):
            lo, hi = self.bounds[g], self.bounds[g + 1]
            with torch.cuda.stream(self.streams[g]):
                ch.fused_step(p[lo:hi], row=row, row_stride=row_stride, row_offset=row_offset + lo * row_stride,
                              first=first, counter=counter)

    def join(self):
        cur = self.mc.torch.cuda.current_stream(self.mc.device)
        for s in self.streams:
            cur.wait_stream(s)
        for ch in self.children:
            self.mc.n_forward += ch.n_forward
            ch.n_forward = 0
        self.mc._ev_i = self.children[0]._ev_i
        self.children[0].event_ring = None


class MetropolisBatch:
    """C chains in lock step.

    to_model(params[C, N] float64 tensor) -> (model[C, 5, L] float32 tensor, nlay[C] int32 or None)
    isgood(params) -> bool[C] tensor (None: always good, ``MCinv.isgood`` default, models.py:220-224)
    c_obs, uncer: [P] or [C, P]; entries with uncer <= 0 or NaN c_obs are masked out (the
    reference uses a masked array, point.py:23-26).
    data: instead of (periods, c_obs, uncer), a list of ``obsdata.DispersionData`` - Rayleigh and / or Love, phase and / or
    group velocity, each [P_d] or [C, P_d] - fitted jointly (the misfit, period lists and failure rule of
    ``pysurfinv_amd.obsdata``): one solve per wave type and lock step, both from the one ``to_model`` output.
    """

    AUTO_INDEP_CHAINS = 3072        # 64-lane teams of fewer chains leave the chip's 196 608 lanes partly empty
    COUNTER_LIMIT = 1 << 40         # Philox call counters stay below: from 2^40 on the counter's high word reaches the bits of the stream tags
    PLAN_CACHE = 8             # plans kept: the speculative lock step alternates between two stack counts, two wave types each

    def __init__(self, spec: ParamSpec, to_model, periods=None, c_obs=None, uncer=None, device="cuda:0",
                 isgood=None, proposer=None, seed=None, forward=None, independent=False, fast_scan=False,
                 local_rows=None, data=None):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.spec = spec
        self.to_model = to_model
        self.isgood = isgood
        self.proposer = proposer if proposer is not None else TorchProposer(spec, self.device, seed)
        self.joint = None
        self._fresh_state()
        if data is not None:
            if periods is not None or c_obs is not None or uncer is not None:
                raise ValueError("MetropolisBatch: pass either data= or (periods, c_obs, uncer), not both")
            self.data = data
        else:
            if periods is None or c_obs is None or uncer is None:
                raise ValueError("MetropolisBatch: needs (periods, c_obs, uncer) or data=")
            self.periods = torch.as_tensor(np.asarray(periods, np.float32), device=self.device)
            self._set_obs(c_obs, uncer)
        # test hook: callable(model, nlay) -> (c, status); with data=: -> dict(cR, uR, cL, uL, statusR, statusL)
        self._forward = forward
        # independent=True: period-parallel root search (SURFDISP_INDEPENDENT) - lower latency for few
        # chains; only for smooth parameterisations (no low-velocity roughness), see include/surfdisp.h.
        # independent="auto": that decomposition whenever the lock step is too small to fill the chip with whole-stack
        # teams (fewer than AUTO_INDEP_CHAINS chains: 100 chains x 96 layers take 0.92 ms per step in the faithful period
        # walk - a 19-period dependent chain on 100 of 4 096 wavefront slots - against 0.3 ms), the faithful walk
        # otherwise.  NOT the default: the two agree to 4e-6 with identical zero patterns on 40 000 prior draws of the
        # continental and the thermal model (scripts/indep_vs_faithful.py, profiles/r03a), but on rough stacks the
        # reference's answer depends on its period list (start rule 0.9 c(k-1), stale deep layers: up to 2.4e-3,
        # tests/test_gpu_parity.py) and a default must not change results with the number of chains.
        if independent not in (True, False, "auto"):
            raise ValueError("independent must be True, False or 'auto'")
        self.independent = independent
        # fast_scan=True: opt into the count-guided coarse-to-fine scan (SURFDISP_FASTSCAN); the default walks every
        # grid point of the reference's scan, so root selection and failures are the reference's on every input
        self.fast_scan = bool(fast_scan)
        # local_rows [C]: row of the model's per-point local-information table (Model1DBatch.set_local_info) each chain
        # belongs to; to_model is then called as to_model(params, rows)
        self.local_rows = None if local_rows is None else torch.as_tensor(np.asarray(local_rows), dtype=torch.int64,
                                                                          device=self.device)
        self._counter = 0                                       # calls of the fused kernels so far: the Philox counter of the next one
        self._pipelined = False                                 # a chain group: another group's solve is in flight beside this one
        self._chain0 = 0                                        # index of this object's chain 0 in the whole sampler (chain groups)
        self._exh = ExhaustedCounter(self.device)               # what the redrawing propose kernels count in, shared with the chain groups
        self._given = None                                      # set_proposal: a proposal.Factor
        self._steps = None                                      # the proposal made from isgood (proposal())
        self._shared = None                                     # a chain group's child: the proposal its parent had in force at the fork
        self._last_groups = None                                # the ChainGroups of the last run (last_prior_tries)
        self._adaptation = None                                 # set_adaptive: a proposal.Adaptation
        self._adapted = None                                    # the Adaptation of the last run that adapted (adaptation())

    def _fresh_state(self):
        """What a sampler owns and a chain group's child (a shallow copy of its parent) must not share with it."""
        self._plans = {}                                        # (C, L, P, wave) -> forward.BatchPlan
        self._fz = None                                         # the fused path's buffers (_fused_buffers)
        self._groups = {}
        self._side = None                                       # joint data, one chain group: the Love solve's stream
        self.n_forward = 0
        # measurement hook (bench.py): a forward.EventRing whose next slot brackets the solver's kernels of each call
        self.event_ring = None
        self._ev_i = 0

    def _set_obs(self, c_obs, uncer):
        torch = self.torch
        co = torch.as_tensor(np.asarray(c_obs, np.float64), device=self.device)
        un = torch.as_tensor(np.asarray(uncer, np.float64), device=self.device)
        self.mask = torch.isfinite(co) & torch.isfinite(un) & (un > 0)
        self.c_obs = torch.where(self.mask, co, torch.zeros_like(co))
        self.uncer = torch.where(self.mask, un, torch.ones_like(un))

    @property
    def data(self):
        """The ``DispersionData`` sets of a joint sampler (None: the (periods, c_obs, uncer) form).  Assigning a new list
        replaces the observations (``c_obs`` / ``uncer`` / ``mask`` are then their concatenated columns, [Ptot] or [C, Ptot]);
        the fused path's buffers are keyed on the data object, so the next lock step uses the new data."""
        return None if self.joint is None else self.joint.datasets

    @data.setter
    def data(self, data):
        from .obsdata import JointData
        self.joint = JointData(data, device=self.device)
        self.periods = None
        self._set_obs(self.joint.obs_raw, self.joint.uncer_raw)
        self._fz = None

    # ------------------------------------------------------------------ forward + misfit
    def forward_c(self, params, rows=None):
        """Rayleigh phase velocities c[C, P] and status[C] for the stacks of ``params`` (``rows``: the chain each row
        of ``params`` belongs to, when it is not simply row i = chain i)."""
        model, nlay = self._stacks(params, rows)
        if self._forward is not None:
            self.n_forward += model.shape[0]
            return self._forward(model, nlay)
        if self.joint is not None:
            return self._solve_joint(model, nlay)
        c, st = self._solve_model(model, nlay)
        return c.to(self.torch.float64), st

    def _stacks(self, params, rows=None):
        """(model[C, 5, L], nlay) of ``to_model`` for the rows of ``params``, each with the local information of its chain."""
        if self.local_rows is None:
            return self.to_model(params)
        if rows is None and params.shape[0] != self.local_rows.shape[0]:
            raise ValueError(f"{params.shape[0]} models against {self.local_rows.shape[0]} chains with local information: pass rows=")
        return self.to_model(params, self.local_rows if rows is None else self.local_rows[rows])

    def forward_joint(self, params, rows=None):
        """Joint data: dict(cR, uR, cL, uL, statusR, statusL, eR) of the stacks of ``params`` (None for a wave type without
        data; a wave type without U data is solved phase-only, its u is not meaningful).  eR: the ellipticity of the Rayleigh
        solve (``BatchPlan.run(want_ratio=True)``) when there is an ellipticity data set, None otherwise."""
        if self.joint is None:
            raise ValueError("forward_joint needs a sampler built with data=")
        return self.forward_c(params, rows)

    def misfit(self, params, rows=None, return_c=False):
        """(misfit, chiSqr, L) per row of ``params`` - point.py:15-31.  With per-chain observations (``c_obs``
        [C, P]) row i of ``params`` is compared with observation row i, or with row ``rows[i]`` when ``rows`` (an
        index tensor) is given - the speculative sampler evaluates several proposals per chain, the grid driver
        one average model per point."""
        torch = self.torch
        if self.joint is not None:                              # cP: the predictions of the observation columns
            cP, failed = self.joint.predictions(self.forward_joint(params, rows))
        else:
            cP, st = self.forward_c(params, rows)
            failed = (st != 0) | (cP < 0.01).any(dim=1)        # models.py:29-33
        c_obs, uncer, mask = self.c_obs, self.uncer, self.mask
        if c_obs.ndim == 2:
            if rows is not None:
                c_obs, uncer, mask = c_obs[rows], uncer[rows], mask[rows]
            elif c_obs.shape[0] != cP.shape[0]:
                raise ValueError(f"{cP.shape[0]} models against {c_obs.shape[0]} rows of observations: pass rows=")
        r = torch.where(mask, (c_obs - cP) / uncer, torch.zeros_like(cP))
        chi = (r * r).sum(dim=1) if self.joint is None else (self.joint.weights * r * r).sum(dim=1)
        N = mask.sum(dim=-1).to(torch.float64)
        mis = torch.sqrt(chi / N)
        chi = torch.where(chi < 50, chi, torch.sqrt(chi * 50.0))
        L = torch.exp(-0.5 * chi)
        big = torch.full_like(chi, FAIL)
        out = (torch.where(failed, big, mis), torch.where(failed, big, chi),
               torch.where(failed, torch.zeros_like(L), L))
        return out + (cP,) if return_c else out

    # ------------------------------------------------------------------ fused device path (csrc/surfdisp_mcmc.hip)
    def fused_available(self):
        """The lock step can run as propose kernel -> stacks -> solver -> accept kernel (no torch glue, no host
        synchronisation): device proposer, the HIP forward path, and no ``isgood`` callback - or a ``PriorRules`` one, whose
        redraw loop runs on the device too (``proposal.ReferenceSteps``, or ``proposal.KernelRedraw`` with ``redraw="kernel"``)."""
        dev_prior = self.isgood is None or (isinstance(self.isgood, PriorRules) and self.device.type == "cuda"
                                            and self.local_rows is None and self.isgood.device_flags() is not None)
        return (dev_prior and isinstance(self.proposer, TorchProposer) and self.device.type == "cuda"
                and self._forward is None)

    def _fused_buffers(self, C):
        """The fused path's buffers of C chains: made anew whenever C, the joint data or one of the ``c_obs`` / ``uncer`` / ``mask``
        tensors is no longer the object they were made from (they hold contiguous copies of the three)."""
        torch = self.torch
        st = self._fz
        made = (self.joint, self.c_obs, self.uncer, self.mask)
        if st is None or st["C"] != C or any(a is not b for a, b in zip(made, st["made"])):
            N = self.spec.n
            st = dict(C=C, made=made, p1=torch.empty((C, N), dtype=torch.float64, device=self.device),
                      chi=torch.zeros(C, dtype=torch.float64, device=self.device),
                      mask8=self.mask.to(torch.uint8).contiguous(), c_obs=self.c_obs.contiguous(), uncer=self.uncer.contiguous())
            self._fz = st
        return st

    # ------------------------------------------------------------------ the proposal in force
    def proposal(self):
        """The proposal in force now (``pysurfinv_amd.proposal``): the working factors of the adaptation while an adaptive run is in
        progress, else ``set_proposal``'s factors, else the kernel redraw if ``isgood`` is a ``PriorRules(redraw="kernel")``, else
        the reference's steps (with the redraw rounds of a ``PriorRules``).  A chain group's child: its parent's."""
        if self._shared is not None:
            return self._shared
        ad, isgood = self._adaptation, self.isgood
        pr = ad.working if ad is not None and ad.working is not None else self._given
        if pr is not None:
            pr.isgood = isgood                                     # (isgood may be assigned after set_proposal)
            return pr
        pr = self._steps
        if pr is None or pr.isgood is not isgood:
            kernel = isinstance(isgood, PriorRules) and isgood.redraw == "kernel"
            pr = self._steps = KernelRedraw(self.proposer, isgood, self._exh) if kernel else ReferenceSteps(self.proposer, isgood)
        return pr

    def prior_exhausted(self):
        """How many proposals of this sampler (tree nodes of all fused lock steps so far) found no model the prior accepts within
        ``gauss_tries + uniform_tries`` redraws and proposed the state they drew from - where the reference raises
        ``RuntimeError`` (models.py:219) - with a proposal factor (``set_proposal``): within the caps of ``proposal.Factor``, box
        included.  0 for every other redraw mode.  Synchronises once; ``run()`` itself never does."""
        return self._exh.count()

    def last_prior_tries(self):
        """uint16 [C, M]: the retry index every proposal of the last fused lock step was accepted at by the prior (M = 2^depth - 1
        tree nodes, 1 for a plain step; ``gauss_tries + uniform_tries``: exhausted), or None before the first such step."""
        torch = self.torch
        owners = self._last_groups.children if self._last_groups is not None else [self]
        ts = [o._fz.get("tries") if o._fz is not None else None for o in owners]
        if any(t is None for t in ts):
            return None
        return ts[0] if len(ts) == 1 else torch.cat([t.view(torch.int16) for t in ts], dim=0).view(torch.uint16)

    # ------------------------------------------------------------------ covariance-shaped proposals
    def set_proposal(self, factor, chains_per_point=1):
        """Proposals ``x + F z`` (z standard normal) in place of the reference's independent steps ``spec.step``: ``factor`` is a
        float64 device tensor, lower triangular (the strict upper triangle is not read), [N, N] for every chain or [n_points, N, N]
        with chain c taking ``factor[c // chains_per_point]`` (the chain order of ``run_points``) - e.g. the Cholesky factor of a
        scaled Laplace covariance, ``ParamLsqBatch.proposal_factor``.  It is transposed once into the kernel's layout
        (``surfdisp_mcmc_propose_cov_device``).  ``None`` returns to the reference's proposal: the sampler then launches the kernels
        and draws the numbers of one that was never given a factor (and turns ``set_adaptive`` off, which proposes with a factor too).

        The whole proposal is redrawn inside the kernel while it leaves the open prior box or breaks the rules of a ``PriorRules``
        (either ``redraw`` mode; its ``gauss_tries`` / ``uniform_tries``, 1000 / 10000 without rules), at every node of the
        speculative tree; ``prior_exhausted()`` and ``last_prior_tries()`` report for this kernel too.  Like the reference's
        per-scalar redraw, redrawing into the box makes the proposal slightly asymmetric near the walls; no correction is applied.
        Needs the fused path: ValueError otherwise."""
        torch = self.torch
        if factor is None:
            self._given = None
            self._adaptation = None                                # (adaptation proposes with a factor: off with it)
            return
        N = self.spec.n
        if not torch.is_tensor(factor) or factor.dtype != torch.float64 or factor.ndim not in (2, 3) or tuple(factor.shape[-2:]) != (N, N):
            raise ValueError(f"set_proposal: a float64 tensor [{N}, {N}] or [n_points, {N}, {N}] expected, got "
                             f"{getattr(factor, 'dtype', type(factor).__name__)} {tuple(getattr(factor, 'shape', ()))}")
        if N > COV_MAX_N:
            raise ValueError(f"set_proposal: {N} random-walk parameters, the kernel takes at most {COV_MAX_N}")
        if int(chains_per_point) < 1:
            raise ValueError("set_proposal: chains_per_point >= 1 expected")
        self._require_cov_path("set_proposal")
        if factor.device != self.device:
            raise ValueError(f"set_proposal: the factor lives on {factor.device}, the sampler on {self.device}")
        ft = torch.tril(factor).transpose(-1, -2).contiguous()     # factor_t[f][k][n] = L_f[n][k]
        ft, cpf = (ft[None], 1 << 62) if factor.ndim == 2 else (ft, chains_per_point)
        self._given = Factor(self.proposer, self.isgood, self._exh, ft, cpf)

    def _require_cov_path(self, who):
        """ValueError unless the propose kernel of ``set_proposal`` / ``set_adaptive`` can serve this sampler."""
        if self.isgood is not None and not (isinstance(self.isgood, PriorRules) and self.isgood.device_flags() is not None):
            raise ValueError(f"{who}: isgood must be None or a PriorRules the device can evaluate (an arbitrary callback cannot "
                             "run inside the propose kernel)")
        if self.isgood is not None and self.local_rows is not None:
            raise ValueError(f"{who}: PriorRules together with local_rows are not evaluated inside the propose kernel")
        if not self.fused_available():
            raise ValueError(f"{who} needs the fused device path: a HIP device, the device proposer and the HIP forward path")

    # ------------------------------------------------------------------ adaptive proposals
    def set_adaptive(self, chains_per_point, every=10, start=20, until=None, forget=1.0, target_accept=0.25, gain=1.0, decay=0.6,
                     min_weight=None, ridge=1e-3, log_scale_bounds=(-3.0, 3.0)):
        """Adaptive Metropolis (Haario et al. 2001) pooled over the ``chains_per_point`` chains of every grid point (the chain order
        of ``run_points``), inside ``run()`` / ``run_points()`` and without a host synchronisation: after step i with ``start <= i <
        until`` and ``(i - start) % every == 0`` the chains' current states update the point's running mean and scatter (weights
        times ``forget`` per update), the accept rate a of the rows since the previous update moves the log scale by
        ``gain k^-decay (a - target_accept)`` (k-th update; kept within ``log_scale_bounds``; ``target_accept < 0``: the scale stays
        1), and once the weight has reached ``min_weight`` (None: 4 N) the point proposes ``x + F z`` with F F^T = scale^2 2.38^2 / N
        (S / W + ridge diag(step^2)) (``surfdisp_mcmc_adapt_device`` -> ``surfdisp_mcmc_cov_factor_device``; a matrix that cannot be
        factored: the reference's steps, counted).  Until a point first refactors it proposes with the factor given by
        ``set_proposal`` before this call, or with diag(spec.step) through the same kernel.  ``until=None``: ``chainL // 2``.
        On the speculative path an update that falls due inside a tree call happens once, at the call's end; with chain groups the
        groups join for the update and fork again.

        WHAT IS A SAMPLE.  While the proposal adapts the chain is not a Markov chain with the posterior as its fixed distribution:
        the rows before ``until`` are adaptation (burn-in) and no valid sample.  From row ``until`` on the factor is frozen, and the
        rows come from a fixed Metropolis kernel as with ``set_proposal``.

        Needs the fused path and the ``isgood`` conditions of ``set_proposal`` (ValueError otherwise, and in ``run_graphed``).  Any
        model the sampler runs qualifies - a thermal layer, H/V data, models without rules.  ``set_adaptive(None)`` and
        ``set_proposal(None)`` turn it off: the sampler then launches the kernels and draws the numbers it did before.
        ``adaptation()`` reports; the state is reset at the start of every run."""
        if chains_per_point is None:
            self._adaptation = None
            return
        ad = Adaptation(self.proposer, self.spec.n, self._exh, chains_per_point, every, start, until, forget, target_accept, gain, decay,
                        min_weight, ridge, log_scale_bounds)
        self._require_cov_path("set_adaptive")
        self._adaptation = ad

    def adaptation(self):
        """The adaptation of the last run, device tensors (None before the first): weight [F], mean [F, N], cov [F, N, N] (S / W,
        symmetric), scale [F] (exp of the log scale), n_updates [F], fallbacks [F] (refactorings that kept the reference's steps),
        factor [F, N, N] (lower triangular: the view ``cov_factor`` returns, of the factors the chains proposed with last)."""
        return None if self._adapted is None else self._adapted.report()

    def _solve_raw(self, params, rows=None):
        """The solver's own fp32 output tensors (no copies) for the stacks of ``params``: (c[C, P], status[C]), or with joint
        data the dict of ``_solve_joint``."""
        model, nlay = self._stacks(params, rows)
        return self._solve_joint(model, nlay) if self.joint is not None else self._solve_model(model, nlay)

    def _plans_for(self, C, L, waves):
        """The ``BatchPlan`` of C stacks x L layers for each (wave, periods) of ``waves``.  The cache is emptied when it would
        grow beyond ``PLAN_CACHE`` plans - after the new ones are counted, so the plans of one lock step always stay together."""
        keys = [(C, L, P, w) for w, P in waves]
        try:
            return [self._plans[k] for k in keys]
        except KeyError:
            from .forward import BatchPlan
            new = [k for k in keys if k not in self._plans]
            if len(self._plans) + len(new) > self.PLAN_CACHE:
                self._plans.clear()
                new = keys
            for k in new:
                self._plans[k] = BatchPlan(C, L, k[2], device=self.device)
            return [self._plans[k] for k in keys]

    def _next_events(self):
        """The next slot of ``event_ring`` (None without a ring)."""
        if self.event_ring is None:
            return None
        self._ev_i += 1
        return self.event_ring.slot(self._ev_i - 1)

    def _indep(self, C):
        """Whether a solve of C stacks takes the period-parallel root search (``independent``)."""
        return (C < self.AUTO_INDEP_CHAINS) if self.independent == "auto" else bool(self.independent)

    def _solve_model(self, model, nlay):
        self.n_forward += model.shape[0]
        C, _, L = model.shape
        plan, = self._plans_for(C, L, [("R", self.periods.numel())])
        c, _, st = plan.run(model.contiguous(), self.periods, kind=_lib.KIND_RAYLEIGH | _lib.PHASE_ONLY,
                            nlay=nlay, independent=self._indep(C), fast_scan=self.fast_scan, events=self._next_events(),
                            pipelined=self._pipelined)
        return c, st

    def _solve_joint(self, model, nlay):
        """Joint data: one solve per wave type with data, both on the same stacks -> dict(cR, uR, cL, uL, statusR, statusL, eR)
        of the solver's own fp32 output tensors (None for a wave type without data; eR, the Rayleigh solve's ellipticity, only
        with an ellipticity data set: that solve then runs with ``want_ratio``).  Kind flags: ``JointData.kind`` (phase
        only unless the wave type has U data), ``independent`` / ``fast_scan`` as for the Rayleigh-only sampler.  Two solves:
        SURFDISP_PIPELINED for both; as one chain group the Love solve runs on a second stream forked from, and joined back
        into, the current one (as ``forward.JointPlan``; no host synchronisation), inside a chain group after the Rayleigh
        solve on the group's stream.  ``n_forward`` counts stacks (models), not solves."""
        torch = self.torch
        jd = self.joint
        self.n_forward += model.shape[0]
        C, _, L = model.shape
        model = model.contiguous()
        ev, indep = self._next_events(), self._indep(C)
        plans = self._plans_for(C, L, [(w, jd.solve_periods[w].size) for w in jd.waves])
        two = len(jd.waves) == 2
        fork = two and not self._pipelined
        cur = torch.cuda.current_stream(self.device)
        if fork:                                               # (after the plans' allocation: their zero fills run on cur)
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.device)
            self._side.wait_stream(cur)
        out = dict(cR=None, uR=None, cL=None, uL=None, statusR=None, statusL=None, eR=None)
        for i, (w, plan) in enumerate(zip(jd.waves, plans)):
            with (torch.cuda.stream(self._side) if (fork and i == 1) else contextlib.nullcontext()):
                res = plan.run(model, jd.periods_t[w], kind=jd.kind(w), nlay=nlay, independent=indep,
                               fast_scan=self.fast_scan, events=ev if i == 0 else None,
                               pipelined=self._pipelined or two, want_ratio=jd.with_ratio and w == "R")
            out["c" + w], out["u" + w], out["status" + w] = res[:3]
            if len(res) > 3:
                out["eR"] = res[3]
        if fork:
            cur.wait_stream(self._side)
        return out

    def _joint_table(self, pred, st, C):
        """The arguments of the joint accept entries that describe the solves of ``pred`` and the observation columns."""
        jd = self.joint
        if st["c_obs"].shape[-1] != jd.Ptot or (st["c_obs"].ndim == 2 and st["c_obs"].shape[0] != C):
            raise ValueError(f"joint accept: observations of shape {tuple(st['c_obs'].shape)} against {C} chains x {jd.Ptot} columns")
        arrs = [pred["cR"], pred["uR"] if jd.with_group.get("R") else None,
                pred["cL"], pred["uL"] if jd.with_group.get("L") else None]
        if jd.with_ratio:
            if pred.get("eR") is None:
                raise ValueError("joint accept: an ellipticity data set, but the Rayleigh solve returned no ratio")
            arrs.append(pred["eR"])
        for a in arrs:
            if a is not None and (a.dtype != self.torch.float32 or a.stride(1) != 1):
                raise ValueError("joint accept: predictions must be float32 rows of the solver's outputs")
        predp = (ctypes.c_void_p * len(arrs))(*[a.data_ptr() if a is not None else None for a in arrs])
        strides = (ctypes.c_long * len(arrs))(*[a.stride(0) if a is not None else 0 for a in arrs])
        nper = (ctypes.c_int * 2)(*[int(jd.solve_periods[w].size) if w in jd.solve_periods else 0 for w in ("R", "L")])
        stat = (ctypes.c_void_p * 2)(*[pred["status" + w].data_ptr() if pred["status" + w] is not None else None
                                       for w in ("R", "L")])
        return (predp, strides, nper, stat, jd.Ptot, _ptr(jd.cols), _ptr(jd.weights))

    def _accept(self, stream, pred, st, p1, p, rowp, row_stride, counter, tree, first=False, depth=1, nsteps=1, step_stride=0):
        """The accept kernel on the solve ``pred`` (``_solve_raw``) of the proposals ``p1``: misfit, accept rule, state ``p`` and
        chi-square update, mcTrack rows.  ``tree``: the tree entries (``nsteps`` steps through the tree ``p1`` of ``depth``, rows
        ``step_stride`` doubles apart; with joint data a tree of depth 1 goes through the plain entry); joint data: the joint
        entries, with an ellipticity set their five-array forms."""
        C, N = p.shape
        if self.joint is not None:
            tree = tree and depth > 1
        if self.joint is None:
            c, status = pred
            kind, head, table = "c", (int(self.periods.numel()),), (_ptr(c), _ptr(status))
        else:
            kind, head, table = "joint5" if self.joint.with_ratio else "joint", (), self._joint_table(pred, st, C)
        entry = getattr(_lib.lib(), _ACCEPT_ENTRIES[kind, tree])
        _lib.check(entry(stream, C, N, *head, *((int(depth), int(nsteps)) if tree else ()), *table,
                         _ptr(st["c_obs"]), _ptr(st["uncer"]), _ptr(st["mask8"]), 1 if st["c_obs"].ndim == 2 else 0,
                         _ptr(p1), _ptr(p), _ptr(st["chi"]), rowp, int(row_stride), *((int(step_stride),) if tree else ()),
                         self.proposer.seed_int, counter, *(() if tree else (1 if first else 0,)), self._chain0))

    def _fused_call(self, C, row, row_offset, counter):
        """What one launch sequence of the fused path starts from: the buffers, the current stream, this step's Philox
        counter (default: one more than the last call's) and the address of chain 0's mcTrack row."""
        if counter is None:
            self._counter += 1
            counter = self._counter
        if not 0 <= counter < self.COUNTER_LIMIT:
            raise OverflowError(f"Philox call counter {counter}: the kernels' streams are distinct below 2^40 lock steps only")
        st = self._fused_buffers(C)
        stream = ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)
        rowp = ctypes.c_void_p(row.data_ptr() + 8 * int(row_offset) if row is not None else 0)
        return st, stream, counter, rowp

    def fused_step(self, p, row=None, row_stride=0, first=False, counter=None, row_offset=0):
        """One Metropolis step of every chain, in place on the state ``p`` [C, N] (float64, contiguous): proposal
        (``first``: none - the states themselves are evaluated and accepted, a chain's first row), stacks, forward solve,
        misfit / accept / update.  ``row``: a float64 tensor whose element ``row_offset`` is where chain 0's mcTrack row
        goes, chain c's ``row_stride`` doubles further.  ``counter``: the Philox counter of this step (default: one more
        than the last call's).  Everything stream-ordered on the current stream."""
        C, N = p.shape
        st, stream, counter, rowp = self._fused_call(C, row, row_offset, counter)
        with self.torch.cuda.device(self.device):
            if first:
                p1 = p
            else:
                p1 = st["p1"]
                self.proposal().draw(stream, p, p1, 1, counter, st, self._chain0)
            self._accept(stream, self._solve_raw(p1), st, p1, p, rowp, row_stride, counter, False, first=first)
        return p

    SPEC_MAX_STACKS = 2048          # stacks per speculative lock step: a 64-lane team = one wavefront each, the chip holds 4 096

    def auto_spec_depth(self, C):
        """Depth of the speculative lock step the fused path takes by default: the deepest tree (<= 4) whose
        C * (2^d - 1) stacks stay within ``SPEC_MAX_STACKS`` - a lock step of so few stacks is one wavefront per stack walking
        its periods one after the other on a mostly idle chip, and costs the same 0.9-1.0 ms for 100 stacks as for 700
        (100 chains x 96 layers: 0.96 ms per step plain, 0.345 with d = 3, 0.31 with d = 4 at 4.1 forward solves per step;
        scripts/time_speculative.py): 4 up to 136 chains, 3 up to 292, 2 up to 682, 1 from 683 chains on, and 1 where the (stack, period) decomposition fills the chip
        instead (``independent``: 0.24 ms per step plain, 0.29 with d = 3).  A ``PriorRules`` in its default ``redraw="rounds"`` mode
        keeps depth 1 (the rounds know no tree); with ``redraw="kernel"``, or with a proposal factor (``set_proposal``), every node
        is redrawn until the rules hold and the depth is the one above."""
        if self._indep(C):
            return 1
        for d in range(self.proposal().max_depth, 1, -1):         # (prior rules in rounds: those belong to the plain lock step)
            if C * ((1 << d) - 1) <= self.SPEC_MAX_STACKS:
                return d
        return 1

    def _check_depth(self, depth):
        """ValueError for a speculative depth the fused path, or the proposal in force, cannot draw."""
        if depth > MAX_DEPTH:
            raise ValueError("spec_depth of the fused path is at most 4")
        if depth > self.proposal().max_depth:
            raise ValueError(f"spec_depth = {depth}: the redraw rounds of a PriorRules follow one proposal per chain, not a tree; "
                             'pass spec_depth=1 (the default with these rules) or PriorRules(redraw="kernel"), whose kernel '
                             "redraws every node of the tree")

    def fused_tree_step(self, p, depth, nsteps, row=None, row_stride=0, row_offset=0, step_stride=0, counter=None):
        """``nsteps`` <= ``depth`` Metropolis steps of every chain from ONE batched solve (speculative / "prefetching"
        Metropolis on the device: ``surfdisp_mcmc_propose_tree_device`` lays out the binary tree of the next ``depth``
        accept / reject outcomes, 2^depth - 1 proposals per chain, each drawn from the state its branch would be in; all go
        through one forward solve; ``surfdisp_mcmc_accept_tree_device`` walks the tree with the usual test).  Every
        proposal is drawn from and tested against the state the chain is in at that step: the chain is distributed exactly
        as with ``fused_step``.  mcTrack rows of the steps ``step_stride`` doubles apart, the first at ``row_offset``."""
        torch = self.torch
        C, N = p.shape
        M = (1 << int(depth)) - 1
        pr = self.proposal()
        if depth > pr.max_depth:
            self._check_depth(int(depth))                          # (raises, before the call is counted)
        st, stream, counter, rowp = self._fused_call(C, row, row_offset, counter)
        if st.get("M") != M:
            st["M"] = M
            st["q"] = torch.empty((C, M, N), dtype=torch.float64, device=self.device)
            st["qrows"] = torch.arange(C, device=self.device).repeat_interleave(M) if self.local_rows is not None else None
        with torch.cuda.device(self.device):
            pr.draw(stream, p, st["q"], depth, counter, st, self._chain0)
            self._accept(stream, self._solve_raw(st["q"].view(C * M, N), rows=st["qrows"]), st, st["q"], p, rowp, row_stride, counter,
                         True, depth=depth, nsteps=nsteps, step_stride=step_stride)
        return p

    # ------------------------------------------------------------------ chain groups
    GROUP_MIN_CHAINS = 4096         # fewer chains: one group (see chain_groups)

    def chain_groups(self, C, groups=None):
        """None, or a ``ChainGroups`` that advances the C chains as ``groups`` contiguous groups, each on its own stream.

        Chains are independent, so nothing orders one group's lock step against another's: while one group's root search
        drains (its last wavefronts leave SIMDs idle) and its small kernels run (proposal, stacks, prep, accept), the
        other group's root search has the chip - 25 600 chains x 96 layers: 6.3 -> 5.4 ms per step of all chains with two
        groups, 16 400 chains (one workgroup more than a full round of the root search): 5.1 -> 3.9 ms; never slower from
        1 600 chains on (three groups: as two; four lose 10-25 %; profiles/r03b/chain_groups.txt).  A group's solve
        carries SURFDISP_PIPELINED, so the library sizes its teams for both groups' stacks.  The random streams are
        indexed by the chain's index in the whole sampler (``chain0``), so every chain draws the same numbers for any number
        of groups: the chains - every mcTrack row - are then identical whenever the groups' launches use the lanes per stack
        the whole batch would (deep stacks: always 16 from 2 048 per launch on; tests/test_mcmc.py), and otherwise differ by
        what the solver's answers differ between team sizes (1e-6, which can flip a borderline accept).  Default: two groups from ``GROUP_MIN_CHAINS`` chains on (``PYSURFINV_CHAIN_GROUPS``
        overrides), one below."""
        if groups is None:
            env = os.environ.get("PYSURFINV_CHAIN_GROUPS")
            groups = int(env) if env else (2 if C >= self.GROUP_MIN_CHAINS else 1)
        groups = max(1, min(int(groups), C))
        if groups == 1 or not self.fused_available():
            return None
        key = (C, groups)
        if key not in self._groups:
            self._groups[key] = ChainGroups(self, C, groups)
        return self._groups[key]

    # ------------------------------------------------------------------ proposals
    def _good(self, p):
        if self.isgood is None:
            return self.torch.ones(p.shape[0], dtype=self.torch.bool, device=self.device)
        return self.isgood(p)

    def perturb(self, p):
        """MCinv.perturb: redraw the WHOLE proposal while isgood() rejects it (models.py:192-205)."""
        torch = self.torch
        new = self.proposer.move(p)
        if self.isgood is None:                                    # always good (models.py:220-224): no redraw loop,
            return new                                             # and no host synchronisation in the lock step
        bad = ~self._good(new)
        tries = 1
        while tries < 1000 and bool(bad.any()):
            idx = bad.nonzero(as_tuple=True)[0]
            new = new.clone(); new[idx] = self.proposer.move(p[idx])
            bad = ~self._good(new)
            tries += 1
        if bool(bad.any()):
            new = torch.where(bad[:, None], self.reset(p.shape[0]), new)
        return new

    def reset(self, C):
        """MCinv.reset: uniform prior draw, redrawn while isgood() rejects (models.py:206-219)."""
        new = self.proposer.reset(C)
        if self.isgood is None:
            return new
        bad = ~self._good(new)
        tries = 1
        while tries < 10000 and bool(bad.any()):
            idx = bad.nonzero(as_tuple=True)[0]
            new = new.clone(); new[idx] = self.proposer.reset(idx.numel())
            bad = ~self._good(new)
            tries += 1
        if bool(bad.any()):
            raise RuntimeError("Error: Cound not find a good model through reset.")   # models.py:219
        return new

    # ------------------------------------------------------------------ the sampler
    def run(self, n_chains, chainL, init_first=True, priori=False, _init_mask=None, spec_depth=None, fused=None, groups=None,
            start=None, _start_mask=None):
        """Advance ``n_chains`` chains for ``chainL`` steps each (= MCinvMP with runN = n_chains*chainL).

        Returns mcTrack float64 [n_chains, chainL, 3+N]; chain 0 starts at the initial model when
        ``init_first`` (point.py:48-51, MCinvMP passes init = (i==0), :97).

        spec_depth = d > 1: speculative ("prefetching") Metropolis for small chain counts, where one
        lock step is latency-bound and the GPU is mostly idle.  The binary tree of the next d
        accept/reject outcomes is laid out in advance (2^d - 1 proposals per chain, each drawn from
        the state its branch would be in), all of them go through ONE batched forward solve, and the
        chain then walks the tree with the usual accept rule: d Metropolis steps per lock step.
        Every proposal is still drawn from q(current state, .) and tested against the current state,
        so the chain is distributed exactly as with d = 1; only the order in which random numbers are
        consumed differs (the exact-replay path of the reference trace uses d = 1).  Default (None): on the fused device
        path ``auto_spec_depth`` (4 for up to 136 chains, 3 up to 292, 2 up to 682, else 1), on the torch path 1.  A depth the
        proposal in force cannot draw on the fused path - any d > 1 under a ``PriorRules`` in its default ``redraw="rounds"`` mode,
        whose rounds follow one proposal per chain - raises ValueError before anything is launched.

        ``fused`` (default: whenever ``fused_available()``): the lock step as device kernels around the solver
        (``fused_step``: Philox random numbers keyed by the proposer's seed; same proposal and accept distributions).
        ``groups``: chain groups of the fused path (``chain_groups``; every chain's random numbers do not depend on it).
        ``start``: a float64 tensor [n_chains, N] of rows the chains start from instead of ``v0`` / prior draws - row 0 of every
        chain is that model, accepted, as today (e.g. the fitted rows of ``ParamLsqBatch``).  Rows outside the open prior box or
        breaking ``isgood`` raise ValueError before anything is launched (one host synchronisation, outside the stepping loop).
        With ``set_adaptive`` the run carries the adaptation (fused path only; ``n_chains`` a whole number of points): its rows
        before ``until`` are adaptation and no valid samples, the rows from ``until`` on come from a fixed Metropolis kernel."""
        torch = self.torch
        C, N = int(n_chains), self.spec.n
        ad = self._adaptation
        if ad is None:
            return self._run(C, chainL, init_first, priori, _init_mask, spec_depth, fused, groups, start, _start_mask)
        if priori or fused is False or not self.fused_available():
            raise ValueError("run: adaptive proposals (set_adaptive) are drawn by the fused path only; set_adaptive(None) for the torch loop")
        ad.begin(C, int(chainL), self._given, self.isgood)         # its working factors are the proposal in force until end()
        self._adapted = ad
        try:
            return self._run(C, chainL, init_first, priori, _init_mask, spec_depth, fused, groups, start, _start_mask)
        finally:
            ad.end()

    def _walk(self, p, track, cg, depth, calls):
        """The fused lock steps ``calls`` (items of ``fused_schedule``) of the chains ``p`` [C, N] into ``track`` [C, chainL, 3 + N]:
        every call advances the chains - the chain groups ``cg``, else a speculative call at ``depth`` > 1, else the plain step -
        under the next Philox counter, and where an update instant of a running adaptation falls among its rows the update follows,
        once, with the window up to the call's last row (the groups join for it and fork again: the chains of a point may straddle
        two groups)."""
        N = self.spec.n
        width, stride = 3 + N, track.shape[1] * (3 + N)
        ad = self._adaptation if self._adaptation is not None and self._adaptation.working is not None else None
        base, n = self._counter, 0
        if cg is not None:
            cg.fork()
        for n, (i, ns, first) in enumerate(calls, 1):
            if cg is not None:
                cg.step(p, row=track, row_stride=stride, row_offset=i * width, first=first, counter=base + n)
            elif depth > 1 and not first:
                self.fused_tree_step(p, depth, ns, row=track, row_stride=stride, row_offset=i * width, step_stride=width, counter=base + n)
            else:
                self.fused_step(p, row=track, row_stride=stride, row_offset=i * width, first=first, counter=base + n)
            if ad is not None and ad.due(i, i + ns):
                if cg is not None:
                    cg.join()
                ad.update(p, track, stride, width, i + ns - 1)
                if cg is not None:
                    cg.fork()
        if cg is not None:
            cg.join()
        self._counter = base + n

    def _run(self, C, chainL, init_first, priori, _init_mask, spec_depth, fused, groups, start, _start_mask):
        torch = self.torch
        N = self.spec.n
        if start is not None:
            start = self._checked_start(start, C, _start_mask)
        if fused is None:
            fused = self.fused_available()
        fused = bool(fused) and not priori                         # a priori run evaluates nothing: the torch loop below
        if fused and not self.fused_available():
            raise ValueError("fused=True needs the device proposer, no isgood callback (or a PriorRules one) and the HIP forward path")
        if self._given is not None and not fused:
            raise ValueError("run: a proposal factor (set_proposal) is drawn by the fused path only; set_proposal(None) for the torch loop")
        if spec_depth is None:
            spec_depth = self.auto_spec_depth(C) if (fused and groups in (None, 1)) else 1
        spec_depth = int(spec_depth)
        if spec_depth > 1 and groups not in (None, 1):
            raise ValueError("run: chain groups and speculative lock steps (spec_depth > 1) cannot be combined")
        if spec_depth > 1 and not priori and not fused:
            return self._run_speculative(C, chainL, init_first, _init_mask, spec_depth, start, _start_mask)
        if fused:
            self._check_depth(spec_depth)                          # before anything is launched or counted
        track = torch.zeros((C, chainL, 3 + N), dtype=torch.float64, device=self.device)
        if fused:
            # propose / accept kernels around the solver: mcTrack rows are written by the accept kernel itself
            p = self._start(C, init_first, _init_mask, start, _start_mask).contiguous().clone()
            cg = self.chain_groups(C, groups) if spec_depth <= 1 else None
            self._last_groups = cg
            self._walk(p, track, cg, spec_depth, fused_schedule(chainL, spec_depth))
            return track
        p0 = self._start(C, init_first, _init_mask, start, _start_mask)
        chi0 = self._first_row(track, p0)
        for i in range(1, chainL):
            p1 = self.perturb(p0)
            if priori:                                             # point.py:66-69
                _put_row(track, i, 0.0, 1.0, 1.0, p1)
                p0 = p1
                continue
            mis1, chi1, L1 = self.misfit(p1)
            # the reference draws random() only when chi1 >= chi0 (point.py:35-37)
            u = self.proposer.uniform(C) if bool((~(chi1 < chi0)).any()) else torch.zeros_like(chi1)
            acc = _accept_rule(torch, chi0, chi1, u)
            _put_row(track, i, mis1, L1, acc, p1)
            p0 = torch.where(acc[:, None], p1, p0)
            chi0 = torch.where(acc, chi1, chi0)
        return track

    def _checked_start(self, start, C, mask=None):
        """``start`` [C, N] as a float64 tensor on the sampler's device; ValueError for a wrong shape or type, and for a row (of the
        chains in ``mask``; None: all) outside the open prior box or refused by ``isgood``.  Synchronises once."""
        torch = self.torch
        N = self.spec.n
        if not torch.is_tensor(start) or start.dtype != torch.float64 or tuple(start.shape) != (C, N):
            raise ValueError(f"start: a float64 tensor [{C}, {N}] expected, got {getattr(start, 'dtype', type(start).__name__)} "
                             f"{tuple(getattr(start, 'shape', ()))}")
        start = start.to(self.device)
        lo = torch.as_tensor(np.asarray(self.spec.vmin, np.float64), device=self.device)
        hi = torch.as_tensor(np.asarray(self.spec.vmax, np.float64), device=self.device)
        used = torch.ones(C, dtype=torch.bool, device=self.device) if mask is None else mask
        inside = ((start > lo) & (start < hi)).all(dim=1) | ~used
        if not bool(inside.all()):
            raise ValueError(f"start: {int((~inside).sum())} of {C} rows lie outside the open prior box (vmin, vmax)")
        if self.isgood is not None:
            rows = start[used]                                     # (rows of chains that start elsewhere are never looked at)
            if isinstance(self.isgood, PriorRules) and self.local_rows is not None:
                good = self.isgood(rows, rows=self.local_rows[used])
            else:
                good = self.isgood(rows)
            if not bool(good.all()):
                raise ValueError(f"start: {int((~good).sum())} rows break the prior's rules (isgood)")
        return start

    def _start(self, C, init_first, _init_mask, start=None, _start_mask=None):
        torch = self.torch
        if start is not None and _start_mask is None:
            return start
        p0 = self.reset(C) if not (init_first and C == 1) else None
        if init_first or _init_mask is not None:
            v0 = torch.as_tensor(self.spec.v0, dtype=torch.float64, device=self.device)[None, :]
            if not bool(self._good(v0)[0]):
                v0 = self.perturb(v0)                              # point.py:50-51
            if _init_mask is not None:
                p0 = torch.where(_init_mask[:, None], v0.expand_as(p0), p0)
            else:
                p0 = v0 if p0 is None else torch.cat([v0, p0[1:]], dim=0)
        if start is not None:                                      # (run_points: the chains of the mask start at their rows)
            p0 = torch.where(_start_mask[:, None], start, p0)
        return p0

    def _first_row(self, track, p):
        """mcTrack row 0: the start models ``p`` themselves, accepted (point.py:58).  Returns their chi-squares."""
        mis, chi, L = self.misfit(p)
        _put_row(track, 0, mis, L, 1.0, p)
        return chi

    def _run_speculative(self, n_chains, chainL, init_first, _init_mask, d, start=None, _start_mask=None):
        torch = self.torch
        C, N = int(n_chains), self.spec.n
        M = (1 << d) - 1                                           # proposals per chain per lock step
        track = torch.zeros((C, chainL, 3 + N), dtype=torch.float64, device=self.device)
        p = self._start(C, init_first, _init_mask, start, _start_mask)
        chi = self._first_row(track, p)
        ar = torch.arange(C, device=self.device)
        i = 1
        while i < chainL:
            # lay out the tree: node k has children 2k+1 (accepted) and 2k+2 (rejected)
            S = torch.empty((C, 2 * M + 1, N), dtype=torch.float64, device=self.device)
            Q = torch.empty((C, M, N), dtype=torch.float64, device=self.device)
            S[:, 0] = p
            for lev in range(d):
                lo, hi = (1 << lev) - 1, (1 << (lev + 1)) - 1
                st = S[:, lo:hi].reshape(-1, N)
                q = self.perturb(st).reshape(C, hi - lo, N)
                Q[:, lo:hi] = q
                ks = torch.arange(lo, hi, device=self.device)
                S[:, 2 * ks + 1] = q
                S[:, 2 * ks + 2] = S[:, lo:hi]
            # ONE forward solve of C*M stacks; proposal m of chain i is held against chain i's observations
            misQ, chiQ, LQ = self.misfit(Q.reshape(-1, N), rows=ar.repeat_interleave(M) if (self.c_obs.ndim == 2 or self.local_rows is not None) else None)
            misQ, chiQ, LQ = misQ.reshape(C, M), chiQ.reshape(C, M), LQ.reshape(C, M)
            node = torch.zeros(C, dtype=torch.int64, device=self.device)
            for _ in range(min(d, chainL - i)):
                chi1, q = chiQ[ar, node], Q[ar, node]
                acc = _accept_rule(torch, chi, chi1, self.proposer.uniform(C))
                _put_row(track, i, misQ[ar, node], LQ[ar, node], acc, q)
                p = torch.where(acc[:, None], q, p)
                chi = torch.where(acc, chi1, chi)
                node = torch.where(acc, 2 * node + 1, 2 * node + 2)
                i += 1
        return track

    def run_points(self, n_points, chains_per_point, chainL, on_device=False, groups=None, spec_depth=None, start=None):
        """MCinvMP for n_points at once: chain index = point * chains_per_point + k; chain k = 0 of
        every point starts at the initial model, the others at prior draws (point.py:95-99).
        ``start``: float64 [n_points, N] - chain k = 0 of a point starts at its row instead, the others at prior draws as now - or
        [n_points, chains_per_point, N] for all chains (checked as ``run(start=)`` checks its rows).
        With ``set_adaptive`` the chains of a point pool their states (``chains_per_point`` must be the one given there: ValueError);
        every chain's rows before ``until`` are adaptation and no valid samples.
        Returns float64 [n_points, chains_per_point, chainL, 3+N] (numpy, or the device tensor)."""
        torch = self.torch
        if self._adaptation is not None and int(chains_per_point) != self._adaptation.cpp:
            raise ValueError(f"run_points: {chains_per_point} chains per point, set_adaptive was given chains_per_point = {self._adaptation.cpp}")
        C = n_points * chains_per_point
        first = (torch.arange(C, device=self.device) % chains_per_point) == 0
        if start is not None:
            N = self.spec.n
            if not torch.is_tensor(start) or start.dtype != torch.float64 or \
                    tuple(start.shape) not in ((n_points, N), (n_points, chains_per_point, N)):
                raise ValueError(f"start: a float64 tensor [{n_points}, {N}] or [{n_points}, {chains_per_point}, {N}] expected, got "
                                 f"{getattr(start, 'dtype', type(start).__name__)} {tuple(getattr(start, 'shape', ()))}")
            if start.ndim == 2:
                rows, kw = start.repeat_interleave(chains_per_point, dim=0), dict(_start_mask=first)
            else:
                rows, kw = start.reshape(C, N), {}
            tr = self.run(C, chainL, init_first=False, groups=groups, spec_depth=spec_depth, start=rows, **kw)
            tr = tr.reshape(n_points, chains_per_point, chainL, -1)
            return tr if on_device else tr.cpu().numpy()
        tr = self.run(C, chainL, init_first=False, _init_mask=first, groups=groups, spec_depth=spec_depth).reshape(n_points, chains_per_point, chainL, -1)
        return tr if on_device else tr.cpu().numpy()

    def summarise_points(self, track, obs_rows):
        """What the reference's ``PostPoint`` derives from one point's ``mcTrack`` (point.py:147-171), for all
        points at once on the device.  ``track`` [n_points, R, 3+N] (R = chains * chainL rows per point, chains one
        after the other as in the ``.npz``); ``obs_rows`` [n_points]: observation row of each point.

        * rejected rows take the parameters of the last accepted row before them (``trueMarkovChain``, :154-159);
        * ``minMod`` = row of the smallest misfit (:161-165); ``thres = max(2 min, min + 0.5)`` (:308-309);
        * ``avgMod`` = mean of the parameters of all rows with misfit < thres (:166-169), forward-solved once more
          for its misfit, likelihood (:171) and predicted curve (``pvelp``, model3D.py:32-35).
        Returns float64 [n_points, 6 + 2N + P]: min_misfit, min_L, thres, n_accepted_final, avg_misfit, avg_L,
        min_params[N], avg_params[N], pvelp[P]."""
        torch = self.torch
        npnt, R, W = track.shape
        N = W - 3
        acc = track[:, :, 2] > 0.5
        idx = torch.arange(R, device=track.device)[None, :].expand(npnt, R)
        last = torch.cummax(torch.where(acc, idx, torch.zeros_like(idx)), dim=1).values     # row 0 of a chain is accepted
        paras = torch.gather(track[:, :, 3:], 1, last[:, :, None].expand(npnt, R, N))
        mis = torch.nan_to_num(track[:, :, 0], nan=float("inf"))
        imin = mis.argmin(dim=1)
        ar = torch.arange(npnt, device=track.device)
        min_mis, min_L, min_par = mis[ar, imin], track[ar, imin, 1], paras[ar, imin]
        thres = torch.maximum(2.0 * min_mis, min_mis + 0.5)
        final = mis < thres[:, None]
        nfin = final.sum(dim=1)
        avg_par = (paras * final[:, :, None]).sum(dim=1) / nfin.clamp(min=1)[:, None]
        avg_mis, _, avg_L, cP = self.misfit(avg_par, rows=obs_rows, return_c=True)
        return torch.cat([min_mis[:, None], min_L[:, None], thres[:, None], nfin.to(torch.float64)[:, None],
                          avg_mis[:, None], avg_L[:, None], min_par, avg_par, cP], dim=1)

    def run_graphed(self, n_chains, chainL, init_first=True, rounds=24):
        """``run()`` with the whole Metropolis step - proposal, parameters -> stack, the forward
        kernels, misfit, accept/reject, bookkeeping - captured ONCE in a HIP graph and replayed
        ``chainL - 1`` times: at small chain counts the step is bound by the ~100 kernel launches of
        the torch glue, not by the solver.  Requirements: device proposer (TorchProposer), no
        ``isgood`` callback, a parameterisation with static structure (``Model1DBatch._static_sig``).
        The bound-rejection loop of ``BrownianVar.move`` (<= 1000 tries, brownian.py:20-27) becomes a
        fixed ``rounds`` redraws followed by the uniform fallback: a variable sitting exactly on a
        bound survives 24 redraws with probability 6e-8, so the proposal distribution is unchanged
        for all practical purposes.  Random numbers come from torch's default device generator
        (graph-safe Philox)."""
        torch = self.torch
        if self._adaptation is not None:
            raise ValueError("run_graphed: adaptive proposals (set_adaptive) are not supported: the update instants are placed by run()")
        if self.joint is not None:
            raise ValueError("run_graphed: joint data (data=) are not supported; use run()")
        if self.isgood is not None or not self.fused_available():
            # (the captured step is torch glue with torch's graph-safe generator - the fused kernels take their Philox counter by
            # value, which a graph would freeze -, and that glue has no redraw loop: no predicate here, PriorRules or callback)
            raise ValueError("run_graphed needs the device proposer, no isgood predicate and the HIP forward path")
        C, N = int(n_chains), self.spec.n
        dev = self.device
        pr = self.proposer
        track = torch.zeros((C, chainL, 3 + N), dtype=torch.float64, device=dev)
        p = self._start(C, init_first, None)
        chi = self._first_row(track, p)
        step = torch.ones(1, dtype=torch.int64, device=dev)          # row the next step writes
        p = p.clone(); chi = chi.clone()

        def one_step():
            # all redraw rounds at once: [C, rounds, N] candidates, take the first one inside the bounds
            draws = p[:, None, :] + pr.step * torch.randn((C, rounds, N), dtype=torch.float64, device=dev)
            ok = (draws < pr.vmax) & (draws > pr.vmin)
            first = ok.to(torch.int8).argmax(dim=1, keepdim=True)
            chosen = torch.gather(draws, 1, first).squeeze(1)
            uni = pr.vmin + (pr.vmax - pr.vmin) * torch.rand((C, N), dtype=torch.float64, device=dev)
            new = torch.where(ok.any(dim=1), chosen, uni)
            mis1, chi1, L1 = self.misfit(new)
            acc = _accept_rule(torch, chi, chi1, torch.rand(C, dtype=torch.float64, device=dev))
            row = torch.cat([mis1[:, None], L1[:, None], acc.to(torch.float64)[:, None], new], dim=1)
            track.index_copy_(1, step, row[:, None, :])
            p.copy_(torch.where(acc[:, None], new, p))
            chi.copy_(torch.where(acc, chi1, chi))
            step.add_(1)

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                                # warm-up off the capture stream
            one_step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        if chainL > 2:                                              # rows 0 and 1 are written; capture
            g = torch.cuda.CUDAGraph()                              # records one_step without running it
            with torch.cuda.graph(g):
                one_step()
            for _ in range(chainL - 2):
                g.replay()
            self.n_forward += (chainL - 2) * C
        return track

    # ------------------------------------------------------------------ output (point.py:82-85,120-123)
    @staticmethod
    def save_npz(outdir, pid, mc_track, setting, obs, chainL):
        os.makedirs(outdir, exist_ok=True)
        mc = np.asarray(mc_track, dtype=np.float64).reshape(-1, np.asarray(mc_track).shape[-1])
        np.savez_compressed(f"{outdir}/{pid}.npz", mcTrack=mc, setting=dict(setting), obs=obs,
                            invMeta={"pid": pid, "chainL": chainL})
        return f"{outdir}/{pid}.npz"
