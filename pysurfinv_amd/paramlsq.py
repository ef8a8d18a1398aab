"""Linearised inversion in the sampler's own parameters: the least-squares companion of ``MetropolisBatch`` on the SAME unknowns.

``LinearizedBatch`` fits the Vs of the free layers of a stack (plus hand-made thickness modes); ``MetropolisBatch`` samples the
reference's model parameters - the ``setting`` dictionaries of ``models.py``: B-spline Vs coefficients per group, group
thicknesses, ``BottomDepth`` - as ``ParamSpec`` rows through ``Model1DBatch``.  This module is the Gauss-Newton /
Levenberg-Marquardt fit of those rows: a maximum a posteriori point to start chains from, a ``toYML``-able model comparable with the
sampler's ``avgMod``, and a Gaussian (Laplace) covariance of the parameters to size proposal steps with -
``ParamLsqBatch.proposal_factor`` hands its Cholesky factor to ``MetropolisBatch.set_proposal``, the fitted rows to ``run(start=)``.

The map parameters -> stack is smooth and analytic for every layer class but the thermal mantle, so its Jacobian is exact
(``surfdisp_params_jacobian_device``, one thread per (chain, layer, unknown) carrying a dual number), and the chain rule through
the analytic kernels dc/dm, dU/dm, dc/dh, dU/dh gives the data Jacobian in parameter space from one kernel call each, where finite
differences cost 2 N + 1 forward solves.  One step per stack, over its n free unknowns (include/surfdisp.h section (6i)):

    G[r, j] = sg_r (sum_{i<nlay} K_b[r,i] J_vs[i,j] + K_a[r,i] J_vp[i,j] + K_rho[r,i] J_rho[i,j] + sum_{i<nlay-1} K_h[r,i] J_h[i,j])
    A = G^T W G + lam diag(1 / scale_j^2) + diag(beta_j),     rhs = G^T W res - beta_j (p_j - ref_j),     delta = A^-1 rhs

* ``Model1DBatch.jacobian`` (``model_jacobian``): (layer, jac) device tensors of a parameter block.
* ``jacobian_reference`` / ``param_lsq_reference``: the numpy float64 statements the kernels are tested against; the second is
  ``linearized._System`` with no Vs unknown and the parameters in the place of its modes - one solve block in the module family.
* ``ParamLsqPlan``: kernels + Jacobian + step of one batch as device tensors.
* ``ParamLsqBatch``: the accept loop of ``LinearizedBatch.run`` on parameter rows, inside the open prior box of the ``ParamSpec``.

Out of scope: thermal (``OceanMantleHybrid``) layers, the Gaussian crust term, models without a static layer structure, ellipticity
data (the library has no dchi/dh).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, linearized
from .linearized import FAIL, _mode_data, _ptr, _ptrs
from .obsdata import JointData

MAX_UNKNOWNS = 64        # unknowns per stack the two entries take (SD_PLSQ_MAX_UNKNOWNS)
BOX_MARGIN = 1e-6        # a trial is clamped into [vmin + m w, vmax - m w], w = vmax - vmin: the prior box is open


def model_jacobian(mb, params, rows=None):
    """``Model1DBatch.jacobian``: (layer [C, 4, L], jac [C, 4, L, Nu]) float64 device tensors of the parameter block ``params``
    [C, Nu] - vp, vs, rho, h of the output layers before their rounding to float32 (the row order of ``to_model``) and their partial
    derivatives with respect to random-walk parameter j.  One launch of ``surfdisp_params_jacobian_device``, no host
    synchronisation.  ``rows``: the local-info row of each parameter vector (the per-point constants are never unknowns).
    ValueError for a model with a thermal layer, SurfdispError without a static native descriptor or a HIP device."""
    torch = mb.torch
    if any(lay["kind"] == "hybrid" for lay in mb.layers):
        raise ValueError("jacobian: a thermal (OceanMantleHybrid) layer has no analytic parameter Jacobian")
    desc = mb.native_descriptor()
    if desc is None or params.device.type != "cuda":
        raise _lib.SurfdispError("the parameter Jacobian needs a static layer structure (native descriptor) and a HIP device")
    Nu = mb.spec.n
    if not 1 <= Nu <= MAX_UNKNOWNS or params.ndim != 2 or params.shape[1] != Nu:
        raise ValueError(f"jacobian: params [C, {Nu}] expected with 1 <= {Nu} <= {MAX_UNKNOWNS}, got {tuple(params.shape)}")
    idesc, fdesc, L = desc
    p = mb._full(params, rows).contiguous()
    C, N = p.shape
    layer = torch.empty((C, 4, L), dtype=torch.float64, device=p.device)
    jac = torch.empty((C, 4, L, Nu), dtype=torch.float64, device=p.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(p.device).cuda_stream)
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().surfdisp_params_jacobian_device(stream, C, N, Nu, L, _ptr(p), _ptr(idesc), _ptr(fdesc), _ptr(layer), _ptr(jac)))
    return layer, jac


def jacobian_reference(model_batch, params, rel_step=1e-5, rows=None):
    """(layer [C, 4, L], jac [C, 4, L, Nu]) numpy float64: central differences of ``Model1DBatch.seis_prop_layers`` (the torch
    statement of the map, evaluated on the CPU whatever the model's device), parameter j stepped by ``rel_step`` of its prior
    width.  ``params`` [C, Nu] numpy or tensor.  The model must keep its layer structure over the steps."""
    import torch
    from .layers_batch import Model1DBatch
    mb = model_batch
    cpu = Model1DBatch(mb.setting, device="cpu", local_keys=mb.aux_names)
    if mb.n_aux and mb._aux is not None:
        cpu.set_local_info(mb._aux.cpu().numpy())
    p = np.asarray(params.detach().cpu().numpy() if hasattr(params, "detach") else params, np.float64)
    C, Nu = p.shape
    h = rel_step * (np.asarray(mb.spec.vmax, np.float64) - np.asarray(mb.spec.vmin, np.float64))
    block = np.repeat(p[:, None, :], 2 * Nu + 1, axis=1)                    # [C, 1 + 2 Nu, Nu]: centre, minus, plus
    for j in range(Nu):
        block[:, 1 + j, j] -= h[j]
        block[:, 1 + Nu + j, j] += h[j]
    rr = None
    if mb.n_aux:
        rr = np.repeat(np.arange(C) if rows is None else np.asarray(rows), 2 * Nu + 1)
    (hh, vs, vp, rho, _, _), nlay = cpu.seis_prop_layers(torch.as_tensor(block.reshape(-1, Nu)), rows=rr)
    L = hh.shape[1]
    assert (nlay == L).all(), "jacobian_reference: the layer structure changed over the finite-difference steps"
    v = torch.stack([vp, vs, rho, hh], dim=1).numpy().reshape(C, 2 * Nu + 1, 4, L)
    jac = (v[:, 1 + Nu:] - v[:, 1:1 + Nu]) / (2.0 * h)[None, :, None, None]
    return v[:, 0].copy(), np.ascontiguousarray(jac.transpose(0, 2, 3, 1))


def param_columns(Kb, Ka, Kr, Kh, jac, nlay=None, sign=None):
    """G [N, Nu] float64: the chain rule of section (6i) for N data rows of one stack.  ``Kb``, ``Ka``, ``Kr``, ``Kh`` [N, L]: the
    rows' kernels d/dVs, d/dVp, d/drho, d/dh as the library returns them (``Ka`` / ``Kr`` None: absent); ``jac`` [4, L, Nu] (vp, vs,
    rho, h).  Layers i < nlay (h: i < nlay - 1) count; a term whose jac entry is exactly 0 is skipped (a NaN kernel entry does not
    reach the sum there); ``sign`` [N]: the sign of a source-5 row."""
    jac = np.asarray(jac, np.float64)
    L, Nu = jac.shape[1:]
    nl = L if nlay is None else int(nlay)
    N = np.shape(Kb)[0]
    G = np.zeros((N, Nu))
    for K, q, m in ((Kb, 1, nl), (Ka, 0, nl), (Kr, 2, nl), (Kh, 3, nl - 1)):
        if K is None or m <= 0:
            continue
        K = np.asarray(K, np.float64).reshape(N, L)[:, :m]
        J = jac[q, :m, :]
        with np.errstate(invalid="ignore"):
            term = K[:, :, None] * J[None, :, :]
        G += np.where(J[None, :, :] == 0.0, 0.0, term).sum(axis=1)
    return G if sign is None else G * np.asarray(sign, np.float64)[:, None]


def param_lsq_reference(Kb, Ka, Kr, Kh, jac, r, w_over_sigma2, lam, scale, prior_w=None, prior_ref=None, p=None, free=None, nlay=None,
                        sign=None):
    """One least-squares step of one stack in parameter space, numpy float64 - the statement ``surfdisp_lsq_step_params_device`` is
    tested against.  ``Kb`` .. ``Kh``, ``jac``, ``nlay``, ``sign``: as ``param_columns``, for the rows the rules of section (6d) keep;
    a row with a column that is not finite is dropped here.  r [N] the residuals obs - pred, w_over_sigma2 [N]; lam a scalar;
    ``scale`` [Nu] (> 0), ``prior_w`` beta [Nu] (None: 0), ``prior_ref`` and ``p`` [Nu] (read with a prior); ``free`` bool [Nu] (None:
    all).  The problem is ``linearized._System`` without Vs unknowns, the free parameters in the place of its modes: mode_scale =
    1 / scale^2, mode_prior = beta, mode_y = p - ref.  Returns dict(delta [Nu] (0 at fixed unknowns), misfit, prior, predicted,
    flag (1 without rows, 2 when the factorisation fails: zeros), used, kept [N] bool, G [used, n], A [n, n], g [n] (the normal
    equations over the free unknowns), cov [Nu, Nu], sigma [Nu], logdet)."""
    G = param_columns(Kb, Ka, Kr, Kh, jac, nlay, sign)
    Nu = G.shape[1]
    fr = np.ones(Nu, bool) if free is None else np.asarray(free, bool).ravel()
    idx = np.nonzero(fr)[0]
    G = G[:, idx]
    kept = np.isfinite(G).all(axis=1)
    G, r, w = G[kept], np.asarray(r, np.float64).ravel()[kept], np.asarray(w_over_sigma2, np.float64).ravel()[kept]
    n = idx.size
    beta = np.zeros(n) if prior_w is None else np.asarray(prior_w, np.float64).ravel()[idx]
    y = np.zeros(n) if prior_w is None else (np.asarray(p, np.float64).ravel()[:Nu] - np.asarray(prior_ref, np.float64).ravel())[idx]
    ms = 1.0 / np.asarray(scale, np.float64).ravel()[idx] ** 2
    none = np.zeros((G.shape[0], 0))
    st = linearized.lsq_modes_step_reference(none, r, w, np.zeros(0), 0.0, np.zeros(0), lam, G, ms, beta, y)
    rs = linearized.lsq_modes_resolution_reference(none, w, 0, 0.0, np.zeros(0), lam, G, ms, beta)
    A, g = linearized.modes_normal_equations(none, G, r, w, np.zeros(0), 0.0, np.zeros(0), lam, ms, beta, y)
    flag = st["flag"] or rs["flag"]
    delta, sigma, cov = np.zeros(Nu), np.zeros(Nu), np.zeros((Nu, Nu))
    if flag == 0:
        delta[idx], sigma[idx] = st["delta_y"], rs["sigma_post"]
        cov[np.ix_(idx, idx)] = rs["cov"]
    prior = float((beta * y * y).sum())
    return dict(delta=delta, misfit=st["misfit"], prior=prior, predicted=st["predicted"] if flag == 0 else st["misfit"] + prior,
                flag=flag, used=int(kept.sum()), kept=kept, G=G, A=A, g=g, cov=cov, sigma=sigma, logdet=rs["logdet"] if flag == 0 else 0.0)


def _per_unknown(name, v, Nu, default=None):
    """A scalar or [Nu] argument as float64 [Nu] (None: ``default``); ValueError otherwise."""
    a = np.asarray(default if v is None else v, np.float64)
    if a.shape not in ((), (Nu,)):
        raise ValueError(f"{name}: shape {a.shape}, expected a scalar or ({Nu},)")
    a = np.array(np.broadcast_to(a, (Nu,)))
    if not np.isfinite(a).all():
        raise ValueError(f"{name}: entries that are not finite")
    return a


class ParamLsqPlan:
    """Kernels, parameter Jacobian and least-squares step of B parameter rows of ``model_batch`` (a ``Model1DBatch`` on a HIP device
    with a static native descriptor and no thermal layer) against ``datasets`` (as ``LsqPlan``; phase- and group-velocity sets - an
    ellipticity set is refused: the library has no dchi/dh).  Owns an ``LsqPlan(..., group_modes=True)`` - its ``BatchPlan`` per wave
    type, the ``JointData`` table, the observation tensors - and the step's output buffers."""

    def __init__(self, model_batch, B, datasets, device="cuda:0", mask=None):
        mb = self.model = model_batch
        if any(lay["kind"] == "hybrid" for lay in mb.layers):
            raise ValueError("ParamLsqPlan: a thermal (OceanMantleHybrid) layer has no analytic parameter Jacobian")
        jd = datasets if isinstance(datasets, JointData) else JointData(datasets, device="cpu")
        _mode_data(jd, True)                                               # (an ellipticity set: ValueError)
        desc = mb.native_descriptor()
        if desc is None:
            raise _lib.SurfdispError("ParamLsqPlan needs a model with a static layer structure (native descriptor)")
        self.Nu = mb.spec.n
        if not 1 <= self.Nu <= MAX_UNKNOWNS:
            raise ValueError(f"{self.Nu} random-walk parameters: the step kernel takes 1..{MAX_UNKNOWNS}")
        self.B, self.L = int(B), int(desc[2])
        self.lsq = linearized.LsqPlan(self.B, self.L, jd, device=device, mask=mask, group_modes=True)   # (no HIP device: SurfdispError)
        self.torch, self.device = self.lsq.torch, self.lsq.device
        if mb.device.type != self.device.type:
            raise ValueError(f"the model lives on {mb.device}, the plan on {self.device}")
        buf = self.lsq._buffer
        self.delta, self.stats = buf("p_delta", self.B, self.Nu), buf("p_stats", self.B, 3)
        self.info = buf("p_info", self.B, 3, dtype=self.torch.int32)

    def step(self, params, lam, scale, free=None, prior_w=None, prior_ref=None, rows=None, want_cov=False):
        """The stacks of ``params`` (float64 [B, Nu], device), their kernels (``LsqPlan.kernels(model, thickness=True)``), the
        Jacobian of the map and one step: one launch each, no host synchronisation.  Device tensors: ``lam`` float64 [B]; ``scale``
        float64 [Nu] (> 0); ``free`` uint8 [Nu] or [B, Nu] (None: every parameter); ``prior_w``, ``prior_ref`` float64 [Nu] (None: no
        prior).  Returns dict(delta [B, Nu] float64 (0 at fixed parameters), misfit, prior, predicted [B] float64, used, dropped,
        flag [B] int32 (0 solved, 1 no usable row, 2 pivot <= 0 or not finite), model, layer, jac, pred, part, part_h; with
        ``want_cov`` cov [B, Nu, Nu], sigma [B, Nu], logdet [B]: A^-1 in parameter order (zeros at fixed parameters), its root
        diagonal, log det A) - views of the plan's buffers, rewritten by the next call."""
        torch, B, Nu, L, dev, mb, lsq = self.torch, self.B, self.Nu, self.L, self.device, self.model, self.lsq

        def chk(name, t, dtype, *shapes):
            if t is None:
                return 0
            if t.dtype != dtype or t.device != dev or not t.is_contiguous() or tuple(t.shape) not in shapes:
                raise ValueError(f"{name}: expected contiguous {dtype} {' or '.join(map(str, shapes))} on {dev}, got {t.dtype} "
                                 f"{tuple(t.shape)}")
            return shapes.index(tuple(t.shape))

        chk("params", params, torch.float64, (B, Nu))
        chk("lam", lam, torch.float64, (B,))
        if scale is None:
            raise ValueError("scale: a float64 tensor expected")
        chk("scale", scale, torch.float64, (Nu,))
        free_ps = chk("free", free, torch.uint8, (Nu,), (B, Nu))
        chk("prior_w", prior_w, torch.float64, (Nu,))
        chk("prior_ref", prior_ref, torch.float64, (Nu,))
        if prior_w is not None and prior_ref is None:
            raise ValueError("prior_w needs prior_ref")
        model, _ = mb.to_model(params, rows)
        pred, part, part_h = lsq.kernels(model, thickness=True)
        layer, jac = mb.jacobian(params, rows)
        jd = lsq.joint
        arrs = [pred["cR"], pred["uR"], pred["cL"], pred["uL"], None]
        strides = (ctypes.c_long * 5)(*[a.stride(0) if a is not None else 0 for a in arrs])
        nper = (ctypes.c_int * 2)(*[int(jd.solve_periods[w].size) if w in jd.solve_periods else 0 for w in ("R", "L")])
        out = dict(delta=self.delta, misfit=self.stats[:, 0], prior=self.stats[:, 1], predicted=self.stats[:, 2], used=self.info[:, 0],
                   dropped=self.info[:, 1], flag=self.info[:, 2], model=model, layer=layer, jac=jac, pred=pred, part=part, part_h=part_h)
        if want_cov:
            out.update(cov=lsq._buffer("p_cov", B, Nu, Nu), sigma=lsq._buffer("p_sigma", B, Nu), logdet=lsq._buffer("p_logdet", B))
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().surfdisp_lsq_step_params_device(
                stream, B, L, None, Nu, _ptr(jac), _ptrs(part), _ptrs(part_h[:4] + [None]), _ptrs(arrs), strides, nper,
                jd.Ptot, _ptr(jd.cols), _ptr(jd.weights), _ptr(lsq.obs), _ptr(lsq.uncer), _ptr(lsq.mask8), 1 if lsq.obs.ndim == 2 else 0,
                _ptr(free), free_ps, _ptr(scale), _ptr(prior_w), _ptr(prior_ref), _ptr(params), Nu, _ptr(lam),
                _ptr(self.delta), _ptr(self.stats), _ptr(self.info), _ptr(out.get("cov")), _ptr(out.get("sigma")), _ptr(out.get("logdet"))))
        return out


class ParamLsqBatch:
    """Damped least-squares fit of the random-walk parameters of ``model_batch`` at M points at once.

    ``datasets``: as ``MetropolisBatch(data=...)`` - per-point values [M, P] fix M; shared values need ``params0`` [M, Nu].
    ``params0`` (default: ``spec.v0`` at every point); ``free`` bool [Nu] or [M, Nu] (default: all); ``scale`` [Nu] > 0 (default: the
    spec's clipped ``step``): unknown j takes lam / scale_j^2 on its diagonal, so lam = 1 damps a step to about one proposal step;
    ``prior_w`` beta >= 0 and ``prior_ref`` (default ``spec.v0``), scalars or [Nu]: the Gaussian pull beta_j (p_j - ref_j)^2;
    ``lam0``, ``nu``, ``lam_min``: the Levenberg-Marquardt damping and its factor; ``rules``: a ``mcmc.PriorRules`` of the same
    model - a trial that breaks them is rejected (``surfdisp_prior_device``); ``rows``: the local-info row of each point.

    ``run(n_iter)``, per iteration and without a host synchronisation: kernels, Jacobian and step at p; trial = p + delta at the
    free parameters, clamped into [vmin + m w, vmax - m w] with w = vmax - vmin and m = ``BOX_MARGIN`` (the box of the spec is
    open); ONE ``to_model`` and ONE forward solve of the trials; objective = chi-square (``obsdata``) + sum beta (p - ref)^2, inf for a
    failed solve, a flagged step or a broken rule; per point, where the objective fell: accept, lam <- max(lam / nu, lam_min), else
    keep p and lam <- lam nu."""

    def __init__(self, model_batch, datasets, params0=None, free=None, scale=None, prior_w=0.0, prior_ref=None, lam0=1.0, nu=4.0,
                 lam_min=1e-9, rules=None, rows=None, mask=None, device=None):
        mb = self.model_batch = model_batch
        spec = mb.spec
        Nu = spec.n
        jd = datasets if isinstance(datasets, JointData) else JointData(datasets, device="cpu")      # (data errors: ValueError)
        if params0 is None:
            if jd.C is None:
                raise ValueError("shared observations: give params0 [M, Nu] to fix the number of points")
            p0 = np.tile(np.asarray(spec.v0, np.float64), (jd.C, 1))
        else:
            p0 = np.asarray(params0.detach().cpu().numpy() if hasattr(params0, "detach") else params0, np.float64)
            if p0.ndim != 2 or p0.shape[1] != Nu:
                raise ValueError(f"params0: shape {p0.shape}, expected (M, {Nu})")
        M = self.M = p0.shape[0]
        lo, hi = np.asarray(spec.vmin, np.float64), np.asarray(spec.vmax, np.float64)
        if not ((p0 > lo).all() and (p0 < hi).all()):
            raise ValueError("params0: every parameter strictly inside (vmin, vmax) of the spec expected")
        fr = np.ones(Nu, bool) if free is None else np.asarray(free, bool)
        if fr.shape not in ((Nu,), (M, Nu)):
            raise ValueError(f"free: shape {fr.shape}, expected ({Nu},) or ({M}, {Nu})")
        if not fr.any():
            raise ValueError("no free parameter")
        sc = _per_unknown("scale", scale, Nu, spec.step)
        beta = _per_unknown("prior_w", prior_w, Nu)
        ref = _per_unknown("prior_ref", prior_ref, Nu, spec.v0)
        if not (sc > 0).all() or not (beta >= 0).all():
            raise ValueError("scale > 0 and prior_w >= 0 expected")
        if not (lam0 > 0 and nu > 1 and lam_min >= 0):
            raise ValueError("lam0 > 0, nu > 1, lam_min >= 0 expected")
        if rules is not None and getattr(rules, "model", None) is not mb:
            raise ValueError("rules: a PriorRules of the same Model1DBatch expected")
        self.nu, self.lam_min = float(nu), float(lam_min)
        self.plan = plan = ParamLsqPlan(mb, M, jd, device=mb.device if device is None else device, mask=mask)
        import torch
        self.torch = torch
        dev = self.device = plan.device
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
        self.params = t(p0)
        self.free, self.free8 = t(np.broadcast_to(fr, (M, Nu))), t(fr.astype(np.uint8))
        self.n_free = fr.sum(axis=-1)                                      # free parameters: an integer, or [M] with per-point masks
        self.scale, self.prior_w, self.prior_ref = t(sc), t(beta), t(ref)
        self.has_prior = bool((beta > 0).any())
        w = hi - lo
        self.lo, self.hi = t(lo + BOX_MARGIN * w), t(hi - BOX_MARGIN * w)
        self.rows = rows
        self.rules = rules
        if rules is not None:
            self._flags = rules.device_flags()
            if self._flags is None:
                raise _lib.SurfdispError("rules: the model has no native descriptor for the prior kernel")
            self._tags = torch.zeros(M, dtype=torch.uint8, device=dev)
        self.lam = torch.full((M,), float(lam0), dtype=torch.float64, device=dev)
        model, nlay = mb.to_model(self.params, rows)
        chi, rms, failed = plan.lsq.chi_square(model, nlay)
        self.objective = torch.where(failed, torch.full_like(chi, float("inf")), chi + self.prior_term(self.params))
        self.rms = rms

    def prior_term(self, params):
        """sum_j beta_j (p_j - ref_j)^2 [M] float64."""
        d = params - self.prior_ref
        return (self.prior_w * d * d).sum(dim=1)

    def trial(self, params, delta):
        """params + delta at the free parameters, clamped strictly inside the prior box; the fixed ones as they are."""
        torch = self.torch
        return torch.where(self.free, torch.minimum(torch.maximum(params + delta, self.lo), self.hi), params)

    def breaks_rules(self, params):
        """bool [M]: the rows that break ``rules``, by ``surfdisp_prior_device`` (no host synchronisation)."""
        torch, mb, rules = self.torch, self.model_batch, self.rules
        idesc, fdesc, Lout = mb.native_descriptor()
        q = (params if mb.n_aux == 0 else mb._full(params, self.rows)).contiguous()
        self._tags.zero_()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().surfdisp_prior_device(stream, self.M, q.shape[1], int(Lout), _ptr(q), _ptr(idesc), _ptr(fdesc),
                                                        _ptr(self._flags), ctypes.c_double(-1.0 if rules.vs_max is None else rules.vs_max),
                                                        -1, 1, _ptr(self._tags)))
        return self._tags != 0

    def _step(self, lam, want_cov=False):
        kw = dict(prior_w=self.prior_w, prior_ref=self.prior_ref) if self.has_prior else {}
        return self.plan.step(self.params, lam, self.scale, free=self.free8, rows=self.rows, want_cov=want_cov, **kw)

    def run(self, n_iter, keep_params=False):
        """``n_iter`` iterations from the current state (a second call goes on).  Returns dict(params [M, Nu] the final parameters;
        per iteration, [n_iter, M]: objective, rms (88888 for a model whose solve fails) of the state AFTER the iteration, lam
        after its update, accepted (bool), flag, used, dropped (of the step), predicted (the step's linear prediction of the
        objective); params_all [n_iter, M, Nu] with ``keep_params``)."""
        torch, plan, mb = self.torch, self.plan, self.model_batch
        keys = ("objective", "rms", "lam", "accepted", "flag", "used", "dropped", "predicted")
        hist = {k: [] for k in keys}
        kept = []
        inf = torch.full((self.M,), float("inf"), dtype=torch.float64, device=self.device)
        for _ in range(int(n_iter)):
            st = self._step(self.lam)
            flag, used, dropped, predicted = (st[k].clone() for k in ("flag", "used", "dropped", "predicted"))
            tr = self.trial(self.params, st["delta"])
            model, nlay = mb.to_model(tr, self.rows)
            chi, rms, failed = plan.lsq.chi_square(model, nlay)
            obj = torch.where(failed | (flag != 0), inf, chi + self.prior_term(tr))
            if self.rules is not None:
                obj = torch.where(self.breaks_rules(tr), inf, obj)
            acc = obj < self.objective
            self.params = torch.where(acc[:, None], tr, self.params)
            self.objective = torch.where(acc, obj, self.objective)
            self.rms = torch.where(acc, rms, self.rms)
            self.lam = torch.where(acc, torch.clamp(self.lam / self.nu, min=self.lam_min), self.lam * self.nu)
            for k, v in zip(keys, (self.objective, self.rms, self.lam, acc, flag, used, dropped, predicted)):
                hist[k].append(v)
            if keep_params:
                kept.append(self.params)
        out = {k: torch.stack(v) for k, v in hist.items()} if n_iter > 0 else {}
        out["params"] = self.params
        if keep_params:
            out["params_all"] = torch.stack(kept)
        return out

    def covariance(self, lam=None):
        """The Gaussian (Laplace) approximation at the CURRENT point: dict(cov [M, Nu, Nu] = A^-1 in parameter order (zeros at
        fixed parameters), sigma [M, Nu], logdet [M], flag [M]).  ``lam``: the damping - None: the batch's current ``lam``; a
        scalar or [M]; 0.0 leaves the prior as the only regularisation (a singular A is flag 2: zeros).  Does not advance the
        iteration.  No host synchronisation."""
        torch = self.torch
        if lam is None:
            lam_t = self.lam
        else:
            lam_t = torch.as_tensor(lam, dtype=torch.float64, device=self.device)
            if lam_t.ndim == 0:
                lam_t = lam_t.expand(self.M)
            if tuple(lam_t.shape) != (self.M,):
                raise ValueError(f"lam: a scalar or ({self.M},) expected, got {tuple(lam_t.shape)}")
            lam_t = lam_t.contiguous()
        st = self._step(lam_t, want_cov=True)
        return {k: st[k] for k in ("cov", "sigma", "logdet", "flag")}

    def proposal_factor(self, scale=None, box_prior=True):
        """The proposal of a Metropolis sampler from the Laplace approximation at the CURRENT point: dict(factor [M, Nu, Nu] lower
        triangular, flag [M] int32) on the device, no host synchronisation - ``MetropolisBatch.set_proposal(factor,
        chains_per_point)`` then proposes x + factor z at every chain of point m.  factor factor^T = scale^2 cov, cov = A^-1 of
        ``plan.step(..., want_cov=True)`` at lam = 0 (``surfdisp_mcmc_cov_factor_device``; a fixed parameter has a zero row and
        column and never moves).  ``box_prior``: the variance of the uniform prior box enters A as a Gaussian pull, prior_w_j + 12 /
        (vmax_j - vmin_j)^2 - a parameter the data do not constrain then gets the box's own spread instead of an unbounded one
        (without it such a parameter makes every Gaussian candidate leave the box).  ``scale``: None = 2.38 / sqrt(n_free), the
        optimal random-walk scaling of Roberts, Gelman and Gilks (1997).  A point whose step has flag != 0, or whose
        matrix cannot be factored, gets diag(spec.step) - the reference's proposal - and flag = 1."""
        torch = self.torch
        spec = self.model_batch.spec
        pw = self.prior_w
        if box_prior:
            w = torch.as_tensor(np.asarray(spec.vmax, np.float64) - np.asarray(spec.vmin, np.float64), device=self.device)
            pw = (pw + 12.0 / (w * w)).contiguous()
        kw = dict(prior_w=pw, prior_ref=self.prior_ref) if (box_prior or self.has_prior) else {}
        lam = torch.zeros(self.M, dtype=torch.float64, device=self.device)
        st = self.plan.step(self.params, lam, self.scale, free=self.free8, rows=self.rows, want_cov=True, **kw)
        cov = st["cov"]
        if scale is None:
            s = 2.38 / np.sqrt(np.maximum(self.n_free, 1))
            if np.ndim(s):                                                 # per-point masks: scaled here, the kernel takes one scalar
                cov, s = cov * torch.as_tensor(s * s, device=self.device)[:, None, None], 1.0
        else:
            s = float(scale)
        nan = torch.full((), float("nan"), dtype=torch.float64, device=self.device)
        cov = torch.where((st["flag"] != 0)[:, None, None], nan, cov)      # a flagged step left zeros: NaN takes the kernel's fallback
        from .mcmc import cov_factor
        return cov_factor(cov, float(s), np.asarray(spec.step, np.float64))

    def to_yml(self, point=None):
        """``Model1DBatch.to_yml`` of the current parameters: the dict of point ``point``, or the list over all points."""
        p = self.params.cpu().numpy()
        if point is not None:
            return self.model_batch.to_yml(p[int(point)])
        return [self.model_batch.to_yml(row) for row in p]
