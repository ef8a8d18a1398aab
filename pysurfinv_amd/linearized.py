"""Linearised inversion of the layers' shear velocities: the classical companion of the Metropolis sampler.

An iterated, damped, smoothed least-squares fit (Gauss-Newton with Levenberg-Marquardt damping, as in the surf96 family) of
the Vs of the FREE layers of every stack of a batch, fed by the analytic sensitivity kernels of the library (dc/dm, dU/dm,
dchi/dm for Rayleigh, dc/dm, dU/dm for Love) and solved on the device, one workgroup per stack
(``surfdisp_lsq_step_device``, csrc/surfdisp_lsq.hip).  Fundamental mode; the thicknesses are fixed unless THICKNESS MODES are
given (below).

One step, per stack, with x the Vs of the n free layers and x0 the current model:

    G[r, i] = K_b[r, i] + p_i K_a[r, i] + q_i K_rho[r, i]          (p, q: dVp/dVs, drho/dVs of layer i; 0 = held fixed)
    res_r   = obs_r - pred_r,    W = diag(w_r / uncer_r^2)
    (G^T W G + alpha D^T Q D + lam I) delta = G^T W res - alpha D^T Q D x0

D is the first difference between consecutive free layers, Q its weights (``consecutive_weights``), lam the damping of the
stack.

What the result is reported with (``surfdisp_lsq_resolution_device``, the same file): with H = G^T W G and A the matrix above, the
posterior covariance C = A^-1, the resolution matrix R = C H, the layers' standard errors sqrt(C_jj) and their data share
sqrt((C H C)_jj), dof = trace R and log det A.

Thickness modes (``surfdisp_lsq_step_modes_device`` / ``surfdisp_lsq_resolution_modes_device``, include/surfdisp.h section (6h)):
K <= 8 more unknowns per stack behind the Vs - mode k has a shape T_k [L] and an amplitude y_k in km, the thickness of layer i
changes by sum_k T_k[i] y_k (``thickness_mode``: a layer group thickens, everything below shifts; ``interface_mode``: the
interface between two groups moves, the total depth stays).  Its column is G[r, n + k] = sum_i dcdh[r, i] T_k[i] from the
thickness kernels of the phase velocity (``BatchPlan.run_thickness_kernels``), its damping lam mode_scale_k, its prior
mode_prior_k (y_k + delta_k)^2.  By default phase-velocity data only; with ``group_modes=True`` group-velocity sets are taken
next to modes, their columns from dudh (``BatchPlan.run_group_thickness_kernels``).  An ellipticity set is refused with modes
either way: the library has no dchi/dh.

The kernels are tested against ONE numpy float64 statement, ``_System``: (H, A, g) of n Vs unknowns followed by K >= 0 modes, K = 0
being the problem without modes.  ``lsq_modes_step_reference`` and ``lsq_modes_resolution_reference`` are the step and the resolution
read from it, with one solve block (A finite, Cholesky, flag 2 on failure, zeros on a flag); ``normal_equations``,
``modes_normal_equations``, ``lsq_step_reference`` and ``lsq_resolution_reference`` are calls of those.  The same holds on the device
side of the module: the rules of the mode arguments are ``_mode_count`` and ``_mode_data`` for ``LinearizedBatch`` and ``LsqPlan``
alike, and a call of ``LsqPlan.step`` or ``resolution``, with or without modes, is one ``_Launch``.

* ``LsqPlan``: the kernels + step (``step``) or covariance and resolution (``resolution``) of one batch as device tensors.
* ``LinearizedBatch``: the iteration - kernels and step at x, ONE forward solve of the trials, accept where the objective
  (chi-square of ``obsdata`` + alpha roughness) fell, lam down on accept, up on reject - without a host synchronisation.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

from . import _lib
from .obsdata import JointData

MAX_FREE = 128          # unknowns per stack the step and resolution kernels take (SD_LSQ_MAX_FREE)
MAX_MODES = 8           # thickness modes per stack behind them (SD_LSQ_MAX_MODES)
MODES_NEED_PHASE = "thickness modes need phase-velocity data only: the library has no dU/dh or dchi/dh yet"
MODES_NEED_NO_ELLIPTICITY = "thickness modes take phase- and group-velocity data (group_modes=True): the library has no dchi/dh"
FAIL = 88888.0          # the misfit of a failed solve (point.py:20-21)

# d(Vp, rho) / dVs of the layer groups of senskernel.GROUP_RULES (sensModel._convert)
GROUP_SLOPES = {"water": (0.0, 0.0), "sediment": (1.23, 0.3601 * 1.23), "crust": (1.8, 0.3601 * 1.8), "mantle": (1.76, 1.0 / 4.5)}


def group_slopes(grp):
    """(vp_slope, rho_slope) [L] of a list of layer group names: the slopes of ``senskernel.GROUP_RULES``."""
    try:
        s = np.array([GROUP_SLOPES[g] for g in grp], np.float64)
    except KeyError as e:
        raise ValueError(f"group_slopes: unknown layer group {e.args[0]!r} (expected {sorted(GROUP_SLOPES)})")
    return s[:, 0].copy(), s[:, 1].copy()


def consecutive_weights(free, Q=None):
    """Weights of the first differences between CONSECUTIVE FREE layers: ``free`` bool [L], ``Q`` [L-1] the weight of the
    interface between the layers k and k+1 (None: 1).  Two consecutive free layers a < b take min(Q[a:b]) - an interface of
    weight 0 anywhere between them cuts the smoothing.  Returns (layers [n], weights [n-1])."""
    idx = np.nonzero(np.asarray(free, bool))[0]
    Q = np.ones(max(len(free) - 1, 0)) if Q is None else np.asarray(Q, np.float64)
    w = np.array([Q[a:b].min() for a, b in zip(idx[:-1], idx[1:])], np.float64)
    return idx, w


def _group(name, h, layers):
    """The layer indices of one group of a mode shape, checked: not empty, inside the stack, without the last layer (the half
    space has no thickness), of positive total thickness."""
    idx = np.unique(np.asarray(layers, np.int64).ravel())
    if idx.size == 0:
        raise ValueError(f"{name}: an empty layer group")
    if idx[0] < 0 or idx[-1] >= h.size - 1:
        raise ValueError(f"{name}: layers {idx.tolist()} - a group lies in 0..{h.size - 2}, the last layer has no thickness")
    tot = float(h[idx].sum())
    if not (np.isfinite(tot) and tot > 0.0):
        raise ValueError(f"{name}: group thickness {tot}, a positive value expected")
    return idx, tot


def thickness_mode(h, layers):
    """Shape T [L] float64 of the mode "the group ``layers`` thickens by y km, everything below shifts rigidly": T[i] =
    h_i / sum(h[layers]) on the group, 0 elsewhere (the layers of the group keep their proportions; sum of T over the group 1).
    ``h`` [L]: the thicknesses of the stack, the last layer being the half space.  ValueError for an empty group, a group
    thickness that is not positive, a group that contains the last layer."""
    h = np.asarray(h, np.float64).ravel()
    idx, tot = _group("thickness_mode", h, layers)
    T = np.zeros(h.size)
    T[idx] = h[idx] / tot
    return T


def interface_mode(h, above, below):
    """Shape T [L] float64 of the mode "the interface between the groups ``above`` and ``below`` moves down by y km": +h_i /
    sum(h[above]) on ``above``, -h_i / sum(h[below]) on ``below`` - the upper group thickens by y, the lower one thins by y, the
    total depth does not change (a Moho, a sediment base, a sea floor).  ValueError as ``thickness_mode``, and for groups that
    share a layer."""
    h = np.asarray(h, np.float64).ravel()
    ia, ta = _group("interface_mode (above)", h, above)
    ib, tb = _group("interface_mode (below)", h, below)
    if np.intersect1d(ia, ib).size:
        raise ValueError("interface_mode: the two groups share a layer")
    T = np.zeros(h.size)
    T[ia] = h[ia] / ta
    T[ib] = -h[ib] / tb
    return T


def mode_columns(kh, T, nlay=None):
    """Gy [N, K] float64: the mode columns of N data rows - ``kh`` [N, L] their thickness kernels dcdh (float32 as the library
    returns them), ``T`` [K, L] the shapes; only the layers i < nlay - 1 are read (nlay None: L)."""
    kh = np.atleast_2d(np.asarray(kh)).astype(np.float64)
    T = np.atleast_2d(np.asarray(T, np.float64))
    m = max((kh.shape[1] if nlay is None else int(nlay)) - 1, 0)
    return kh[:, :m] @ T[:, :m].T


class _System:
    """The numpy float64 statement of one stack's problem, read by every reference below: n Vs unknowns x0 followed by K >= 0
    thickness modes (``Gy`` None or [N, 0]: K = 0, the plain case of the same lines).  With Ga = [G | Gy] and S = D^T Q D, D the
    first difference of consecutive Vs unknowns:

        H = Ga^T W Ga
        A = H,        its Vs block (H + alpha S) + lam I,    its mode diagonal + lam ms_k + beta_k
        g = Ga^T W r, its Vs part - alpha S x0,              its mode part - beta_k y_k

    G [N, n], Gy [N, K], r (None: zeros) and w_over_sigma2 [N], x0 [n], Q [n-1]; mode_scale ms, mode_prior beta, mode_y y:
    scalars or [K] (None: 1, 0, 0)."""

    def __init__(self, G, Gy, r, w_over_sigma2, x0, alpha, Q, lam, mode_scale=None, mode_prior=None, mode_y=None):
        self.x0 = x0 = np.asarray(x0, np.float64).ravel()
        self.n = n = x0.size
        self.G = G = np.asarray(G, np.float64).reshape(np.shape(G)[0] if n == 0 else -1, n)   # (n = 0: modes only, paramlsq)
        N = G.shape[0]
        if Gy is not None and np.ndim(Gy) != 2:
            raise ValueError("Gy: a [N, K] array expected")
        self.K = K = 0 if Gy is None else np.shape(Gy)[1]
        self.Gy = Gy = np.zeros((N, 0)) if Gy is None else np.asarray(Gy, np.float64).reshape(N, K)
        self.r = r = np.zeros(N) if r is None else np.asarray(r, np.float64).ravel()
        self.w = w = np.asarray(w_over_sigma2, np.float64).ravel()
        self.alpha, lam = float(alpha), float(lam)
        self.Q = np.asarray(Q, np.float64).ravel()[:max(n - 1, 0)]
        vec = lambda v, default: np.full(K, default) if v is None else np.broadcast_to(np.asarray(v, np.float64), (K,)).copy()
        ms, self.beta, self.y = vec(mode_scale, 1.0), vec(mode_prior, 0.0), vec(mode_y, 0.0)
        D = np.zeros((max(n - 1, 0), n))
        for k in range(n - 1):
            D[k, k], D[k, k + 1] = -1.0, 1.0
        S = D.T @ np.diag(self.Q) @ D
        Ga = np.concatenate([G, Gy], axis=1) if K else G
        self.H = Ga.T @ (w[:, None] * Ga)
        self.A = self.H.copy()
        self.A[:n, :n] = self.H[:n, :n] + self.alpha * S + lam * np.eye(n)
        self.A[n:, n:] += np.diag(lam * ms + self.beta)
        self.g = Ga.T @ (w * r)
        self.g[:n] -= self.alpha * (S @ x0)
        self.g[n:] -= self.beta * self.y

    def objective(self, misfit, x, y):
        """misfit + alpha roughness(x) + sum beta y^2."""
        return misfit + self.alpha * self.roughness(x) + float((self.beta * y * y).sum())

    def roughness(self, x):
        return float((self.Q * np.diff(x) ** 2).sum())

    def factor(self):
        """(flag, Lc) - the solve block of every reference: flag 1 and None without rows, flag 2 and None when A is not finite
        or its Cholesky factorisation fails, else 0 and the lower factor of A."""
        if self.G.shape[0] == 0:
            return 1, None
        try:
            if not np.isfinite(self.A).all():
                raise np.linalg.LinAlgError
            return 0, np.linalg.cholesky(self.A)
        except np.linalg.LinAlgError:
            return 2, None


def modes_normal_equations(G, Gy, r, w_over_sigma2, x0, alpha, Q, lam, mode_scale=None, mode_prior=None, mode_y=None):
    """(A, g) of the step with K >= 0 thickness modes behind the n Vs unknowns, numpy float64 (``_System``): A = [G | Gy]^T W [G | Gy]
    with alpha D^T Q D + lam I on the Vs block - D acts on the Vs unknowns only - and lam ms_k + beta_k on the diagonal of mode k;
    g = [G | Gy]^T W r with - alpha D^T Q D x0 on the Vs part and - beta_k y_k on mode k."""
    p = _System(G, Gy, r, w_over_sigma2, x0, alpha, Q, lam, mode_scale, mode_prior, mode_y)
    return p.A, p.g


def normal_equations(G, r, w_over_sigma2, x0, alpha, Q, lam):
    """(A, g) of the step, numpy float64: A = G^T W G + alpha D^T Q D + lam I, g = G^T W r - alpha D^T Q D x0.  G [N, n], r and
    w_over_sigma2 [N], x0 [n], Q [n-1] (weights of the differences of consecutive unknowns).  ``modes_normal_equations`` without
    modes."""
    return modes_normal_equations(G, None, r, w_over_sigma2, x0, alpha, Q, lam)


def lsq_modes_step_reference(G, r, w_over_sigma2, x0, alpha, Q, lam, Gy=None, mode_scale=None, mode_prior=None, mode_y=None):
    """One damped least-squares step of one stack in numpy float64 - the statement ``surfdisp_lsq_step_modes_device`` and, without
    modes, ``surfdisp_lsq_step_device`` are tested against.  G [N, n]: the effective Jacobian rows of the USED data rows, r [N] their
    residuals obs - pred, w_over_sigma2 [N], x0 [n] the free layers' Vs, Q [n-1] the weights of the differences of consecutive
    free layers, alpha, lam scalars; ``Gy`` [N, K]: the mode columns of the used rows (``mode_columns``; None: K = 0);
    mode_scale, mode_prior, mode_y: scalars or [K] (None: 1, 0, 0).  Returns dict(delta [n], delta_y [K], misfit = sum W r^2,
    roughness = x0^T D^T Q D x0, predicted = sum W (r - G delta - Gy delta_y)^2 + alpha roughness(x0 + delta) + sum beta
    (y + delta_y)^2, flag): flag 1 without rows, 2 when A is not finite or the Cholesky factorisation fails - then the deltas are
    zeros and predicted = misfit + alpha roughness + sum beta y^2."""
    p = _System(G, Gy, r, w_over_sigma2, x0, alpha, Q, lam, mode_scale, mode_prior, mode_y)
    n = p.n
    misfit = float((p.w * p.r * p.r).sum())
    out = dict(delta=np.zeros(n), delta_y=np.zeros(p.K), misfit=misfit, roughness=p.roughness(p.x0),
               predicted=p.objective(misfit, p.x0, p.y), flag=0)
    out["flag"], Lc = p.factor()
    if Lc is not None:
        d = np.linalg.solve(Lc.T, np.linalg.solve(Lc, p.g))
        t = p.r - p.G @ d[:n] - p.Gy @ d[n:]
        out.update(delta=d[:n], delta_y=d[n:], predicted=p.objective(float((p.w * t * t).sum()), p.x0 + d[:n], p.y + d[n:]))
    return out


def lsq_step_reference(G, r, w_over_sigma2, x0, alpha, Q, lam):
    """``lsq_modes_step_reference`` without modes - the statement ``surfdisp_lsq_step_device`` is tested against; the result has no
    delta_y."""
    out = lsq_modes_step_reference(G, r, w_over_sigma2, x0, alpha, Q, lam)
    del out["delta_y"]
    return out


def lsq_modes_resolution_reference(G, w_over_sigma2, x0_or_n, alpha, Q, lam, Gy=None, mode_scale=None, mode_prior=None):
    """Posterior covariance and resolution of one stack's damped, smoothed problem in numpy float64 - the statement
    ``surfdisp_lsq_resolution_modes_device`` and, without modes, ``surfdisp_lsq_resolution_device`` are tested against.  G, Gy,
    w_over_sigma2, Q, alpha, lam, mode_scale, mode_prior as ``lsq_modes_step_reference``; ``x0_or_n``: the Vs unknowns' vector or
    just their number n (the matrices do not depend on x0).  With H and A of ``_System`` over the n + K unknowns, the modes last:

        cov = A^-1,   res = cov H,   sigma_post = sqrt(diag cov),   sigma_data = sqrt(diag(res cov)),   rdiag = diag res,
        dof = trace res

    Returns dict(cov, res [n + K, n + K], sigma_post, sigma_data, rdiag [n + K], dof, logdet = log det A, flag): flag 1 without
    rows, 2 when the Cholesky factorisation fails or A, cov or res is not finite - then every array is zeros, dof and logdet 0."""
    n = int(x0_or_n) if np.ndim(x0_or_n) == 0 else np.size(x0_or_n)
    p = _System(G, Gy, None, w_over_sigma2, np.zeros(n), alpha, Q, lam, mode_scale, mode_prior)
    nu = n + p.K
    z = np.zeros(nu)
    out = dict(cov=np.zeros((nu, nu)), res=np.zeros((nu, nu)), sigma_post=z.copy(), sigma_data=z.copy(), rdiag=z.copy(), dof=0.0,
               logdet=0.0, flag=0)
    out["flag"], Lc = p.factor()
    if Lc is not None:
        T = np.linalg.solve(Lc, np.eye(nu))
        cov = T.T @ T
        cov = 0.5 * (cov + cov.T)
        res = cov @ p.H
        cd = np.einsum("ij,ji->i", res, cov)
        if not (np.isfinite(cov).all() and np.isfinite(res).all() and np.isfinite(cd).all()):
            out["flag"] = 2
            return out
        out.update(cov=cov, res=res, sigma_post=np.sqrt(np.diag(cov)), sigma_data=np.sqrt(np.maximum(cd, 0.0)), rdiag=np.diag(res).copy(),
                   dof=float(np.trace(res)), logdet=float(2.0 * np.log(np.diag(Lc)).sum()))
    return out


def lsq_resolution_reference(G, w_over_sigma2, x0_or_n, alpha, Q, lam):
    """``lsq_modes_resolution_reference`` without modes - the statement ``surfdisp_lsq_resolution_device`` is tested against: every
    array over the n Vs unknowns."""
    return lsq_modes_resolution_reference(G, w_over_sigma2, x0_or_n, alpha, Q, lam)


def _per_layer(name, v, M, L, cols=None):
    """A scalar, [cols] or [M, cols] argument as float64 (cols = L unless given); ValueError otherwise."""
    cols = L if cols is None else cols
    a = np.asarray(v, np.float64)
    if a.ndim == 0:
        return np.full(cols, float(a))
    if a.shape not in ((cols,), (M, cols)):
        raise ValueError(f"{name}: shape {a.shape}, expected a scalar, ({cols},) or ({M}, {cols})")
    return np.ascontiguousarray(a)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _ptrs(arrs):
    return (ctypes.c_void_p * len(arrs))(*[a.data_ptr() if a is not None else None for a in arrs])


def _mode_count(modes, B, L):
    """(K, per_stack) of a thickness-mode array or tensor: [K, L] or [B, K, L] with 1 <= K <= MAX_MODES, ValueError otherwise."""
    s = tuple(modes.shape)
    if len(s) not in (2, 3) or s[-1] != L or (len(s) == 3 and s[0] != B) or not 1 <= s[-2] <= MAX_MODES:
        raise ValueError(f"modes: shape {s}, expected (K, {L}) or ({B}, K, {L}) with 1 <= K <= {MAX_MODES}")
    return int(s[-2]), len(s) == 3


def _mode_data(jd, group_modes=False):
    """ValueError when the data hold a set thickness modes have no column for: they need dcdh (dudh) of every row.  Without
    ``group_modes`` that is a group-velocity or ellipticity set, with it an ellipticity set."""
    if group_modes:
        if any(d.quantity not in ("c", "U") for d in jd.datasets):
            raise ValueError(MODES_NEED_NO_ELLIPTICITY)
    elif any(d.quantity != "c" for d in jd.datasets):
        raise ValueError(MODES_NEED_PHASE)


@dataclasses.dataclass
class _Launch:
    """The checked arguments of one ``LsqPlan.step`` / ``resolution`` call after its ``kernels`` call.  ``head``: the arguments the four
    entries share, up to and including lam; ``mode_in``: the mode entries' inputs behind them, () when K = 0.  The two tuples
    keep their ctypes arrays alive."""
    nmax: int
    K: int
    pred: dict
    part: list
    part_h: list
    head: tuple
    mode_in: tuple

    def __call__(self, name, outs, mode_outs, tail):
        """surfdisp_lsq_<name>_device on the tensors ``outs`` + ``tail`` (None: NULL), or, with modes, surfdisp_lsq_<name>_modes_device
        with ``mode_outs`` between the two."""
        fn = getattr(_lib.lib(), f"surfdisp_lsq_{name}{'_modes' if self.K else ''}_device")
        _lib.check(fn(*self.head, *self.mode_in, *map(_ptr, outs + (mode_outs if self.K else []) + tail)))


class LsqPlan:
    """The sensitivity kernels and the least-squares step of B stacks of L layers against ``datasets`` (``obsdata``
    ``DispersionData`` sets, their dict form, or a ``JointData`` of them), on ``device``.  Owns the ``BatchPlan`` of each wave type
    with data, the ``JointData`` table and the output buffers.  ``mask``: bool [Ptot] or [B, Ptot], rows to leave out on top of the
    data's own unusable entries (columns in data-set order).  ``group_modes``: thickness modes are taken next to
    group-velocity sets (see ``kernels``); False keeps them to phase-velocity data."""

    def __init__(self, B, L, datasets, device="cuda:0", mask=None, group_modes=False):
        import torch
        self.torch = torch
        self.B, self.L = int(B), int(L)
        self.group_modes = bool(group_modes)
        self.joint = jd = datasets if isinstance(datasets, JointData) else JointData(datasets, device="cpu")
        if jd.C is not None and jd.C != self.B:
            raise ValueError(f"per-stack data of {jd.C} rows against {self.B} stacks")
        obs, unc = np.asarray(jd.obs_raw, np.float64), np.asarray(jd.uncer_raw, np.float64)
        ok = np.isfinite(obs) & np.isfinite(unc) & (unc > 0)              # the rule of DispersionData
        if mask is not None:
            m = np.asarray(mask, bool)
            if m.shape not in ((jd.Ptot,), (self.B, jd.Ptot)):
                raise ValueError(f"mask: shape {m.shape}, expected ({jd.Ptot},) or ({self.B}, {jd.Ptot})")
            if m.ndim == 2 and obs.ndim == 1:
                obs, unc, ok = (np.broadcast_to(a, (self.B, jd.Ptot)) for a in (obs, unc, ok))
            ok = ok & m
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SurfdispError("LsqPlan needs a HIP device (no CPU fallback)")
        from .forward import BatchPlan
        jd.to(self.device)
        dev = self.device
        self.mask = torch.as_tensor(np.ascontiguousarray(ok), device=dev)
        self.obs = torch.as_tensor(np.where(ok, obs, 0.0), device=dev).contiguous()
        self.uncer = torch.as_tensor(np.where(ok, unc, 1.0), device=dev).contiguous()
        self.mask8 = self.mask.to(torch.uint8).contiguous()
        self.plans = {w: BatchPlan(self.B, self.L, jd.solve_periods[w].size, device=dev) for w in jd.waves}
        self._buffers = {}
        self.delta, self.stats = self._buffer("delta", self.B, self.L), self._buffer("stats", self.B, 3)
        self.info = self._buffer("info", self.B, 3, dtype=torch.int32)
        self._sets = {w: {d.quantity for d in jd.datasets if d.wave == w} for w in jd.waves}

    def _buffer(self, name, *shape, dtype=None, fill=0):
        """The plan's buffer ``name``: allocated (filled with ``fill``) at its first use and again when another shape is asked for.
        The entries rewrite an output buffer as a whole at every call."""
        t = self._buffers.get(name)
        if t is None or tuple(t.shape) != shape:
            t = self._buffers[name] = self.torch.full(shape, fill, dtype=dtype or self.torch.float64, device=self.device)
        return t

    def check_modes(self):
        """ValueError when the data hold a set thickness modes have no column for (``_mode_data``)."""
        _mode_data(self.joint, self.group_modes)

    def kernels(self, model, nlay=None, want_vp=True, want_rho=True, thickness=False):
        """The kernel entries the data need, once per wave type: U data -> ``run_group_kernels``, an "E" set ->
        ``run_ellip_kernels``, both -> both calls (``senskernel.analytic_kernels``), otherwise ``run_kernels``.  Returns (pred,
        part): the forward dict of ``JointData.predictions`` (the plans' own output tensors) and the 15 partial arrays
        [source 0..4][Vs, Vp, rho] (None where absent).  ``thickness`` (no "E" set; U sets with ``group_modes`` only):
        ``run_thickness_kernels`` in place of ``run_kernels`` - the same bits plus dcdh - or, for a wave type with U data,
        ``run_group_thickness_kernels`` in place of ``run_group_kernels`` - the same bits plus dcdh and dudh - and a third
        result, the five thickness arrays [source 0..4] (cR, uR, cL, uL; None where absent).  No host synchronisation."""
        jd = self.joint
        pred = dict(cR=None, uR=None, cL=None, uL=None, statusR=None, statusL=None, eR=None)
        part, part_h = [None] * 15, [None] * 5
        if thickness:
            self.check_modes()
        for w in jd.waves:
            plan, per, q = self.plans[w], jd.periods_t[w], self._sets[w]
            kw = dict(kind=_lib.KIND_RAYLEIGH if w == "R" else _lib.KIND_LOVE, nlay=nlay, want_vp=want_vp, want_rho=want_rho)
            o = 0 if w == "R" else 6
            if thickness and "U" in q:
                c, u, st, kb, ka, kr, ub, ua, ur, kh, _, uh, _, _, _ = plan.run_group_thickness_kernels(
                    model, per, want_dcdz=False, want_dudz=False, count=False, **kw)
                part[o + 3:o + 6] = [ub, ua, ur]
                part_h[o // 3], part_h[o // 3 + 1] = kh, uh
                pred["u" + w] = u
            elif thickness:
                c, u, st, kb, ka, kr, kh, _, _ = plan.run_thickness_kernels(model, per, want_dcdz=False, count=False, **kw)
                part_h[o // 3] = kh
            elif not q & {"U", "E"}:
                c, u, st, kb, ka, kr = plan.run_kernels(model, per, **kw)
            if "U" in q and not thickness:
                c, u, st, kb, ka, kr, ub, ua, ur, _ = plan.run_group_kernels(model, per, count=False, **kw)
                part[o + 3:o + 6] = [ub, ua, ur]
                pred["u" + w] = u
            if "E" in q:
                c, u, st, ratio, kb, ka, kr, eb, ea, er, _ = plan.run_ellip_kernels(model, per, count=False, **kw)
                part[12:15] = [eb, ea, er]
                pred["eR"] = ratio
            part[o:o + 3] = [kb, ka, kr]
            pred["c" + w], pred["status" + w] = c, st
        return (pred, part, part_h) if thickness else (pred, part)

    def _prepare(self, model, lam, nlay, free, nfree_max, vp_slope, rho_slope, alpha, Q, modes, mode_scale, mode_prior, mode_y):
        """The argument checks of ``step`` / ``resolution`` and one call of ``kernels`` -> the ``_Launch`` of the call."""
        torch = self.torch
        B, L, dev = self.B, self.L, self.device

        def chk(name, t, dtype, *shapes):
            """0 for None or the first of ``shapes``, 1 for the second; ValueError for another shape, dtype, device or layout."""
            if t is None:
                return 0
            if t.dtype != dtype or t.device != dev or not t.is_contiguous() or tuple(t.shape) not in shapes:
                raise ValueError(f"{name}: expected contiguous {dtype} {' or '.join(map(str, shapes))} on {dev}, got {t.dtype} "
                                 f"{tuple(t.shape)}")
            return shapes.index(tuple(t.shape))

        K, m_ps = 0, 0
        if modes is not None:
            self.check_modes()
            K, m_ps = _mode_count(modes, B, L)
            chk("modes", modes, torch.float64, tuple(modes.shape))
            per_mode = (B, K) if m_ps else (K,)
            if mode_scale is None:
                mode_scale = self._buffer("mode_scale", *per_mode, fill=1.0)
            chk("mode_scale", mode_scale, torch.float64, per_mode)
            chk("mode_prior", mode_prior, torch.float64, per_mode)
            chk("mode_y", mode_y, torch.float64, (B, K))
        nmax = L if nfree_max is None else int(nfree_max)
        if not 1 <= nmax <= min(MAX_FREE, L):
            raise ValueError(f"nfree_max = {nmax}: the step kernel takes 1..{min(MAX_FREE, L)} free layers per stack (give nfree_max "
                             "when L > 128)")
        free_ps = chk("free", free, torch.uint8, (L,), (B, L))
        sl_ps = chk("vp_slope", vp_slope, torch.float64, (L,), (B, L))
        if rho_slope is not None and vp_slope is not None and rho_slope.ndim != vp_slope.ndim:
            raise ValueError("vp_slope and rho_slope: both [L] or both [B, L]")
        sl_ps = max(sl_ps, chk("rho_slope", rho_slope, torch.float64, (L,), (B, L)))
        q_ps = chk("Q", Q, torch.float64, (L - 1,), (B, L - 1)) if L > 1 else 0
        chk("lam", lam, torch.float64, (B,))
        kern = self.kernels(model, nlay, want_vp=vp_slope is not None, want_rho=rho_slope is not None, thickness=K > 0)
        pred, part, part_h = kern if K else (*kern, None)
        jd = self.joint
        arrs = [pred["cR"], pred["uR"], pred["cL"], pred["uL"], pred["eR"]]
        strides = (ctypes.c_long * 5)(*[a.stride(0) if a is not None else 0 for a in arrs])
        nper = (ctypes.c_int * 2)(*[int(jd.solve_periods[w].size) if w in jd.solve_periods else 0 for w in ("R", "L")])
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        head = (stream, B, L, _ptr(nlay), _ptr(model), _ptr(free), free_ps, nmax, _ptrs(part), _ptrs(arrs), strides, nper,
                jd.Ptot, _ptr(jd.cols), _ptr(jd.weights), _ptr(self.obs), _ptr(self.uncer), _ptr(self.mask8),
                1 if self.obs.ndim == 2 else 0, _ptr(vp_slope), _ptr(rho_slope), sl_ps, float(alpha), _ptr(Q), q_ps, _ptr(lam))
        mode_in = (K, _ptr(modes), int(m_ps), _ptrs(part_h), _ptr(mode_scale), _ptr(mode_prior), _ptr(mode_y)) if K else ()
        return _Launch(nmax, K, pred, part, part_h, head, mode_in)

    def step(self, model, lam, nlay=None, free=None, nfree_max=None, vp_slope=None, rho_slope=None, alpha=0.0, Q=None,
             modes=None, mode_scale=None, mode_prior=None, mode_y=None):
        """Kernels at ``model`` (float32 [B, 5, L]) and one least-squares step.  Device tensors: ``lam`` float64 [B]; ``nlay``
        int32 [B]; ``free`` uint8 [L] or [B, L] (None: every layer); ``vp_slope`` / ``rho_slope`` float64 [L] or [B, L] (None:
        held fixed, the Vp / rho partials are not computed); ``Q`` float64 [L-1] or [B, L-1] (None: 1).  ``nfree_max``: an
        upper bound of the free layers of any stack (default L; at most 128).  Returns dict(delta [B, L] float64, misfit,
        roughness, predicted [B] float64, used, dropped, flag [B] int32, pred, part) - views of the plan's buffers, rewritten by
        the next call.  Flags: 0 solved, 1 no usable row, 2 pivot <= 0 or not finite, 3 more free layers than nfree_max.
        Thickness modes (``surfdisp_lsq_step_modes_device``; phase-velocity data, group-velocity data too on a plan with
        ``group_modes``, ValueError otherwise): ``modes`` float64
        [K, L] or [B, K, L], ``mode_scale`` and ``mode_prior`` float64 [K] ([B, K] with per-stack modes; None: 1 and 0),
        ``mode_y`` float64 [B, K] (None: 0); the result then holds delta_y [B, K] float64 and part_h, the five thickness
        arrays, as well.  Without ``modes`` the entry without modes is launched."""
        call = self._prepare(model, lam, nlay, free, nfree_max, vp_slope, rho_slope, alpha, Q, modes, mode_scale, mode_prior, mode_y)
        out = dict(delta=self.delta, misfit=self.stats[:, 0], roughness=self.stats[:, 1], predicted=self.stats[:, 2],
                   used=self.info[:, 0], dropped=self.info[:, 1], flag=self.info[:, 2], pred=call.pred, part=call.part)
        if call.K:
            out.update(delta_y=self._buffer("delta_y", self.B, call.K), part_h=call.part_h)
        with self.torch.cuda.device(self.device):
            call("step", [self.delta], [out.get("delta_y")], [self.stats, self.info])
        return out

    def resolution(self, model, lam, nlay=None, free=None, nfree_max=None, vp_slope=None, rho_slope=None, alpha=0.0, Q=None,
                   want_cov=True, want_res=True, modes=None, mode_scale=None, mode_prior=None, mode_y=None):
        """Kernels at ``model`` and the posterior covariance and resolution of the step's problem there
        (``surfdisp_lsq_resolution_device``; arguments as ``step``): with H = G^T W G and A = H + alpha D^T Q D + lam I, cov = A^-1,
        res = cov H.  One ``kernels`` call, one launch, no host synchronisation.  Returns dict(cov, res [B, nmax, nmax] float64 in
        unknown order (zeros beyond a stack's unknowns; None when not wanted), sigma_post = sqrt(diag cov), sigma_data =
        sqrt(diag(cov H cov)), rdiag = diag res [B, L] float64 (0 at layers that are not free), dof = trace res, logdet = log det A
        [B] float64, used, dropped, flag [B] int32 (flags as ``step``; every output of a stack with a flag is zeros), free_index
        [B, nmax] int64 (layer of unknown j, -1 as padding), nfree [B] int64, pred, part) - the plan's buffers, allocated at
        the first call and rewritten by the next.
        Thickness modes (``surfdisp_lsq_resolution_modes_device``; arguments as ``step``, ``mode_y`` is not read): cov and res are
        [B, nmax + K, nmax + K], the K modes behind a stack's n Vs unknowns (zeros beyond n + K); dof and logdet are over all
        unknowns; the result holds sigma_post_y, sigma_data_y, rdiag_y [B, K] float64 and part_h as well."""
        torch = self.torch
        call = self._prepare(model, lam, nlay, free, nfree_max, vp_slope, rho_slope, alpha, Q, modes, mode_scale, mode_prior, mode_y)
        B, L, nmax, K, dev = self.B, self.L, call.nmax, call.K, self.device
        cov, res = (self._buffer(k, B, nmax + K, nmax + K) if want else None for k, want in (("cov", want_cov), ("res", want_res)))
        per_layer = {k: self._buffer("res_" + k, B, L) for k in ("sigma_post", "sigma_data", "rdiag")}
        per_mode = {k + "_y": self._buffer("res_" + k + "_y", B, K) for k in per_layer} if K else {}
        stats, info = self._buffer("res_stats", B, 2), self._buffer("res_info", B, 3, dtype=torch.int32)
        with torch.cuda.device(dev):
            call("resolution", [cov, res, *per_layer.values()], [*per_mode.values()], [stats, info])
        lay = torch.arange(L, device=dev)
        fr = torch.ones(B, L, dtype=torch.bool, device=dev) if free is None else (free != 0).expand(B, L)
        if nlay is not None:
            fr = fr & (lay[None, :] < nlay[:, None])
        order = torch.where(fr, lay[None, :], L).sort(dim=1).values[:, :nmax]
        extra = dict(per_mode, part_h=call.part_h) if K else {}
        return dict(cov=cov, res=res, **per_layer, dof=stats[:, 0], logdet=stats[:, 1], used=info[:, 0], dropped=info[:, 1],
                    flag=info[:, 2], free_index=torch.where(order < L, order, -1), nfree=fr.sum(dim=1), pred=call.pred, part=call.part,
                    **extra)

    def forward(self, model, nlay=None):
        """ONE forward solve per wave type of ``model`` (``BatchPlan.run``, with the ratio when an "E" set is present; kind
        flags of ``JointData.kind``) -> the forward dict of ``JointData.predictions``."""
        jd = self.joint
        out = dict(cR=None, uR=None, cL=None, uL=None, statusR=None, statusL=None, eR=None)
        for w in jd.waves:
            res = self.plans[w].run(model, jd.periods_t[w], kind=jd.kind(w), nlay=nlay, want_ratio=jd.with_ratio and w == "R")
            out["c" + w], out["u" + w], out["status" + w] = res[:3]
            if len(res) > 3:
                out["eR"] = res[3]
        return out

    def chi_square(self, model, nlay=None):
        """(chi2, rms, failed) [B] of ``model`` by the definition of ``obsdata``: chi2 = sum_d w_d sum ((obs - pred) / uncer)^2
        over the usable entries, rms = sqrt(chi2 / N) with N their count (88888 for a failed solve - status, c < 0.01, a group
        velocity or ellipticity the data read: the rule of the module ``obsdata``)."""
        torch = self.torch
        cP, failed = self.joint.predictions(self.forward(model, nlay))
        r = torch.where(self.mask, (self.obs - cP) / self.uncer, torch.zeros_like(cP))
        chi = (self.joint.weights * r * r).sum(dim=1)
        N = self.mask.sum(dim=-1).to(torch.float64)
        rms = torch.where(failed, torch.full_like(chi, FAIL), torch.sqrt(chi / N))
        return chi, rms, failed


class LinearizedBatch:
    """Damped least-squares inversion of the Vs of M stacks at once.

    ``model0`` float32 [M, 5, L] (vp, vs, rho, h, 1/Qs; numpy or torch): the starting models.  ``datasets``: as
    ``MetropolisBatch(data=...)``.  ``free`` bool [L] or [M, L]: the layers whose Vs is an unknown (default: every layer with
    Vs > 0 above the half space, plus the half space); at most 128 per stack.  ``vp_slope`` / ``rho_slope``: dVp/dVs and
    drho/dVs, a scalar, [L] or [M, L] (default 0: Vp and rho stay fixed; ``group_slopes`` gives the slopes of
    ``senskernel.GROUP_RULES``).  ``alpha``: weight of the roughness; ``Q`` [L-1] or [M, L-1]: weights of the layer
    interfaces (0 cuts the smoothing across a discontinuity; ``consecutive_weights``).  ``lam0``, ``nu``, ``lam_min``: the
    Levenberg-Marquardt damping and its factor.  ``vs_bounds`` = (lo, hi), scalars or arrays that broadcast to [M, L]: the
    trial Vs of the free layers is clamped into them.  ``nlay`` int [M]: layers of each stack.  ``mask``: see ``LsqPlan``.

    ``run(n_iter)``, per iteration and with no host synchronisation (everything is ``torch.where`` on device tensors):
    kernels and step at x; trial = clamp(x + delta), Vp and rho moved along their slopes by the Vs change; ONE forward solve of
    the trials; objective = chi-square + alpha roughness of the trial, by the misfit rule of ``obsdata`` (a failed solve is a
    rejected trial: its objective is inf); per stack, where the objective fell: accept, lam <- max(lam / nu, lam_min), else keep
    x and lam <- lam nu.  A rejected stack's kernels are computed again in the next iteration although x did not move (they
    are not cached per stack): the batch stays one launch, and a rejected step is the rare case.

    Thickness modes (phase-velocity data only; with ``group_modes=True`` group-velocity data as well, never an ellipticity
    set): ``modes`` [K, L] or [M, K, L], the shapes (``thickness_mode``,
    ``interface_mode``; entries at layers >= nlay - 1 are set to 0); ``mode_scale`` (> 0) and ``mode_prior`` (>= 0): a scalar,
    [K] or [M, K]; ``mode_bounds`` = (lo, hi), scalars or arrays that broadcast to [M, K], on the amplitude ``y`` [M, K]
    accumulated since ``model0`` (km); ``h_min`` (km).  The trial then also has h <- float32(h + T (y_new - y)) with y_new =
    clamp(y + delta_y), it is rejected (objective inf) when a layer with a non-zero shape entry would be thinner than ``h_min``,
    and the objective is chi-square + alpha roughness + sum_k mode_prior_k y_k^2."""

    def __init__(self, model0, datasets, free=None, vp_slope=0.0, rho_slope=0.0, alpha=1.0, Q=None, lam0=1.0, nu=4.0,
                 lam_min=1e-9, vs_bounds=None, nlay=None, mask=None, device="cuda:0", modes=None, mode_scale=1.0, mode_prior=0.0,
                 mode_bounds=None, h_min=1e-3, group_modes=False):
        m0 = model0.detach().cpu().numpy() if hasattr(model0, "detach") else np.asarray(model0)
        if m0.ndim != 3 or m0.shape[1] != 5:
            raise ValueError("model0 must be [M, 5, L]")
        m0 = np.ascontiguousarray(m0, np.float32)
        M, _, L = m0.shape
        self.M, self.L = M, L
        nl = np.full(M, L, np.int64) if nlay is None else np.asarray(nlay, np.int64).ravel()
        if nl.size != M or (nl < 2).any() or (nl > L).any():
            raise ValueError(f"nlay: {M} entries in 2..{L} expected")
        inside = np.arange(L)[None, :] < nl[:, None]
        if free is None:
            fr = (m0[:, 1, :] > 0) | (np.arange(L)[None, :] == nl[:, None] - 1)
        else:
            fr = np.asarray(free, bool)
            if fr.shape not in ((L,), (M, L)):
                raise ValueError(f"free: shape {fr.shape}, expected ({L},) or ({M}, {L})")
            fr = np.broadcast_to(fr, (M, L))
        fr = fr & inside
        nfree = fr.sum(axis=1)
        if nfree.max() > MAX_FREE:
            raise ValueError(f"{int(nfree.max())} free layers in a stack: the step kernel takes at most {MAX_FREE}")
        if nfree.max() < 1:
            raise ValueError("no free layer")
        self.nfree_max = int(nfree.max())
        ps = _per_layer("vp_slope", vp_slope, M, L)
        qs = _per_layer("rho_slope", rho_slope, M, L)
        Qa = None if Q is None else _per_layer("Q", Q, M, L, cols=L - 1)
        if not (np.isfinite(alpha) and alpha >= 0):
            raise ValueError("alpha must be finite and >= 0")
        if not (lam0 > 0 and nu > 1 and lam_min >= 0):
            raise ValueError("lam0 > 0, nu > 1, lam_min >= 0 expected")
        self.alpha, self.nu, self.lam_min = float(alpha), float(nu), float(lam_min)
        # the differences of consecutive free layers, padded to nfree_max - 1 per stack (weight 0 on the padding)
        K = max(self.nfree_max - 1, 1)
        ia, ib, qw = np.zeros((M, K), np.int64), np.zeros((M, K), np.int64), np.zeros((M, K))
        for m in range(M):
            idx, w = consecutive_weights(fr[m], None if Qa is None else (Qa if Qa.ndim == 1 else Qa[m]))
            ia[m, :w.size], ib[m, :w.size], qw[m, :w.size] = idx[:-1], idx[1:], w
        if vs_bounds is not None:
            lo, hi = (np.broadcast_to(np.asarray(b, np.float64), (M, L)) for b in vs_bounds)
        if modes is not None:
            T = np.array(modes, np.float64)
            K, per_stack = _mode_count(T, M, L)
            if not per_stack and nlay is not None:
                T, per_stack = np.broadcast_to(T, (M, K, L)).copy(), True
            if per_stack:
                T[~np.broadcast_to((np.arange(L)[None, :] < nl[:, None] - 1)[:, None, :], T.shape)] = 0.0
            else:
                T[:, L - 1] = 0.0
            if not np.isfinite(T).all():
                raise ValueError("modes: entries that are not finite")
            shape = (M, K) if per_stack else (K,)

            def per_mode(name, v):
                a = np.asarray(v, np.float64)
                if a.shape not in ((), (K,), shape):
                    raise ValueError(f"{name}: shape {a.shape}, expected a scalar, ({K},) or ({M}, {K}) (per stack only with per-stack modes)")
                return np.array(np.broadcast_to(a, shape))
            m_scale, m_prior = per_mode("mode_scale", mode_scale), per_mode("mode_prior", mode_prior)
            if not ((m_scale > 0).all() and np.isfinite(m_scale).all() and (m_prior >= 0).all() and np.isfinite(m_prior).all()):
                raise ValueError("mode_scale > 0 and mode_prior >= 0, finite, expected")
            if mode_bounds is not None:
                ylo, yhi = (np.array(np.broadcast_to(np.asarray(b, np.float64), (M, K))) for b in mode_bounds)
            if not (np.isfinite(h_min) and h_min >= 0):
                raise ValueError("h_min must be finite and >= 0")
        jd = JointData(datasets, device="cpu")                                    # (data errors: ValueError)
        if modes is not None:
            _mode_data(jd, group_modes)
        self.plan = plan = LsqPlan(M, L, jd, device=device, mask=mask, group_modes=group_modes)            # (no HIP device: SurfdispError)
        import torch
        self.torch = torch
        dev = self.device = plan.device
        t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), device=dev) if dt is None else \
            torch.as_tensor(np.ascontiguousarray(a), device=dev).to(dt).contiguous()
        self.model = t(m0)
        self.nlay = None if nlay is None else t(nl, torch.int32)
        self.free = t(fr)
        self.free8 = t(fr.astype(np.uint8))
        self.has_vp, self.has_rho = bool((ps != 0).any()), bool((qs != 0).any())
        self.vp_slope, self.rho_slope = t(ps), t(qs)
        self.Q = None if Qa is None else t(Qa)
        self._ia, self._ib, self._qw = t(ia), t(ib), t(qw)
        self.bounds = None if vs_bounds is None else (t(lo), t(hi))
        self.lam = torch.full((M,), float(lam0), dtype=torch.float64, device=dev)
        self.modes = None
        if modes is not None:
            self.modes, self.mode_scale, self.mode_prior = t(T), t(m_scale), t(m_prior)
            self._touched = t((T != 0).any(axis=-2))                       # [L] or [M, L]: layers a mode moves
            self.mode_bounds = None if mode_bounds is None else (t(ylo), t(yhi))
            self.h_min = float(h_min)
            self.y = torch.zeros(M, K, dtype=torch.float64, device=dev)
        chi, rms, failed = plan.chi_square(self.model, self.nlay)
        self.objective = torch.where(failed, torch.full_like(chi, float("inf")), chi + self.alpha * self.roughness(self.model))
        self.rms = rms

    def roughness(self, model):
        """x^T D^T Q D x [M] float64 of the free layers' Vs of ``model`` [M, 5, L]."""
        vs = model[:, 1, :].to(self.torch.float64)
        d = vs.gather(1, self._ib) - vs.gather(1, self._ia)
        return (self._qw * d * d).sum(dim=1)

    def trial(self, model, delta):
        """model with Vs + delta on the free layers (clamped into ``vs_bounds``), Vp and rho moved along their slopes by the Vs
        change that float32 holds."""
        torch = self.torch
        vs = model[:, 1, :].to(torch.float64)
        nv = vs + delta
        if self.bounds is not None:
            nv = torch.minimum(torch.maximum(nv, self.bounds[0]), self.bounds[1])
        nv32 = torch.where(self.free, nv.to(torch.float32), model[:, 1, :])
        out = model.clone()
        out[:, 1, :] = nv32
        dv = nv32.to(torch.float64) - vs
        if self.has_vp:
            out[:, 0, :] = (model[:, 0, :].to(torch.float64) + self.vp_slope * dv).to(torch.float32)
        if self.has_rho:
            out[:, 2, :] = (model[:, 2, :].to(torch.float64) + self.rho_slope * dv).to(torch.float32)
        return out

    def _mode_kw(self):
        """The thickness-mode arguments of ``LsqPlan.step`` / ``resolution`` at the current state ({} without modes)."""
        if self.modes is None:
            return {}
        return dict(modes=self.modes, mode_scale=self.mode_scale, mode_prior=self.mode_prior, mode_y=self.y)

    def move_modes(self, model, delta_y):
        """(h [M, L] float32, y_new [M, K], thin [M] bool) of the mode step ``delta_y`` from the current ``y``: y_new = y + delta_y
        clamped into ``mode_bounds``, h = float32(h + sum_k T_k (y_new - y)_k) (the sum taken mode by mode, in float64), thin:
        a layer that a mode moves would be thinner than ``h_min``."""
        torch = self.torch
        y_new = self.y + delta_y
        if self.mode_bounds is not None:
            y_new = torch.minimum(torch.maximum(y_new, self.mode_bounds[0]), self.mode_bounds[1])
        dy = y_new - self.y
        T = self.modes if self.modes.ndim == 3 else self.modes[None]
        upd = T[:, 0, :] * dy[:, 0, None]
        for k in range(1, T.shape[1]):
            upd = upd + T[:, k, :] * dy[:, k, None]
        h = (model[:, 3, :].to(torch.float64) + upd).to(torch.float32)
        thin = (self._touched & (h.to(torch.float64) < self.h_min)).any(dim=-1)
        return h, y_new, thin

    def run(self, n_iter, keep_models=False):
        """``n_iter`` iterations from the current state (a second call goes on).  Returns dict(model [M, 5, L] the final models;
        per iteration, [n_iter, M]: objective and rms (the data rms misfit sqrt(chi2 / N) of ``obsdata``; 88888 for a model
        whose solve fails) of the state AFTER the iteration, lam after its update, accepted (bool), flag, used, dropped (of the
        step), predicted (the step's linear prediction of the objective); models [n_iter, M, 5, L] with ``keep_models``).  With
        thickness modes also y [n_iter, M, K], the amplitudes after each iteration (``self.y`` holds the current ones)."""
        torch = self.torch
        plan = self.plan
        with_modes = self.modes is not None
        keys = ("objective", "rms", "lam", "accepted", "flag", "used", "dropped", "predicted") + (("y",) if with_modes else ())
        hist = {k: [] for k in keys}
        models = []
        inf = torch.full((self.M,), float("inf"), dtype=torch.float64, device=self.device)
        for _ in range(int(n_iter)):
            st = plan.step(self.model, self.lam, nlay=self.nlay, free=self.free8, nfree_max=self.nfree_max,
                           vp_slope=self.vp_slope if self.has_vp else None, rho_slope=self.rho_slope if self.has_rho else None,
                           alpha=self.alpha, Q=self.Q, **self._mode_kw())
            flag, used, dropped, predicted = (st[k].clone() for k in ("flag", "used", "dropped", "predicted"))
            tr = self.trial(self.model, st["delta"])
            if with_modes:
                tr[:, 3, :], y_new, thin = self.move_modes(self.model, st["delta_y"])
            chi, rms, failed = plan.chi_square(tr, self.nlay)
            obj = torch.where(failed, inf, chi + self.alpha * self.roughness(tr))
            if with_modes:
                obj = torch.where(thin, inf, obj + (self.mode_prior * y_new * y_new).sum(dim=1))
            acc = obj < self.objective
            self.model = torch.where(acc[:, None, None], tr, self.model)
            self.objective = torch.where(acc, obj, self.objective)
            self.rms = torch.where(acc, rms, self.rms)
            self.lam = torch.where(acc, torch.clamp(self.lam / self.nu, min=self.lam_min), self.lam * self.nu)
            if with_modes:
                self.y = torch.where(acc[:, None], y_new, self.y)
            for k, v in zip(keys, (self.objective, self.rms, self.lam, acc, flag, used, dropped, predicted) + ((self.y,) if with_modes else ())):
                hist[k].append(v)
            if keep_models:
                models.append(self.model)
        out = {k: torch.stack(v) for k, v in hist.items()} if n_iter > 0 else {}
        out["model"] = self.model
        if keep_models:
            out["models"] = torch.stack(models)
        return out

    def resolution(self, lam=None, want_cov=True, want_res=True):
        """Posterior covariance and resolution of the linearised problem at the CURRENT model (``LsqPlan.resolution``): the
        Gaussian approximation of the posterior the iteration ends on.  ``lam``: the damping - None: the batch's current
        ``lam``; a scalar or [M]; 0.0 leaves the smoothing as the only regularisation (a singular A is flag 2).  Does not advance
        the iteration: ``model``, ``lam`` and ``objective`` stay as they are.  No host synchronisation."""
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
        return self.plan.resolution(self.model, lam_t, nlay=self.nlay, free=self.free8, nfree_max=self.nfree_max,
                                    vp_slope=self.vp_slope if self.has_vp else None,
                                    rho_slope=self.rho_slope if self.has_rho else None, alpha=self.alpha, Q=self.Q,
                                    want_cov=want_cov, want_res=want_res, **self._mode_kw())
