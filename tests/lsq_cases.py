"""What the tests of the least-squares inversion (tests/test_lsq*.py) share: their random problems, the rows of a stack by the rules
of include/surfdisp.h section (6d), the recovery problem of the iteration, and ONE launch of the four C entries
(surfdisp_lsq_step_device, surfdisp_lsq_resolution_device and their _modes_ forms).  A plain module, not a conftest."""
import ctypes

import numpy as np

from pysurfinv_amd import _lib, linearized, synth
from pysurfinv_amd.obsdata import DispersionData

CASES = [(1, 2, 1), (5, 3, 7), (3, 17, 40), (2, 64, 100), (2, 96, 100), (1, 128, 256), (300, 9, 12)]       # (B, Lmax, N)
NU, LAM0, LAM_MIN, ALPHA, N_ITER = 4.0, 1.0, 1e-9, 0.05, 8                                                # the iteration
SETS3 = (("R", "c"), ("R", "U"), ("L", "c"))
LAM_FACTOR = 30.0      # the damping of a mode case over that of ``_case`` (see _mode_case)
KEY = {("R", "c"): "cR", ("R", "U"): "uR", ("L", "c"): "cL", ("R", "E"): "eR"}                            # forward dict key of a set

INPUTS = ("nlay", "model", "free", "cols", "weights", "obs", "uncer", "mask", "vp_slope", "rho_slope", "Q")
MODE_INPUTS = ("modes", "mode_scale", "mode_prior", "mode_y")
# entry -> (C symbol, output names in argument order)
ENTRIES = {
    "step": ("surfdisp_lsq_step_device", ("delta", "stats", "info")),
    "res": ("surfdisp_lsq_resolution_device", ("cov", "res", "sigma_post", "sigma_data", "rdiag", "stats", "info")),
    "step_modes": ("surfdisp_lsq_step_modes_device", ("delta", "delta_y", "stats", "info")),
    "res_modes": ("surfdisp_lsq_resolution_modes_device", ("cov", "res", "sigma_post", "sigma_data", "rdiag", "sigma_post_y", "sigma_data_y",
                                                           "rdiag_y", "stats", "info")),
}


def _problem(N, n, seed):
    """Random G with orthonormal-ish columns times a modest spectrum, so that cond(A) <= 1e4 whatever (N, n)."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, n))
    r = rng.standard_normal(N)
    w = rng.uniform(0.5, 2.0, N)
    x0 = rng.uniform(2.0, 4.5, n)
    Q = rng.uniform(0.5, 1.5, max(n - 1, 0))
    if n > 2:
        Q[n // 2] = 0.0                                   # a cut interface
    return G, r, w, x0, 0.7, Q, 0.3


def _case(B, Lmax, N, seed):
    """Random inputs of one launch, numpy.  Mixed in: ragged nlay, a water top layer that is not free, a free mask with gaps,
    Q with a zero, slopes per stack, sources 0-5 with negative chi, a masked row, a NaN kernel row, an unsolved period,
    per-stack or shared observations (alternating with the case), a stack with every row masked (per-stack cases)."""
    rng = np.random.default_rng(seed)
    P = N // 6 + 2
    per_stack = (B > 1) and (Lmax % 2 == 1)
    c = dict(B=B, Lmax=Lmax, N=N, P=P, alpha=0.8)
    c["nlay"] = np.array([max(2, Lmax - (b % 3)) for b in range(B)], np.int32)
    model = rng.uniform(2.0, 4.5, (B, 5, Lmax)).astype(np.float32)
    free = np.ones((B, Lmax), np.uint8)
    if Lmax >= 9:
        free[:, 4::5] = 0                                      # gaps
    if Lmax >= 3:
        free[::2, 0] = 0; model[::2, 1, 0] = 0.0               # a water top layer
    c["model"], c["free"] = model, (free if per_stack else free[0].copy())
    c["part"] = [rng.normal(0, 0.3, (B, P, Lmax)).astype(np.float32) for _ in range(15)]
    c["part"][7] = c["part"][10] = None                        # Love has no d/dVp
    pred = [rng.uniform(2.5, 4.5, (B, P)).astype(np.float32) for _ in range(4)]
    pred.append((rng.uniform(0.5, 1.0, (B, P)) * rng.choice([-1.0, 1.0], (B, P))).astype(np.float32))
    cols = np.stack([np.arange(N) % 6, np.arange(N) // 6], axis=1).astype(np.int32)
    if N > 12:
        for a in c["part"][3:6]:
            a[0, 1, :] = np.nan                                # a failed unit of the group entry: source 1, period 1, stack 0
        pred[0][B - 1, 2] = 0.0                                # an unsolved Rayleigh period of the last stack (c and chi rows)
    c["pred"], c["cols"] = pred, cols
    c["weights"] = rng.uniform(0.5, 2.0, N)
    shape = (B, N) if per_stack else (N,)
    c["obs"] = rng.uniform(2.5, 4.5, shape)
    c["uncer"] = rng.uniform(0.02, 0.05, shape)
    mask = np.ones(shape, np.uint8)
    if N > 1:
        mask[..., N // 2] = 0
    if N > 2:
        c["obs"][..., 0] = np.nan                              # unusable by the rule of DispersionData
        c["uncer"][..., 1] = -1.0
    if per_stack and B >= 3:
        mask[2] = 0                                            # flag 1, between two good neighbours
    c["mask"] = mask
    slope = lambda: rng.uniform(0.0, 2.0, (B, Lmax)) * (rng.random((B, Lmax)) > 0.2)
    c["vp_slope"], c["rho_slope"] = slope(), slope()
    Q = rng.uniform(0.5, 1.5, (B, max(Lmax - 1, 1)))
    if Lmax >= 3:
        Q[:, (Lmax - 1) // 2] = 0.0
    c["Q"] = Q if per_stack else Q[0].copy()
    c["lam"] = rng.uniform(5.0, 20.0, B)
    return c


def _nan_row(N):
    """The data row whose thickness kernel gets a NaN in stack 0: period 1 of source 0 (row 6), or of source 2 (row 8) where
    ``_case`` masks row 6 out; None when the case has no such row."""
    r = 8 if N // 2 == 6 else 6
    return r if N > r else None


def _mode_case(B, Lmax, N, K, seed=None):
    """``_case`` plus K modes.  Mixed in: T per stack or shared (as the case's observations), a mode
    that touches the top (water) layer, T entries at and beyond nlay - 1, part_h of the sources 1, 3, 4 absent, one part_h row
    with a NaN (``_nan_row``), mode_scale and mode_prior per stack or shared, a prior of 0, a non-zero mode_y.  Lmax = 128:
    every layer of the stack free, n = 128 - with 8 modes the largest triangle and LDS request."""
    c = _case(B, Lmax, N, seed=1000 + Lmax if seed is None else seed)
    if Lmax == 128:
        c["free"] = np.ones_like(c["free"])
        c["nlay"][:] = Lmax
    rng = np.random.default_rng(77 + Lmax + K)
    per_stack = c["obs"].ndim == 2
    lead = (B,) if per_stack else ()
    T = rng.normal(0.0, 1.0, lead + (K, Lmax)) * (rng.random(lead + (K, Lmax)) > 0.3)
    T[..., 0, 0] = 0.7                                           # the top layer: water in every other stack
    T[..., Lmax - 1] = 1.5                                       # beyond nlay - 1 in every stack: not read
    part_h = [rng.normal(0, 0.3, (B, c["P"], Lmax)).astype(np.float32) if k in (0, 2) else None for k in range(5)]
    if _nan_row(N) is not None:
        part_h[_nan_row(N) % 6][0, 1, 0] = np.nan
    c.update(K=K, modes=T, part_h=part_h, mode_scale=rng.uniform(0.5, 30.0, lead + (K,)),
             mode_prior=rng.uniform(0.0, 2.0, lead + (K,)), mode_y=rng.normal(0.0, 1.0, (B, K)))
    c["mode_prior"][..., K - 1] = 0.0
    # two rows in three are dropped here (no part_h of their source), which leaves fewer rows than unknowns at the larger shapes and
    # the damping alone to bound cond(A); 30 x the damping of _case keeps it below the 1e4 that the relative bars of
    # tests/test_lsq_resolution_gpu.py are derived for (asserted in _check_resolution)
    c["lam"] = c["lam"] * LAM_FACTOR
    return c


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if x is not None else 0)


def _ptrs(arrs):
    return (ctypes.c_void_p * len(arrs))(*[a.data_ptr() if a is not None else None for a in arrs])


def head(c, keep, part, pred, nfree_max=None):
    """The argument list the four least-squares entries share, up to and including lam, from the case ``c`` and its device
    tensors ``keep`` (by name), ``part`` [15] and ``pred`` [5]."""
    strides = (ctypes.c_long * 5)(*[c["P"]] * 5)
    nper = (ctypes.c_int * 2)(c["P"], c["P"])
    return (None, c["B"], c["Lmax"], _ptr(keep["nlay"]), _ptr(keep["model"]), _ptr(keep["free"]), int(c["free"].ndim == 2),
            c["Lmax"] if nfree_max is None else nfree_max, _ptrs(part), _ptrs(pred), strides, nper, c["N"], _ptr(keep["cols"]),
            _ptr(keep["weights"]), _ptr(keep["obs"]), _ptr(keep["uncer"]), _ptr(keep["mask"]), int(c["obs"].ndim == 2),
            _ptr(keep["vp_slope"]), _ptr(keep["rho_slope"]), 1, float(c["alpha"]), _ptr(keep["Q"]), int(c["Q"].ndim == 2), _ptr(keep["lam"]))


def launch(entry, c, K=None, nfree_max=None, lam_scale=1.0, no_part_h=False, no_cov=False, no_res=False, **null):
    """The C entry ``entry`` (a key of ENTRIES) on the arrays of ``c``, lam times ``lam_scale``.  ``null``: names of inputs or
    outputs passed as NULL; ``no_cov`` / ``no_res``: that output passed as NULL.  The mode entries: ``K`` the number of modes passed
    (default c["K"]), ``no_part_h``: the part_h array passed as NULL.  Every output is pre-filled with 7.  Returns (rc, dict of
    numpy outputs)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    symbol, names = ENTRIES[entry]
    with_modes = entry.endswith("_modes")
    B, Lmax = c["B"], c["Lmax"]
    keep = {k: t(None if null.get(k) else c[k]) for k in INPUTS + (MODE_INPUTS if with_modes else ())}
    keep["lam"] = None if null.get("lam") else t(c["lam"] * lam_scale)
    part, pred = [t(a) for a in c["part"]], [t(a) for a in c["pred"]]
    mode_in, Ko = (), 0
    if with_modes:
        K = c["K"] if K is None else K
        part_h = [t(a) for a in c["part_h"]]
        mode_in = (K, _ptr(keep["modes"]), int(c["modes"].ndim == 3), None if no_part_h else _ptrs(part_h), _ptr(keep["mode_scale"]),
                   _ptr(keep["mode_prior"]), _ptr(keep["mode_y"]))
        Ko = max(min(K, 8), 0)
    f7 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)
    no = min(Lmax if nfree_max is None else nfree_max, 128) + Ko          # (a refused launch writes nothing)
    per_mode = lambda: f7(B, max(Ko, 1))
    out = dict(delta=f7(B, Lmax), delta_y=per_mode(), stats=f7(B, 3)) if entry.startswith("step") else \
        dict(cov=f7(B, no, no), res=f7(B, no, no), sigma_post=f7(B, Lmax), sigma_data=f7(B, Lmax), rdiag=f7(B, Lmax),
             sigma_post_y=per_mode(), sigma_data_y=per_mode(), rdiag_y=per_mode(), stats=f7(B, 2))
    out["info"] = torch.full((B, 3), 7, dtype=torch.int32, device=dev)
    out = {k: out[k] for k in names}
    absent = lambda k: null.get(k) or (k == "cov" and no_cov) or (k == "res" and no_res)
    rc = getattr(_lib.lib(), symbol)(*head(c, keep, part, pred, nfree_max), *mode_in, *[_ptr(None if absent(k) else out[k]) for k in names])
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _rows_of(c, b):
    """(idx, Qw, G, res, w) of stack b in numpy float64, by the rules of include/surfdisp.h section (6d)."""
    pick = lambda a, nd: a[b] if a.ndim == nd else a
    fr = pick(c["free"], 2).astype(bool) & (np.arange(c["Lmax"]) < c["nlay"][b])
    idx, Qw = linearized.consecutive_weights(fr, pick(c["Q"], 2))
    obs, unc, mask = pick(c["obs"], 2), pick(c["uncer"], 2), pick(c["mask"], 2)
    ps, qs = c["vp_slope"][b, idx], c["rho_slope"][b, idx]
    G, res, w = [], [], []
    for r, (src, k) in enumerate(c["cols"]):
        sa = 4 if src == 5 else int(src)
        o, sg = obs[r], unc[r]
        if not (mask[r] and np.isfinite(o) and np.isfinite(sg) and sg > 0):
            continue
        v, sign = float(c["pred"][sa][b, k]), 1.0
        if sa == 4:
            if not (np.isfinite(v) and c["pred"][0][b, k] >= 0.01):
                continue
            if src == 5 and v < 0:
                sign, v = -1.0, -v
        elif not v >= 0.01:
            continue
        kb, ka, kr = (None if a is None else a[b, k, idx].astype(np.float64) for a in c["part"][3 * sa:3 * sa + 3])
        g = kb.copy()
        if ka is not None:
            g += np.where(ps != 0, ps * ka, 0.0)
        g += np.where(qs != 0, qs * kr, 0.0)
        g *= sign
        if not np.isfinite(g).all():
            continue
        G.append(g); res.append(o - v); w.append(c["weights"][r] / (sg * sg))
    return idx, Qw, np.array(G).reshape(len(G), idx.size), np.array(res), np.array(w)


# ------------------------------------------------------------------------------------------------- on real kernels
def _datasets(per, values, sets, frac, C=None):
    """DispersionData of ``sets`` ((wave, quantity), ...) from the forward dict ``values`` (numpy), uncer = frac |value|."""
    out = []
    for w, q in sets:
        v = np.asarray(values[KEY[w, q]], np.float64)
        out.append(DispersionData(w, q, per, v, frac * np.abs(v)))
    return out


def _forward_all(model, per, ratio=True):
    """dict(cR, uR, cL, eR) float64 numpy [B, P] of the GPU forward solve; every solve must succeed."""
    import torch
    from pysurfinv_amd.forward import BatchPlan
    B, _, L = model.shape
    dm, dp = torch.from_numpy(model).cuda(), torch.from_numpy(per).cuda()
    plan = BatchPlan(B, L, per.size)
    cR, uR, st, eR = (x.cpu().numpy().astype(np.float64) for x in plan.run(dm, dp, kind=2, want_ratio=True))
    assert (st == 0).all()
    cL, _, stL = (x.cpu().numpy().astype(np.float64) for x in plan.run(dm, dp, kind=1))
    assert (stL == 0).all()
    return dict(cR=cR, uR=uR, cL=cL, eR=eR)


def _true_and_start(seed=31):
    """16 stacks of 8 layers and their starts: Vs times a smooth +-5 % perturbation (half a cosine over depth, sign and
    phase per stack)."""
    true = synth.synth_models(16, 8, seed=seed)
    rng = np.random.default_rng(seed + 1)
    z = np.linspace(0.0, 1.0, 8)
    pert = 0.05 * rng.choice([-1.0, 1.0], (16, 1)) * np.cos(np.pi * (z[None, :] + rng.uniform(0, 1, (16, 1))))
    start = true.copy()
    start[:, 1, :] = (true[:, 1, :] * (1.0 + pert)).astype(np.float32)
    return true, start


def _chi_rms(pred, data, mask=None):
    """chi2 and rms [B] of the forward dict ``pred`` (numpy float64) by the definition of obsdata (weights 1)."""
    r = np.concatenate([(d.values - pred[KEY[d.wave, d.quantity]]) / d.uncer for d in data], axis=1)
    if mask is not None:
        r = np.where(mask, r, 0.0)
    n = r.shape[1] if mask is None else mask.sum(axis=1)
    chi = (r * r).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return chi, np.sqrt(chi / n)


def cpu_route(start, per, data, n_iter, T=None, mode_scale=None, above=()):
    """The iteration of LinearizedBatch in numpy float64 on the CPU checker: forward solves by oracle.cport.forward_batch, Jacobians
    by its central differences (1 % of Vs, as tests/test_group_kernels.py), steps by lsq_modes_step_reference, the same accept rule.
    ``T`` [L] (None: Vs only): one thickness mode as one more unknown - its column the central difference of the amplitude, +-1 % of
    the thickness of the layers ``above``; damped by ``mode_scale``, no prior.  Returns (model, rms, y [M])."""
    from oracle import cport
    M, _, L = start.shape
    eps, nb = 0.01, 2 * L + (0 if T is None else 2)
    keys = [KEY[d.wave, d.quantity] for d in data]

    def fwd(m):
        cR, uR, sR = cport.forward_batch(m, per, 2, nthreads=8)
        cL, _, sL = cport.forward_batch(m, per, 1, nthreads=8)
        return dict(cR=cR.astype(np.float64), uR=uR.astype(np.float64), cL=cL.astype(np.float64)), (sR != 0) | (sL != 0)

    def objective(m):
        p, bad = fwd(m)
        chi, rms = _chi_rms(p, data)
        rough = (np.diff(m[:, 1, :].astype(np.float64), axis=1) ** 2).sum(axis=1)
        return np.where(bad, np.inf, chi + ALPHA * rough), rms

    model, y = start.copy(), np.zeros(M)
    obj, rms = objective(model)
    assert np.isfinite(obj).all()
    lam = np.full(M, LAM0)
    sig = np.concatenate([d.uncer for d in data], axis=1)                                   # [M, N]: the data are per stack
    obsv = np.concatenate([d.values for d in data], axis=1)
    for _ in range(n_iter):
        big = np.repeat(model, nb, axis=0).reshape(M, nb, 5, L)
        for i in range(L):
            big[:, i, 1, i] *= (1 - eps); big[:, L + i, 1, i] *= (1 + eps)
        if T is not None:
            ey = 0.01 * model[:, 3, above].astype(np.float64).sum(axis=1)                   # [M] km
            big[:, 2 * L, 3, :] = (model[:, 3, :].astype(np.float64) - T[None, :] * ey[:, None]).astype(np.float32)
            big[:, 2 * L + 1, 3, :] = (model[:, 3, :].astype(np.float64) + T[None, :] * ey[:, None]).astype(np.float32)
        pb, bad = fwd(big.reshape(M * nb, 5, L))
        assert not bad.any()
        pc, _ = fwd(model)
        trial, ty = model.copy(), y.copy()
        for m in range(M):
            v = np.concatenate([pb[k].reshape(M, nb, per.size)[m] for k in keys], axis=1)   # [nb, N]
            f0 = np.concatenate([pc[k][m] for k in keys])
            x = model[m, 1].astype(np.float64)
            G = ((v[L:2 * L] - v[:L]) / (2 * eps * x)[:, None]).T
            Gy = None if T is None else ((v[2 * L + 1] - v[2 * L]) / (2 * ey[m]))[:, None]
            st = linearized.lsq_modes_step_reference(G, obsv[m] - f0, 1.0 / sig[m] ** 2, x, ALPHA, np.ones(L - 1), lam[m], Gy, mode_scale,
                                                     0.0, y[m])
            trial[m, 1] = (x + st["delta"]).astype(np.float32)
            if T is not None:
                trial[m, 3] = (model[m, 3].astype(np.float64) + T * st["delta_y"][0]).astype(np.float32)
                ty[m] = y[m] + st["delta_y"][0]
        tobj, trms = objective(trial)
        acc = tobj < obj
        model, y = np.where(acc[:, None, None], trial, model), np.where(acc, ty, y)
        obj, rms = np.where(acc, tobj, obj), np.where(acc, trms, rms)
        lam = np.where(acc, np.maximum(lam / NU, LAM_MIN), lam * NU)
    return model, rms, y
