"""What the tests of the inversion in parameter space (tests/test_param_*.py) share: the two settings, their parameter rows, the
bar of the Jacobian against finite differences, and the random inputs of the step entry.  A plain module, not a conftest."""
import ctypes

import numpy as np

from pysurfinv_amd import _lib, paramlsq, settings
from pysurfinv_amd.layers_batch import Model1DBatch

# An oceanic setting without a thermal layer: a water layer, the Cascadia sediment whose Vs is a function of its free thickness (kind
# 7), a crust with one constant coefficient, a mantle hung on a free BottomDepth (the thicknesses above enter its own with the
# opposite sign) with one constant coefficient, and the reference mantle below
OCEAN_SETTING = {
    'OceanWater': {'H': 2.6},
    'OceanSedimentCascadia': {'H': [0.3, 'abs', 0.2, 0.03]},
    'OceanCrust': {'H': 6.5, 'Vs': [[3.25, 'abs', 0.3, 0.02], 3.94]},
    'OceanMantle': {'BottomDepth': [200., 'abs', 10., 1.0],
                    'Vs': [[4.4, 'abs', 0.4, 0.02], [4.35, 'abs', 0.4, 0.02], [4.4, 'abs', 0.4, 0.02], [4.5, 'abs', 0.4, 0.02], 4.6]},
    'Info': {'modelType': 'MCInv', 'refLayer': True},
}
SETTINGS = {"mcmc": settings.MCMC_SETTING, "ocean": OCEAN_SETTING}
REL_STEP = 1e-5          # central step of jacobian_reference, in prior widths
JAC_BAR = 1e-6           # |jac - fd| <= JAC_BAR * max(1, max |column|)


def param_rows(mb, seed=5):
    """[3, Nu]: v0 and two prior draws."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(mb.spec.vmin, np.float64), np.asarray(mb.spec.vmax, np.float64)
    return np.stack([np.asarray(mb.spec.v0, np.float64)] + [lo + (hi - lo) * rng.uniform(0.02, 0.98, lo.size) for _ in range(2)])


def jac_error(jac, fd):
    """(worst ratio error / bar, largest error) of jac [C, 4, L, Nu] against fd, per column j: bar = JAC_BAR max(1, max |column|)."""
    err = np.abs(jac - fd).max(axis=(1, 2))                                  # [C, Nu]
    bar = JAC_BAR * np.maximum(1.0, np.abs(fd).max(axis=(1, 2)))
    return float((err / bar).max()), float(err.max())


def host_descriptor(setting, local_keys=None, table=None):
    """(Model1DBatch on the CPU, idesc int32, fdesc float64, L) as numpy arrays."""
    mb = Model1DBatch(setting, device="cpu", local_keys=local_keys)
    if table is not None:
        mb.set_local_info(table)
    idesc, fdesc, L = mb.native_descriptor()
    return mb, np.ascontiguousarray(idesc.numpy()), np.ascontiguousarray(fdesc.numpy()), L


# ------------------------------------------------------------------------------------------------- the step entry
STEP_CASES = [(1, 2, 1, 1), (5, 3, 7, 2), (3, 17, 40, 5), (2, 96, 100, 13), (2, 64, 100, 64), (300, 9, 12, 4)]   # (B, Lmax, N, Nu)


def step_case(B, Lmax, N, Nu, seed=None):
    """Random inputs of one launch of surfdisp_lsq_step_params_device, numpy, built as ``lsq_cases._case`` builds them: ragged nlay,
    a water top layer (NaN d/dVs in every kernel row, zero jac[vs] and jac[vp], jac[rho] there), sources 0-3 (Love without d/dVp),
    part_h of source 3 absent (its rows are dropped), a masked row, an unusable observation and uncertainty, a NaN kernel row, a NaN
    thickness row, an unsolved period, per-stack or shared observations and free masks (alternating with the case), a stack with
    every row masked (per-stack cases), some fixed unknowns, a prior on some unknowns.  jac = orthonormal-ish columns over
    (quantity, layer) scaled so that cond(A) stays below 1e4 with the damping of the case."""
    rng = np.random.default_rng(4000 + 7 * Lmax + Nu if seed is None else seed)
    P = N // 4 + 2
    per_stack = (B > 1) and (Lmax % 2 == 1)
    c = dict(B=B, Lmax=Lmax, N=N, Nu=Nu, P=P)
    c["nlay"] = np.array([max(2, Lmax - (b % 3)) for b in range(B)], np.int32)
    c["part"] = [rng.normal(0, 0.3, (B, P, Lmax)).astype(np.float32) for _ in range(12)] + [None] * 3
    c["part"][7] = c["part"][10] = None                        # Love has no d/dVp
    c["part_h"] = [rng.normal(0, 0.3, (B, P, Lmax)).astype(np.float32) if k < 3 else None for k in range(5)]
    jac = rng.normal(0, 1.0, (B, 4, Lmax, Nu)) * (rng.random((B, 4, Lmax, Nu)) > 0.3)
    if Lmax >= 3:                                              # a water top layer in every other stack
        jac[::2, :3, 0, :] = 0.0
        for k in (0, 3, 6, 9):
            c["part"][k][::2, :, 0] = np.nan
    c["jac"] = jac
    pred = [rng.uniform(2.5, 4.5, (B, P)).astype(np.float32) for _ in range(4)] + [None]
    cols = np.stack([np.arange(N) % 4, np.arange(N) // 4], axis=1).astype(np.int32)
    if N > 12:
        for a in c["part"][3:6]:
            a[0, 1, :] = np.nan                                # a failed unit of the group entry: source 1, period 1, stack 0
        c["part_h"][2][0, 2, 1] = np.nan                       # a NaN thickness row: source 2, period 2, stack 0
        pred[0][B - 1, 2] = 0.0                                # an unsolved Rayleigh period of the last stack
    c["pred"], c["cols"] = pred, cols
    c["weights"] = rng.uniform(0.5, 2.0, N)
    shape = (B, N) if per_stack else (N,)
    c["obs"] = rng.uniform(2.5, 4.5, shape)
    c["uncer"] = rng.uniform(0.02, 0.05, shape)
    mask = np.ones(shape, np.uint8)
    if N > 1:
        mask[..., N // 2] = 0
    if N > 2:
        c["obs"][..., 0] = np.nan
        c["uncer"][..., 1] = -1.0
    if per_stack and B >= 3:
        mask[2] = 0                                            # flag 1, between two good neighbours
    c["mask"] = mask
    free = np.ones((B, Nu), np.uint8)
    if Nu >= 2:
        free[:, Nu // 2] = 0
    if Nu >= 3:
        free[1::2, 0] = 0
    c["free"] = free if per_stack else free[0].copy()
    c["scale"] = rng.uniform(0.02, 0.1, Nu)
    c["prior_w"] = rng.uniform(0.0, 2e4, Nu) * (rng.random(Nu) > 0.4)
    c["prior_ref"] = rng.uniform(2.0, 4.0, Nu)
    # Np = Nu + 2: two local constants behind the unknowns of a row
    c["params"] = np.concatenate([c["prior_ref"][None, :] + rng.normal(0, 0.05, (B, Nu)), rng.normal(0, 1, (B, 2))], axis=1)
    # the data term of an unknown is about N L 4 0.7 0.3^2 / 0.035^2 ~ 2e2 N L; lam / scale^2 of that order bounds cond(A)
    c["lam"] = rng.uniform(0.5, 2.0, B) * 0.5 * N * Lmax
    return c


def step_rows(c, b):
    """(rows kept by the rules of (6d) / (6h) before the finite test of the columns, Kb, Ka, Kr, Kh [n, Lmax], res, w, sign) of stack b."""
    pick = lambda a, nd: a[b] if a.ndim == nd else a
    obs, unc, mask = pick(c["obs"], 2), pick(c["uncer"], 2), pick(c["mask"], 2)
    rows, K, res, w = [], [[], [], [], []], [], []
    for r, (src, k) in enumerate(c["cols"]):
        src = int(src)
        o, sg = obs[r], unc[r]
        if not (mask[r] and np.isfinite(o) and np.isfinite(sg) and sg > 0):
            continue
        if c["pred"][src] is None or not k < c["pred"][src].shape[1]:
            continue
        v = float(c["pred"][src][b, k])
        if not v >= 0.01 or c["part_h"][src] is None:
            continue
        rows.append(r)
        for q, a in enumerate(c["part"][3 * src:3 * src + 3] + [c["part_h"][src]]):
            K[q].append(None if a is None else a[b, k].astype(np.float64))
        res.append(o - v); w.append(c["weights"][r] / (sg * sg))
    L = c["Lmax"]
    stack = lambda rows_q: np.array([np.zeros(L) if x is None else x for x in rows_q]).reshape(len(rows_q), L)
    absent = lambda rows_q: np.array([x is None for x in rows_q], bool)
    return rows, [stack(q) for q in K], [absent(q) for q in K], np.array(res), np.array(w)


def step_reference(c, b, lam=None):
    """``paramlsq.param_lsq_reference`` of stack b (rows whose source lacks d/dVp take a zero kernel row: their term is absent)."""
    rows, K, absent, res, w = step_rows(c, b)
    free = c["free"][b] if c["free"].ndim == 2 else c["free"]
    Kb, Ka, Kr, Kh = K
    Ka = np.where(absent[1][:, None], 0.0, Ka)                 # an absent array contributes nothing (0 x a finite jac entry)
    return paramlsq.param_lsq_reference(Kb, Ka, Kr, Kh, c["jac"][b], res, w, c["lam"][b] if lam is None else lam, c["scale"],
                                        c["prior_w"], c["prior_ref"], c["params"][b], free, c["nlay"][b]), rows


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if x is not None else 0)


def _ptrs(arrs):
    return (ctypes.c_void_p * len(arrs))(*[a.data_ptr() if a is not None else None for a in arrs])


OUTS = ("delta", "stats", "info", "cov", "sigma", "logdet")


def step_launch(c, **null):
    """surfdisp_lsq_step_params_device on the arrays of ``c``, on the GPU.  ``null``: names of inputs or outputs passed as NULL.  Every
    output is pre-filled with 7.  Returns (rc, dict of numpy outputs)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    names = ("nlay", "jac", "cols", "weights", "obs", "uncer", "mask", "free", "scale", "prior_w", "prior_ref", "params", "lam")
    keep = {k: t(None if null.get(k) else c[k]) for k in names}
    part, part_h, pred = [t(a) for a in c["part"]], [t(a) for a in c["part_h"]], [t(a) for a in c["pred"]]
    Bc, Lc, Nuc = c["B"], c["Lmax"], c["Nu"]
    f7 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)
    out = dict(delta=f7(Bc, Nuc), stats=f7(Bc, 3), info=torch.full((Bc, 3), 7, dtype=torch.int32, device=dev), cov=f7(Bc, Nuc, Nuc),
               sigma=f7(Bc, Nuc), logdet=f7(Bc))
    strides = (ctypes.c_long * 5)(*[c["P"]] * 5)
    nper = (ctypes.c_int * 2)(c["P"], c["P"])
    rc = _lib.lib().surfdisp_lsq_step_params_device(
        None, Bc, Lc, _ptr(keep["nlay"]), Nuc, _ptr(keep["jac"]), _ptrs(part), _ptrs(part_h), _ptrs(pred), strides, nper,
        c["N"], _ptr(keep["cols"]), _ptr(keep["weights"]), _ptr(keep["obs"]), _ptr(keep["uncer"]), _ptr(keep["mask"]),
        int(c["obs"].ndim == 2), _ptr(keep["free"]), int(c["free"].ndim == 2), _ptr(keep["scale"]), _ptr(keep["prior_w"]),
        _ptr(keep["prior_ref"]), _ptr(keep["params"]), c["params"].shape[1], _ptr(keep["lam"]),
        *[_ptr(None if null.get(k) else out[k]) for k in OUTS])
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}
