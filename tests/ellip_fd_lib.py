"""Shared statements of tests/test_ellip_fd.py: the units of tests/golden/ellip_fd.npz (float64 central differences of the
Rayleigh ellipticity chi, tests/golden/make_golden_ellip.py), the ragged batches that carry them through
forward.BatchPlan.run_ellip_kernels, and the figures of the library's rows against them."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
with np.load(os.path.join(HERE, "golden", "ellip_fd.npz")) as _z:
    FD = {k: _z[k] for k in _z.files}
NAMES = [str(n) for n in FD["names"]]
PERIODS_OF = {n: [float(t) for t in FD[f"{n}_periods"]] for n in NAMES}
UNITS = [(n, T) for n in NAMES for T in PERIODS_OF[n]]
LMAX = max(FD[f"{n}_model"].shape[1] for n in NAMES)
COLS = ("vs", "vp", "rho")
# "" : the float64-flattened layer values of thickness_fd.npz; "32": the fp32 layer values the library's prep stage holds
SETS = ("", "32")
KEYS = ("mmax", "zreg", "zliq") + tuple(f"{q}{x}" for x in SETS for q in ("lay", "c", "chi", "dchidc")) \
    + tuple(f"{p}{x}_{k}" for x in SETS for p in ("fd", "part", "dc") for k in COLS) + tuple(f"fd{x}_err" for x in SETS)
LIST4 = (6.0, 16.0, 40.0, 100.0)                    # the period list of the P = 4 launch
TEAMS = (0, 4, 16, 64)


def model(name):
    return np.asarray(FD[f"{name}_model"], np.float32)


def wet(name):
    return not (model(name)[1, 0] > 0)


def unit(name, T):
    ip = PERIODS_OF[name].index(float(T))
    return {k: FD[f"{name}_{k}"][ip] for k in KEYS}


def batch(names):
    """The stacks as one ragged batch: model float32 [B, 5, LMAX] (zeros beyond a stack's layers), nlay int32 [B]."""
    m = np.zeros((len(names), 5, LMAX), np.float32)
    nlay = np.zeros(len(names), np.int32)
    for b, n in enumerate(names):
        x = model(n)
        m[b, :, :x.shape[1]] = x
        nlay[b] = x.shape[1]
    return m, nlay


def oracle_ratio(name, T):
    """chi of the project's CPU oracle, a P = 1 call."""
    from oracle import cport
    O = cport.lib()
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    m = np.ascontiguousarray(model(name))
    per = np.array([T], np.float32)
    c, u, r = (np.zeros(1, np.float32) for _ in range(3))
    O.surfdisp_oracle_forward_dbg(m.shape[1], 2, fp(m[0]), fp(m[1]), fp(m[2]), fp(m[3]), fp(m[4]), fp(per), 1, fp(c), fp(u), fp(r))
    return float(c[0]), float(r[0])


def column_figure(lib, ref, first, mmax, peak=None):
    """worst |lib - ref| over layers first .. mmax-1 as a fraction of the largest |ref| (or of ``peak``) there."""
    ref = np.asarray(ref, np.float64)[first:mmax]
    lib = np.asarray(lib, np.float64)[first:mmax]
    return float(np.abs(lib - ref).max() / (np.abs(ref).max() if peak is None else peak))


def figures(name, T, c, ratio, de, dc, x="", fix=None):
    """The figures of one unit against the set ``x`` of the fixture: ``c``, ``ratio`` the library's root and chi, ``de`` =
    (dedb, deda, dedr) and ``dc`` = (dcdb, dcda, dcdr) its rows [L].  c, ratio: relative; de, dc: the worst column against
    fd_* / dc_* over layers 0 .. mmax-1 as a fraction of that column's largest |fd_*| / |dc_*| (the water column left
    out); piece: de - dchidc dc (the fixture's dchidc) against part_*, on the yardstick of de (the column's largest
    |fd_*|).  ``fix``: the unit's fixture entries, if not the committed ones."""
    f = unit(name, T) if fix is None else fix
    first, mmax = (1 if wet(name) else 0), int(f["mmax"])
    out = dict(c=abs(float(c) - float(f["c" + x])) / float(f["c" + x]), ratio=abs(float(ratio) - float(f["chi" + x])) / abs(float(f["chi" + x])),
               de=0.0, dc=0.0, piece=0.0)
    for k, e, c_ in zip(COLS, de, dc):
        e, c_ = np.asarray(e, np.float64), np.asarray(c_, np.float64)
        out["de"] = max(out["de"], column_figure(e, f[f"fd{x}_{k}"], first, mmax))
        out["dc"] = max(out["dc"], column_figure(c_, f[f"dc{x}_{k}"], first, mmax))
        peak = np.abs(f[f"fd{x}_{k}"][first:mmax]).max()
        out["piece"] = max(out["piece"], column_figure(e - float(f["dchidc" + x]) * c_, f[f"part{x}_{k}"], first, mmax, peak))
    return out


def launch(names, periods, team=0):
    """run_ellip_kernels on the ragged batch of ``names`` at ``periods`` with the given team size (0: the library's choice):
    dict of numpy arrays c, ratio [B, P], status [B], dc, de [3][B, P, L] (Vs, Vp, rho), nnf."""
    import torch
    from pysurfinv_amd import _lib, forward
    m, nlay = batch(names)
    per = np.ascontiguousarray(periods, np.float32)
    plan = forward.BatchPlan(len(names), LMAX, per.size)
    lib = _lib.lib()
    assert lib.surfdisp_set_team(int(team)) == 0
    try:
        c, u, st, ratio, kb, ka, kr, eb, ea, er, nnf = plan.run_ellip_kernels(
            torch.from_numpy(m).cuda(), torch.from_numpy(per).cuda(), nlay=torch.from_numpy(nlay).cuda())
        torch.cuda.synchronize()
    finally:
        lib.surfdisp_set_team(0)
    g = lambda t: t.cpu().numpy().copy()
    return dict(names=list(names), periods=[float(t) for t in periods], c=g(c), ratio=g(ratio), status=g(st),
                dc=[g(kb), g(ka), g(kr)], de=[g(eb), g(ea), g(er)], nnf=int(nnf))


def unit_figures(res, b, ip, x=""):
    """figures() of stack b, period ip of a launch() result against the set ``x``."""
    return figures(res["names"][b], res["periods"][ip], res["c"][b, ip], res["ratio"][b, ip], [y[b, ip] for y in res["de"]],
                   [y[b, ip] for y in res["dc"]], x)


def names_at(T):
    return [n for n in NAMES if float(T) in PERIODS_OF[n]]


def all_periods():
    return sorted({T for _, T in UNITS})


def fresh_launches(team):
    """(a): one P = 1 launch per period of the fixture, each on the stacks that have that period: {period: launch()}."""
    return {T: launch(names_at(T), [T], team) for T in all_periods()}
