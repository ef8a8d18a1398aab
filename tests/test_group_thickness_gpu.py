"""Thickness and interface-depth kernels of the GROUP velocity on the device (surfdisp_forward_group_thickness_kernels_device,
include/surfdisp.h section (5h)): the fixture stacks against the host statement fed with the thickness entry's rows at the
shifted periods and against the float64 central differences of U, a ragged batch across the tile edges against one-stack
launches, the smallest stacks, the bits of the three entries it contains, the NULL-output variants, repeatability, the
refusals and senskernel.group_thickness_kernels.

Figures measured on MI355X are in the docstrings and in profiles/group_thickness/parity.txt."""
import ctypes

import numpy as np
import pytest

import eigen_ref as E
import thickcheck_lib as TL
from eigen_batch import BAD, WATER, ragged_batch
from group_thickness_lib import FD_RATIO_BAR, fd_rows
from test_kernel_rows_gpu import DU_BAR

KINDS = [("R", 2), ("L", 1)]
D = 0.01
DLNT = float(np.log((1.0 + float(np.float32(D))) / (1.0 - float(np.float32(D)))))
# the outputs of run_group_thickness_kernels, in order
NAMES = ("c", "u", "status", "dcdb", "dcda", "dcdr", "dudb", "duda", "dudr", "dcdh", "dcdz", "dudh", "dudz")
ROWS = NAMES[3:]
# dudz[j] against dudh[j - 1] - dudh[j], in fp32 ulps (2^-24) of the largest term (|f1| + |f2|) M, f1 = (U/c)(2 - U/c) / 2, f2 =
# (U/c)^2 / ln((1+d)/(1-d)), M the largest entry of the unit's four thickness rows: before their rounding to fp32 the rows obey
# dcdz[j] = dcdh[j - 1] - dcdh[j] to 2^-53; each of the six entries that meet in the identity is rounded once (half an ulp of at
# most M each, carried by |f1| + |f2|: 6 in all), and each of the three results takes four fp32 operations - a sum, a difference,
# two products - and the final difference on terms of at most 2 (|f1| + |f2|) M: 6 each, 18 in all
IDENTITY_ULPS = 24.0


def _np(*ts):
    return [t.detach().cpu().numpy().copy() if hasattr(t, "detach") else t for t in ts]


def _dev(m, per, nlay=None):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(m, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(per, np.float32)).cuda(),
            None if nlay is None else torch.from_numpy(np.ascontiguousarray(nlay, np.int32)).cuda())


def _bits_equal(x, y):
    """Bit for bit (NaN rows included)."""
    import torch
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _gt(plan, m, per, kind, nlay=None, **kw):
    dm, dp, dn = _dev(m, per, nlay)
    return _np(*plan.run_group_thickness_kernels(dm, dp, kind=kind, nlay=dn, dlnT_frac=D, **kw))


def _host_statement(m, per, kind, out, nlay=None):
    """dudh and dudz of senskernel.group_thickness_reference fed with run_thickness_kernels(kind | INDEPENDENT) at the fp32 periods
    T (1 - d), T (1 + d) and the entry's own c and u; (ref_h, ref_z, side rows dcdh-, dcdh+, dcdz-, dcdz+, mask of the units with a
    root at both shifted periods)."""
    from pysurfinv_amd import _lib, forward, senskernel
    B, _, L = m.shape
    plan = forward.BatchPlan(B, L, len(per))
    d = np.float32(D)
    side = []
    for f in (np.float32(1) - d, np.float32(1) + d):                   # the fp32 periods the shift kernel forms
        dm, dps, dn = _dev(m, np.asarray(per, np.float32) * f, nlay)
        side.append(_np(*plan.run_thickness_kernels(dm, dps, kind=kind | _lib.INDEPENDENT, nlay=dn)))
        assert side[-1][8] == 0
    c, u = out[0].astype(np.float64)[:, :, None], out[1].astype(np.float64)[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        ref_h = senskernel.group_thickness_reference(c, u, side[0][6], side[1][6], DLNT)
        ref_z = senskernel.group_thickness_reference(c, u, side[0][7], side[1][7], DLNT)
    return ref_h, ref_z, (side[0][6], side[1][6], side[0][7], side[1][7]), (side[0][0] > 0) & (side[1][0] > 0)


def _figures(out, ref_h, ref_z, both):
    """Worst |row - host statement| as a fraction of the row's peak of the statement over the comparable units, and their number."""
    ok = (out[0] > 0) & both & ~np.isnan(out[11]).any(axis=2) & (out[11] != 0).any(axis=2)
    worst = 0.0
    for got, ref in ((out[11], ref_h), (out[12], ref_z)):
        peak = np.abs(ref).max(axis=2)
        err = np.abs(got.astype(np.float64) - ref).max(axis=2)
        worst = max(worst, float((err[ok] / peak[ok]).max()))
    return worst, int(ok.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("w,kind", KINDS)
def test_group_thickness_fixture_stacks(w, kind):
    """The six stacks of ref_eigen.npz, 8 periods, B = 1, INDEPENDENT.  dudh and dudz against the host statement fed with the
    thickness entry's own rows at the fp32 shifted periods, as a fraction of the row's peak: the construction and the bar (DU_BAR)
    of test_group_combination_matches_its_host_statement - the mismatch of the two root searches (<= 2e-6) amplified by 1 / (2 d).
    dudz[j] = dudh[j - 1] - dudh[j] within IDENTITY_ULPS of the largest term.  Against the float64 central differences of U of
    group_thickness_fd.npz: A_Uh <= FD_RATIO_BAR x A_Ub with A_Ub from the entry's own dudb (group_thickness_lib: 4, or twice
    the ratio float64 alone reaches with the attenuation correction at the shifted period)."""
    from pysurfinv_amd import _lib, forward
    worst, n, A_h, A_b, worst_id = 0.0, 0, 0.0, 0.0, 0.0
    for name in E.NAMES:
        m = np.asarray(E.FIX[f"{name}_model"], np.float32)[None]
        plan = forward.BatchPlan(1, m.shape[2], E.PERIODS.size)
        out = _gt(plan, m, E.PERIODS, kind | _lib.INDEPENDENT)
        assert out[13] == 0 and out[14] == 0 and (out[0] > 0).all()
        ref_h, ref_z, side, both = _host_statement(m, E.PERIODS, kind, out)
        f, k = _figures(out, ref_h, ref_z, both)
        worst = max(worst, f); n += k
        uh, uz = out[11][0].astype(np.float64), out[12][0].astype(np.float64)
        assert not out[12][0][:, 0].any() and not out[11][0][:, -1].any()
        assert np.array_equal(out[11] != 0, out[9] != 0)                    # zeros exactly where dcdh is zero
        assert np.array_equal(out[12][:, :, 1:] != 0, out[9][:, :, :-1] != 0)
        r = out[1][0].astype(np.float64) / out[0][0].astype(np.float64)
        scale = (np.abs(0.5 * r * (2.0 - r)) + r * r / DLNT) * np.max([np.abs(s[0]).max(axis=1) for s in side], axis=0)     # [P]
        ident = np.abs(uz[:, 1:] - (uh[:, :-1] - uh[:, 1:])).max(axis=1) / (2.0 ** -24 * scale)
        worst_id = max(worst_id, float(ident.max()))
        assert (ident <= IDENTITY_ULPS).all(), (name, ident)
        if name in TL.FD_NAMES:
            for T in TL.FD_PERIODS:
                ip = int(np.flatnonzero(E.PERIODS == np.float32(T))[0])
                fd = fd_rows(name, w, T)
                a_h, a_b = TL.figure(out[11][0, ip], fd["fd_uh"][1]), TL.figure(out[6][0, ip], fd["fd_ub"])
                print(f"{name} {w} T={T:g}: A_Uh {a_h:.2e} A_Ub {a_b:.2e}")
                A_h, A_b = max(A_h, a_h), max(A_b, a_b)
    print(f"\n{w}: {n} units against the host statement: worst {worst:.3e} of the row's peak (bar {DU_BAR:.1e}); identity worst "
          f"{worst_id:.2f} ulps of the largest term (bar {IDENTITY_ULPS:g}); A_Uh {A_h:.3e} A_Ub {A_b:.3e} ratio {A_h / A_b:.2f} "
          f"(bar {FD_RATIO_BAR[w]:.2f})")
    assert n == 48
    assert worst < DU_BAR
    assert A_h <= FD_RATIO_BAR[w] * A_b


def _call(lib, dm, dp, dn, B, L, P, kind, bufs, status, ws, nbytes, null=(), guard=0, dfrac=D):
    import torch
    p = lambda k: ctypes.c_void_p(0 if k in null else (status if k == "status" else bufs[k]).data_ptr() + 4 * guard)
    return lib.surfdisp_forward_group_thickness_kernels_device(
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), B, L, ctypes.c_void_p(0 if dn is None else dn.data_ptr()),
        ctypes.c_void_p(dm.data_ptr()), P, ctypes.c_void_p(dp.data_ptr()), int(kind), ctypes.c_float(dfrac),
        *[p(k) for k in NAMES], p("nsf"), p("nnf"), ctypes.c_void_p(ws.data_ptr()), nbytes)


@pytest.fixture(scope="module")
def ragged():
    """The ragged batch through the C entry, both wave types, with guard words around every output: name -> arrays."""
    import torch
    from pysurfinv_amd import _lib
    m, nlay, per = ragged_batch()
    B, _, L = m.shape
    P = per.size
    dm, dp, dn = _dev(m, per, nlay)
    lib = _lib.lib()
    G, S = 64, -7.5
    res = {}
    for w, kind in KINDS:
        ws_bytes = int(lib.surfdisp_group_thickness_kernels_workspace_size(B, L, P))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        sizes = {k: B * P * (L if k in ROWS else 1) for k in NAMES if k != "status"}
        bufs = {k: torch.full((n + 2 * G,), S, dtype=torch.float32, device="cuda") for k, n in sizes.items()}
        for k in ("nsf", "nnf"):
            bufs[k] = torch.full((1 + 2 * G,), -7, dtype=torch.int32, device="cuda")
        status = torch.full((B + 2 * G,), -7, dtype=torch.int32, device="cuda")
        rc = _call(lib, dm, dp, dn, B, L, P, kind, bufs, status, ws, ws_bytes, guard=G)
        assert rc == _lib.SUCCESS, lib.surfdisp_last_error()
        torch.cuda.synchronize()
        r = {}
        for k, n in sizes.items():
            a = bufs[k].cpu().numpy()
            assert (a[:G] == S).all() and (a[G + n:] == S).all(), (w, k)       # nothing written outside the array
            if k in ("dcda", "duda") and kind == 1:
                continue
            r[k] = a[G:G + n].reshape((B, P) if n == B * P else (B, P, L))
        s = status.cpu().numpy()
        assert (s[:G] == -7).all() and (s[G + B:] == -7).all()
        r["status"] = s[G:G + B]
        for k in ("nsf", "nnf"):
            q = bufs[k].cpu().numpy()
            assert (q[:G] == -7).all() and (q[G + 1:] == -7).all()
            r[k] = int(q[G])
        res[w] = r
    return dict(m=m, nlay=nlay, per=per, res=res)


@pytest.mark.gpu
@pytest.mark.parametrize("w,kind", KINDS)
def test_group_thickness_ragged_batch(ragged, w, kind):
    """B = 130, Lmax = 70, nlay 3 .. 70: every row equals the one-stack launch of the same stack bit for bit (same team size);
    zeros exactly where dcdh is zero (unsolved periods, the bad stack, beyond nlay, dudh[nlay - 1], dudz[0]); NaN rows exactly
    for the units of dudb's NaN rows, as many as n_shift_failed says; a deep stack at 100 s carries dudh in both layer tiles; the
    water stack is finite with a water-depth entry for Rayleigh."""
    from pysurfinv_amd import _lib, forward
    m, nlay, per, r = ragged["m"], ragged["nlay"], ragged["per"], ragged["res"][w]
    B, _, L = m.shape
    P = per.size
    lib = _lib.lib()
    uh, uz, dh = r["dudh"], r["dudz"], r["dcdh"]
    solved = r["c"] > 0
    failed = np.isnan(r["dudb"]).any(axis=2)
    assert r["nnf"] == 0 and r["nsf"] == failed.sum() and not failed[~solved].any()
    assert np.isfinite(dh).all() and np.isfinite(r["dcdz"]).all()
    for x in (uh, uz):
        assert np.array_equal(np.isnan(x).all(axis=2), failed) and np.array_equal(np.isnan(x).any(axis=2), failed)
    assert r["status"][BAD] == _lib.BADMODEL and not solved[BAD].any()
    if w == "L":
        assert (~solved[:, -1]).sum() >= 3 and solved[:, -1].any()             # the unsolved long period
    good = ~failed
    assert np.array_equal((uh != 0)[good], (dh != 0)[good])                    # zeros exactly where dcdh is zero ...
    assert np.array_equal((uz[:, :, 1:] != 0)[good], (dh[:, :, :-1] != 0)[good]) and not uz[good][:, 0].any()
    assert np.array_equal((uz != 0)[good], (r["dcdz"] != 0)[good])             # ... and where dcdz is
    for x in (uh, uz):
        assert not x[~solved].any()                                            # unsolved units and the bad stack: zeros
    idx = np.arange(L)[None, None, :]
    assert not np.where((idx >= nlay[:, None, None] - 1) & good[:, :, None], uh, 0).any()      # dudh[nlay - 1] and beyond
    assert not np.where((idx >= nlay[:, None, None]) & good[:, :, None], uz, 0).any()
    ok = solved & good
    assert ok.sum() >= 0.9 * solved.sum()
    assert (uh[:, :, 0][ok] != 0).all() and (uz[:, :, 1][ok] != 0).all()
    deep = (nlay > 65) & ok[:, -2]
    assert deep.sum() >= 3
    assert (uh[deep][:, -2, 64:69] != 0).any() and (uh[deep][:, -2, :64] != 0).all()   # both layer tiles carry values at 100 s
    assert ok[WATER].any() and np.isfinite(uh[WATER][ok[WATER]]).all() and (uz[WATER, :, 1][ok[WATER]] != 0).all()
    if w == "R":
        assert (uh[WATER, :, 0][ok[WATER]] != 0).all()                         # the water depth
    team = lib.surfdisp_get_team2(B, L, P, kind)
    plan1 = forward.BatchPlan(1, L, P)
    assert lib.surfdisp_set_team(team) == 0
    try:
        for b in range(B):
            one = _gt(plan1, m[b:b + 1], per, kind, nlay[b:b + 1])
            for k, x in zip(NAMES, one[:13]):
                if x is not None:
                    assert x[0].tobytes() == r[k][b].tobytes(), (b, k)
    finally:
        lib.surfdisp_set_team(0)


@pytest.mark.gpu
@pytest.mark.parametrize("w,kind", KINDS)
@pytest.mark.parametrize("B,n", [(1, 2), (1, 3), (65, 2), (65, 3)])
def test_group_thickness_smallest_stacks(w, kind, B, n):
    """nlay = 2 (one interface, no regular layer below it) and 3, one stack and 65 (a full unit tile and one more): the host
    statement at the bar of the fixture stacks, the zero pattern and the identity."""
    from pysurfinv_amd import forward, synth
    m = synth.synth_models(B, n, seed=40 + n, noise=0.03, total_thickness=35.0)
    per = np.array([8.0, 20.0, 45.0], np.float32)
    out = _gt(forward.BatchPlan(B, n, per.size), m, per, kind)
    assert out[14] == 0 and (out[0] > 0).sum() >= 2 * B
    ref_h, ref_z, side, both = _host_statement(m, per, kind, out)
    worst, k = _figures(out, ref_h, ref_z, both)
    print(f"{w} B={B} nlay={n}: {k} units, worst {worst:.3e} of the row's peak (bar {DU_BAR:.1e}), {out[13]} shifted roots failed")
    ok = (out[0] > 0) & ~np.isnan(out[11]).any(axis=2)
    assert k >= 0.9 * (out[0] > 0).sum()
    assert (out[11][:, :, 0][ok] != 0).all() and not out[11][:, :, -1][ok].any() and not out[12][:, :, 0][ok].any()
    assert np.array_equal((out[11] != 0)[ok], (out[9] != 0)[ok])
    assert worst < DU_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("w,kind", KINDS)
def test_group_thickness_entry_keeps_the_three_entries_bits(ragged, w, kind):
    """c .. dcdr bit-equal to surfdisp_forward_kernels_device, dudb, duda, dudr to surfdisp_forward_group_kernels_device at the
    same dlnT_frac (and its failure count), dcdh, dcdz to surfdisp_forward_thickness_kernels_device, also with INDEPENDENT; dudh
    identical for every NULL pattern of the optional pointers; two calls give the same bits."""
    import torch
    from pysurfinv_amd import _lib, forward
    m, nlay, per = ragged["m"], ragged["nlay"], ragged["per"]
    B, _, L = m.shape
    P = per.size
    dm, dp, dn = _dev(m, per, nlay)
    plan, plant = forward.BatchPlan(B, L, P), forward.BatchPlan(B, L, P)
    keep = lambda ts: [t.clone() if hasattr(t, "clone") else t for t in ts]
    same = lambda x, y: (x is None and y is None) or _bits_equal(x, y)
    full = None
    for flags in (0, _lib.INDEPENDENT):
        kw = dict(kind=kind | flags, nlay=dn)
        ref_k = keep(plan.run_kernels(dm, dp, **kw))
        ref_g = keep(plan.run_group_kernels(dm, dp, dlnT_frac=D, **kw))
        ref_t = keep(plan.run_thickness_kernels(dm, dp, **kw))
        out = plant.run_group_thickness_kernels(dm, dp, dlnT_frac=D, **kw)
        for q in range(6):
            assert same(ref_k[q], out[q]), (flags, NAMES[q])
        for q in range(9):
            assert same(ref_g[q], out[q]), (flags, NAMES[q])
        assert ref_g[9] == out[13]
        assert same(ref_t[6], out[9]) and same(ref_t[7], out[10]) and ref_t[8] == 0 and out[14] == 0, flags
        if flags == 0:
            full = keep(out)
            for k, x in zip(NAMES, _np(*full[:13])):
                if x is not None:
                    assert x.tobytes() == ragged["res"][w][k].tobytes(), k       # ... and the guarded call's bits
    again = plant.run_group_thickness_kernels(dm, dp, kind=kind, nlay=dn, dlnT_frac=D)
    for x, y in zip(full[:13], again[:13]):
        assert same(x, y)
    wants = ("want_vp", "want_rho", "want_dcdz", "want_dudz")
    where = dict(want_vp=(4, 7), want_rho=(5, 8), want_dcdz=(10,), want_dudz=(12,))
    for off in ((0,), (1,), (2,), (3,), (0, 1), (2, 3), (0, 1, 2, 3)):
        kw = {wants[i]: False for i in off}
        lean = plant.run_group_thickness_kernels(dm, dp, kind=kind, nlay=dn, dlnT_frac=D, **kw)
        assert _bits_equal(lean[11], full[11]), kw
        gone = {q for name in kw for q in where[name]}
        for q in range(13):
            if q in gone:
                assert lean[q] is None, (kw, q)
            else:
                assert same(lean[q], full[q]), (kw, q)
    # the counters NULL, alone and with every optional row NULL: the C entry directly
    lib = _lib.lib()
    ws_bytes = int(lib.surfdisp_group_thickness_kernels_workspace_size(B, L, P))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    optional = ("dcda", "dcdr", "duda", "dudr", "dcdz", "dudz")
    for null in (("nsf", "nnf"), ("nsf",), ("nsf", "nnf") + optional):
        bufs = {k: torch.full((B, P, L) if k in ROWS else (B, P), -7.5, dtype=torch.float32, device="cuda") for k in NAMES if k != "status"}
        bufs["nsf"], bufs["nnf"] = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
        status = torch.zeros(B, dtype=torch.int32, device="cuda")
        assert _call(lib, dm, dp, dn, B, L, P, kind, bufs, status, ws, ws_bytes, null=null) == _lib.SUCCESS
        torch.cuda.synchronize()
        assert _bits_equal(bufs["dudh"], full[11]) and _bits_equal(bufs["dcdh"], full[9]) and _bits_equal(bufs["dudb"], full[6]), null
        for k in ("dcdr", "dudr", "dcdz", "dudz"):
            assert bool((bufs[k] == -7.5).all()) == (k in null), (null, k)


@pytest.mark.gpu
def test_group_thickness_refusals_touch_nothing():
    """PHASE_ONLY, KERN_REFCOORD, a NULL c, u, status, dcdb, dudb, dcdh or dudh, dlnT_frac outside [1e-3, 0.05] and a workspace
    one byte short each return SURFDISP_ERR_INVALID before anything is launched: the outputs keep their sentinel.  The size
    function is larger than the group entry's and the thickness entry's."""
    import torch
    from pysurfinv_amd import _lib, synth
    lib = _lib.lib()
    B, L, P = 3, 6, 4
    dm = torch.from_numpy(synth.synth_models(B, L, seed=1)).cuda()
    dp = torch.from_numpy(synth.default_periods(P)).cuda()
    ws_bytes = int(lib.surfdisp_group_thickness_kernels_workspace_size(B, L, P))
    ws_group, ws_thick = int(lib.surfdisp_group_kernels_workspace_bytes(B, L, P)), int(lib.surfdisp_thickness_kernels_workspace_bytes(B, L, P))
    assert ws_bytes > max(ws_group, ws_thick) + 4 * B * L * P * 4              # ... by the four row planes at least
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    S = -7.5
    bufs = {k: torch.full((B, P, L) if k in ROWS else (B, P), S, dtype=torch.float32, device="cuda") for k in NAMES if k != "status"}
    bufs["nsf"], bufs["nnf"] = (torch.full((1,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    call = lambda kind=2, null=(), nbytes=ws_bytes, dfrac=D: _call(lib, dm, dp, None, B, L, P, kind, bufs, status, ws, nbytes, null=null, dfrac=dfrac)
    cases = ([dict(kind=k | f) for k in (2, 1) for f in (_lib.PHASE_ONLY, _lib.KERN_REFCOORD)]
             + [dict(null=(k,)) for k in ("c", "u", "status", "dcdb", "dudb", "dcdh", "dudh")]
             + [dict(dfrac=5.0e-4), dict(dfrac=0.06), dict(dfrac=float("nan")), dict(nbytes=ws_bytes - 1), dict(nbytes=ws_group), dict(nbytes=ws_thick)])
    for kw in cases:
        assert call(**kw) == _lib.ERR_INVALID, kw
        torch.cuda.synchronize()
        for k, t in bufs.items():
            assert bool((t == (-7 if k in ("nsf", "nnf") else S)).all()), (kw, k)
        assert bool((status == -7).all()), kw
    for kind in (2, 1):
        assert call(kind=kind) == _lib.SUCCESS                      # ... and the same buffers are accepted as they are
        torch.cuda.synchronize()
        assert bool((bufs["dudh"][:, :, 0] != 0).all()) and bool((status == 0).all())
        assert int(bufs["nsf"][0]) == 0 and int(bufs["nnf"][0]) == 0


@pytest.mark.gpu
def test_group_thickness_kernels_keys():
    """senskernel.group_thickness_kernels: the keys of analytic_kernels(group=True) and of analytic_kernels(thickness=True) with the
    separate calls' numbers, plus dudh and dudz.  analytic_kernels itself keeps refusing the two flags together, with the text
    tests/test_thickness_host.py matches."""
    import torch
    from pysurfinv_amd import senskernel, synth
    m = synth.synth_models(4, 7, seed=2)
    per = synth.default_periods(5)
    dm, dp, _ = _dev(m, per)
    for w in ("R", "L"):
        grp = senskernel.analytic_kernels(dm, dp, wtype=w, group=True)
        thk = senskernel.analytic_kernels(dm, dp, wtype=w, thickness=True)
        full = senskernel.group_thickness_kernels(dm, dp, wtype=w)
        assert set(full) == set(grp) | set(thk) | {"dudh", "dudz"} and {"n_failed", "n_nonfinite"} <= set(full)
        for src in (grp, thk):
            for k, v in src.items():
                if hasattr(v, "shape"):
                    assert _bits_equal(v, full[k]), (w, k)
                else:
                    assert v == full[k], (w, k)
        assert full["n_failed"] == 0 and full["n_nonfinite"] == 0 and full["dudh"].shape == (4, 5, 7)
        assert bool((full["dudh"][:, :, 0] != 0).all()) and bool((full["dudh"][:, :, -1] == 0).all()) and bool((full["dudz"][:, :, 0] == 0).all())
        with pytest.raises(ValueError, match="thickness=True is an entry of its own"):
            senskernel.analytic_kernels(dm, dp, wtype=w, group=True, thickness=True)
