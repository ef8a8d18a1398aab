"""Thickness and interface-depth kernels of the phase velocity on the device (surfdisp_forward_thickness_kernels_device,
include/surfdisp.h section (5g)): the fixture stacks against the numpy statement fed with the device's own rows and against
the float64 central differences, a ragged batch across the tile edges and the tile carry against one-stack launches, the
smallest stacks, the kernels entry's bits, the NULL-output variants, repeatability and the refusals."""
import ctypes

import numpy as np
import pytest

import eigen_ref as E
import thickcheck_lib as TL
from eigen_batch import BAD, WATER, ragged_batch

KINDS = [("R", 2), ("L", 1)]
NAMES6 = ("c", "u", "status", "dcdb", "dcda", "dcdr")


def _np(*ts):
    return [t.cpu().numpy() if hasattr(t, "cpu") else t for t in ts]


def _dev(m, per, nlay=None):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(m, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(per, np.float32)).cuda(),
            None if nlay is None else torch.from_numpy(np.ascontiguousarray(nlay, np.int32)).cuda())


def _thick(plan, m, per, kind, nlay=None, **kw):
    dm, dp, dn = _dev(m, per, nlay)
    return _np(*plan.run_thickness_kernels(dm, dp, kind=kind, nlay=dn, **kw))


def _rows(plan, m, per, kind, nlay=None):
    """The thickness entry's outputs and, from run_eigen on the same inputs, the layer tops [B, P, 4, L] and I0 [B, P]."""
    t = _thick(plan, m, per, kind, nlay)
    dm, dp, dn = _dev(m, per, nlay)
    c, u, st, ur, uz, tz, tr, en = _np(*plan.run_eigen(dm, dp, kind=kind, nlay=dn))
    assert np.array_equal(c, t[0]) and np.allclose(u, t[1], rtol=1e-6, atol=0)    # (the same roots; the entry's own U is the one used)
    return t, np.stack([ur, uz, tz, tr], axis=2), en[..., 0]


def _against_numpy(m, per, w, t, vt, I0, nlay=None):
    """Worst figure of dcdh and dcdz over the solved units of a batch, and their number."""
    c, u, st, kb, ka, kr, dh, dz, nnf = t
    worst, n = 0.0, 0
    for b in range(m.shape[0]):
        for ip, T in enumerate(per):
            if not c[b, ip] > 0:
                assert not dh[b, ip].any() and not dz[b, ip].any()
                continue
            nl = None if nlay is None else int(nlay[b])
            rh, rz, _ = TL.reference_unit(m[b], T, w, c[b, ip], u[b, ip], I0[b, ip], vt[b, ip], kb[b, ip], None if ka is None else ka[b, ip], kr[b, ip], nl)
            assert np.array_equal(rh != 0, dh[b, ip] != 0) and np.array_equal(rz != 0, dz[b, ip] != 0), (b, ip)
            worst = max(worst, TL.figure(dh[b, ip], rh), TL.figure(dz[b, ip], rz)); n += 1
    return worst, n


@pytest.mark.gpu
@pytest.mark.parametrize("w,kind", KINDS)
def test_thickness_fixture_stacks(w, kind):
    """The six stacks of ref_eigen.npz (a water top, L = 68 across the 64-layer tile carry, cuts inside a layer), 8 periods,
    B = 1, INDEPENDENT (one-period roots as the fixture's), at the library's own roots: dcdh and dcdz against the numpy
    statement fed with the device's own rows (the bar of tests/test_thickness_host.py), A_h <= 4 A_b against the float64
    central differences of thickness_fd.npz, dcdz[j] = dcdh[j-1] - dcdh[j] within 2 ulp of the larger term."""
    from pysurfinv_amd import _lib, forward
    worst, n, A_h, A_b = 0.0, 0, 0.0, 0.0
    for name in E.NAMES:
        m = np.asarray(E.FIX[f"{name}_model"], np.float32)[None]
        plan = forward.BatchPlan(1, m.shape[2], E.PERIODS.size)
        t, vt, I0 = _rows(plan, m, E.PERIODS, kind | _lib.INDEPENDENT)
        c, u, st, kb, ka, kr, dh, dz, nnf = t
        assert nnf == 0 and (c > 0).all()
        f, k = _against_numpy(m, E.PERIODS, w, t, vt, I0)
        worst = max(worst, f); n += k
        a, b_ = dh[0].astype(np.float64), dz[0].astype(np.float64)
        big = np.maximum(np.maximum(np.abs(a[:, :-1]), np.abs(a[:, 1:])), np.abs(b_[:, 1:])).astype(np.float32)
        assert (np.abs(b_[:, 1:] - (a[:, :-1] - a[:, 1:])) <= 2.0 * np.spacing(big).astype(np.float64)).all(), name
        assert not dz[0][:, 0].any() and not dh[0][:, -1].any()
        if name in TL.FD_NAMES:
            for T in TL.FD_PERIODS:
                ip = int(np.flatnonzero(E.PERIODS == np.float32(T))[0])
                fd = TL.fd_unit(name, w, T)
                a_h, a_b = TL.figure(dh[0, ip], fd["fd_h"]), TL.figure(kb[0, ip], fd["fd_vs"])
                print(f"{name} {w} T={T:g}: A_h {a_h:.2e} A_b {a_b:.2e}")
                A_h, A_b = max(A_h, a_h), max(A_b, a_b)
    print(f"\n{w}: {n} units against the numpy statement: worst {worst:.3e} (bar {TL.PARITY_BAR[w]:.3e}); A_h {A_h:.3e} A_b {A_b:.3e} (bar 4 x)")
    assert n == 48
    assert worst <= TL.PARITY_BAR[w]
    assert A_h <= 4.0 * A_b


def _call(lib, dm, dp, dn, B, L, P, kind, bufs, status, ws, nbytes, null=(), guard=0):
    import torch
    p = lambda k, t: ctypes.c_void_p(0 if k in null else t.data_ptr() + 4 * guard)
    return lib.surfdisp_forward_thickness_kernels_device(
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), B, L, ctypes.c_void_p(0 if dn is None else dn.data_ptr()),
        ctypes.c_void_p(dm.data_ptr()), P, ctypes.c_void_p(dp.data_ptr()), int(kind), p("c", bufs["c"]), p("u", bufs["u"]), p("status", status),
        p("dcdb", bufs["dcdb"]), p("dcda", bufs["dcda"]), p("dcdr", bufs["dcdr"]), p("dcdh", bufs["dcdh"]), p("dcdz", bufs["dcdz"]),
        p("nnf", bufs["nnf"]), ctypes.c_void_p(ws.data_ptr()), nbytes)


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
        ws_bytes = int(lib.surfdisp_thickness_kernels_workspace_bytes(B, L, P))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        sizes = dict(c=B * P, u=B * P, dcdb=B * P * L, dcda=B * P * L, dcdr=B * P * L, dcdh=B * P * L, dcdz=B * P * L)
        bufs = {k: torch.full((n + 2 * G,), S, dtype=torch.float32, device="cuda") for k, n in sizes.items()}
        bufs["nnf"] = torch.full((1 + 2 * G,), -7, dtype=torch.int32, device="cuda")
        status = torch.full((B + 2 * G,), -7, dtype=torch.int32, device="cuda")
        rc = _call(lib, dm, dp, dn, B, L, P, kind, bufs, status, ws, ws_bytes, guard=G)
        assert rc == _lib.SUCCESS, lib.surfdisp_last_error()
        torch.cuda.synchronize()
        r = {}
        for k, n in sizes.items():
            a = bufs[k].cpu().numpy()
            if k == "dcda" and kind == 1:
                assert (a[:G] == S).all() and (a[G + n:] == S).all()
                continue
            assert (a[:G] == S).all() and (a[G + n:] == S).all(), (w, k)       # nothing written outside the array
            r[k] = a[G:G + n].reshape((B, P) if n == B * P else (B, P, L))
        s, q = status.cpu().numpy(), bufs["nnf"].cpu().numpy()
        assert (s[:G] == -7).all() and (s[G + B:] == -7).all() and (q[:G] == -7).all() and (q[G + 1:] == -7).all()
        r["status"], r["nnf"] = s[G:G + B], int(q[G])
        res[w] = r
    return dict(m=m, nlay=nlay, per=per, res=res)


@pytest.mark.gpu
@pytest.mark.parametrize("w,kind", KINDS)
def test_thickness_ragged_batch(ragged, w, kind):
    """B = 130 (two full 64-unit tiles and a partial one), Lmax = 70 (a full 64-layer tile, a partial one and the carry
    between them), nlay 3 .. 70: every row equals the one-stack launch of the same stack bit for bit (same team size); zero
    rows for the bad stack and unsolved periods, zeros beyond nlay, in dcdh[nlay - 1] and dcdz[0]; the water stack finite
    with a water-depth derivative."""
    from pysurfinv_amd import _lib, forward
    m, nlay, per, r = ragged["m"], ragged["nlay"], ragged["per"], ragged["res"][w]
    B, _, L = m.shape
    P = per.size
    lib = _lib.lib()
    dh, dz = r["dcdh"], r["dcdz"]
    solved = r["c"] > 0
    assert r["nnf"] == 0 and np.isfinite(dh).all() and np.isfinite(dz).all()
    assert r["status"][BAD] == _lib.BADMODEL and not solved[BAD].any()
    if w == "L":
        assert (~solved[:, -1]).sum() >= 3 and solved[:, -1].any()             # the unsolved long period
    for x in (dh, dz):
        assert not x[~solved].any()                                            # unsolved units and the bad stack: zeros
    idx = np.arange(L)[None, None, :]
    assert not np.where(idx >= nlay[:, None, None] - 1, dh, 0).any()           # dcdh[nlay - 1] and beyond
    assert not np.where(idx >= nlay[:, None, None], dz, 0).any() and not dz[:, :, 0].any()
    assert (dh[:, :, 0][solved] != 0).all() and (dz[:, :, 1][solved] != 0).all()
    deep = (nlay > 65) & solved[:, -2]
    assert deep.sum() >= 3
    assert (dh[deep][:, -2, 64:69] != 0).any() and (dh[deep][:, -2, :64] != 0).all()   # both layer tiles carry values at 100 s
    assert np.isfinite(dh[WATER]).all() and (dz[WATER, :, 1][solved[WATER]] != 0).all()
    if w == "R":
        assert (dh[WATER, :, 0][solved[WATER]] != 0).all()
    team = lib.surfdisp_get_team2(B, L, P, kind)
    plan1 = forward.BatchPlan(1, L, P)
    assert lib.surfdisp_set_team(team) == 0
    try:
        for b in range(B):
            one = _thick(plan1, m[b:b + 1], per, kind, nlay[b:b + 1])
            for k, x in zip(NAMES6 + ("dcdh", "dcdz"), one[:8]):
                if x is not None:
                    assert np.array_equal(x[0], r[k][b]), (b, k)
    finally:
        lib.surfdisp_set_team(0)


@pytest.mark.gpu
@pytest.mark.parametrize("w,kind", KINDS)
@pytest.mark.parametrize("B,n", [(1, 2), (1, 3), (65, 2), (65, 3)])
def test_thickness_smallest_stacks(w, kind, B, n):
    """nlay = 2 (one interface, no regular layer below it) and 3, one stack and 65 (a full unit tile and one more)."""
    from pysurfinv_amd import forward, synth
    m = synth.synth_models(B, n, seed=40 + n, noise=0.03, total_thickness=35.0)
    per = np.array([8.0, 20.0, 45.0], np.float32)
    plan = forward.BatchPlan(B, n, per.size)
    t, vt, I0 = _rows(plan, m, per, kind)
    assert t[8] == 0 and (t[0] > 0).sum() >= 2 * B
    worst, k = _against_numpy(m, per, w, t, vt, I0)
    print(f"{w} B={B} nlay={n}: {k} units, worst {worst:.3e} (bar {TL.PARITY_BAR[w]:.3e})")
    assert (t[6][:, :, 0][t[0] > 0] != 0).all()
    assert worst <= TL.PARITY_BAR[w]


@pytest.mark.gpu
@pytest.mark.parametrize("w,kind", KINDS)
def test_thickness_entry_keeps_the_kernels_bits(ragged, w, kind):
    """c, u, status, dcdb, dcda, dcdr torch.equal to surfdisp_forward_kernels_device, also with INDEPENDENT; dcdh identical
    for every NULL pattern of dcda, dcdr, dcdz and n_nonfinite; two calls give the same bits."""
    import torch
    from pysurfinv_amd import _lib, forward
    m, nlay, per = ragged["m"], ragged["nlay"], ragged["per"]
    B, _, L = m.shape
    P = per.size
    dm, dp, dn = _dev(m, per, nlay)
    plan, plant = forward.BatchPlan(B, L, P), forward.BatchPlan(B, L, P)
    full = None
    for flags in (0, _lib.INDEPENDENT):
        ref = [None if t is None else t.clone() for t in plan.run_kernels(dm, dp, kind=kind | flags, nlay=dn)]
        out = plant.run_thickness_kernels(dm, dp, kind=kind | flags, nlay=dn)
        for x, y in zip(ref, out[:6]):
            assert (x is None and y is None) or torch.equal(x, y), flags
        if flags == 0:
            full = [t.clone() if hasattr(t, "clone") else t for t in out]
            for k, x in zip(NAMES6 + ("dcdh", "dcdz"), _np(*full[:8])):
                if x is not None:
                    assert np.array_equal(x, ragged["res"][w][k]), k           # ... and the guarded call's bits
    again = plant.run_thickness_kernels(dm, dp, kind=kind, nlay=dn)
    for x, y in zip(full[:8], again[:8]):
        assert (x is None and y is None) or torch.equal(x, y)
    for kw in (dict(want_vp=False), dict(want_rho=False), dict(want_dcdz=False), dict(want_vp=False, want_rho=False),
               dict(want_vp=False, want_rho=False, want_dcdz=False)):
        lean = plant.run_thickness_kernels(dm, dp, kind=kind, nlay=dn, **kw)
        assert torch.equal(lean[6], full[6]), kw
        for q, name in ((4, "want_vp"), (5, "want_rho"), (7, "want_dcdz")):
            if kw.get(name) is False:
                assert lean[q] is None
            else:
                assert (lean[q] is None and full[q] is None) or torch.equal(lean[q], full[q]), (kw, q)
    # n_nonfinite NULL, alone and with every optional row NULL: the C entry directly
    lib = _lib.lib()
    ws_bytes = int(lib.surfdisp_thickness_kernels_workspace_bytes(B, L, P))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    for null in (("nnf",), ("nnf", "dcda", "dcdr", "dcdz")):
        bufs = {k: torch.full((B, P, L) if k.startswith("dcd") else (B, P), -7.5, dtype=torch.float32, device="cuda")
                for k in ("c", "u", "dcdb", "dcda", "dcdr", "dcdh", "dcdz")}
        bufs["nnf"] = torch.zeros(1, dtype=torch.int32, device="cuda")
        status = torch.zeros(B, dtype=torch.int32, device="cuda")
        assert _call(lib, dm, dp, dn, B, L, P, kind, bufs, status, ws, ws_bytes, null=null) == _lib.SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(bufs["dcdh"], full[6]), null
        for k in ("dcdr", "dcdz"):
            assert bool((bufs[k] == -7.5).all()) == (k in null)


@pytest.mark.gpu
def test_thickness_refusals_touch_nothing():
    """PHASE_ONLY, KERN_REFCOORD, a NULL dcdh or dcdb and a workspace one byte short each return SURFDISP_ERR_INVALID before
    anything is launched: the outputs keep their sentinel."""
    import torch
    from pysurfinv_amd import _lib, synth
    lib = _lib.lib()
    B, L, P = 3, 6, 4
    dm = torch.from_numpy(synth.synth_models(B, L, seed=1)).cuda()
    dp = torch.from_numpy(synth.default_periods(P)).cuda()
    ws_bytes = int(lib.surfdisp_thickness_kernels_workspace_bytes(B, L, P))
    assert ws_bytes > int(lib.surfdisp_kernels_workspace_bytes(B, L, P)) + 4 * B * L * P * 4
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    S = -7.5
    mk = lambda *shape: torch.full(shape, S, dtype=torch.float32, device="cuda")
    bufs = dict(c=mk(B, P), u=mk(B, P), dcdb=mk(B, P, L), dcda=mk(B, P, L), dcdr=mk(B, P, L), dcdh=mk(B, P, L), dcdz=mk(B, P, L))
    bufs["nnf"] = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    call = lambda kind=2, null=(), nbytes=ws_bytes: _call(lib, dm, dp, None, B, L, P, kind, bufs, status, ws, nbytes, null=null)
    cases = (dict(kind=2 | _lib.PHASE_ONLY), dict(kind=1 | _lib.PHASE_ONLY), dict(kind=2 | _lib.KERN_REFCOORD), dict(kind=1 | _lib.KERN_REFCOORD),
             dict(null=("dcdh",)), dict(null=("dcdb",)), dict(null=("c",)), dict(null=("u",)), dict(null=("status",)),
             dict(nbytes=ws_bytes - 1), dict(nbytes=int(lib.surfdisp_kernels_workspace_bytes(B, L, P))))
    for kw in cases:
        assert call(**kw) == _lib.ERR_INVALID, kw
        torch.cuda.synchronize()
        for k, t in bufs.items():
            assert bool((t == (S if k != "nnf" else -7)).all()), (kw, k)
        assert bool((status == -7).all()), kw
    for kind in (2, 1):
        assert call(kind=kind) == _lib.SUCCESS                      # ... and the same buffers are accepted as they are
        torch.cuda.synchronize()
        assert bool((bufs["dcdh"][:, :, 0] != 0).all()) and bool((status == 0).all()) and int(bufs["nnf"][0]) == 0


@pytest.mark.gpu
def test_analytic_kernels_thickness_keys():
    """senskernel.analytic_kernels(thickness=True): the documented keys on top of the plain call's, the same numbers."""
    import torch
    from pysurfinv_amd import senskernel, synth
    m = synth.synth_models(4, 7, seed=2)
    per = synth.default_periods(5)
    dm, dp, _ = _dev(m, per)
    for w in ("R", "L"):
        base = senskernel.analytic_kernels(dm, dp, wtype=w)
        full = senskernel.analytic_kernels(dm, dp, wtype=w, thickness=True)
        assert set(full) == set(base) | {"dcdh", "dcdz", "n_nonfinite"}
        for k in base:
            assert base[k] is None or torch.equal(base[k], full[k]), k
        assert full["n_nonfinite"] == 0 and full["dcdh"].shape == (4, 5, 7) and bool((full["dcdh"][:, :, 0] != 0).all())
        assert bool((full["dcdh"][:, :, -1] == 0).all()) and bool((full["dcdz"][:, :, 0] == 0).all())
