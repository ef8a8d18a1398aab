"""Apparent attenuation of the mode on the device (surfdisp_forward_atten_device, include/surfdisp.h section (5e)):
1/Q_apparent, the attenuation coefficient and the linear kernel d(1/Q)/d(1/Qs_i), against the reference's own partials
(COMMON /rar1/ dwx), the fp64 toolkit's TEST1/test.{R,L}.att, an identity of Love waves, the float64 host restatement
on the call's own outputs, and the parent entry's bits.

Bars (from the issue): tests 1 and 3: 2e-4 relative (dqdq: 2e-4 of the period's peak) = the project's 1e-4 bar on U plus
its 1e-4-of-peak bar on the partials, c^2 adding a few 1e-6; test 2: 3e-4 = the same plus 1e-4 for the fp32 reference
against its fp64 twin; test 4: 1e-5 relative (fp32 storage of the outputs against an fp64 sum of fp32 inputs)."""
import ctypes
import os

import numpy as np
import pytest

from test_atten_host import ATT, PART, qinv_from_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
EUS = np.load(os.path.join(HERE, "golden", "test1_eus.npz"))
NAMES = [str(n) for n in PART["names"]]


def _np(*ts):
    return [t.cpu().numpy() if t is not None else None for t in ts]


def _run(plan, m, per, kind, nlay=None, **kw):
    import torch
    out = plan.run_atten(torch.from_numpy(np.ascontiguousarray(m, np.float32)).cuda(),
                         torch.from_numpy(np.ascontiguousarray(per, np.float32)).cuda(), kind=kind,
                         nlay=None if nlay is None else torch.from_numpy(nlay).cuda(), **kw)
    return _np(*out)


@pytest.mark.gpu
def test_atten_vs_reference_partials_rayleigh():
    """(1) All six stacks of ref_partials.npz (a water top, a five-sublayer split, L = 68 > one 64-layer tile), 8 periods,
    B = 1, Rayleigh | INDEPENDENT (the fixture holds one-period calls): qinv against sum dwx qsinv U / c^2 of the
    reference's own numbers, 2e-4 relative; dqdq against dwx_layer U / c^2, 2e-4 of the period's peak.  Every unit the
    reference solved is checked (all 48); a unit it left unsolved must be 0."""
    from pysurfinv_amd import _lib, forward
    per = PART["periods"].astype(np.float32)
    nchk, wq, wd = 0, 0.0, 0.0
    for name in NAMES:
        m = PART[f"{name}_model"][None]
        qref, rows = qinv_from_fixture(name)
        c, u, st, kb, ka, kr, qinv, gamma, dqdq = _run(forward.BatchPlan(1, m.shape[2], per.size), m, per,
                                                       _lib.KIND_RAYLEIGH | _lib.INDEPENDENT)
        for ip in range(per.size):
            if qref[ip] == 0:
                assert qinv[0, ip] == 0 and gamma[0, ip] == 0 and not dqdq[0, ip].any()
                continue
            eq = abs(qinv[0, ip] / qref[ip] - 1.0)
            ed = np.abs(dqdq[0, ip].astype(np.float64) - rows[ip]).max() / np.abs(rows[ip]).max()
            eg = abs(gamma[0, ip] / (np.pi * qref[ip] / (PART[f"{name}_R_meta"][ip, 1] * float(per[ip]))) - 1.0)
            wq, wd = max(wq, eq, eg), max(wd, ed)
            assert eq < 2e-4 and eg < 2e-4, (name, per[ip], qinv[0, ip], qref[ip], eq, eg)
            assert ed < 2e-4, (name, per[ip], ed)
            nchk += 1
        if m[0, 1, 0] <= 0:
            assert not dqdq[0, :, 0].any()                          # a water layer has no share
    print(f"atten vs COMMON /rar1/ dwx, Rayleigh: {nchk} units, worst qinv/gamma {wq:.2e} (bar 2e-4), dqdq {wd:.2e} of peak (bar 2e-4)")
    assert nchk >= 48


@pytest.mark.gpu
@pytest.mark.parametrize("w,kind", [("R", 2), ("L", 1)])
def test_atten_vs_fp64_toolkit(w, kind):
    """(2) eus_L68, the ten TEST1 periods in one faithful call: 1/qinv against the toolkit's test.{R,L}.att, mode 0, 3e-4."""
    from pysurfinv_amd import forward
    m = EUS["model"].astype(np.float32)
    per = ATT["periods"].astype(np.float32)
    c, u, st, kb, ka, kr, qinv, gamma, dqdq = _run(forward.BatchPlan(1, m.shape[2], per.size), m, per, kind)
    assert st[0] == 0 and np.all(qinv[0] > 0)
    err = np.abs(1.0 / qinv[0].astype(np.float64) / ATT[f"Q_{w}"][0] - 1.0)
    print(f"atten vs test.{w}.att: worst {err.max():.2e} (bar 3e-4), per period {np.array2string(err, precision=1)}")
    assert err.max() < 3e-4, err
    assert np.allclose(gamma[0], np.pi * qinv[0].astype(np.float64) / (u[0].astype(np.float64) * per), rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_atten_love_constant_q():
    """(3) Love, the six stacks with the 1/Qs row set to q = 0.005: sum_i b_i dc/db_i = c^2 / U (c is homogeneous of
    degree one in the layers' b at fixed wavenumber), so qinv == q, 2e-4 relative, at every unit the reference's Love
    fixture solved."""
    from pysurfinv_amd import _lib, forward
    per = PART["periods"].astype(np.float32)
    q = np.float32(0.005)
    nchk, worst = 0, 0.0
    for name in NAMES:
        m = PART[f"{name}_model"][None].copy()
        m[0, 4, :] = q
        c, u, st, kb, ka, kr, qinv, gamma, dqdq = _run(forward.BatchPlan(1, m.shape[2], per.size), m, per,
                                                       _lib.KIND_LOVE | _lib.INDEPENDENT)
        assert ka is None
        for ip in range(per.size):
            if PART[f"{name}_L_meta"][ip, 0] <= 0 and c[0, ip] == 0:
                assert qinv[0, ip] == 0
                continue
            err = abs(float(qinv[0, ip]) / float(q) - 1.0)
            worst = max(worst, err); nchk += 1
            assert err < 2e-4, (name, per[ip], qinv[0, ip])
    print(f"atten Love, constant q: {nchk} units, worst {worst:.2e} (bar 2e-4)")
    assert nchk >= 40


def _mixed_batch(B=130, L=12):
    """130 stacks (the 64-unit tile is crossed twice): water tops, ragged nlay, a low-velocity layer, a NaN stack, a
    stack whose half space is slower than the mode at long periods (Rayleigh: 4 of 8 periods solved, Love: 2)."""
    from pysurfinv_amd import synth
    m = synth.synth_models(B, L, seed=21, noise=0.05, monotone=False)
    m[:10, 1, 0] = 0.0; m[:10, 0, 0] = 1.475; m[:10, 2, 0] = 1.027; m[:10, 4, 0] = 1e-4; m[:10, 3, 0] = 2.0
    m[30, 1, 4] = 0.4
    m[31, 1, 3] = np.nan
    m[33, 1, -1] = 3.2; m[33, 0, -1] = 1.76 * 3.2
    nlay = np.random.default_rng(2).integers(3, L + 1, B).astype(np.int32)
    nlay[31] = nlay[33] = L
    nlay[64] = nlay[129] = L
    per = np.linspace(5, 120, 8).astype(np.float32)
    return m, nlay, per


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [2, 1])
def test_atten_own_output_consistency(kind):
    """(4) One call of B = 130, L = 12, P = 8: attenuation_from_kernels on that call's own c, u, kb, ka in float64
    reproduces qinv, gamma, dqdq to 1e-5 relative at every tile position; bad and unsolved rows are exactly 0, never NaN."""
    from pysurfinv_amd import forward, senskernel
    m, nlay, per = _mixed_batch()
    B = m.shape[0]
    c, u, st, kb, ka, kr, qinv, gamma, dqdq = _run(forward.BatchPlan(B, m.shape[2], per.size), m, per, kind, nlay=nlay)
    assert np.isfinite(qinv).all() and np.isfinite(gamma).all() and np.isfinite(dqdq).all()
    qr, gr, dr = senskernel.attenuation_from_kernels(m, per, c, u, kb, ka)
    solved = c > 0
    assert st[31] == 4 and not solved[31].any()
    assert solved[33].any() and not solved[33, -1] and st[33] == 1
    for lo, hi in ((0, 64), (64, 128), (128, B)):
        assert solved[lo:hi].all(axis=1).any()
    # unsolved periods and bad stacks: zeros
    assert not qinv[~solved].any() and not gamma[~solved].any() and not dqdq[~solved].any()
    # layers at and below nlay, and water layers: zeros
    for b in range(B):
        assert not dqdq[b, :, nlay[b]:].any()
    assert not dqdq[:10, :, 0].any()
    nz = solved & (kb != 0).any(axis=2)                               # (a solved unit may come without partials: zeros)
    assert nz.sum() > 0.9 * solved.sum()
    assert not qinv[solved & ~nz].any()
    eq = np.abs(qinv[nz] / qr[nz] - 1.0).max()
    eg = np.abs(gamma[nz] / gr[nz] - 1.0).max()
    has = dr != 0
    assert np.array_equal(has, dqdq != 0)
    ed = np.abs(dqdq[has] / dr[has] - 1.0).max()
    print(f"atten own outputs kind {kind}: {int(nz.sum())} units, worst qinv {eq:.2e} gamma {eg:.2e} dqdq {ed:.2e} (bar 1e-5)")
    assert eq < 1e-5 and eg < 1e-5 and ed < 1e-5
    # qinv is the contraction of its kernel with the 1/Qs row
    assert np.allclose((dqdq.astype(np.float64) * m[:, 4, None, :]).sum(axis=2)[nz], qinv[nz], rtol=1e-5, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [2, 1])
def test_atten_linear_in_qs_at_one_second(kind):
    """(5) A sediment stack (oracle/cport solves it at T = 1 s, checked here) at T = 1.0 s: ln(1/T) = 0, the velocities do
    not see Qs; doubling the 1/Qs row leaves c, u and dqdq bit-identical and doubles qinv to within 2 ulp."""
    from oracle import cport
    from pysurfinv_amd import forward, synth
    m = synth.sediment_models(1, 10, seed=7, total_thickness=120.0)
    per = np.array([1.0], np.float32)
    co, uo, so = cport.forward_batch(m, per, kind)
    assert so[0] == 0 and co[0, 0] > 0
    m2 = m.copy(); m2[:, 4, :] *= 2.0
    plan = forward.BatchPlan(1, 10, 1)
    a = _run(plan, m, per, kind)
    b = _run(plan, m2, per, kind)
    assert a[0][0, 0] > 0 and abs(a[0][0, 0] / co[0, 0] - 1) < 1e-4
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[8], b[8])
    q1, q2 = a[6][0, 0], b[6][0, 0]
    assert q1 > 0
    assert abs(np.float64(q2) - 2.0 * np.float64(q1)) <= 2.0 * np.spacing(q2), (q1, q2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [2, 1])
def test_atten_entry_leaves_the_other_outputs_bit_identical(kind):
    """(6) c, u, status, dcdb, dcda, dcdr of the new entry equal run_kernels' bit for bit; a repeat call on the same
    workspace gives identical bits; NULL gamma, NULL dqdq, NULL dcda and NULL dcdr work and leave qinv as it is."""
    import torch
    from pysurfinv_amd import forward
    m, nlay, per = _mixed_batch()
    B, _, L = m.shape
    dm, dp, dn = torch.from_numpy(m).cuda(), torch.from_numpy(per).cuda(), torch.from_numpy(nlay).cuda()
    plan = forward.BatchPlan(B, L, per.size)
    ref = _np(*plan.run_kernels(dm, dp, kind=kind, nlay=dn))
    out = _np(*plan.run_atten(dm, dp, kind=kind, nlay=dn))
    for q, (x, y) in enumerate(zip(ref, out[:6])):
        if x is None:
            assert y is None and kind == 1 and q == 4
            continue
        assert np.array_equal(x, y, equal_nan=True), q
    assert (out[6] != 0).any()
    again = _np(*plan.run_atten(dm, dp, kind=kind, nlay=dn))
    for x, y in zip(out, again):
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True)
    lean = _np(*plan.run_atten(dm, dp, kind=kind, nlay=dn, want_vp=False, want_rho=False, want_kernel=False, want_gamma=False))
    assert lean[4] is None and lean[5] is None and lean[7] is None and lean[8] is None
    assert np.array_equal(lean[3], out[3]) and np.array_equal(lean[6], out[6])


@pytest.mark.gpu
def test_atten_refusals_touch_nothing():
    """(7) PHASE_ONLY, KERN_REFCOORD, NULL qinv, NULL dcdb and a workspace below surfdisp_atten_workspace_bytes each return
    SURFDISP_ERR_INVALID before anything is launched: the outputs keep their sentinel."""
    import torch
    from pysurfinv_amd import _lib, synth
    lib = _lib.lib()
    B, L, P = 3, 6, 4
    dm = torch.from_numpy(synth.synth_models(B, L, seed=1)).cuda()
    dp = torch.from_numpy(synth.default_periods(P)).cuda()
    ws_bytes = int(lib.surfdisp_atten_workspace_bytes(B, L, P))
    assert ws_bytes >= int(lib.surfdisp_kernels_workspace_bytes(B, L, P)) > int(lib.surfdisp_workspace_bytes(B, L, P))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    S = -7.5
    mk = lambda *shape: torch.full(shape, S, dtype=torch.float32, device="cuda")
    bufs = dict(c=mk(B, P), u=mk(B, P), kb=mk(B, P, L), ka=mk(B, P, L), kr=mk(B, P, L), qinv=mk(B, P), gamma=mk(B, P),
                dqdq=mk(B, P, L))
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(kind=2, qinv=True, kb=True, nbytes=ws_bytes):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        return lib.surfdisp_forward_atten_device(
            ctypes.c_void_p(stream), B, L, ctypes.c_void_p(0), p(dm), P, p(dp), int(kind), p(bufs["c"]), p(bufs["u"]), p(status),
            p(bufs["kb"]) if kb else ctypes.c_void_p(0), p(bufs["ka"]), p(bufs["kr"]),
            p(bufs["qinv"]) if qinv else ctypes.c_void_p(0), p(bufs["gamma"]), p(bufs["dqdq"]), p(ws), nbytes)

    cases = (dict(kind=2 | _lib.PHASE_ONLY), dict(kind=1 | _lib.PHASE_ONLY), dict(kind=2 | _lib.KERN_REFCOORD),
             dict(qinv=False), dict(kb=False), dict(nbytes=ws_bytes - 1),
             dict(nbytes=int(lib.surfdisp_workspace_bytes(B, L, P))))
    for kw in cases:
        assert call(**kw) == _lib.ERR_INVALID, kw
        torch.cuda.synchronize()
        for k, t in bufs.items():
            assert bool((t == S).all()), (kw, k)
        assert bool((status == -7).all()), kw
    assert call() == _lib.SUCCESS                                   # ... and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert bool((bufs["qinv"] > 0).all()) and bool((status == 0).all())


@pytest.mark.gpu
def test_analytic_kernels_attenuation_keys():
    """senskernel.analytic_kernels(attenuation=True): the default keys plus qinv, gamma, dqdq, Qapp = 1 / qinv (inf where
    qinv is 0); without the flag the dict is as before."""
    import torch
    from pysurfinv_amd import senskernel
    m, nlay, per = _mixed_batch()
    dm, dp, dn = torch.from_numpy(m).cuda(), torch.from_numpy(per).cuda(), torch.from_numpy(nlay).cuda()
    base = senskernel.analytic_kernels(dm, dp, wtype="R", nlay=dn)
    out = senskernel.analytic_kernels(dm, dp, wtype="R", nlay=dn, attenuation=True)
    assert set(out) == set(base) | {"qinv", "gamma", "dqdq", "Qapp"}
    for k in base:
        assert torch.equal(torch.nan_to_num(base[k].float(), nan=-1.0), torch.nan_to_num(out[k].float(), nan=-1.0)), k   # (phv of the NaN stack is NaN)
    q, Q = out["qinv"].cpu().numpy(), out["Qapp"].cpu().numpy()
    assert np.isinf(Q[q == 0]).all() and (q == 0).any()
    assert np.allclose(Q[q != 0] * q[q != 0], 1.0, rtol=1e-6)
