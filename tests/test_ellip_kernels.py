"""Analytic partials of the Rayleigh ellipticity chi (H/V, ``surfdisp_forward_ellip_kernels_device``, include/surfdisp.h (5d)):
argument checks without a device; on the GPU, against central differences of the CPU oracle's chi, the density-scaling
identity, bit-identity of the (5b) outputs, zero rows, batch independence and the senskernel drop-ins."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EUS = np.load(os.path.join(HERE, "golden", "test1_eus.npz"))
PERIODS = list(range(10, 101, 10))


def _kernel_cases():
    from pysurfinv_amd import synth
    cases = {"synth_L12": synth.synth_models(2, 12, seed=3)[:1], "eus_L68": EUS["model"].astype(np.float32)}
    wm = synth.synth_models(1, 9, seed=5)
    wm[0, 1, 0] = 0.0; wm[0, 0, 0] = 1.5; wm[0, 2, 0] = 1.03; wm[0, 3, 0] = 3.0
    cases["water_L9"] = wm
    return cases


def _oracle_ratio(model, per):
    from oracle import cport
    O = cport.lib()
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    B, _, L = model.shape
    P = len(per)
    c = np.zeros((B, P), np.float32); u = np.zeros((B, P), np.float32); r = np.zeros((B, P), np.float32)
    p32 = np.ascontiguousarray(per, np.float32)
    for i in range(B):
        m = np.ascontiguousarray(model[i])
        O.surfdisp_oracle_forward_dbg(L, 2, fp(m[0]), fp(m[1]), fp(m[2]), fp(m[3]), fp(m[4]), fp(p32), P, fp(c[i]), fp(u[i]), fp(r[i]))
    return c, r


def _fd_oracle_chi(m, per, row, eps=0.01):
    """Central differences of the CPU oracle's chi, 1 % perturbations of one column (1 Vs, 0 Vp, 2 rho)."""
    L = m.shape[2]
    big = np.repeat(m, 2 * L, axis=0)
    for i in range(L):
        big[i, row, i] *= (1 - eps); big[L + i, row, i] *= (1 + eps)
    c, r = _oracle_ratio(big, per)
    assert (c > 0).all()
    fd = ((r[L:].astype(np.float64) - r[:L]) / (2 * eps * np.where(m[0, row] != 0, m[0, row], 1.0)[:, None])).T
    fd[:, m[0, row] == 0] = 0
    return fd


def test_ellip_entry_rejects_bad_arguments():
    """Love kind, PHASE_ONLY, KERN_REFCOORD, NULL ratio / dedb and an undersized workspace are refused before anything is
    launched (no device needed); the workspace holds that of (5b); wtype='L' with ellipticity=True is a ValueError."""
    from pysurfinv_amd import _lib, senskernel
    L = _lib.lib()
    B, Lm, P = 64, 12, 5
    ws = L.surfdisp_ellip_kernels_workspace_bytes(B, Lm, P)
    assert ws >= L.surfdisp_kernels_workspace_bytes(B, Lm, P) + 5 * Lm * P * B * 8
    nz = ctypes.c_void_p(16)
    calls = [  # (kind, ratio, dedb, workspace bytes)
        (1, nz, nz, ws), (2 | _lib.PHASE_ONLY, nz, nz, ws), (2 | _lib.KERN_REFCOORD, nz, nz, ws),
        (2, None, nz, ws), (2, nz, None, ws), (2, nz, nz, ws - 1),
        (2, nz, nz, L.surfdisp_workspace_bytes(B, Lm, P) - 1),
    ]
    for kind, ratio, dedb, wb in calls:
        rc = L.surfdisp_forward_ellip_kernels_device(None, B, Lm, None, nz, P, nz, kind, nz, nz, ratio, None,
                                                     nz, None, None, dedb, None, None, None, nz, wb)
        assert rc == _lib.ERR_INVALID, (kind, ratio, dedb, wb)
    with pytest.raises(ValueError):
        senskernel.analytic_kernels(None, None, wtype="L", ellipticity=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["synth_L12", "eus_L68", "water_L9"])
def test_ellip_kernels_match_oracle_finite_differences_of_chi(name):
    """dchi/dVs, dchi/dVp, dchi/drho of every layer against central differences of the CPU oracle's chi (1 % perturbations,
    2L solves per column); bar 2e-2 of each period's largest |FD| entry.  Measured on MI355X: 3.5e-4 .. 2.1e-3 (synth_L12),
    1.5e-3 .. 4.9e-3 (eus_L68), 4.6e-4 (water_L9, dchi/dVs) - the fp32 differences of chi under 1 % perturbations.  Water rows
    are exactly zero (a liquid layer gets no partials, as in (5b); its Vp and rho do move chi through the root, so the water
    column is left out of the comparison).  This ties the rows to the reference's own fp32 chi; the sharp comparison, 3e-4 of
    the peak against float64 differences, is tests/test_ellip_fd.py::test_fresh_stack_rows_against_float64_differences."""
    import torch
    from pysurfinv_amd import senskernel
    m = _kernel_cases()[name]
    per = np.asarray(PERIODS, np.float32)
    out = senskernel.analytic_kernels(torch.from_numpy(m).cuda(), torch.from_numpy(per).cuda(), wtype="R", ellipticity=True)
    assert int(out["status"][0]) == 0 and out["n_nonfinite"] == 0
    _, r0 = _oracle_ratio(m, per)
    np.testing.assert_allclose(out["ratio"][0].cpu().numpy(), r0[0], rtol=1e-3)
    for row, key in ((1, "dedb"), (0, "deda"), (2, "dedr")):
        an = out[key][0].cpu().numpy().astype(np.float64)
        fd = _fd_oracle_chi(m, per, row)
        if name == "water_L9":
            assert (an[:, 0] == 0).all()
            an, fd = an[:, 1:], fd[:, 1:]
        scale = np.abs(fd).max(axis=1, keepdims=True)
        err = (np.abs(an - fd) / scale).max()
        print(f"ell vs FD of chi {name} {key}: {err:.3e} of the period's peak")
        assert err < 2e-2, (name, key, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["synth_L12", "eus_L68"])
def test_ellip_density_scaling_identity(name):
    """chi does not change when every density is scaled by one factor: sum_i rho_i dchi/drho_i = 0 (solid stacks)."""
    import torch
    from pysurfinv_amd import senskernel
    m = _kernel_cases()[name]
    per = np.asarray(PERIODS, np.float32)
    out = senskernel.analytic_kernels(torch.from_numpy(m).cuda(), torch.from_numpy(per).cuda(), wtype="R", ellipticity=True)
    t = out["dedr"][0].cpu().numpy().astype(np.float64) * m[0, 2][None, :].astype(np.float64)
    rel = np.abs(t.sum(axis=1)) / np.abs(t).sum(axis=1)
    print(f"density identity {name}: {rel.max():.3e}")
    assert rel.max() <= 1e-4


def _mixed_batch(B=4096, L=20, seed=7):
    from pysurfinv_amd import synth
    m = synth.synth_models(B, L, seed=seed)
    wm = _kernel_cases()["water_L9"][0]
    m[1] = 0.0; m[1, :, :9] = wm; m[1, 3, 8:] = 0.0   # water stack, 9 layers
    m[2, 1, 3] = np.nan                                # bad stack
    nlay = np.full(B, L, np.int32); nlay[1] = 9
    return m, nlay


@pytest.mark.gpu
def test_ellip_entry_bit_identity_and_zero_rows():
    """c, u, status, dcdb, dcda, dcdr bit-identical to run_kernels; ratio bit-identical to run(want_ratio=True) (same
    team size); zero rows for unsolved periods, bad stacks and layers below the half space; water layers zero."""
    import torch
    from pysurfinv_amd import forward
    m, nlay = _mixed_batch()
    B, _, L = m.shape
    per = torch.from_numpy(np.asarray(PERIODS, np.float32)).cuda()
    dm, dn = torch.from_numpy(m).cuda(), torch.from_numpy(nlay).cuda()
    p1 = forward.BatchPlan(B, L, per.numel(), device=dm.device)
    c, u, st, ratio, kb, ka, kr, eb, ea, er, nnf = p1.run_ellip_kernels(dm, per, nlay=dn)
    c, u, st = c.clone(), u.clone(), st.clone()
    p2 = forward.BatchPlan(B, L, per.numel(), device=dm.device)
    c2, u2, st2, kb2, ka2, kr2 = p2.run_kernels(dm, per, nlay=dn)
    for x, y in ((c, c2), (u, u2), (st, st2), (kb, kb2), (ka, ka2), (kr, kr2)):
        assert torch.equal(x, y)
    p3 = forward.BatchPlan(B, L, per.numel(), device=dm.device)
    _, _, _, r3 = p3.run(dm, per, nlay=dn, want_ratio=True)
    assert torch.equal(ratio, r3)
    c, eb, ea, er, st = c.cpu().numpy(), eb.cpu().numpy(), ea.cpu().numpy(), er.cpu().numpy(), st.cpu().numpy()
    print(f"n_nonfinite {nnf} of {B * per.numel()} units")
    assert nnf <= B * per.numel() // 1000
    for e in (eb, ea, er):
        assert (e[c == 0] == 0).all()                  # unsolved periods, bad stack
        assert (e[2] == 0).all()
        assert (e[1, :, 0] == 0).all()                 # water layer
        assert (e[1, :, 9:] == 0).all()                # beyond the stack
    # layers below the half space: rows of the dcdb kernel are zero there too
    kb = kb.cpu().numpy()
    fin = np.isfinite(eb).all(axis=2)
    deep = (np.abs(eb) > 0) & fin[:, :, None]
    assert deep.any()


@pytest.mark.gpu
def test_ellip_rows_independent_of_batch():
    """A stack's rows from a one-stack launch and from a mixed 4 096-stack batch agree (different team sizes)."""
    import torch
    from pysurfinv_amd import forward
    m, nlay = _mixed_batch()
    B, _, L = m.shape
    per = torch.from_numpy(np.asarray(PERIODS, np.float32)).cuda()
    pb = forward.BatchPlan(B, L, per.numel(), device="cuda:0")
    outb = pb.run_ellip_kernels(torch.from_numpy(m).cuda(), per, nlay=torch.from_numpy(nlay).cuda())
    worst = 0.0
    for s in (0, 1, 5):
        n = int(nlay[s])
        p1 = forward.BatchPlan(1, n, per.numel(), device="cuda:0")
        out1 = p1.run_ellip_kernels(torch.from_numpy(np.ascontiguousarray(m[s:s + 1, :, :n])).cuda(), per)
        np.testing.assert_allclose(out1[3][0].cpu().numpy(), outb[3][s].cpu().numpy(), rtol=1e-5)
        for j in (7, 8, 9):
            a1 = out1[j][0].cpu().numpy().astype(np.float64)
            ab = outb[j][s, :, :n].cpu().numpy().astype(np.float64)
            scale = np.abs(ab).max(axis=1, keepdims=True)
            worst = max(worst, float((np.abs(a1 - ab) / scale).max()))
    print(f"one stack vs batch: {worst:.3e} of the period's peak")
    assert worst < 1e-3


def _frame():
    import pandas as pd
    m = EUS["model"][0].astype(np.float64)
    return pd.DataFrame({"H": m[3], "Vp": m[0], "Vs": m[1], "Rho": m[2], "Qs": 1.0 / np.where(m[4] > 0, m[4], 1e-4)})


@pytest.mark.gpu
def test_senskernel_pert_ellipticity_fd_vs_analytic():
    """SensKernelPert(ellipticity=True): method='fd' (ratio of the perturbed batch) and method='analytic' agree.  The fd route
    differences an fp32 ratio under 0.1 % perturbations: measured on MI355X 5.9e-2 (Vs) and 3.1e-1 (Vp, the smaller kernel) of
    each period's peak; bars 0.1 and 0.5.  The 1 % oracle comparison above is the accuracy test."""
    import matplotlib
    matplotlib.use("Agg")
    from pysurfinv_amd import senskernel
    df = _frame()
    fd = senskernel.SensKernelPert(df, wtype="R", Tmin=10, Tmax=100, Tstep=10, method="fd", ellipticity=True)
    an = senskernel.SensKernelPert(df, wtype="R", Tmin=10, Tmax=100, Tstep=10, method="analytic", ellipticity=True)
    for x, bar in (("Vs", 0.1), ("Vp", 0.5)):
        a, f = an.kernel_ell[x], fd.kernel_ell[x]
        err = (np.abs(a - f).max(axis=1) / np.abs(f).max(axis=1)).max()
        print(f"SensKernelPert kernel_ell {x}: fd vs analytic {err:.3e} of the period's peak")
        assert err < bar
    an.plot(ytype="ell")
    plain = senskernel.SensKernelPert(df, wtype="R", Tmin=10, Tmax=100, Tstep=10, method="analytic")
    assert plain.kernel_ell == {}
    np.testing.assert_array_equal(plain.kernel["Vs"], an.kernel["Vs"])


@pytest.mark.gpu
def test_senskernel_ellipticity_shape_and_plot():
    import matplotlib
    matplotlib.use("Agg")
    from pysurfinv_amd import senskernel
    sk = senskernel.SensKernel(_frame(), wtype="R", ellipticity=True)
    assert sk.kernel_ell.shape == (1, 3, len(list(sk.periods)), sk.zdeps.size)
    assert np.isfinite(sk.kernel_ell).all()
    sk.plot(ytype="ell")
