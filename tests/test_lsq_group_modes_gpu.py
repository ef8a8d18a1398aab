"""Thickness modes with group-velocity data (``group_modes=True`` of pysurfinv_amd.linearized): the step and the resolution on the
device's own rows - the mode columns of the U rows come from dudh of surfdisp_forward_group_thickness_kernels_device, part_h slots 1
and 3 - and the recovery of a displaced interface from U data alone against a float64 route on the host.

The checks and bars of the step are those of tests/test_lsq_modes_gpu.py::test_step_with_modes_on_real_kernels; the recovery
problem is that of profiles/lsq_modes/recovery.txt.  Figures measured on MI355X: profiles/group_thickness/recovery.txt."""
import numpy as np
import pytest

from lsq_cases import ALPHA, LAM0, LAM_MIN, N_ITER, NU, _true_and_start
from test_lsq_modes_gpu import ABOVE, BELOW, MODE_SCALE, _rows_with_modes
from pysurfinv_amd import linearized, synth
from pysurfinv_amd.obsdata import DispersionData

pytestmark = pytest.mark.gpu

KEY = {("R", "c"): "cR", ("R", "U"): "uR", ("L", "c"): "cL", ("L", "U"): "uL", ("R", "E"): "eR"}
SETS4 = (("R", "c"), ("R", "U"), ("L", "c"), ("L", "U"))
SETS_U = (("R", "U"), ("L", "U"))


def _forward4(model, per):
    """dict(cR, uR, cL, uL, eR) float64 numpy [B, P] of the GPU forward solve; every solve must succeed."""
    import torch
    from pysurfinv_amd.forward import BatchPlan
    B, _, L = model.shape
    dm, dp = torch.from_numpy(model).cuda(), torch.from_numpy(per).cuda()
    plan = BatchPlan(B, L, per.size)
    cR, uR, st, eR = (x.cpu().numpy().astype(np.float64) for x in plan.run(dm, dp, kind=2, want_ratio=True))
    assert (st == 0).all()
    cL, uL, stL = (x.cpu().numpy().astype(np.float64) for x in plan.run(dm, dp, kind=1))
    assert (stL == 0).all()
    return dict(cR=cR, uR=uR, cL=cL, uL=uL, eR=eR)


def _datasets(per, values, sets, frac):
    out = []
    for w, q in sets:
        v = np.asarray(values[KEY[w, q]], np.float64)
        out.append(DispersionData(w, q, per, v, frac * np.abs(v)))
    return out


@pytest.mark.parametrize("name", ["synth_L8", "water_L9"])
def test_step_and_resolution_with_modes_and_group_data(name):
    """LsqPlan(group_modes=True).step and .resolution with (R c, R U, L c, L U) data and two modes per stack, on the stacks of
    test_step_with_modes_on_real_kernels: the plan's rows are those of senskernel.group_thickness_kernels bit for bit; the
    backward error of (delta, delta_y) against modes_normal_equations built from them - dudh contracted with T for the U rows - is
    within 1e-11 (||A||inf ||d||inf + ||g||inf), the bar of that test; no row is dropped and every mode column of the U rows is
    non-zero; cov is the inverse of the same A.  The same plan with group_modes=False raises today's text, an "E" set the new
    one."""
    import torch
    from pysurfinv_amd import senskernel
    model = synth.synth_models(4, 8, seed=21) if name == "synth_L8" else synth.water_models(4)
    B, _, L = model.shape
    per = synth.default_periods(8)
    truth = model.copy(); truth[:, 1, :] *= 1.03
    values = _forward4(truth, per)
    data = _datasets(per, values, SETS4, 0.01)
    dm, dp = torch.from_numpy(model).cuda(), torch.from_numpy(per).cuda()
    free = (model[:, 1, :] > 0)
    ps, qs = np.where(model[0, 1] > 0, 1.7, 0.0), np.where(model[0, 1] > 0, 0.3, 0.0)
    lam = np.full(B, 3.0)
    T = np.stack([[linearized.interface_mode(model[b, 3], [0, 1, 2], [3, 4]), linearized.thickness_mode(model[b, 3], [0])]
                  for b in range(B)])
    ms, beta, y = np.array([1e-3, 1e-2]), np.array([0.0, 0.4]), np.tile([0.5, -0.25], (B, 1))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    kw = dict(free=t(free.astype(np.uint8)), vp_slope=t(ps), rho_slope=t(qs), alpha=0.5, modes=t(T),
              mode_scale=t(np.tile(ms, (B, 1))), mode_prior=t(np.tile(beta, (B, 1))), mode_y=t(y))
    plan = linearized.LsqPlan(B, L, data, group_modes=True)
    st = plan.step(dm, t(lam), **kw)
    delta, dy = st["delta"].cpu().numpy(), st["delta_y"].cpu().numpy()
    stats, info = plan.stats.cpu().numpy(), plan.info.cpu().numpy()
    kr_ = senskernel.group_thickness_kernels(dm, dp, wtype="R")
    kl = senskernel.group_thickness_kernels(dm, dp, wtype="L")
    f64 = lambda x: None if x is None else x.cpu().numpy()
    for src, a in ((0, kr_), (2, kl)):                                     # the plan's kernels are these, bit for bit
        for k, got in (("dcdb", st["part"][3 * src]), ("dudb", st["part"][3 * src + 3]), ("dcdh", st["part_h"][src]), ("dudh", st["part_h"][src + 1])):
            assert np.isfinite(f64(a[k])).all() and torch.equal(got, a[k]), (k, src)
    assert st["part_h"][4] is None
    c = dict(B=B, Lmax=L, N=plan.joint.Ptot, K=2, nlay=np.full(B, L), free=free.astype(np.uint8), Q=np.ones(L - 1),
             vp_slope=np.tile(ps, (B, 1)), rho_slope=np.tile(qs, (B, 1)), cols=np.stack([plan.joint.col_src, plan.joint.col_idx], axis=1),
             weights=plan.joint.col_w, obs=plan.obs.cpu().numpy(), uncer=plan.uncer.cpu().numpy(), mask=plan.mask.cpu().numpy(),
             part=[f64(kr_[k]) for k in ("dcdb", "dcda", "dcdr", "dudb", "duda", "dudr")]
             + [f64(kl["dcdb"]), None, f64(kl["dcdr"]), f64(kl["dudb"]), None, f64(kl["dudr"])] + [None] * 3,
             pred=[f64(kr_["c0"]), f64(kr_["u0"]), f64(kl["c0"]), f64(kl["u0"]), None], modes=T,
             part_h=[f64(kr_["dcdh"]), f64(kr_["dudh"]), f64(kl["dcdh"]), f64(kl["dudh"]), None])
    N = plan.joint.Ptot
    assert N == 4 * per.size
    src_of = np.asarray(plan.joint.col_src)
    u_rows = np.isin(src_of, (1, 3))
    assert (src_of == 1).sum() == per.size and (src_of == 3).sum() == per.size
    As = []
    for b in range(B):
        tag = f"{name} stack {b}"
        idx, Qw, G, Gy, res, w = _rows_with_modes(c, b)
        x0 = model[b, 1, idx].astype(np.float64)
        ref = linearized.lsq_modes_step_reference(G, res, w, x0, 0.5, Qw, lam[b], Gy, ms, beta, y[b])
        assert info[b].tolist() == [N, 0, 0] and ref["flag"] == 0, tag        # every row kept, the U rows among them
        A, g = linearized.modes_normal_equations(G, Gy, res, w, x0, 0.5, Qw, lam[b], ms, beta, y[b])
        As.append((idx, A))
        d = np.concatenate([delta[b, idx], dy[b]])
        be = np.abs(A @ d - g).max()
        bar = 1e-11 * (np.abs(A).sum(axis=1).max() * np.abs(d).max() + np.abs(g).max())
        print(f"{tag}: backward error {be:.2e} (bar {bar:.2e})  delta_y {dy[b]}  |Gy| of the U rows {np.abs(Gy[u_rows]).min(axis=0)} .. {np.abs(Gy[u_rows]).max(axis=0)}")
        assert be <= bar, (tag, be, bar)
        for src in (1, 3):                                                  # every mode column of the U rows is non-zero
            assert np.abs(Gy[src_of == src]).max(axis=0).min() > 0, (tag, src)
        for k, nm in enumerate(("misfit", "roughness", "predicted")):
            assert abs(stats[b, k] - ref[nm]) <= 1e-12 * abs(ref[nm]), (tag, nm, stats[b, k], ref[nm])
    rs = plan.resolution(dm, t(lam), **kw)
    cov, flag = rs["cov"].cpu().numpy(), rs["flag"].cpu().numpy()
    for b, (idx, A) in enumerate(As):
        nu = idx.size + 2
        assert flag[b] == 0 and int(rs["used"][b]) == N
        e, bar = np.abs(A @ cov[b, :nu, :nu] - np.eye(nu)).max(), 1e-11 * (np.abs(A).sum(axis=1).max() * np.abs(cov[b]).max() + 1)
        print(f"{name} stack {b}: |A cov - I| {e:.2e} (bar {bar:.2e})")
        assert e <= bar, (b, e, bar)
    off = linearized.LsqPlan(B, L, data, group_modes=False)
    for call in (off.step, off.resolution):
        with pytest.raises(ValueError, match="thickness modes need phase-velocity data only: the library has no dU/dh or dchi/dh yet"):
            call(dm, t(lam), modes=t(T))
    with_e = linearized.LsqPlan(B, L, _datasets(per, values, (("R", "c"), ("R", "E")), 0.01), group_modes=True)
    with pytest.raises(ValueError, match="the library has no dchi/dh"):
        with_e.step(dm, t(lam), modes=t(T))


def _cpu_route_u(start, per, data, n_iter, T, mode_scale, above):
    """The iteration of LinearizedBatch in numpy float64 on the CPU checker for the sets of ``data`` (any of KEY but "E"), as
    lsq_cases.cpu_route: forward solves by oracle.cport.forward_batch, Jacobians by central differences of its float64 outputs (1 %
    of Vs; for the mode +-1 % of the thickness of the layers ``above``), steps by lsq_modes_step_reference, the same accept rule.
    Returns (model, rms, y [M])."""
    from oracle import cport
    M, _, L = start.shape
    eps, nb = 0.01, 2 * L + 2
    keys = [KEY[d.wave, d.quantity] for d in data]

    def fwd(m):
        cR, uR, sR = cport.forward_batch(m, per, 2, nthreads=8)
        cL, uL, sL = cport.forward_batch(m, per, 1, nthreads=8)
        return dict(cR=cR.astype(np.float64), uR=uR.astype(np.float64), cL=cL.astype(np.float64), uL=uL.astype(np.float64)), (sR != 0) | (sL != 0)

    def chi_rms(p):
        r = np.concatenate([(d.values - p[KEY[d.wave, d.quantity]]) / d.uncer for d in data], axis=1)
        chi = (r * r).sum(axis=1)
        return chi, np.sqrt(chi / r.shape[1])

    def objective(m):
        p, bad = fwd(m)
        chi, rms = chi_rms(p)
        rough = (np.diff(m[:, 1, :].astype(np.float64), axis=1) ** 2).sum(axis=1)
        return np.where(bad, np.inf, chi + ALPHA * rough), rms

    model, y = start.copy(), np.zeros(M)
    obj, rms = objective(model)
    assert np.isfinite(obj).all()
    lam = np.full(M, LAM0)
    sig = np.concatenate([d.uncer for d in data], axis=1)
    obsv = np.concatenate([d.values for d in data], axis=1)
    for _ in range(n_iter):
        big = np.repeat(model, nb, axis=0).reshape(M, nb, 5, L)
        for i in range(L):
            big[:, i, 1, i] *= (1 - eps); big[:, L + i, 1, i] *= (1 + eps)
        ey = 0.01 * model[:, 3, above].astype(np.float64).sum(axis=1)
        big[:, 2 * L, 3, :] = (model[:, 3, :].astype(np.float64) - T[None, :] * ey[:, None]).astype(np.float32)
        big[:, 2 * L + 1, 3, :] = (model[:, 3, :].astype(np.float64) + T[None, :] * ey[:, None]).astype(np.float32)
        pb, bad = fwd(big.reshape(M * nb, 5, L))
        assert not bad.any()
        pc, _ = fwd(model)
        trial, ty = model.copy(), y.copy()
        for m in range(M):
            v = np.concatenate([pb[k].reshape(M, nb, per.size)[m] for k in keys], axis=1)
            f0 = np.concatenate([pc[k][m] for k in keys])
            x = model[m, 1].astype(np.float64)
            G = ((v[L:2 * L] - v[:L]) / (2 * eps * x)[:, None]).T
            Gy = ((v[2 * L + 1] - v[2 * L]) / (2 * ey[m]))[:, None]
            st = linearized.lsq_modes_step_reference(G, obsv[m] - f0, 1.0 / sig[m] ** 2, x, ALPHA, np.ones(L - 1), lam[m], Gy, mode_scale,
                                                     0.0, y[m])
            trial[m, 1] = (x + st["delta"]).astype(np.float32)
            trial[m, 3] = (model[m, 3].astype(np.float64) + T * st["delta_y"][0]).astype(np.float32)
            ty[m] = y[m] + st["delta_y"][0]
        tobj, trms = objective(trial)
        acc = tobj < obj
        model, y = np.where(acc[:, None, None], trial, model), np.where(acc, ty, y)
        obj, rms = np.where(acc, tobj, obj), np.where(acc, trms, rms)
        lam = np.where(acc, np.maximum(lam / NU, LAM_MIN), lam * NU)
    return model, rms, y


def test_recovery_of_a_displaced_interface_from_group_velocities_alone():
    """The recovery problem of profiles/lsq_modes/recovery.txt (16 stacks of 8 layers, Vs off by a smooth +-5 %, the interface
    between the layers 0..3 and 4..6 displaced by +-10 km), fitted to U data ALONE - Rayleigh and Love, 12 periods, 0.5 % - with
    group_modes=True: 8 iterations, alpha 0.05, one interface mode, mode_scale 1e-4, no prior.  The float64 route on the host
    (_cpu_route_u: differences of U for every column, the mode's included) runs beside it.
    Bar: the interface ends no farther from the truth than twice the distance the host route reaches - the distance a route
    reaches being that of its worst stack, max_b |y_end - y_true|: both routes stop where the fp32 forward solver's noise over
    the 0.5 % uncertainty sits (recovery.txt of the phase-velocity problem: rms 0.001 either way), so stack by stack the two
    distances are two draws of that noise, while the worst of 16 is a stable figure of either route.  And every stack that
    accepted a step moved the right way and less than twice as far, as in test_recovery_of_a_displaced_interface.
    Both distances, stack by stack, go to profiles/group_thickness/recovery.txt."""
    true, start = _true_and_start()
    T = linearized.interface_mode(true[0, 3], ABOVE, BELOW)
    sign = np.where(np.arange(16) % 2 == 0, 1.0, -1.0)
    shift = 0.1 * true[:, 3, ABOVE].astype(np.float64).sum(axis=1) * sign
    start = start.copy()
    start[:, 3, :] = (true[:, 3, :].astype(np.float64) + T[None, :] * shift[:, None]).astype(np.float32)
    y_true = -shift
    per = synth.default_periods(12)
    data = _datasets(per, _forward4(true, per), SETS_U, 0.005)
    kw = dict(alpha=ALPHA, lam0=LAM0, nu=NU, lam_min=LAM_MIN)
    with pytest.raises(ValueError, match="thickness modes need phase-velocity data only"):
        linearized.LinearizedBatch(start, data, modes=T[None], mode_scale=MODE_SCALE, **kw)
    inv = linearized.LinearizedBatch(start, data, modes=T[None], mode_scale=MODE_SCALE, group_modes=True, **kw)
    rms0 = inv.rms.cpu().numpy()
    out = inv.run(N_ITER)
    rms_dev, y_end = out["rms"][-1].cpu().numpy(), out["y"][-1, :, 0].cpu().numpy()
    accepted = out["accepted"].cpu().numpy().any(axis=0)
    _, rms_cpu, y_cpu = _cpu_route_u(start, per, data, N_ITER, T, MODE_SCALE, ABOVE)
    d_dev, d_cpu = np.abs(y_end - y_true), np.abs(y_cpu - y_true)
    print("stack  rms_start  rms_device  rms_cpu   y_true    y_end    y_cpu   |y_end - y_true|  |y_cpu - y_true|")
    for b in range(16):
        print(f"{b:5d}  {rms0[b]:9.3f}  {rms_dev[b]:10.4f}  {rms_cpu[b]:7.4f}  {y_true[b]:7.2f}  {y_end[b]:7.2f}  {y_cpu[b]:7.2f}  {d_dev[b]:16.3f}  {d_cpu[b]:16.3f}")
    print(f"worst distance from the truth: device {d_dev.max():.3f} km, host route {d_cpu.max():.3f} km (bar: 2 x the host route's)")
    assert accepted.any()
    assert (d_dev[accepted] < np.abs(y_true)[accepted]).all(), (y_end, y_true)
    assert d_dev.max() <= 2.0 * d_cpu.max(), (d_dev, d_cpu)
