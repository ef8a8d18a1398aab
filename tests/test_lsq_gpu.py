"""surfdisp_lsq_step_device and the linearised inversion built on it (pysurfinv_amd.linearized), on the GPU.

Bars.  Backward error of the solve: ||A delta - g||inf <= 1e-11 (||A||inf ||delta||inf + ||g||inf), with A and g formed in
numpy float64 from the same fp32 inputs: the fp64 Cholesky bound gamma_{3n+1} plus the N-term accumulation is
(3 * 128 + 1 + 256) * 1.1e-16 ~ 7e-14 (Higham, Accuracy and Stability of Numerical Algorithms); the bar is ~100 x that and does
not depend on the conditioning.  Misfit, roughness and predicted objective: relative 1e-12; counts exact."""
import numpy as np
import pytest

from lsq_cases import (ALPHA, CASES, LAM0, LAM_MIN, N_ITER, NU, SETS3, _case, _chi_rms, _datasets, _forward_all, _rows_of,
                       _true_and_start, cpu_route, launch)
from pysurfinv_amd import _lib, linearized, synth

pytestmark = pytest.mark.gpu


def _launch(c, **kw):
    """surfdisp_lsq_step_device on the arrays of ``c`` (``lsq_cases.launch``).  Returns (rc, delta, stats, info)."""
    rc, o = launch("step", c, **kw)
    return rc, o["delta"], o["stats"], o["info"]


def _check_stack(tag, idx, Qw, G, res, w, x0, alpha, lam, delta_row, stats, info, N):
    """One stack's outputs against the reference step: flag, counts, zeros, backward error, the three objectives."""
    ref = linearized.lsq_step_reference(G, res, w, x0, alpha, Qw, lam)
    used, dropped, flag = (int(v) for v in info)
    assert (used, dropped) == (len(res), N - len(res)), (tag, used, dropped, len(res))
    assert flag == ref["flag"], (tag, flag, ref["flag"])
    off = np.ones(delta_row.size, bool); off[idx] = False
    assert np.isfinite(delta_row).all() and not delta_row[off].any(), tag
    d = delta_row[idx]
    if flag != 0:
        assert not d.any(), tag
    else:
        A, g = linearized.normal_equations(G, res, w, x0, alpha, Qw, lam)
        be = np.abs(A @ d - g).max()
        bar = 1e-11 * (np.abs(A).sum(axis=1).max() * np.abs(d).max() + np.abs(g).max())
        print(f"{tag}: n {idx.size} rows {used} backward error {be:.2e} (bar {bar:.2e})")
        assert be <= bar, (tag, be, bar)
    for k, name in enumerate(("misfit", "roughness", "predicted")):
        assert abs(stats[k] - ref[name]) <= 1e-12 * abs(ref[name]), (tag, name, stats[k], ref[name])
    return flag


@pytest.mark.parametrize("B,Lmax,N", CASES)
def test_step_kernel_matches_the_reference_step(B, Lmax, N):
    c = _case(B, Lmax, N, seed=1000 + Lmax)
    rc, delta, stats, info = _launch(c)
    assert rc == _lib.SUCCESS, _lib.lib().surfdisp_last_error()
    flags = []
    for b in range(B):
        idx, Qw, G, res, w = _rows_of(c, b)
        x0 = c["model"][b, 1, idx].astype(np.float64)
        flags.append(_check_stack(f"({B},{Lmax},{N}) stack {b}", idx, Qw, G, res, w, x0, c["alpha"], c["lam"][b], delta[b],
                                  stats[b], info[b], N))
    if c["obs"].ndim == 2 and B >= 3:
        assert flags[2] == 1 and flags[1] == 0 and flags[3 % B] == 0          # every row masked: flag 1, its neighbours solved
    assert info[:, 1].sum() > 0 or N == 1                                  # rows were dropped somewhere


def test_failed_pivot_is_flag_2_and_leaves_the_neighbours_alone():
    """N < n, alpha = 0, lam = 0, and layers the data do not see (kernel columns exactly 0): a pivot that is exactly 0 - an
    arithmetic outcome, flag 2, delta = 0, everything finite; the stacks on both sides of it in the same launch stay right."""
    c = _case(3, 8, 3, seed=77)
    c["alpha"] = 0.0
    c["lam"] = np.array([4.0, 0.0, 4.0])
    c["free"] = np.ones(8, np.uint8)
    c["nlay"][:] = 8
    c["obs"], c["uncer"], c["mask"] = np.array([3.0, 3.1, 3.2]), np.array([0.03, 0.03, 0.03]), np.ones(3, np.uint8)
    for a in c["part"]:
        if a is not None:
            a[:, :, 5:] = 0.0
    rc, delta, stats, info = _launch(c)
    assert rc == _lib.SUCCESS
    assert info[:, 2].tolist() == [0, 2, 0]
    assert not delta[1].any() and np.isfinite(stats).all() and np.isfinite(delta).all()
    assert stats[1, 2] == stats[1, 0] + 0.0 * stats[1, 1]                   # the predicted objective at x0 itself
    for b in (0, 2):
        idx, Qw, G, res, w = _rows_of(c, b)
        _check_stack(f"beside a failed pivot, stack {b}", idx, Qw, G, res, w, c["model"][b, 1, idx].astype(np.float64), 0.0,
                     c["lam"][b], delta[b], stats[b], info[b], 3)


def test_step_entry_refuses_bad_arguments_before_launching():
    c = _case(1, 200, 6, seed=5)
    rc, delta, stats, info = _launch(c, nfree_max=129)
    assert rc == _lib.ERR_INVALID and (delta == 7.0).all() and (info == 7).all()
    for name in ("lam", "model", "obs", "mask", "cols"):
        rc, delta, stats, info = _launch(c, nfree_max=128, **{name: True})
        assert rc == _lib.ERR_INVALID and (delta == 7.0).all() and (info == 7).all(), name
    rc, delta, stats, info = _launch(c, nfree_max=128)                       # 200 free layers against nfree_max 128: not solved
    assert rc == _lib.SUCCESS and info[0].tolist() == [0, 6, 3] and not delta.any()


# ------------------------------------------------------------------------------------------------- on real kernels
@pytest.mark.parametrize("name", ["synth_L8", "water_L9"])
def test_step_on_real_kernels(name):
    """LsqPlan.step against G, r re-formed on the host from analytic_kernels of the same model; its data misfit against the
    obsdata misfit of BatchPlan.run's predictions (relative 1e-10)."""
    import torch
    from pysurfinv_amd import senskernel
    model = synth.synth_models(4, 8, seed=21) if name == "synth_L8" else synth.water_models(4)
    B, _, L = model.shape
    per = synth.default_periods(8)
    sets = (("R", "c"), ("R", "U"), ("L", "c"), ("R", "E"))
    truth = model.copy(); truth[:, 1, :] *= 1.03
    data = _datasets(per, _forward_all(truth, per), sets, 0.01, C=B)
    dm, dp = torch.from_numpy(model).cuda(), torch.from_numpy(per).cuda()
    free = (model[:, 1, :] > 0)
    ps, qs = np.where(model[0, 1] > 0, 1.7, 0.0), np.where(model[0, 1] > 0, 0.3, 0.0)
    lam = np.full(B, 3.0)
    plan = linearized.LsqPlan(B, L, data)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    st = plan.step(dm, t(lam), free=t(free.astype(np.uint8)), vp_slope=t(ps), rho_slope=t(qs), alpha=0.5)
    delta, stats, info = st["delta"].cpu().numpy(), plan.stats.cpu().numpy(), plan.info.cpu().numpy()
    chi, rms, failed = (x.cpu().numpy() for x in plan.chi_square(dm))
    kg = senskernel.analytic_kernels(dm, dp, wtype="R", group=True)
    ke = senskernel.analytic_kernels(dm, dp, wtype="R", ellipticity=True)
    kl = senskernel.analytic_kernels(dm, dp, wtype="L")
    f64 = lambda x: None if x is None else x.cpu().numpy()
    c = dict(B=B, Lmax=L, nlay=np.full(B, L), free=free.astype(np.uint8), Q=np.ones(L - 1), vp_slope=np.tile(ps, (B, 1)),
             rho_slope=np.tile(qs, (B, 1)), cols=np.stack([plan.joint.col_src, plan.joint.col_idx], axis=1),
             weights=plan.joint.col_w, obs=plan.obs.cpu().numpy(), uncer=plan.uncer.cpu().numpy(), mask=plan.mask.cpu().numpy(),
             part=[f64(kg[k]) for k in ("dcdb", "dcda", "dcdr", "dudb", "duda", "dudr")] + [f64(kl["dcdb"]), None, f64(kl["dcdr"])]
             + [None] * 3 + [f64(ke[k]) for k in ("dedb", "deda", "dedr")],
             pred=[f64(kg["c0"]), f64(kg["u0"]), f64(kl["c0"]), None, f64(ke["ratio"])])
    N = plan.joint.Ptot
    for b in range(B):
        idx, Qw, G, res, w = _rows_of(c, b)
        _check_stack(f"{name} stack {b}", idx, Qw, G, res, w, model[b, 1, idx].astype(np.float64), 0.5, lam[b], delta[b],
                     stats[b], info[b], N)
        assert info[b, 0] == N and not failed[b]
        assert abs(stats[b, 0] - chi[b]) <= 1e-10 * chi[b], (b, stats[b, 0], chi[b])


# ------------------------------------------------------------------------------------------------- the iteration
@pytest.fixture(scope="module")
def loop_problem():
    true, start = _true_and_start()
    per = synth.default_periods(12)
    obs = _forward_all(true, per)
    return true, start, per, obs


def test_loop_invariants(loop_problem):
    true, start, per, obs = loop_problem
    sets = SETS3 + (("R", "E"),)
    data = _datasets(per, obs, sets, 0.005)
    Ptot = 12 * len(sets)
    mask = np.ones((16, Ptot), bool); mask[5] = False
    lo, hi = 2.6, 4.62
    inv = linearized.LinearizedBatch(start, data, alpha=ALPHA, lam0=LAM0, nu=NU, lam_min=LAM_MIN, vs_bounds=(lo, hi), mask=mask)
    obj0 = inv.objective.cpu().numpy()
    out = {k: v.cpu().numpy() for k, v in inv.run(N_ITER, keep_models=True).items()}
    obj = np.concatenate([obj0[None], out["objective"]])
    assert (np.diff(obj, axis=0) <= 0).all()                                # never increases
    lam = np.full(16, LAM0)
    models = np.concatenate([start[None], out["models"]])
    for it in range(N_ITER):
        acc = out["accepted"][it]
        lam = np.where(acc, np.maximum(lam / NU, LAM_MIN), lam * NU)
        assert np.array_equal(lam, out["lam"][it])                          # the stated rule, exactly
        same = (models[it + 1] == models[it]).reshape(16, -1).all(axis=1)
        assert same[~acc].all()                                             # a rejected stack's model is bit-unchanged
        assert (obj[it + 1][acc] < obj[it][acc]).all() and np.array_equal(obj[it + 1][~acc], obj[it][~acc])
        moved = models[it + 1][:, 1, :] != start[:, 1, :]
        vs = models[it + 1][:, 1, :]
        assert (vs[moved] >= np.float32(lo)).all() and (vs[moved] <= np.float32(hi)).all()
        assert np.array_equal(models[it + 1][:, 3:], start[:, 3:]) and np.array_equal(models[it + 1][:, 0], start[:, 0])
    assert (out["flag"][:, 5] == 1).all() and not out["accepted"][:, 5].any() and np.array_equal(out["model"][5], start[5])
    assert (out["flag"][:, np.arange(16) != 5] == 0).all()
    chi, rms = _chi_rms(_forward_all(out["model"], per), data, mask)
    assert np.allclose(rms, out["rms"][-1], rtol=1e-12, atol=0, equal_nan=True)
    print("rms start -> end:", np.round(inv.rms.cpu().numpy(), 3))


def _cpu_route(start, per, data, n_iter):
    """The same iteration in numpy float64 on the CPU checker (``lsq_cases.cpu_route`` without a mode).  Returns (model, rms)."""
    return cpu_route(start, per, data, n_iter)[:2]


def test_recovery_against_the_cpu_route(loop_problem):
    """Per stack rms_gpu <= max(2 rms_cpu, 0.02): 0.02 is the project's 1e-4 parity bar over the 5e-3 relative uncertainty (the
    floor below which the two forward solvers differ anyway); the factor 2 lets the fp32 kernels' documented error against
    finite differences (<= 4.5e-3 of a period's peak for dU) cost an iteration."""
    true, start, per, obs = loop_problem
    data = _datasets(per, obs, SETS3, 0.005)
    inv = linearized.LinearizedBatch(start, data, alpha=ALPHA, lam0=LAM0, nu=NU, lam_min=LAM_MIN)
    rms0 = inv.rms.cpu().numpy()
    out = inv.run(N_ITER)
    rms_gpu = out["rms"][-1].cpu().numpy()
    _, rms_cpu = _cpu_route(start, per, data, N_ITER)
    print("stack  rms_start  rms_gpu  rms_cpu")
    for b in range(16):
        print(f"{b:5d}  {rms0[b]:9.3f}  {rms_gpu[b]:7.4f}  {rms_cpu[b]:7.4f}")
    assert (rms_gpu <= np.maximum(2 * rms_cpu, 0.02)).all(), (rms_gpu, rms_cpu)
