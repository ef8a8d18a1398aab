"""Thickness modes as unknowns of the least-squares step and of the resolution kernel (surfdisp_lsq_step_modes_device,
surfdisp_lsq_resolution_modes_device, include/surfdisp.h section (6h)) and the Python layers on them, on the GPU.

The random inputs are those of tests/test_lsq_gpu.py (``_case`` of tests/lsq_cases.py) plus the mode arguments; the rows of a stack come
from ``_rows_of`` with the two extra drop rules applied through the mask.  Bars: those of tests/test_lsq_gpu.py for the step (backward
error 1e-11 (||A||inf ||delta||inf + ||g||inf): the fp64 Cholesky bound plus the N-term accumulation is (3 x 136 + 1 + 256) x 1.1e-16
~ 7e-14 at the largest size, a hundred times under; objectives relative 1e-12; counts and flags exact) and those of
tests/test_lsq_resolution_gpu.py for the resolution."""
import numpy as np
import pytest

from lsq_cases import (ALPHA, LAM0, LAM_MIN, LAM_FACTOR, N_ITER, NU, _chi_rms, _datasets, _forward_all, _mode_case, _nan_row, _rows_of,
                       _true_and_start, cpu_route, launch)
from pysurfinv_amd import _lib, linearized, synth

pytestmark = pytest.mark.gpu

CASES = [(1, 2, 1, 1), (5, 3, 7, 2), (3, 17, 40, 3), (2, 64, 100, 8), (1, 128, 256, 8), (300, 9, 12, 1)]


def _launch(c, entry, **kw):
    """surfdisp_lsq_step_modes_device (entry "step") or surfdisp_lsq_resolution_modes_device ("res") on the arrays of ``c``
    (``lsq_cases.launch``).  Returns (rc, dict of numpy outputs)."""
    return launch(entry + "_modes", c, **kw)


def _launch_step_old(c):
    rc, o = launch("step", c)
    return rc, o["delta"], o["stats"], o["info"]


def _launch_res_old(c):
    return launch("res", c)


def _kept_rows(c, b):
    """The indices of the rows of stack b that ``_rows_of`` keeps: with weights r + 1 and every valid uncertainty 1 (the drop
    rules see the same values), the w it returns for row r is r + 1."""
    unc = c["uncer"]
    c1 = dict(c, weights=np.arange(1.0, c["N"] + 1), uncer=np.where(np.isfinite(unc) & (unc > 0), 1.0, unc))
    return np.rint(_rows_of(c1, b)[4]).astype(int) - 1


def _mode_columns(c, b):
    """gy [N, K]: the mode columns of every row of stack b by the formula of section (6h); NaN for a row whose source has no
    part_h array."""
    T = c["modes"][b] if c["modes"].ndim == 3 else c["modes"]
    gy = np.full((c["N"], c["K"]), np.nan)
    for r, (src, k) in enumerate(c["cols"]):
        ph = c["part_h"][4 if src == 5 else int(src)]
        if ph is not None and k < ph.shape[1]:
            gy[r] = linearized.mode_columns(ph[b, k], T, c["nlay"][b])[0]
    return gy


def _mode_mask(c, b, gy=None):
    """The mask [N] of stack b with the two drop rules of section (6h) applied: no part_h array, a mode column that is not finite."""
    gy = _mode_columns(c, b) if gy is None else gy
    return ((c["mask"][b] if c["mask"].ndim == 2 else c["mask"]).astype(bool) & np.isfinite(gy).all(axis=1)).astype(np.uint8)


def _rows_with_modes(c, b):
    """(idx, Qw, G, Gy, res, w) of stack b: the rows ``_rows_of`` keeps under ``_mode_mask``, and their mode columns."""
    gy = _mode_columns(c, b)
    c2 = dict(c, mask=_mode_mask(c, b, gy))
    rows = _kept_rows(c2, b)
    idx, Qw, G, res, w = _rows_of(c2, b)
    assert len(rows) == len(w)
    return idx, Qw, G, gy[rows].reshape(len(rows), c["K"]), res, w


def _mode_vectors(c, b):
    pick = lambda a: a[b] if a.ndim == 2 else a
    return pick(c["mode_scale"]), pick(c["mode_prior"]), c["mode_y"][b]


# ------------------------------------------------------------------------------------------------- 1. the step entry
@pytest.mark.parametrize("B,Lmax,N,K", CASES)
def test_step_modes_kernel_matches_the_reference_step(B, Lmax, N, K):
    c = _mode_case(B, Lmax, N, K)
    rc, o = _launch(c, "step")
    assert rc == _lib.SUCCESS, _lib.lib().surfdisp_last_error()
    flags, nan_row_dropped = [], False
    for b in range(B):
        tag = f"({B},{Lmax},{N},{K}) stack {b}"
        idx, Qw, G, Gy, res, w = _rows_with_modes(c, b)
        ms, beta, y = _mode_vectors(c, b)
        x0 = c["model"][b, 1, idx].astype(np.float64)
        ref = linearized.lsq_modes_step_reference(G, res, w, x0, c["alpha"], Qw, c["lam"][b], Gy, ms, beta, y)
        used, dropped, flag = (int(v) for v in o["info"][b])
        assert (used, dropped) == (len(res), N - len(res)), (tag, used, dropped, len(res))
        assert flag == ref["flag"], (tag, flag, ref["flag"])
        delta, dy = o["delta"][b], o["delta_y"][b]
        off = np.ones(Lmax, bool); off[idx] = False
        assert np.isfinite(delta).all() and np.isfinite(dy).all() and not delta[off].any(), tag
        if flag != 0:
            assert not delta.any() and not dy.any(), tag
        else:
            A, g = linearized.modes_normal_equations(G, Gy, res, w, x0, c["alpha"], Qw, c["lam"][b], ms, beta, y)
            d = np.concatenate([delta[idx], dy])
            be = np.abs(A @ d - g).max()
            bar = 1e-11 * (np.abs(A).sum(axis=1).max() * np.abs(d).max() + np.abs(g).max())
            print(f"{tag}: n {idx.size} + {K} rows {used} backward error {be:.2e} (bar {bar:.2e})")
            assert be <= bar, (tag, be, bar)
        for k, name in enumerate(("misfit", "roughness", "predicted")):
            assert abs(o["stats"][b, k] - ref[name]) <= 1e-12 * abs(ref[name]), (tag, name, o["stats"][b, k], ref[name])
        flags.append(flag)
    if c["obs"].ndim == 2 and B >= 3:
        assert flags[2] == 1 and flags[1] == 0 and flags[3 % B] == 0          # every row masked: flag 1, its neighbours solved
    r = _nan_row(N)
    if r is not None:                    # the row of the NaN thickness kernel: the Vs rules keep it, the mode rule drops it
        assert r in _kept_rows(c, 0) and r not in _kept_rows(dict(c, mask=_mode_mask(c, 0)), 0)
    assert (o["info"][:, 1] >= np.isin(c["cols"][:, 0], (1, 3, 4, 5)).sum()).all()     # the rows of the sources without part_h


# ------------------------------------------------------------------------------------------------- 2. K = 0
@pytest.mark.parametrize("B,Lmax,N", [(3, 17, 40), (2, 64, 100)])
def test_no_modes_through_the_new_entries_is_the_old_entries_bit_for_bit(B, Lmax, N):
    c = _mode_case(B, Lmax, N, 1)
    rc, delta, stats, info = _launch_step_old(c)
    assert rc == _lib.SUCCESS
    for null in ({}, dict(modes=True, mode_scale=True, mode_prior=True, mode_y=True, delta_y=True)):
        rc, o = _launch(c, "step", K=0, no_part_h=bool(null), **null)
        assert rc == _lib.SUCCESS, _lib.lib().surfdisp_last_error()
        assert np.array_equal(o["delta"], delta) and np.array_equal(o["stats"], stats) and np.array_equal(o["info"], info)
        assert (o["delta_y"] == 7.0).all()
    rc, old = _launch_res_old(c)
    assert rc == _lib.SUCCESS
    for null in ({}, dict(modes=True, mode_scale=True, mode_prior=True, mode_y=True, sigma_post_y=True, sigma_data_y=True, rdiag_y=True)):
        rc, o = _launch(c, "res", K=0, no_part_h=bool(null), **null)
        assert rc == _lib.SUCCESS, _lib.lib().surfdisp_last_error()
        for k in old:
            assert np.array_equal(o[k], old[k]), k
        assert all((o[k] == 7.0).all() for k in ("sigma_post_y", "sigma_data_y", "rdiag_y"))


# ------------------------------------------------------------------------------------------------- 3. the resolution entry
def _check_resolution(tag, c, o, b, lam):
    """The outputs of stack b against lsq_modes_resolution_reference: the checks and bars of _check_stack of
    tests/test_lsq_resolution_gpu.py over the n + K unknowns."""
    K, N, Lmax = c["K"], c["N"], c["Lmax"]
    idx, Qw, G, Gy, _, w = _rows_with_modes(c, b)
    ms, beta, _ = _mode_vectors(c, b)
    n = idx.size
    nu = n + K
    ref = linearized.lsq_modes_resolution_reference(G, w, n, c["alpha"], Qw, lam, Gy, ms, beta)
    used, dropped, flag = (int(v) for v in o["info"][b])
    assert (used, dropped) == (len(w), N - len(w)), (tag, used, dropped, len(w))
    assert flag == ref["flag"], (tag, flag, ref["flag"])
    cov, res = o["cov"][b], o["res"][b]
    per_layer = [o[k][b] for k in ("sigma_post", "sigma_data", "rdiag")]
    per_mode = [o[k][b] for k in ("sigma_post_y", "sigma_data_y", "rdiag_y")]
    for a in (cov, res, o["stats"][b], *per_layer, *per_mode):
        assert np.isfinite(a).all(), tag
    off = np.ones(Lmax, bool); off[idx] = False
    for a in per_layer:
        assert not a[off].any(), tag
    for a in (cov, res):                                                    # rows and columns >= n + K
        assert a.shape == (Lmax + K, Lmax + K) and not a[nu:, :].any() and not a[:, nu:].any(), tag
    if flag != 0:
        assert not cov.any() and not res.any() and not o["stats"][b].any(), tag
        assert not any(a.any() for a in per_layer) and not any(a.any() for a in per_mode), tag
        return flag
    cov, res = cov[:nu, :nu], res[:nu, :nu]
    assert np.array_equal(cov, cov.T), tag
    A, _ = linearized.modes_normal_equations(G, Gy, np.zeros(len(w)), w, np.zeros(n), c["alpha"], Qw, lam, ms, beta, None)
    Ga = np.concatenate([G, Gy], axis=1)
    H = Ga.T @ (w[:, None] * Ga)
    na = np.abs(A).sum(axis=1).max()
    e1, bar1 = np.abs(A @ cov - np.eye(nu)).max(), 1e-11 * (na * np.abs(cov).max() + 1)
    e2, bar2 = np.abs(A @ res - H).max(), 1e-11 * (na * np.abs(res).max() + np.abs(H).max())
    cond = np.linalg.cond(A)
    print(f"{tag}: n {n} + {K} rows {used} |A cov - I| {e1:.2e} (bar {bar1:.2e})  |A res - H| {e2:.2e} (bar {bar2:.2e})  cond(A) {cond:.1e}")
    assert cond <= 1e4, (tag, cond)                                         # the premise of the relative bars below
    assert e1 <= bar1, (tag, e1, bar1)
    assert e2 <= bar2, (tag, e2, bar2)
    both = lambda a, ay: np.concatenate([a[idx], ay])
    for name, got, want in (("rdiag", both(o["rdiag"][b], o["rdiag_y"][b]), ref["rdiag"]),
                            ("sigma_post^2", both(o["sigma_post"][b], o["sigma_post_y"][b]) ** 2, np.diag(ref["cov"])),
                            ("sigma_data^2", both(o["sigma_data"][b], o["sigma_data_y"][b]) ** 2, np.diag(ref["res"] @ ref["cov"]))):
        err, bar = np.abs(got - want), 1e-9 * np.abs(want) + 1e-12 * np.abs(want).max()
        print(f"    {name}: worst error / bar {(err / bar).max():.2e}")
        assert (err <= bar).all(), (tag, name, (err / bar).max())
    dof, logdet = o["stats"][b]
    assert abs(dof - ref["dof"]) <= 1e-9 * nu, (tag, dof, ref["dof"])
    assert abs(logdet - ref["logdet"]) <= 1e-10 * (abs(ref["logdet"]) + nu), (tag, logdet, ref["logdet"])
    return flag


@pytest.mark.parametrize("lam_scale", [1.0, 1000.0 / LAM_FACTOR], ids=["lam_of_the_case", "1000_x_lam_of_test_lsq_gpu"])
@pytest.mark.parametrize("B,Lmax,N,K", CASES)
def test_resolution_modes_kernel_matches_the_reference(B, Lmax, N, K, lam_scale):
    """Both dampings of tests/test_lsq_resolution_gpu.py: the case's own, and 1000 x that of ``_case`` (the strong damping at which
    the entries of R = I - C (...) are small against their absolute error of a few ulp of 1)."""
    c = _mode_case(B, Lmax, N, K)
    rc, o = _launch(c, "res", lam_scale=lam_scale)
    assert rc == _lib.SUCCESS, _lib.lib().surfdisp_last_error()
    flags = [_check_resolution(f"({B},{Lmax},{N},{K}) lam x {lam_scale:g} stack {b}", c, o, b, c["lam"][b] * lam_scale) for b in range(B)]
    if c["obs"].ndim == 2 and B >= 3:
        assert flags[2] == 1 and flags[1] == 0 and flags[3 % B] == 0          # all zeros between two solved neighbours


# ------------------------------------------------------------------------------------------------- 4. bad arguments
def test_mode_entries_refuse_bad_arguments_before_launching():
    c = _mode_case(1, 200, 6, 2, seed=5)
    untouched = lambda o: all((v == 7).all() for v in o.values())
    for entry, outs in (("step", ("delta_y",)), ("res", ("sigma_post_y", "sigma_data_y", "rdiag_y"))):
        for K in (-1, 9):
            rc, o = _launch(c, entry, K=K, nfree_max=128)
            assert rc == _lib.ERR_INVALID and untouched(o), (entry, K)
        for name in ("modes", "mode_scale") + outs:
            rc, o = _launch(c, entry, nfree_max=128, **{name: True})
            assert rc == _lib.ERR_INVALID and untouched(o), (entry, name)
        rc, o = _launch(c, entry, nfree_max=128, no_part_h=True)
        assert rc == _lib.ERR_INVALID and untouched(o), (entry, "part_h")
        rc, o = _launch(c, entry, K=8, nfree_max=129)                        # 129 + 8 unknowns against 136
        assert rc == _lib.ERR_INVALID and untouched(o), (entry, "nfree_max + K")
        rc, o = _launch(c, entry, nfree_max=0)
        assert rc == _lib.ERR_INVALID and untouched(o), (entry, "a condition of (6d)")
        # mode_prior and mode_y may be NULL; 200 free layers against nfree_max 128: not solved, flag 3, zeros
        rc, o = _launch(c, entry, nfree_max=128, mode_prior=True, mode_y=True)
        assert rc == _lib.SUCCESS and o["info"][0].tolist() == [0, 6, 3], entry
        assert not any(v.any() for k, v in o.items() if k != "info"), entry


# ------------------------------------------------------------------------------------------------- 5. on real kernels
@pytest.mark.parametrize("name", ["synth_L8", "water_L9"])
def test_step_with_modes_on_real_kernels(name):
    """LsqPlan.step(modes=...) against G, Gy, r re-formed on the host from analytic_kernels(thickness=True) of the same model - the
    dcdh rows contracted with T; the check and the bars of test_step_on_real_kernels.  The same plan with a U set: ValueError."""
    import torch
    from pysurfinv_amd import senskernel
    model = synth.synth_models(4, 8, seed=21) if name == "synth_L8" else synth.water_models(4)
    B, _, L = model.shape
    per = synth.default_periods(8)
    truth = model.copy(); truth[:, 1, :] *= 1.03
    values = _forward_all(truth, per)
    data = _datasets(per, values, (("R", "c"), ("L", "c")), 0.01, C=B)
    dm, dp = torch.from_numpy(model).cuda(), torch.from_numpy(per).cuda()
    free = (model[:, 1, :] > 0)
    ps, qs = np.where(model[0, 1] > 0, 1.7, 0.0), np.where(model[0, 1] > 0, 0.3, 0.0)
    lam = np.full(B, 3.0)
    # per stack: the interface between the layers 0..2 and 3..4 (water_L9: the sea floor's sediment and crust against the
    # layers below), and the thickness of the top layer (water_L9: the water depth)
    T = np.stack([[linearized.interface_mode(model[b, 3], [0, 1, 2], [3, 4]), linearized.thickness_mode(model[b, 3], [0])]
                  for b in range(B)])
    ms, beta, y = np.array([1e-3, 1e-2]), np.array([0.0, 0.4]), np.tile([0.5, -0.25], (B, 1))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    plan = linearized.LsqPlan(B, L, data)
    st = plan.step(dm, t(lam), free=t(free.astype(np.uint8)), vp_slope=t(ps), rho_slope=t(qs), alpha=0.5, modes=t(T),
                   mode_scale=t(np.tile(ms, (B, 1))), mode_prior=t(np.tile(beta, (B, 1))), mode_y=t(y))
    delta, dy = st["delta"].cpu().numpy(), st["delta_y"].cpu().numpy()
    stats, info = plan.stats.cpu().numpy(), plan.info.cpu().numpy()
    chi, rms, failed = (x.cpu().numpy() for x in plan.chi_square(dm))
    kr_ = senskernel.analytic_kernels(dm, dp, wtype="R", thickness=True)
    kl = senskernel.analytic_kernels(dm, dp, wtype="L", thickness=True)
    f64 = lambda x: None if x is None else x.cpu().numpy()
    assert np.isfinite(f64(kr_["dcdh"])).all() and np.isfinite(f64(kl["dcdh"])).all()
    for k, a in (("dcdb", kr_), ("dcdh", kr_), ("dcdb", kl), ("dcdh", kl)):    # the plan's kernels are these, bit for bit
        src = 0 if a is kr_ else 2
        got = st["part"][3 * src] if k == "dcdb" else st["part_h"][src]
        assert torch.equal(got, a[k]), (k, src)
    c = dict(B=B, Lmax=L, N=plan.joint.Ptot, K=2, nlay=np.full(B, L), free=free.astype(np.uint8), Q=np.ones(L - 1),
             vp_slope=np.tile(ps, (B, 1)), rho_slope=np.tile(qs, (B, 1)), cols=np.stack([plan.joint.col_src, plan.joint.col_idx], axis=1),
             weights=plan.joint.col_w, obs=plan.obs.cpu().numpy(), uncer=plan.uncer.cpu().numpy(), mask=plan.mask.cpu().numpy(),
             part=[f64(kr_[k]) for k in ("dcdb", "dcda", "dcdr")] + [None] * 3 + [f64(kl["dcdb"]), None, f64(kl["dcdr"])] + [None] * 6,
             pred=[f64(kr_["c0"]), None, f64(kl["c0"]), None, None], modes=T,
             part_h=[f64(kr_["dcdh"]), None, f64(kl["dcdh"]), None, None])
    N = plan.joint.Ptot
    for b in range(B):
        tag = f"{name} stack {b}"
        idx, Qw, G, Gy, res, w = _rows_with_modes(c, b)
        x0 = model[b, 1, idx].astype(np.float64)
        ref = linearized.lsq_modes_step_reference(G, res, w, x0, 0.5, Qw, lam[b], Gy, ms, beta, y[b])
        assert info[b].tolist() == [N, 0, 0] and ref["flag"] == 0 and not failed[b], tag
        A, g = linearized.modes_normal_equations(G, Gy, res, w, x0, 0.5, Qw, lam[b], ms, beta, y[b])
        d = np.concatenate([delta[b, idx], dy[b]])
        be = np.abs(A @ d - g).max()
        bar = 1e-11 * (np.abs(A).sum(axis=1).max() * np.abs(d).max() + np.abs(g).max())
        print(f"{tag}: backward error {be:.2e} (bar {bar:.2e})  delta_y {dy[b]}  |Gy| {np.abs(Gy).max(axis=0)}")
        assert be <= bar, (tag, be, bar)
        assert np.abs(Gy).max(axis=0).min() > 0, tag                        # both modes are seen by the data
        for k, nm in enumerate(("misfit", "roughness", "predicted")):
            assert abs(stats[b, k] - ref[nm]) <= 1e-12 * abs(ref[nm]), (tag, nm, stats[b, k], ref[nm])
        assert abs(stats[b, 0] - chi[b]) <= 1e-10 * chi[b], (b, stats[b, 0], chi[b])
    with_u = linearized.LsqPlan(B, L, _datasets(per, values, (("R", "c"), ("R", "U"), ("L", "c")), 0.01, C=B))
    for call in (with_u.step, with_u.resolution):
        with pytest.raises(ValueError, match="thickness modes need phase-velocity data only: the library has no dU/dh or dchi/dh yet"):
            call(dm, t(lam), modes=t(T))
    with pytest.raises(ValueError, match="thickness modes need phase-velocity data only"):
        linearized.LinearizedBatch(model, _datasets(per, values, (("R", "c"), ("R", "E")), 0.01, C=B), modes=T)


def test_one_plan_with_and_without_modes_in_turn_is_a_fresh_plan_each_time_bit_for_bit():
    """The buffers a plan keeps between calls (allocated at first use, reallocated when K changes, rewritten by the next call): six
    calls on ONE LsqPlan - step and resolution, K = 0, 1, 2 in turn - each against the same call on a plan built for it.  The
    kernels use no device atomics, so the bar is equality of every tensor of the result; cov and res are [B, nmax + K, nmax + K]."""
    import torch
    model = synth.synth_models(3, 8, seed=1)
    B, _, L = model.shape
    per = synth.default_periods(6)
    truth = model.copy(); truth[:, 1, :] *= 1.03
    data = _datasets(per, _forward_all(truth, per), (("R", "c"),), 0.01, C=B)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    dm, lam = t(model), t(np.full(B, 3.0))
    h = model[0, 3]
    T = t(np.stack([linearized.interface_mode(h, [0, 1, 2], [3, 4]), linearized.thickness_mode(h, [0])]))
    with_K = lambda K: dict(modes=T[:K].contiguous(), mode_scale=t(np.full(K, 1e-3)), mode_y=t(np.full((B, K), 0.5))) if K else {}

    def flat(out):
        """Every tensor of a result, cloned, by name: pred, part and part_h entry by entry."""
        items = {}
        for k, v in out.items():
            if isinstance(v, (dict, list)):
                items.update({f"{k}[{i}]": x for i, x in (v.items() if isinstance(v, dict) else enumerate(v))})
            else:
                items[k] = v
        return {k: v.clone() for k, v in items.items() if v is not None}

    calls = [("step", 0), ("step", 1), ("resolution", 2), ("resolution", 0), ("step", 2), ("step", 0)]
    plan = linearized.LsqPlan(B, L, data)
    for which, K in calls:
        got = flat(getattr(plan, which)(dm, lam, alpha=0.5, **with_K(K)))
        want = flat(getattr(linearized.LsqPlan(B, L, data), which)(dm, lam, alpha=0.5, **with_K(K)))
        tag = f"{which}, K = {K}"
        assert set(got) == set(want) and ("delta_y" in got or "rdiag_y" in got) == (K > 0), tag
        assert not got["flag"].any(), tag
        if which == "resolution":
            assert tuple(got["cov"].shape) == (B, L + K, L + K) and tuple(got["res"].shape) == (B, L + K, L + K), tag
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (tag, k)
            assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (tag, k)


# ------------------------------------------------------------------------------------------------- 6., 7. the iteration
SETS_C = (("R", "c"), ("L", "c"))
ABOVE, BELOW = [0, 1, 2, 3], [4, 5, 6]
MODE_SCALE = 1e-4      # (0.1 km/s / 10 km)^2: the damping of a Vs step of 0.1 km/s carried to an interface step of 10 km


@pytest.fixture(scope="module")
def moho_problem():
    """The 16 stacks of _true_and_start; the start has, on top of its Vs perturbation, the interface between the layers 0..3 and
    4..6 moved by +-10 % of the upper group's thickness (sign per stack).  y_true: the amplitude that takes the start back."""
    true, start = _true_and_start()
    T = linearized.interface_mode(true[0, 3], ABOVE, BELOW)
    sign = np.where(np.arange(16) % 2 == 0, 1.0, -1.0)
    shift = 0.1 * true[:, 3, ABOVE].astype(np.float64).sum(axis=1) * sign
    start = start.copy()
    start[:, 3, :] = (true[:, 3, :].astype(np.float64) + T[None, :] * shift[:, None]).astype(np.float32)
    per = synth.default_periods(12)
    obs = _forward_all(true, per)
    return true, start, per, obs, T, -shift


def test_loop_invariants_with_modes(moho_problem):
    true, start, per, obs, T0, y_true = moho_problem
    data = _datasets(per, obs, SETS_C, 0.005)
    mask = np.ones((16, 24), bool); mask[5] = False
    T = np.stack([T0, linearized.interface_mode(true[0, 3], [0, 1], [2, 3])])    # two interfaces: the total depth stays
    ylo, yhi, h_min, lo, hi = -8.0, 8.0, 20.0, 2.6, 4.62
    inv = linearized.LinearizedBatch(start, data, alpha=ALPHA, lam0=LAM0, nu=NU, lam_min=LAM_MIN, vs_bounds=(lo, hi), mask=mask,
                                     modes=T, mode_scale=MODE_SCALE, mode_prior=[1e-3, 0.05], mode_bounds=(ylo, yhi), h_min=h_min)
    obj0 = inv.objective.cpu().numpy()
    out = {k: v.cpu().numpy() for k, v in inv.run(N_ITER, keep_models=True).items()}
    assert out["y"].shape == (N_ITER, 16, 2)
    obj = np.concatenate([obj0[None], out["objective"]])
    assert (np.diff(obj, axis=0) <= 0).all()                                # never increases
    lam = np.full(16, LAM0)
    models = np.concatenate([start[None], out["models"]])
    ys = np.concatenate([np.zeros((1, 16, 2)), out["y"]])
    touched = (T != 0).any(axis=0)
    depth0 = start[:, 3, :].astype(np.float64).sum(axis=1)
    for it in range(N_ITER):
        acc = out["accepted"][it]
        lam = np.where(acc, np.maximum(lam / NU, LAM_MIN), lam * NU)
        assert np.array_equal(lam, out["lam"][it])                          # the stated rule, exactly
        same = (models[it + 1] == models[it]).reshape(16, -1).all(axis=1) & (ys[it + 1] == ys[it]).all(axis=1)
        assert same[~acc].all()                                             # a rejected stack's model and y are bit-unchanged
        assert (obj[it + 1][acc] < obj[it][acc]).all() and np.array_equal(obj[it + 1][~acc], obj[it][~acc])
        # h: the float32 update of the iteration replayed on the host, mode by mode, exactly
        dy = ys[it + 1] - ys[it]
        upd = T[None, 0, :] * dy[:, 0, None]
        upd = upd + T[None, 1, :] * dy[:, 1, None]
        h = (models[it][:, 3, :].astype(np.float64) + upd).astype(np.float32)
        assert np.array_equal(models[it + 1][:, 3, :], h)
        # total depth: every accepted iteration rounds 7 layers below 64 km to float32, at most half an ulp (2^-19 km) each
        depth = models[it + 1][:, 3, :].astype(np.float64).sum(axis=1)
        assert (models[it + 1][:, 3, :] < 64).all()
        assert (np.abs(depth - depth0) <= (it + 1) * 7 * 2.0 ** -19 + 1e-12).all()
        assert (ys[it + 1] >= ylo).all() and (ys[it + 1] <= yhi).all()
        assert (models[it + 1][:, 3, touched].astype(np.float64) >= h_min).all()
        assert np.array_equal(models[it + 1][:, 3, ~touched], start[:, 3, ~touched])
        moved = models[it + 1][:, 1, :] != start[:, 1, :]
        vs = models[it + 1][:, 1, :]
        assert (vs[moved] >= np.float32(lo)).all() and (vs[moved] <= np.float32(hi)).all()
        for row in (0, 2, 4):                                               # Vp, rho, 1/Qs: the slopes are 0
            assert np.array_equal(models[it + 1][:, row], start[:, row])
    assert out["accepted"].any() and (ys[-1] != 0).any()                    # the loop did move models and interfaces
    assert (out["flag"][:, 5] == 1).all() and not out["accepted"][:, 5].any() and np.array_equal(out["model"][5], start[5])
    assert not ys[:, 5].any() and (out["flag"][:, np.arange(16) != 5] == 0).all()
    chi, rms = _chi_rms(_forward_all(out["model"], per), data, mask)
    assert np.allclose(rms, out["rms"][-1], rtol=1e-12, atol=0, equal_nan=True)
    prior = (np.array([1e-3, 0.05]) * ys[-1] ** 2).sum(axis=1)
    vsd = np.diff(out["model"][:, 1, :].astype(np.float64), axis=1)
    want = chi + ALPHA * (vsd ** 2).sum(axis=1) + prior
    ok = np.arange(16) != 5
    assert np.allclose(out["objective"][-1][ok], want[ok], rtol=1e-10)      # chi-square + alpha roughness + sum beta y^2
    print("y end:", np.round(ys[-1], 2).tolist())


def _cpu_route_modes(start, per, data, n_iter, T, mode_scale):
    """``lsq_cases.cpu_route`` with the mode T as one more unknown, its finite-difference step 1 % of the upper group's thickness.
    Returns (model, rms, y)."""
    return cpu_route(start, per, data, n_iter, T, mode_scale, ABOVE)


def test_recovery_of_a_displaced_interface(moho_problem):
    """Per stack rms_modes <= max(2 rms_cpu, 0.02) - the rule of test_recovery_against_the_cpu_route, for its reasons - and
    |y_end - y_true| < |y_true| for every stack that accepted a step: the interface moved the right way and less than twice
    as far (a sign or a scale error in the mode column fails it).  The Vs-only inversion of the same start, which cannot move
    the interface, is printed beside it; no bar is set on the ratio."""
    true, start, per, obs, T, y_true = moho_problem
    data = _datasets(per, obs, SETS_C, 0.005)
    kw = dict(alpha=ALPHA, lam0=LAM0, nu=NU, lam_min=LAM_MIN)
    inv = linearized.LinearizedBatch(start, data, modes=T[None], mode_scale=MODE_SCALE, **kw)
    rms0 = inv.rms.cpu().numpy()
    out = inv.run(N_ITER)
    rms_modes, y_end = out["rms"][-1].cpu().numpy(), out["y"][-1, :, 0].cpu().numpy()
    accepted = out["accepted"].cpu().numpy().any(axis=0)
    rms_vs = linearized.LinearizedBatch(start, data, **kw).run(N_ITER)["rms"][-1].cpu().numpy()
    _, rms_cpu, y_cpu = _cpu_route_modes(start, per, data, N_ITER, T, MODE_SCALE)
    print("stack  rms_start  rms_modes  rms_cpu  rms_vs_only   y_true    y_end    y_cpu")
    for b in range(16):
        print(f"{b:5d}  {rms0[b]:9.3f}  {rms_modes[b]:9.4f}  {rms_cpu[b]:7.4f}  {rms_vs[b]:11.4f}  {y_true[b]:7.2f}  {y_end[b]:7.2f}  {y_cpu[b]:7.2f}")
    print(f"median rms_vs_only / rms_modes {np.median(rms_vs / rms_modes):.2f}")
    assert (rms_modes <= np.maximum(2 * rms_cpu, 0.02)).all(), (rms_modes, rms_cpu)
    assert accepted.any()
    assert (np.abs(y_end - y_true)[accepted] < np.abs(y_true)[accepted]).all(), (y_end, y_true)
