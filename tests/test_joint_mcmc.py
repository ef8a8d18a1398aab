"""The joint sampler on the device: Rayleigh / Love, phase / group data through the joint accept kernels
(csrc/surfdisp_mcmc.hip, surfdisp_mcmc_accept_joint_device / _tree_joint_device) against the torch misfit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from settings import CONT                            # noqa: E402
from pysurfinv_amd import _lib
from pysurfinv_amd.forward import BatchPlan
from pysurfinv_amd.layers_batch import Model1DBatch
from pysurfinv_amd.mcmc import MetropolisBatch
from pysurfinv_amd.obsdata import DispersionData

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_driver.npz"))
T_R = G["trace/periods"]
T_U = np.array([5.0, 6.0, 8.0, 10.0, 12.0, 16.0, 20.0, 30.0])
T_L = np.array([10.0, 15.0, 20.0, 30.0, 40.0])
T_LU = np.array([8.0, 10.0, 20.0, 25.0])
DEV = torch.device("cuda:0")


def device_sets(mb, C=None, seed=0):
    """The four curves of a slightly faster start model, solved on the device, 1 % noise; per-chain rows (scaled by chain,
    a few masked entries) when C is given."""
    v = torch.as_tensor(mb.spec.v0, device=DEV)[None, :] * 1.01
    model, nlay = mb.to_model(v)
    rng = np.random.default_rng(seed)
    out = []
    for k, (w, q, T, kind, unc) in enumerate((("R", "c", T_R, 2, 0.02), ("R", "U", T_U, 2, 0.04),
                                              ("L", "c", T_L, 1, 0.03), ("L", "U", T_LU, 1, 0.05))):
        plan = BatchPlan(1, model.shape[2], len(T), device=DEV)
        c, u, st = plan.run(model.contiguous(), torch.as_tensor(np.asarray(T, np.float32), device=DEV), kind=kind, nlay=nlay)
        val = (c if q == "c" else u)[0].double().cpu().numpy() * (1 + 0.01 * rng.standard_normal(len(T)))
        assert int(st[0]) == 0 and (val > 0.5).all()
        un = np.full(len(T), unc)
        if C is not None:
            val = np.tile(val, (C, 1)) * (1 + 0.01 * rng.standard_normal((C, 1)))
            val[:: 7 + k, k % len(T)] = np.nan
            un = np.tile(un, (C, 1))
        out.append(DispersionData(w, q, T, val, un, weight=1.0 + 0.25 * k))
    return out


@pytest.mark.parametrize("case", ["plain", "spec3", "groups2"])
def test_one_rayleigh_phase_set_changes_nothing(case):
    """data=[DispersionData("R", "c", ...)] gives the existing sampler's mcTrack bit for bit (per-chain rows with masked
    entries): one solve with the same period list and flags, the same column order in the accept kernel."""
    mb = Model1DBatch(CONT, device=DEV)
    C = 600 if case == "groups2" else 256
    rng = np.random.default_rng(5)
    c_obs = np.tile(G["trace/c_obs"], (C, 1)) * (1 + 0.01 * rng.standard_normal((C, 1)))
    c_obs[::5, 2] = np.nan
    unc = np.tile(G["trace/uncer"], (C, 1))
    unc[::11, 6] = 0.0
    kw = dict(spec_depth=1, groups=2) if case == "groups2" else dict(spec_depth=3 if case == "spec3" else 1)
    first = (torch.arange(C, device=DEV) % 50) == 0
    old = MetropolisBatch(mb.spec, mb.to_model, T_R, c_obs, unc, device=DEV, seed=21)
    new = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=21, data=[DispersionData("R", "c", T_R, c_obs, unc)])
    if case == "groups2":
        assert new.chain_groups(C, 2) is not None
    t_old = old.run(C, 12, init_first=False, _init_mask=first, **kw).cpu().numpy()
    t_new = new.run(C, 12, init_first=False, _init_mask=first, **kw).cpu().numpy()
    assert np.array_equal(t_old, t_new)
    assert new.n_forward == old.n_forward and 0.05 < t_new[:, 1:, 2].mean() < 0.95


def _sampler(mb, C, seed=4, **kw):
    return MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=seed, data=device_sets(mb, C), **kw)


def _check_rows(mc, rows, states, chi_states, depth):
    """rows [C, S, 3+N] of S consecutive steps from the states [C, N] with chi-squares chi_states: each step's proposal is
    its tree node's, misfit / L are the torch misfit's of the whole tree of proposals (the same C * (2^d - 1) stacks in one
    solve as the lock step's, so the same team size and the same bits), a better chi-square is always accepted, the state
    moves exactly where accepted."""
    C, N = states.shape
    Q = mc._fz["q"] if depth > 1 else mc._fz["p1"][:, None]
    M = Q.shape[1]
    out = mc.misfit(Q.reshape(C * M, N), rows=torch.arange(C, device=DEV).repeat_interleave(M))
    misQ, chiQ, LQ = (t.view(C, M) for t in out)
    ar = torch.arange(C, device=DEV)
    node = torch.zeros(C, dtype=torch.int64, device=DEV)
    p, chi0 = states.clone(), chi_states.clone()
    for s in range(rows.shape[1]):
        prop = rows[:, s, 3:]
        assert torch.equal(prop, Q[ar, node]), s
        mis, chi, L = misQ[ar, node], chiQ[ar, node], LQ[ar, node]
        assert float((rows[:, s, 0] - mis).abs().max()) < 1e-9 and float((rows[:, s, 1] - L).abs().max()) < 1e-12, s
        acc = rows[:, s, 2] > 0.5
        assert bool(acc[chi < chi0].all()), s
        p = torch.where(acc[:, None], prop, p)
        chi0 = torch.where(acc, chi, chi0)
        node = torch.where(acc, 2 * node + 1, 2 * node + 2)
    return p, chi0


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_joint_accept_against_torch(depth):
    """All four data sets on different period lists, masked entries, per-chain rows: the rows of fused_step (depth 1) and
    fused_tree_step (depth 2-4) against MetropolisBatch.misfit of the recorded proposals."""
    mb = Model1DBatch(CONT, device=DEV)
    C, N = 256, mb.spec.n
    mc = _sampler(mb, C)
    jd = mc.joint
    assert jd.solve_periods["R"].tolist() == sorted(set(T_R) | set(T_U)) and jd.solve_periods["L"].tolist() == sorted(set(T_L) | set(T_LU))
    assert mc.fused_available() and bool((~mc.mask).any())
    p = mc.reset(C).contiguous()
    start = p.clone()
    row0 = torch.zeros((C, 3 + N), dtype=torch.float64, device=DEV)
    mc.fused_step(p, row=row0, row_stride=3 + N, first=True)
    mis, chi, L = mc.misfit(start)
    assert float((row0[:, 0] - mis).abs().max()) < 1e-9 and float((row0[:, 1] - L).abs().max()) < 1e-12
    assert bool((row0[:, 2] == 1).all()) and torch.equal(p, start)
    assert float((mc._fz["chi"] - chi).abs().max()) < 1e-9
    for it in range(2):
        before, chi_before = p.clone(), mc._fz["chi"].clone()
        rows = torch.zeros((C, depth, 3 + N), dtype=torch.float64, device=DEV)
        if depth == 1:
            mc.fused_step(p, row=rows, row_stride=depth * (3 + N))
        else:
            mc.fused_tree_step(p, depth, depth, row=rows, row_stride=depth * (3 + N), step_stride=3 + N)
        pe, chie = _check_rows(mc, rows, before, chi_before, depth)
        assert torch.equal(p, pe) and float((mc._fz["chi"] - chie).abs().max()) < 1e-9
    assert 0.02 < float(rows[:, :, 2].mean()) < 0.98


def _np_joint(pred, status, nper, cols, w, obs, unc, mask):
    """§2 of the joint misfit in numpy: pred[4] [C, P_s] (None where absent), status[2], per-chain obs [C, Ptot]."""
    C = obs.shape[0]
    out = np.zeros((C, 3))
    for c in range(C):
        failed = False
        for wv in range(2):
            if pred[2 * wv] is None:
                continue
            failed |= status[wv][c] != 0
            failed |= bool((pred[2 * wv][c, :nper[wv]].astype(np.float64) < 0.01).any())
        chi, n = 0.0, 0
        for j in range(cols.shape[0]):
            s, i = cols[j]
            v = float(pred[s][c, i])
            if s % 2 == 1 and not v >= 0.01:
                failed = True
            if mask[c, j]:
                r = (obs[c, j] - v) / unc[c, j]
                chi += w[j] * r * r
                n += 1
        mis = np.sqrt(chi / n)
        chi = chi if chi < 50 else np.sqrt(50 * chi)
        out[c] = (88888.0, 88888.0, 0.0) if failed else (mis, chi, np.exp(-0.5 * chi))
    return out


def test_joint_accept_entry_on_hand_made_arrays():
    """surfdisp_mcmc_accept_joint_device on hand-made predictions with injected failures (a status per wave type, c < 0.01
    at a period no column reads, a NaN U a column reads, a NaN U no column reads): rows equal the numpy statement."""
    C, N, PR, PL = 97, 3, 6, 4
    rng = np.random.default_rng(1)
    cR = (3.0 + rng.random((C, PR))).astype(np.float32)
    uR = (2.8 + rng.random((C, PR))).astype(np.float32)
    cL = (3.5 + rng.random((C, PL))).astype(np.float32)
    uL = (3.2 + rng.random((C, PL))).astype(np.float32)
    stR, stL = np.zeros(C, np.int32), np.zeros(C, np.int32)
    stR[3] = 1; stL[5] = 2
    cR[7, 5] = 0.005                                                   # c < 0.01 at a period no column reads
    cL[8, 0] = 0.0
    uR[9, 1] = np.nan                                                  # read by a U column
    uR[10, 4] = np.nan                                                 # read by no column: no failure
    uL[11, 2] = 0.001
    cols = np.array([[0, 0], [0, 2], [0, 3], [1, 1], [1, 2], [2, 1], [2, 3], [3, 2], [3, 0]], np.int32)
    w = np.array([1, 1, 1, 2, 2, 0.5, 0.5, 3, 3], np.float64)
    Pt = cols.shape[0]
    src = [cR, uR, cL, uL]
    truth = np.stack([src[s][:, i] for s, i in cols], axis=1).astype(np.float64)
    obs = truth * (1 + 0.02 * rng.standard_normal((C, Pt)))
    unc = np.full((C, Pt), 0.05)
    mask = rng.random((C, Pt)) > 0.15
    mask[:, 0] = True
    obs[~mask] = 0.0; unc[~mask] = 1.0
    ref = _np_joint(src, [stR, stL], [PR, PL], cols, w, obs, unc, mask)
    assert (ref[[3, 5, 7, 8, 9, 11], 0] == 88888).all() and ref[10, 0] < 88888
    d = lambda a: torch.as_tensor(a, device=DEV).contiguous()
    t = [d(a) for a in src]
    ts = [d(stR), d(stL)]
    dcols, dw, dobs, dunc, dmask = d(cols), d(w), d(obs), d(unc), d(mask.astype(np.uint8))
    p1 = torch.rand((C, N), dtype=torch.float64, device=DEV)
    p0 = torch.zeros_like(p1)
    chi0 = torch.zeros(C, dtype=torch.float64, device=DEV)
    row = torch.zeros((C, 3 + N), dtype=torch.float64, device=DEV)
    Lb = _lib.lib()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    predp = (ctypes.c_void_p * 4)(*[x.data_ptr() for x in t])
    strides = (ctypes.c_long * 4)(PR, PR, PL, PL)
    nper = (ctypes.c_int * 2)(PR, PL)
    stat = (ctypes.c_void_p * 2)(*[x.data_ptr() for x in ts])
    args = lambda first, chi: (None, C, N, predp, strides, nper, stat, Pt, ptr(dcols), ptr(dw), ptr(dobs), ptr(dunc), ptr(dmask), 1,
                               ptr(p1), ptr(p0), ptr(chi), ptr(row), 3 + N, 5, 1, first, 0)
    _lib.check(Lb.surfdisp_mcmc_accept_joint_device(*args(1, chi0)))
    torch.cuda.synchronize()
    r = row.cpu().numpy()
    assert np.allclose(r[:, 0], ref[:, 0], rtol=1e-12, atol=0) and np.allclose(r[:, 1], ref[:, 2], rtol=1e-12, atol=0)
    assert (r[:, 2] == 1).all() and torch.equal(row[:, 3:], p1) and torch.equal(p0, p1)
    assert np.allclose(chi0.cpu().numpy(), ref[:, 1], rtol=1e-12, atol=0)
    # not first: a state of higher chi-square is always left for the proposal; p0 follows the rows
    chi_s = torch.as_tensor(ref[:, 1] + np.where(np.arange(C) % 2 == 0, 1.0, -1.0), device=DEV)
    p0.zero_()
    _lib.check(Lb.surfdisp_mcmc_accept_joint_device(*args(0, chi_s)))
    torch.cuda.synchronize()
    acc = row[:, 2].cpu().numpy() > 0.5
    assert acc[::2].all() and np.allclose(row[:, 0].cpu().numpy(), ref[:, 0], rtol=1e-12, atol=0)
    assert torch.equal(p0[torch.as_tensor(acc, device=DEV)], p1[torch.as_tensor(acc, device=DEV)])
    assert not bool(p0[torch.as_tensor(~acc, device=DEV)].any())
    # argument errors: no phase array at all, a group array without its wave type's phase array, nper beyond the stride
    nop = (ctypes.c_void_p * 4)(None, t[1].data_ptr(), None, None)
    a = list(args(1, chi0)); a[3] = nop
    assert Lb.surfdisp_mcmc_accept_joint_device(*a) == _lib.ERR_INVALID
    bad = (ctypes.c_long * 4)(PR - 1, PR, PL, PL)
    a = list(args(1, chi0)); a[4] = bad
    assert Lb.surfdisp_mcmc_accept_joint_device(*a) == _lib.ERR_INVALID


def test_joint_predictions_are_the_solvers():
    """forward_joint = BatchPlan.run per wave type at the same B, period lists and kind flags (two solves in flight:
    SURFDISP_PIPELINED for both); phase-only where a wave type has no U data."""
    mb = Model1DBatch(CONT, device=DEV)
    C = 300
    sets = device_sets(mb)
    params = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=2, data=sets).reset(C).contiguous()
    model, nlay = mb.to_model(params)
    for chosen, pipelined in ((sets, True), (sets[:3], True), (sets[:2], False), (sets[2:3], False)):
        mc = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=2, data=chosen)
        out = {k: (v.clone() if v is not None else None) for k, v in mc.forward_joint(params).items()}
        for w, kind in (("R", _lib.KIND_RAYLEIGH), ("L", _lib.KIND_LOVE)):
            if w not in mc.joint.solve_periods:
                assert out["c" + w] is None
                continue
            hasU = any(d.wave == w and d.quantity == "U" for d in chosen)
            assert mc.joint.kind(w) == (kind if hasU else kind | _lib.PHASE_ONLY)
            plan = BatchPlan(C, model.shape[2], len(mc.joint.solve_periods[w]), device=DEV)
            c, u, st = plan.run(model.contiguous(), mc.joint.periods_t[w], kind=mc.joint.kind(w), nlay=nlay, pipelined=pipelined)
            assert torch.equal(out["c" + w], c) and torch.equal(out["status" + w], st), (len(chosen), w)
            if hasU:
                assert torch.equal(out["u" + w], u), (len(chosen), w)


def test_joint_chain_groups_do_not_change_the_chains():
    mb = Model1DBatch(CONT, device=DEV)
    C = 600
    sets = device_sets(mb, C, seed=3)
    tracks = []
    for groups in (1, 2, 3):
        mc = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=21, data=sets)
        first = (torch.arange(C, device=DEV) % 50) == 0
        tr = mc.run(C, 10, init_first=False, _init_mask=first, groups=groups, spec_depth=1)
        torch.cuda.synchronize()
        assert (mc.chain_groups(C, groups) is None) == (groups == 1) and mc.n_forward == C * 10
        tracks.append(tr.cpu().numpy())
    assert np.array_equal(tracks[0], tracks[1]) and np.array_equal(tracks[0], tracks[2])
    assert 0.02 < tracks[0][:, 1:, 2].mean() < 0.98 and (tracks[0][:, :, 0] < 88888).mean() > 0.5
    # replacing the data takes effect at the next run (the fused buffers are keyed on the data object)
    mc = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=21, data=sets)
    mc.run(C, 3, init_first=False, _init_mask=first, groups=2, spec_depth=1)
    mc.data = sets[:2]
    tr = mc.run(C, 4, init_first=False, _init_mask=first, groups=2, spec_depth=1)
    mis, _, _ = mc.misfit(tr[:, 3, 3:].contiguous())
    assert float((mis - tr[:, 3, 0]).abs().max()) < 1e-9


def test_point_mcinvmp_and_postpoint_with_joint_data(tmp_path):
    from pysurfinv_amd.point import Point, PostPoint
    mb = Model1DBatch(CONT, device=DEV)
    sets = device_sets(mb)
    data = {"RayPhase": (T_R, sets[0].values, sets[0].uncer), "RayGroup": (T_U, sets[1].values, sets[1].uncer),
            "LovePhase": (T_L, sets[2].values, sets[2].uncer), "LoveGroup": (T_LU, sets[3].values, sets[3].uncer)}
    p = Point(CONT, data=data, device="cuda:0")
    mis, chi, L = p.misfit()
    assert 0 < mis < 10
    arr = p.MCinvMP(outdir=str(tmp_path), pid="joint", runN=100 * 12, chainL=12, seed=3)
    assert arr.shape == (1200, 3 + mb.spec.n) and np.isfinite(arr).all()
    f = np.load(tmp_path / "joint.npz", allow_pickle=True)
    obs = f["obs"][()]
    assert np.array_equal(obs["T"], T_R) and len(obs["data"]) == 4
    assert [(d["wave"], d["quantity"]) for d in obs["data"]] == [("R", "c"), ("R", "U"), ("L", "c"), ("L", "U")]
    q = PostPoint(str(tmp_path / "joint.npz"), device="cuda:0")
    assert q.N == 1200 and np.array_equal(q.misfits, arr[:, 0])
    assert q.avgMod.misfit == p.misfit(q.avgMod.params)[0] and np.isfinite(q.avgMod.misfit)
    with pytest.raises(ValueError):
        p._sampler(seed=1).run_graphed(8, 4)
