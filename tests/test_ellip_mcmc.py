"""The Rayleigh ellipticity (H/V) as a fifth curve of the joint sampler on the device: the five-array accept entries
(csrc/surfdisp_mcmc.hip, surfdisp_mcmc_accept_joint5_device / _tree_joint5_device) against numpy, against the four-array
entries (unchanged bits) and against the torch misfit; the ratio of the Rayleigh solve in every route of the sampler."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from settings import CONT                            # noqa: E402
from test_joint_mcmc import DEV, T_R, _check_rows, device_sets
from pysurfinv_amd import _lib
from pysurfinv_amd.forward import BatchPlan, EventRing
from pysurfinv_amd.layers_batch import Model1DBatch
from pysurfinv_amd.mcmc import MetropolisBatch
from pysurfinv_amd.obsdata import DispersionData

pytestmark = pytest.mark.gpu

T_E = np.array([5.0, 8.0, 10.0, 14.0, 20.0, 25.0, 30.0])


def device_ellip_set(mb, T, C=None, absolute=False, seed=11, weight=1.5):
    """An ellipticity curve observed on ONE PRIOR DRAW solved on the device (chi barely moves under the uniform scaling
    device_sets observes c and U on), uncertainty 0.02; per-chain rows (scaled by chain, a few masked entries) with C."""
    draw = MetropolisBatch(mb.spec, mb.to_model, [10.0], [3.0], [0.1], device=DEV, seed=seed).reset(1).contiguous()
    model, nlay = mb.to_model(draw)
    plan = BatchPlan(1, model.shape[2], len(T), device=DEV)
    c, u, st, r = plan.run(model.contiguous(), torch.as_tensor(np.asarray(T, np.float32), device=DEV), nlay=nlay, want_ratio=True)
    val = r[0].double().cpu().numpy()
    assert int(st[0]) == 0 and bool((c[0] > 0.01).all()) and np.isfinite(val).all() and (np.abs(val) > 0.3).all()
    un = np.full(len(T), 0.02)
    if C is not None:
        rng = np.random.default_rng(seed)
        val = np.tile(val, (C, 1)) * (1 + 0.01 * rng.standard_normal((C, 1)))
        val[::9, 3 % len(T)] = np.nan
        un = np.tile(un, (C, 1))
    return DispersionData("R", "E", T, val, un, weight=weight, absolute=absolute)


def data_sets(mb, which, C=None):
    four = device_sets(mb, C)
    if which == "Rc_RE":
        return [four[0], device_ellip_set(mb, T_R, C)]                     # identical period arrays: the solve of {Rc}
    return four + [device_ellip_set(mb, T_E, C, absolute=True)]           # all five, |chi|, the union of three period lists


# ------------------------------------------------------------------------------------------------ the entries themselves
def _np_joint5(pred, status, nper, cols, w, obs, unc, mask):
    """The joint misfit in numpy with the ellipticity sources: pred[5] [C, P_s] (None where absent), sources 0..3 the arrays,
    4 chi, 5 |chi| of pred[4]; a column that names a missing array or a period beyond its solve fails the model."""
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
            a = pred[min(s, 4)]
            if a is None or i >= nper[0 if s >= 4 else s // 2]:
                failed = True
                continue
            v = float(a[c, i])
            if s >= 4:
                if not np.isfinite(v):
                    failed = True
                if s == 5:
                    v = abs(v)
            elif s % 2 == 1 and not v >= 0.01:
                failed = True
            if mask[c, j]:
                r = (obs[c, j] - v) / unc[c, j]
                chi += w[j] * r * r
                n += 1
        mis = np.sqrt(chi / n)
        chi = chi if chi < 50 else np.sqrt(50 * chi)
        out[c] = (88888.0, 88888.0, 0.0) if failed else (mis, chi, np.exp(-0.5 * chi))
    return out


class Entry:
    """One call of a joint accept entry (four- or five-array, plain or tree) on device tensors; state, chi-squares and rows
    are fresh copies per call, returned."""

    def __init__(self, pred, strides, nper, status, cols, w, obs, unc, mask, N, M=1):
        d = lambda a: None if a is None else (a if torch.is_tensor(a) else torch.as_tensor(a, device=DEV)).contiguous()
        self.pred = [d(a) for a in pred]
        self.strides, self.nper = list(strides), list(nper)
        self.status = [d(a) for a in status]
        self.cols, self.w, self.obs, self.unc = d(np.asarray(cols, np.int32)), d(np.asarray(w, np.float64)), d(obs), d(unc)
        self.mask = d(np.asarray(mask).astype(np.uint8))
        self.C, self.N, self.M = obs.shape[0], N, M
        self.q = torch.rand((self.C * M, N), dtype=torch.float64, device=DEV)

    def __call__(self, five, depth=1, first=0, chi0=None, counter=1, null_ratio=False):
        C, N = self.C, self.N
        n = 5 if five else 4
        pred = (self.pred + [None])[:n] if len(self.pred) == 4 else self.pred[:n]
        if five and null_ratio:
            pred = pred[:4] + [None]
        strides = (self.strides + [0])[:n]
        ptr = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None else 0)
        predp = (ctypes.c_void_p * n)(*[a.data_ptr() if a is not None else None for a in pred])
        sp = (ctypes.c_long * n)(*strides)
        nper = (ctypes.c_int * 2)(*self.nper)
        stat = (ctypes.c_void_p * 2)(*[a.data_ptr() if a is not None else None for a in self.status])
        p0 = torch.zeros((C, N), dtype=torch.float64, device=DEV)
        chi = torch.zeros(C, dtype=torch.float64, device=DEV) if chi0 is None else chi0.clone()
        row = torch.zeros((C, depth, 3 + N), dtype=torch.float64, device=DEV)
        table = (predp, sp, nper, stat, self.cols.shape[0], ptr(self.cols), ptr(self.w), ptr(self.obs), ptr(self.unc), ptr(self.mask), 1)
        Lb = _lib.lib()
        if depth == 1:
            f = Lb.surfdisp_mcmc_accept_joint5_device if five else Lb.surfdisp_mcmc_accept_joint_device
            rc = f(None, C, N, *table, ptr(self.q), ptr(p0), ptr(chi), ptr(row), 3 + N, 5, counter, first, 0)
        else:
            f = Lb.surfdisp_mcmc_accept_tree_joint5_device if five else Lb.surfdisp_mcmc_accept_tree_joint_device
            rc = f(None, C, N, depth, depth, *table, ptr(self.q), ptr(p0), ptr(chi), ptr(row), depth * (3 + N), 3 + N, 5, counter, 0)
        torch.cuda.synchronize()
        return rc, row, p0, chi


def _hand_made(rng, C, PR, PL):
    """The arrays of test_joint_accept_entry_on_hand_made_arrays (the four-source case)."""
    cR = (3.0 + rng.random((C, PR))).astype(np.float32)
    uR = (2.8 + rng.random((C, PR))).astype(np.float32)
    cL = (3.5 + rng.random((C, PL))).astype(np.float32)
    uL = (3.2 + rng.random((C, PL))).astype(np.float32)
    stR, stL = np.zeros(C, np.int32), np.zeros(C, np.int32)
    stR[3] = 1; stL[5] = 2
    cR[7, 5] = 0.005
    cL[8, 0] = 0.0
    uR[9, 1] = np.nan
    uR[10, 4] = np.nan
    uL[11, 2] = 0.001
    return [cR, uR, cL, uL], [stR, stL]


def _observe(rng, src, cols, C, per_chain_noise=0.02):
    truth = np.stack([(np.abs(src[4][:, i]) if s == 5 else src[min(s, 4)][:, i]) for s, i in cols], axis=1).astype(np.float64)
    truth = np.where(np.isfinite(truth), truth, 1.0)
    obs = truth * (1 + per_chain_noise * rng.standard_normal(truth.shape))
    unc = np.full(truth.shape, 0.05)
    mask = rng.random(truth.shape) > 0.15
    mask[:, 0] = True
    obs[~mask] = 0.0; unc[~mask] = 1.0
    return obs, unc, mask


def test_four_array_entries_keep_their_bits_on_hand_made_arrays():
    """Old entry and new entry with pred[4] = NULL: torch.equal rows, states and chi-squares, plain and tree (depth 3)."""
    C, N, PR, PL = 97, 3, 6, 4
    rng = np.random.default_rng(1)
    src, st = _hand_made(rng, C, PR, PL)
    cols = np.array([[0, 0], [0, 2], [0, 3], [1, 1], [1, 2], [2, 1], [2, 3], [3, 2], [3, 0]], np.int32)
    w = np.array([1, 1, 1, 2, 2, 0.5, 0.5, 3, 3], np.float64)
    obs, unc, mask = _observe(rng, src + [None], cols, C)
    for depth in (1, 3):
        M = (1 << depth) - 1
        big = [np.repeat(a, M, axis=0) * (1 + 0.01 * rng.standard_normal((C * M, 1))).astype(np.float32) for a in src]
        e = Entry(big, (PR, PR, PL, PL), (PR, PL), [np.repeat(s, M) for s in st], cols, w, obs, unc, mask, N, M)
        for first, chi0 in ((1, None), (0, torch.full((C,), 3.0, dtype=torch.float64, device=DEV))):
            if depth > 1 and first:
                continue
            old, new = e(False, depth, first, chi0), e(True, depth, first, chi0)
            assert old[0] == 0 and new[0] == 0
            for a, b in zip(old[1:], new[1:]):
                assert torch.equal(a, b), (depth, first)
            assert bool((old[1][:, :, 0] == 88888).any()) and bool((old[1][:, :, 0] < 88888).any())
            assert 0 < float(old[1][:, :, 2].mean()) <= 1


@pytest.mark.parametrize("depth", [1, 3])
def test_four_array_entries_keep_their_bits_on_a_real_solve(depth):
    """... and on the four curves of a real solve, per-chain observations with masked entries: the rows, states and chi0 the
    sampler's accept step would write, from the old entries and from the new ones without a ratio array."""
    mb = Model1DBatch(CONT, device=DEV)
    C, N = 256, mb.spec.n
    M = (1 << depth) - 1
    mc = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=4, data=device_sets(mb, C))
    jd = mc.joint
    q = mc.reset(C * M).contiguous()
    pred = {k: (v.clone() if v is not None else None) for k, v in mc.forward_joint(q).items()}
    assert pred["eR"] is None
    arrs = [pred["cR"], pred["uR"], pred["cL"], pred["uL"]]
    e = Entry(arrs, [a.stride(0) for a in arrs], [jd.solve_periods[w].size for w in ("R", "L")], [pred["statusR"], pred["statusL"]],
              jd.cols.cpu().numpy(), jd.col_w, mc.c_obs, mc.uncer, mc.mask.cpu().numpy(), N, M)
    e.q = q
    # states about as good as the proposals: the median chi-square of the first C stacks (prior draws are far from the data)
    chi0 = e(False, 1, 1)[3].median().expand(C).contiguous()
    for first in ((1, 0) if depth == 1 else (0,)):
        old, new = e(False, depth, first, chi0, counter=7), e(True, depth, first, chi0, counter=7)
        assert old[0] == 0 and new[0] == 0
        for a, b in zip(old[1:], new[1:]):
            assert torch.equal(a, b), (depth, first)
        assert float((old[1][:, :, 0] < 88888).double().mean()) > 0.5
    assert 0.02 < float(old[1][:, :, 2].mean()) < 0.98


def test_five_array_entry_on_hand_made_arrays():
    """surfdisp_mcmc_accept_joint5_device against the numpy statement: all six sources, masked entries, per-chain
    observations, weights, a NaN and an inf ratio in a read column (and a NaN in one nobody reads), negative ratios with and
    without `absolute`, then a source-4 column while pred[4] is NULL and a period index beyond nper[0]."""
    C, N, PR, PL = 97, 3, 6, 4
    rng = np.random.default_rng(1)
    src, st = _hand_made(rng, C, PR, PL)
    eR = (0.6 + rng.random((C, PR))).astype(np.float32)
    eR[:, 2] *= -1.0                                                   # a negative ellipticity at period 2: read signed AND absolute
    eR[::4, 4] *= -1.0
    eR[12, 0] = np.nan                                                 # read by a source-4 column
    eR[13, 4] = np.inf                                                 # read by a source-5 column
    eR[14, 2] = -np.inf
    eR[15, 5] = np.nan                                                 # read by no column: no failure
    eR[16, 0] = 0.0                                                    # chi = 0 and a large negative chi: predictions, not failures
    eR[17, 4] = -30.0
    src = src + [eR]
    cols = np.array([[0, 0], [0, 2], [4, 0], [1, 1], [5, 4], [2, 1], [4, 2], [3, 2], [5, 2], [3, 0], [2, 3], [1, 2]], np.int32)
    w = np.array([1, 1, 1.5, 2, 0.75, 0.5, 1.5, 3, 0.75, 3, 0.5, 2], np.float64)
    obs, unc, mask = _observe(rng, src, cols, C)
    mask[12:18] = True; mask[:, 8] = True                              # (the injected rows: every column counts; column 8, |chi| at
    unc[mask] = 0.05                                                   # period 2 where chi < 0, counts for every chain)
    obs = np.where(mask & (obs == 0.0), 1.0, obs)
    nper = (PR, PL)
    ref = _np_joint5(src, st, nper, cols, w, obs, unc, mask)
    assert (ref[[3, 5, 7, 8, 9, 11, 12, 13, 14], 0] == 88888).all() and (ref[[10, 15, 16, 17], 0] < 88888).all()
    e = Entry(src, (PR, PR, PL, PL, PR), nper, st, cols, w, obs, unc, mask, N)
    rc, row, p0, chi = e(True, first=1)
    assert rc == 0
    r = row[:, 0].cpu().numpy()
    assert np.allclose(r[:, 0], ref[:, 0], rtol=1e-12, atol=0) and np.allclose(r[:, 1], ref[:, 2], rtol=1e-12, atol=0)
    assert (r[:, 2] == 1).all() and torch.equal(row[:, 0, 3:], e.q) and torch.equal(p0, e.q)
    assert np.allclose(chi.cpu().numpy(), ref[:, 1], rtol=1e-12, atol=0)
    # not first: a state of higher chi-square is always left for the proposal; p0 follows the rows
    chi_s = torch.as_tensor(ref[:, 1] + np.where(np.arange(C) % 2 == 0, 1.0, -1.0), device=DEV)
    rc, row, p0, chi = e(True, first=0, chi0=chi_s)
    acc = row[:, 0, 2] > 0.5
    assert rc == 0 and bool(acc[::2].all()) and np.allclose(row[:, 0, 0].cpu().numpy(), ref[:, 0], rtol=1e-12, atol=0)
    assert torch.equal(p0[acc], e.q[acc]) and not bool(p0[~acc].any())
    assert np.allclose(chi.cpu().numpy(), np.where(acc.cpu().numpy(), ref[:, 1], chi_s.cpu().numpy()), rtol=1e-12, atol=0)
    # the sign matters: the same table with the absolute columns read signed gives another chi-square where chi < 0
    cols_s = cols.copy(); cols_s[cols_s[:, 0] == 5, 0] = 4
    ref_s = _np_joint5(src, st, nper, cols_s, w, obs, unc, mask)
    e_s = Entry(src, (PR, PR, PL, PL, PR), nper, st, cols_s, w, obs, unc, mask, N)
    r_s = e_s(True, first=1)[1][:, 0].cpu().numpy()
    assert np.allclose(r_s[:, 0], ref_s[:, 0], rtol=1e-12, atol=0)
    ok = (ref[:, 0] < 88888) & (ref_s[:, 0] < 88888)
    assert (ref_s[ok, 0] > ref[ok, 0]).all()                           # (every chain has chi < 0 at period 2)
    # a source-4 column without the array, and the four-array entry given such a table: every model fails, nothing is read
    for five, null in ((True, True), (False, False)):
        rc, row, p0, chi = e(five, first=1, null_ratio=null)
        assert rc == 0 and bool((row[:, 0, 0] == 88888).all()) and bool((row[:, 0, 1] == 0).all()) and bool((chi == 88888).all())
    # a period index beyond nper[0] in an ellipticity column (within the Love solve's count or not): fails the model
    for bad in (PR, PR + 1000, -1):
        cols_b = cols.copy(); cols_b[2, 1] = bad
        e_b = Entry(src, (PR, PR, PL, PL, PR), nper, st, cols_b, w, obs, unc, mask, N)
        rc, row, p0, chi = e_b(True, first=1)
        assert rc == 0 and bool((row[:, 0, 0] == 88888).all())
    # argument errors: a ratio array without the Rayleigh phase array, a ratio stride below nper[0]
    e_l = Entry([None, None, src[2], src[3], eR], (0, 0, PL, PL, PR), (0, PL), [None, st[1]], cols[[5, 7]], w[[5, 7]],
                obs[:, [5, 7]], unc[:, [5, 7]], mask[:, [5, 7]], N)
    assert e_l(True, first=1)[0] == _lib.ERR_INVALID
    e_l.pred[4] = None
    assert e_l(True, first=1)[0] == 0
    e_s = Entry(src, (PR, PR, PL, PL, PR - 1), nper, st, cols, w, obs, unc, mask, N)
    assert e_s(True, first=1)[0] == _lib.ERR_INVALID


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("per_chain", [False, True])
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("which", ["Rc_RE", "five"])
def test_ellip_accept_against_torch(which, depth, per_chain):
    """{Rc, RE} and {Rc, RU, Lc, LU, |RE|}: the rows of fused_step (depth 1) and fused_tree_step (depth 3) against
    MetropolisBatch.misfit of the recorded proposals, shared and per-chain observations."""
    mb = Model1DBatch(CONT, device=DEV)
    C, N = 256, mb.spec.n
    mc = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=4, data=data_sets(mb, which, C if per_chain else None))
    jd = mc.joint
    assert jd.with_ratio and mc.fused_available() and (mc.c_obs.ndim == 2) == per_chain
    if which == "Rc_RE":
        assert np.array_equal(jd.solve_periods["R"], np.asarray(T_R, np.float32)) and jd.kind("R") & _lib.PHASE_ONLY
    p = mc.reset(C).contiguous()
    start = p.clone()
    row0 = torch.zeros((C, 3 + N), dtype=torch.float64, device=DEV)
    mc.fused_step(p, row=row0, row_stride=3 + N, first=True)
    mis, chi, L = mc.misfit(start)
    assert float((mis < 88888).double().mean()) > 0.9
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


@pytest.mark.parametrize("which", ["Rc_RE", "five"])
def test_ellip_chain_groups_do_not_change_the_chains(which):
    mb = Model1DBatch(CONT, device=DEV)
    C = 600
    sets = data_sets(mb, which, C)
    tracks = []
    for groups in (1, 2):
        mc = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=21, data=sets)
        first = (torch.arange(C, device=DEV) % 50) == 0
        tr = mc.run(C, 10, init_first=False, _init_mask=first, groups=groups, spec_depth=1)
        torch.cuda.synchronize()
        assert (mc.chain_groups(C, groups) is None) == (groups == 1) and mc.n_forward == C * 10
        tracks.append(tr)
    assert torch.equal(tracks[0], tracks[1])
    assert 0.02 < float(tracks[0][:, 1:, 2].mean()) < 0.98 and float((tracks[0][:, :, 0] < 88888).double().mean()) > 0.5
    mis, _, L = mc.misfit(tr[:, 9, 3:].contiguous())
    assert float((mis - tr[:, 9, 0]).abs().max()) < 1e-9 and float((L - tr[:, 9, 1]).abs().max()) < 1e-12


def test_small_batch_route_returns_the_ratio():
    """independent="auto" (fewer than AUTO_INDEP_CHAINS chains: SURFDISP_INDEPENDENT): the ratio comes out of that mode too, and
    the sampler's rows are the torch misfit's."""
    mb = Model1DBatch(CONT, device=DEV)
    C, N = 100, mb.spec.n
    assert C < MetropolisBatch.AUTO_INDEP_CHAINS
    mc = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=8, data=data_sets(mb, "Rc_RE", C), independent="auto")
    assert mc.auto_spec_depth(C) == 1
    params = mc.reset(C).contiguous()
    model, nlay = mb.to_model(params)
    out = {k: (v.clone() if v is not None else None) for k, v in mc.forward_joint(params).items()}
    plan = BatchPlan(C, model.shape[2], len(T_R), device=DEV)
    c, u, st, r = plan.run(model.contiguous(), mc.joint.periods_t["R"], kind=mc.joint.kind("R"), nlay=nlay, independent=True,
                           want_ratio=True)
    assert torch.equal(out["eR"], r) and torch.equal(out["cR"], c)
    assert float((r != 0).double().mean()) > 0.9 and float(torch.isfinite(r).double().mean()) > 0.99
    tr = mc.run(C, 6)
    for k in range(6):
        mis, _, L = mc.misfit(tr[:, k, 3:].contiguous())
        assert float((mis - tr[:, k, 0]).abs().max()) < 1e-9 and float((L - tr[:, k, 1]).abs().max()) < 1e-12, k
    assert float((tr[:, :, 0] < 88888).double().mean()) > 0.5 and 0.02 < float(tr[:, 1:, 2].mean()) < 0.98


@pytest.mark.parametrize("independent", [False, True])
def test_forward_joint_ratio_is_the_solvers(independent):
    """pred["eR"] of forward_joint = BatchPlan.run(want_ratio=True) on the same stacks and periods, with and without
    SURFDISP_INDEPENDENT; against the CPU oracle's ratio on the CONT start model at test_ellipticity_output_abi3's bar for
    smooth stacks (1e-4 relative + 3e-5)."""
    from oracle import cport
    mb = Model1DBatch(CONT, device=DEV)
    C = 300
    for which, pipelined in (("Rc_RE", False), ("five", True)):
        mc = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=2, data=data_sets(mb, which), independent=independent)
        params = torch.cat([torch.as_tensor(mb.spec.v0, device=DEV)[None, :], mc.reset(C - 1)]).contiguous()
        model, nlay = mb.to_model(params)
        out = {k: (v.clone() if v is not None else None) for k, v in mc.forward_joint(params).items()}
        per = mc.joint.periods_t["R"]
        plan = BatchPlan(C, model.shape[2], per.numel(), device=DEV)
        c, u, st, r = plan.run(model.contiguous(), per, kind=mc.joint.kind("R"), nlay=nlay, pipelined=pipelined,
                               independent=independent, want_ratio=True)
        assert torch.equal(out["eR"], r) and torch.equal(out["cR"], c) and torch.equal(out["statusR"], st), which
        assert int(st[0]) == 0 and float((st == 0).double().mean()) > 0.9 and float(torch.isfinite(r).double().mean()) > 0.99
        # the start model against the CPU oracle
        O = cport.lib()
        fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        m = np.ascontiguousarray(model[0].cpu().numpy())
        n = m.shape[1] if nlay is None else int(nlay[0])
        m = np.ascontiguousarray(m[:, :n])
        p32 = np.ascontiguousarray(per.cpu().numpy())
        P = p32.size
        co, uo, ro = (np.zeros(P, np.float32) for _ in range(3))
        O.surfdisp_oracle_forward_dbg(n, 2, fp(m[0]), fp(m[1]), fp(m[2]), fp(m[3]), fp(m[4]), fp(p32), P, fp(co), fp(uo), fp(ro))
        assert (co > 0.01).all()
        got = r[0].cpu().numpy()
        assert (np.abs(got - ro) <= 1e-4 * np.abs(ro) + 3e-5).all(), (which, float(np.abs(got - ro).max()))


def test_event_ring_with_an_ellipticity_set():
    """A sampler with an event_ring and an "E" set runs, and the ring's slots bracket its Rayleigh solves (the events variant
    of the ratio entry gives the plain one's bits)."""
    mb = Model1DBatch(CONT, device=DEV)
    C, N = 256, mb.spec.n
    sets = data_sets(mb, "Rc_RE", C)
    ref = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=6, data=sets)
    mc = MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=6, data=sets)
    ring = EventRing(8)
    mc.event_ring = ring
    p = mc.reset(C).contiguous()
    pr = p.clone()
    rows, rows_ref = (torch.zeros((C, 3 + N), dtype=torch.float64, device=DEV) for _ in range(2))
    for k in range(3):
        mc.fused_step(p, row=rows, row_stride=3 + N, first=(k == 0))
        ref.fused_step(pr, row=rows_ref, row_stride=3 + N, first=(k == 0))
    torch.cuda.synchronize()
    assert mc._ev_i == 3 and torch.equal(rows, rows_ref) and torch.equal(p, pr)
    ms = ring.kernel_ms(used=3)
    assert ms.shape == (3, 3) and np.isfinite(ms).all() and (ms[:, 1] > 0).all() and (ms >= 0).all()
    # BatchPlan.run itself: want_ratio with events
    model, nlay = mb.to_model(p)
    plan = BatchPlan(C, model.shape[2], len(T_R), device=DEV)
    a = [t.clone() for t in plan.run(model.contiguous(), mc.joint.periods_t["R"], nlay=nlay, want_ratio=True)]
    b = plan.run(model.contiguous(), mc.joint.periods_t["R"], nlay=nlay, want_ratio=True, events=ring.slot(3))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and ring.kernel_ms(used=4)[3, 1] > 0


def test_point_mcinvmp_and_postpoint_with_hv_data(tmp_path):
    from pysurfinv_amd.point import Point, PostPoint
    mb = Model1DBatch(CONT, device=DEV)
    rc, hv = device_sets(mb)[0], device_ellip_set(mb, T_E, absolute=True)
    data = {"RayPhase": (T_R, rc.values, rc.uncer), "RayHV": (T_E, hv.values, hv.uncer)}
    p = Point(CONT, data=data, device="cuda:0")
    mis, chi, L = p.misfit()
    assert 0 < mis < 88888
    arr = p.MCinvMP(outdir=str(tmp_path), pid="hv", runN=100 * 12, chainL=12, seed=3)
    assert arr.shape == (1200, 3 + mb.spec.n) and np.isfinite(arr).all() and (arr[:, 0] < 88888).mean() > 0.5
    f = np.load(tmp_path / "hv.npz", allow_pickle=True)
    obs = f["obs"][()]
    assert np.array_equal(obs["T"], T_R) and len(obs["data"]) == 2
    assert [(d["wave"], d["quantity"], d["absolute"]) for d in obs["data"]] == [("R", "c", False), ("R", "E", True)]
    q = PostPoint(str(tmp_path / "hv.npz"), device="cuda:0")
    assert [(d.wave, d.quantity, d.absolute) for d in q.data] == [("R", "c", False), ("R", "E", True)]
    assert np.array_equal(q.data[1].values, hv.values) and q.N == 1200 and np.array_equal(q.misfits, arr[:, 0])
    assert q.avgMod.misfit == p.misfit(q.avgMod.params)[0] and np.isfinite(q.avgMod.misfit)
    with pytest.raises(ValueError):
        p._sampler(seed=1).run_graphed(8, 4)
