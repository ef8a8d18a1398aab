"""Posterior predictive curves on the device (csrc/surfdisp_pred.hip, header section (6g)): surfdisp_posterior_sources_device and
surfdisp_posterior_predictive_device each alone against numpy, and pysurfinv_amd.posterior.posterior_predictive end to end
against the statement posterior.predictive_reference run with the same device sampler.

Bars.  Integers (selection, weights, counts, failed weights, histograms) exactly - the histograms while no counted value lies
within 1e-9 of a bin edge, which every test asserts.  Mean / std / min / max: 1e-9, the bar tests/test_posterior_gpu.py uses for
fp64 statistics of values of this size; with at most about 5 000 rows of values below 10 the rounding of the fp64 sums is orders
below it.  End to end the device route solves every DISTINCT final model once and the statement solves every final row, so the
two batches differ: the sampler is built with independent=False and the root search's team is fixed for the duration
(surfdisp_set_team(4)), under which a stack's result does not depend on its place in the batch -
test_a_stack_solves_the_same_alone_and_in_a_batch asserts that bit for bit - and the 1e-9 bar holds end to end too.  `fit`
divides by the uncertainty: its bar is 1e-9 over the smallest uncertainty.  The measured maxima of an MI355X run are in
profiles/predictive/parity.txt."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "golden")]
from settings import CONT                            # noqa: E402
from settings_therm import HYBRID_STATIC, PERIODS as PERIODS_THERM   # noqa: E402
from posterior_cases import (DEV, P_A, SLAB_BOUNDARY_SELECTIONS, _carry_track, _close, _empty_list_inputs, _random_track, _same,   # noqa: E402
                             _slab_boundary_track, _stats_inputs)
from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402
from pysurfinv_amd.mcmc import MetropolisBatch       # noqa: E402
from pysurfinv_amd import posterior, _lib            # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(HERE, "golden", "ref_driver.npz"))
GT = np.load(os.path.join(HERE, "golden", "ref_therm.npz"))
TEAM = 4


def test_header_constants():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "surfdisp.h")).read()
    assert f"#define SURFDISP_PRED_SLAB_ROWS {posterior.PRED_SLAB_ROWS}\n" in hdr
    assert f"#define SURFDISP_PRED_SLABS_MAX {posterior.PRED_SLABS_MAX}\n" in hdr
    assert f"#define SURFDISP_PRED_COLS_MAX {posterior.PRED_COLS_MAX}\n" in hdr


# ------------------------------------------------------------------ (a) the statistics entry alone
# P_A columns, lists of 0, 5 and a slab + 300 rows: posterior_cases._stats_inputs
def _stats_numpy(pred, failed, w, offsets, hist):
    """numpy on the list with row i repeated w[i] times."""
    npnt, P = offsets.size - 1, pred.shape[1]
    vlo, vhi, nb = hist
    o = dict(count=np.zeros((npnt, P), np.int32), n_failed=np.zeros(npnt, np.int32), hist=np.zeros((npnt, P, nb), np.int32),
             below=np.zeros((npnt, P), np.int32), above=np.zeros((npnt, P), np.int32))
    for k in ("pred_mean", "pred_std", "pred_min", "pred_max"):
        o[k] = np.full((npnt, P), np.nan)
    margin = np.inf
    for p in range(npnt):
        rep = np.repeat(np.arange(offsets[p], offsets[p + 1]), w[offsets[p]:offsets[p + 1]])
        o["n_failed"][p] = (failed[rep] != 0).sum()
        rep = rep[failed[rep] == 0]
        for c in range(P):
            v = pred[rep, c].astype(np.float64)
            v = v[np.isfinite(v)]
            o["count"][p, c] = v.size
            if not v.size:
                continue
            o["pred_mean"][p, c], o["pred_std"][p, c], o["pred_min"][p, c], o["pred_max"][p, c] = v.mean(), v.std(), v.min(), v.max()
            edges = np.arange(nb + 1) * ((vhi[c] - vlo[c]) / nb) + vlo[c]
            margin = min(margin, np.abs(v[:, None] - edges[None, :]).min(), np.abs(v - vhi[c]).min())
            o["below"][p, c], o["above"][p, c] = (v < vlo[c]).sum(), (v >= vhi[c]).sum()
            v = v[(v >= vlo[c]) & (v < vhi[c])]
            o["hist"][p, c] = np.histogram(v, edges)[0] if v.size else 0
    return o, margin


def test_statistics_entry_against_numpy_on_the_repeated_rows():
    pred, failed, w, offsets, hist = _stats_inputs()
    want, margin = _stats_numpy(pred, failed, w, offsets, hist)
    assert margin > 1e-9                                                 # exact histograms are a fair demand
    assert want["count"][0].sum() == 0 and (want["count"][:, P_A - 1] == 0).all() and want["count"][2, :P_A - 1].min() > 5000
    assert want["n_failed"][1] == 1 and want["count"][1, 6] == 5 and want["count"][1, 0] == 10
    dev = lambda a: torch.from_numpy(a).to(DEV)
    args = (dev(failed), dev(w), dev(offsets))
    a = posterior.predictive_statistics(dev(pred), *args, hist=hist)
    b = posterior.predictive_statistics(dev(pred), *args, hist=hist)
    wide = torch.full((pred.shape[0], P_A + 3), 9.0, dtype=torch.float32, device=DEV)
    wide[:, :P_A] = dev(pred)
    c = posterior.predictive_statistics(wide[:, :P_A], *args, hist=hist)           # rows ld = P + 3 floats apart
    none = posterior.predictive_statistics(dev(pred), None, dev(w), dev(offsets))  # no failed array, no histogram
    torch.cuda.synchronize()
    assert set(a) == set(want) and "hist" not in none
    for k in ("count", "n_failed", "hist", "below", "above"):
        assert np.array_equal(a[k].cpu().numpy(), want[k]), k
    for k in ("pred_mean", "pred_std", "pred_min", "pred_max"):
        _close(f"statistics entry {k}", a[k], torch.from_numpy(want[k]), 1e-9)
    assert bool(torch.isnan(a["pred_mean"][0]).all()) and bool(torch.isnan(a["pred_std"][:, P_A - 1]).all())
    for k in a:                                                          # two calls, and another row pitch: the same bits
        assert _same(a[k], b[k]) and _same(a[k], c[k]), k
    w_all = _stats_numpy(pred, np.zeros_like(failed), w, offsets, hist)[0]
    assert np.array_equal(none["count"].cpu().numpy(), w_all["count"]) and int(none["n_failed"].sum()) == 0
    _close("statistics entry, no failed array, pred_mean", none["pred_mean"], torch.from_numpy(w_all["pred_mean"]), 1e-9)


def test_statistics_entry_with_an_empty_list():
    pred, failed, w, offsets, hist = _empty_list_inputs()
    r = posterior.predictive_statistics(pred, failed, w, offsets, hist=hist)
    torch.cuda.synchronize()
    assert int(r["count"].sum()) == 0 and int(r["hist"].sum()) == 0 and bool(torch.isnan(r["pred_mean"]).all())


# ------------------------------------------------------------------ (b) the sources entry alone
def _sources_expected(track, **sel):
    mis, imin, thres, final, src = posterior.select_reference(track, sel.get("true_markov_chain", True), sel.get("chainL"),
                                                              sel.get("prefix"))
    npnt, R = final.shape
    weight = np.stack([np.bincount(src[p][final[p]], minlength=R) for p in range(npnt)])
    return dict(min_misfit=mis[np.arange(npnt), imin], thres=thres, imin=imin, n_final=final.sum(axis=1), weight=weight,
                n_sources=(weight > 0).sum(axis=1), imin_source=src[np.arange(npnt), imin])


def _check_sources(track, **sel):
    want = _sources_expected(track, **sel)
    got = posterior.posterior_sources(torch.from_numpy(track).to(DEV), **sel)
    torch.cuda.synchronize()
    assert set(got) == set(want)
    for k, v in want.items():
        assert np.array_equal(got[k].cpu().numpy(), v), (sel, k)
    assert np.array_equal(got["weight"].sum(dim=1).cpu().numpy(), want["n_final"])
    if not sel.get("true_markov_chain", True):
        assert int(got["weight"].max()) <= 1
    return got


@pytest.mark.parametrize("sel", [dict(), dict(true_markov_chain=False), dict(chainL=263, prefix=100)], ids=["tmc", "raw", "prefix"])
def test_sources_across_the_tile_boundary(sel):
    """2 points x 2 * 263 rows: a rejected run across the 256-row tile boundary, a chain with nothing accepted but its first row,
    NaN and 88888 misfits."""
    tr = _carry_track(Model1DBatch(CONT))
    got = _check_sources(tr, **sel)
    if sel.get("true_markov_chain", True) and "chainL" not in sel:
        assert int(got["weight"][0, 199]) >= 2                           # rows 255 and 256 are final and carry row 199's parameters
        assert int(got["weight"][:, 264:].sum()) == 0                    # chain 1: everything sits on its first row


@pytest.mark.parametrize("sel", SLAB_BOUNDARY_SELECTIONS, ids=["tmc", "raw", "prefix"])
def test_sources_across_the_slab_boundary(sel):
    S = posterior.SLAB_ROWS
    tr = _slab_boundary_track(Model1DBatch(CONT))
    got = _check_sources(tr, **sel)
    if sel.get("true_markov_chain", True):
        assert int(got["imin"][0]) == S + 7 and int(got["imin_source"][0]) == S - 41 and int(got["weight"][0, S - 41]) >= 3


# ------------------------------------------------------------------ (c) argument errors
def test_argument_errors_of_the_sources_entry_return_before_launch():
    L = _lib.lib()
    npnt, R, W = 2, 120, 3 + 5
    track = torch.rand((npnt, R, W), dtype=torch.float64, device=DEV)
    f64, i32 = dict(dtype=torch.float64, device=DEV), dict(dtype=torch.int32, device=DEV)
    outs = ([torch.full((npnt,), -5.0, **f64) for _ in range(2)] + [torch.full((npnt,), -5, **i32) for _ in range(2)]
            + [torch.full((npnt, R), -5, **i32)] + [torch.full((npnt,), -5, **i32) for _ in range(2)])
    ws = torch.zeros(int(L.surfdisp_posterior_sources_workspace_bytes(npnt, R)), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0 and L.surfdisp_posterior_sources_workspace_bytes(0, R) == 0
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(npoints=npnt, R=R, track=track.data_ptr(), stride=W, tmc=1, chainL=0, prefix=0, outs=[o.data_ptr() for o in outs],
                 ws=ws.data_ptr(), ws_bytes=ws.numel())
        a.update(kw)
        return L.surfdisp_posterior_sources_device(ctypes.c_void_p(stream), a["npoints"], a["R"], ctypes.c_void_p(a["track"]), a["stride"],
                                                   a["tmc"], a["chainL"], a["prefix"], *[ctypes.c_void_p(p) for p in a["outs"]],
                                                   ctypes.c_void_p(a["ws"]), a["ws_bytes"])

    def outs_without(i):
        p = [o.data_ptr() for o in outs]; p[i] = None
        return p

    cases = dict(npoints=dict(npoints=0), R=dict(R=0), R_big=dict(R=2**30 + 1), stride=dict(stride=2),
                 slabs_big=dict(npoints=2**31 - 1, R=posterior.SLAB_ROWS + 1),
                 prefix0=dict(chainL=60, prefix=0), prefix_big=dict(chainL=60, prefix=61), not_multiple=dict(chainL=50, prefix=10),
                 no_track=dict(track=None), no_workspace=dict(ws=None), small_ws=dict(ws_bytes=ws.numel() - 1))
    for i, nm in enumerate(("min_misfit", "thres", "imin", "n_final", "weight", "n_sources", "imin_source")):
        cases[f"no_{nm}"] = dict(outs=outs_without(i))
    for name, kw in cases.items():
        assert call(**kw) == _lib.ERR_INVALID, name
        assert b"invalid" in L.surfdisp_last_error(), name
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == -5).all())                                    # nothing was written
    assert call() == _lib.SUCCESS and call(chainL=60, prefix=60) == _lib.SUCCESS
    torch.cuda.synchronize()
    assert bool((outs[4] >= 0).all()) and torch.equal(outs[4].sum(dim=1), outs[3])


def test_argument_errors_of_the_statistics_entry_return_before_launch():
    L = _lib.lib()
    npnt, total, P, nb = 2, 40, 5, 8
    pred = torch.rand((total, P), dtype=torch.float32, device=DEV)
    w = torch.ones(total, dtype=torch.int32, device=DEV)
    failed = torch.zeros(total, dtype=torch.uint8, device=DEV)
    offsets = torch.tensor([0, 15, 40], dtype=torch.int32, device=DEV)
    f64, i32 = dict(dtype=torch.float64, device=DEV), dict(dtype=torch.int32, device=DEV)
    outs = ([torch.full((npnt, P), -5, **i32)] + [torch.full((npnt, P), -5.0, **f64) for _ in range(4)] + [torch.full((npnt,), -5, **i32)]
            + [torch.full((npnt, P, nb), -5, **i32), torch.full((npnt, P), -5, **i32), torch.full((npnt, P), -5, **i32)])
    ws = torch.zeros(int(L.surfdisp_posterior_predictive_workspace_bytes(npnt, total, P)), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0 and L.surfdisp_posterior_predictive_workspace_bytes(0, total, P) == 0
    stream = torch.cuda.current_stream().cuda_stream
    lo, hi = np.zeros(P), np.ones(P)

    def call(**kw):
        a = dict(npoints=npnt, total=total, P=P, pred=pred.data_ptr(), ld=P, failed=failed.data_ptr(), w=w.data_ptr(),
                 offsets=offsets.data_ptr(), nbins=nb, vlo=lo, vhi=hi, outs=[o.data_ptr() for o in outs], ws=ws.data_ptr(),
                 ws_bytes=ws.numel())
        a.update(kw)
        host = lambda v: None if v is None else np.ascontiguousarray(v, np.float64)
        vlo, vhi = host(a["vlo"]), host(a["vhi"])
        return L.surfdisp_posterior_predictive_device(
            ctypes.c_void_p(stream), a["npoints"], a["total"], a["P"], ctypes.c_void_p(a["pred"]), a["ld"], ctypes.c_void_p(a["failed"]),
            ctypes.c_void_p(a["w"]), ctypes.c_void_p(a["offsets"]), a["nbins"],
            None if vlo is None else vlo.ctypes.data_as(ctypes.c_void_p), None if vhi is None else vhi.ctypes.data_as(ctypes.c_void_p),
            *[ctypes.c_void_p(p) for p in a["outs"]], ctypes.c_void_p(a["ws"]), a["ws_bytes"])

    def outs_without(i):
        p = [o.data_ptr() for o in outs]; p[i] = None
        return p

    def with_value(arr, i, v):
        b = arr.copy(); b[i] = v
        return b

    big = np.zeros(posterior.PRED_COLS_MAX + 1)
    cases = dict(npoints=dict(npoints=0), total=dict(total=-1), P0=dict(P=0), Pcap=dict(P=posterior.PRED_COLS_MAX + 1, ld=2000, vlo=big, vhi=big + 1),
                 ld=dict(ld=P - 1), no_pred=dict(pred=None), no_w=dict(w=None), no_offsets=dict(offsets=None),
                 no_workspace=dict(ws=None), small_ws=dict(ws_bytes=ws.numel() - 1),
                 nbins=dict(nbins=0), vhi_equal=dict(vhi=with_value(hi, 3, 0.0)), vlo_nan=dict(vlo=with_value(lo, 1, np.nan)),
                 vhi_inf=dict(vhi=with_value(hi, 4, np.inf)), vlo_inf=dict(vlo=with_value(lo, 0, -np.inf)),
                 no_vlo=dict(vlo=None), no_vhi=dict(vhi=None), no_below=dict(outs=outs_without(7)), no_above=dict(outs=outs_without(8)))
    for i, nm in enumerate(("count", "mean", "std", "min", "max", "n_failed")):
        cases[f"no_{nm}"] = dict(outs=outs_without(i))
    for name, kw in cases.items():
        assert call(**kw) == _lib.ERR_INVALID, name
        assert b"invalid" in L.surfdisp_last_error(), name
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == -5).all())                                    # nothing was written
    assert call() == _lib.SUCCESS and call(failed=None) == _lib.SUCCESS
    torch.cuda.synchronize()
    assert bool((outs[0] == torch.tensor([[15], [25]], device=DEV)).all())
    assert int(outs[6].sum() + outs[7].sum() + outs[8].sum()) == int(outs[0].sum()) and int(outs[5].sum()) == 0
    assert call(outs=outs_without(6), vlo=None, vhi=None, nbins=0) == _lib.SUCCESS          # no histogram: its arguments are not read
    torch.cuda.synchronize()


# ------------------------------------------------------------------ (d), (e) end to end
def _sampler_cont():
    mb = Model1DBatch(CONT, device=DEV)
    return mb, MetropolisBatch(mb.spec, mb.to_model, G["trace/periods"], G["trace/c_obs"], G["trace/uncer"], device=DEV, seed=1,
                               independent=False)


def _sampler_thermal():
    mb = Model1DBatch(HYBRID_STATIC, device=DEV)
    return mb, MetropolisBatch(mb.spec, mb.to_model, PERIODS_THERM, GT["hyb_ritz/c"][0] * 1.002, np.full(len(PERIODS_THERM), 0.01),
                               device=DEV, seed=1, independent=False)


T_JOINT = np.array([8.0, 12.0, 18.0, 25.0, 33.0])


def _sampler_joint():
    """Rayleigh phase, group and H/V data on five periods, observed on the initial model solved on the device (c and U scaled by
    1.002): data columns on different scales."""
    from pysurfinv_amd.forward import BatchPlan
    mb = Model1DBatch(CONT, device=DEV)
    model, nlay = mb.to_model(torch.as_tensor(np.asarray(mb.spec.v0, float)[None], device=DEV))
    plan = BatchPlan(1, model.shape[2], len(T_JOINT), device=DEV)
    c, u, st, r = plan.run(model.contiguous(), torch.as_tensor(T_JOINT.astype(np.float32), device=DEV), nlay=nlay, want_ratio=True)
    c, u, r = (t[0].double().cpu().numpy() for t in (c, u, r))
    assert int(st[0]) == 0 and np.isfinite(r).all()
    n = len(T_JOINT)
    data = {"RayPhase": (T_JOINT, c * 1.002, np.full(n, 0.01)), "RayGroup": (T_JOINT, u * 1.002, np.full(n, 0.02)),
            "RayHV": (T_JOINT, np.abs(r), np.full(n, 0.02))}
    return mb, MetropolisBatch(mb.spec, mb.to_model, device=DEV, seed=1, data=data, independent=False)


def _expanded(mc, track, **sel):
    """What the test derives itself: the prediction, recomputed misfit and failed flag of every final row's source parameters
    (no deduplication), with the (point, final row, source row) of each."""
    _, _, _, final, src = posterior.select_reference(track, sel.get("true_markov_chain", True), sel.get("chainL"), sel.get("prefix"))
    pts, rows = np.nonzero(final)
    srow = src[pts, rows]
    par = torch.from_numpy(track[pts, srow, 3:]).to(DEV)
    mis, _, _, cP = mc.misfit(par, return_c=True)
    return pts, rows, srow, cP.cpu().numpy(), mis.cpu().numpy()


def _check(label, mc, track, hist, **sel):
    """posterior_predictive against predictive_reference with the same device sampler, the team fixed; returns the device result."""
    L = _lib.lib()
    assert L.surfdisp_set_team(TEAM) == 0
    try:
        dev = posterior.posterior_predictive(mc, torch.from_numpy(track).to(DEV), hist=hist, **sel)
        torch.cuda.synchronize()
        ref = posterior.predictive_reference(mc, torch.from_numpy(track), hist=hist, **sel)
        pts, rows, srow, cP, mis = _expanded(mc, track, **sel)
    finally:
        L.surfdisp_set_team(0)
    assert set(dev) == set(ref)
    for k in ("min_misfit", "thres", "imin", "n_final", "n_sources", "n_failed", "count"):
        assert torch.equal(dev[k].cpu(), ref[k]), (label, k)
    P = cP.shape[1]
    failed = mis == 88888.0
    vlo, vhi, nb = posterior._hist_args(hist, P)
    for c in range(P):                                                   # exactness of the histograms is a fair demand
        v = cP[~failed, c]
        v = v[np.isfinite(v)]
        edges = np.arange(nb + 1) * ((vhi[c] - vlo[c]) / nb) + vlo[c]
        assert v.size == 0 or min(np.abs(v[:, None] - edges[None, :]).min(), np.abs(v - vhi[c]).min()) > 1e-9, (label, c)
    for k in ("hist", "below", "above"):
        assert torch.equal(dev[k].cpu(), ref[k]), (label, k)
    for k in ("pred_mean", "pred_std", "pred_min", "pred_max", "min_pred", "quantiles", "misfit_dev"):
        _close(f"{label} {k}", dev[k], ref[k], 1e-9)
    _close(f"{label} fit", dev["fit"], ref["fit"], 1e-9 / float(mc.uncer.min()))
    # what the test computes itself: the staleness figure, the curve of minMod, the weighted mean
    npnt = track.shape[0]
    want_dev = np.array([np.nan_to_num(np.abs(mis[pts == p] - track[p, srow[pts == p], 0]), nan=np.inf).max() for p in range(npnt)])
    _close(f"{label} misfit_dev against the test's own", dev["misfit_dev"], torch.from_numpy(want_dev), 1e-9)
    for p in range(npnt):
        ok = (pts == p) & ~failed
        assert int(dev["n_failed"][p]) == int(((pts == p) & failed).sum()) and int(dev["n_final"][p]) == int((pts == p).sum())
        assert np.abs(dev["pred_mean"][p].cpu().numpy() - cP[ok].mean(axis=0)).max() < 1e-9, label
        at = np.nonzero((pts == p) & (rows == int(dev["imin"][p])))[0]
        assert at.size == 1 and np.array_equal(dev["min_pred"][p].cpu().numpy(), cP[at[0]]), label
    assert bool((dev["n_sources"] <= dev["n_final"]).all())
    return dev


def test_a_stack_solves_the_same_alone_and_in_a_batch():
    """What the 1e-9 bar of the end-to-end tests rests on: with the team fixed and independent=False, the solver's fp32 result
    for a stack does not depend on the batch it is solved in (the deduplicated and the expanded batch differ in size and order)."""
    L = _lib.lib()
    assert L.surfdisp_set_team(TEAM) == 0
    try:
        for name, make in (("cont", _sampler_cont), ("thermal", _sampler_thermal), ("joint", _sampler_joint)):
            mb, mc = make()
            par = torch.from_numpy(_random_track(mb, 1, 90, seed=31)[0, :, 3:]).to(DEV)
            mis, _, _, cP = mc.misfit(par, return_c=True)
            for k in (0, 37, 89):
                m1, _, _, c1 = mc.misfit(par[k:k + 1].contiguous(), return_c=True)
                assert _same(c1[0], cP[k]) and _same(m1[0], mis[k]), (name, k)
            back = mc.misfit(par.flip(0).contiguous(), return_c=True)[3].flip(0)
            assert _same(back, cP), name
    finally:
        L.surfdisp_set_team(0)


@pytest.mark.parametrize("sel", [dict(), dict(true_markov_chain=False), dict(chainL=263, prefix=100)], ids=["tmc", "raw", "prefix"])
def test_end_to_end_continental(sel):
    mb, mc = _sampler_cont()
    tr = _random_track(mb, 3, 2 * 263, seed=22, chainL=263)
    dev = _check(f"cont {sel}", mc, tr, (2.0, 5.0, 120), **sel)
    if sel.get("true_markov_chain", True):
        assert bool((dev["n_sources"] < dev["n_final"]).all())           # 40 % accepted: rejected final rows share their source


def test_end_to_end_thermal_model():
    """The thermal OceanMantleHybrid, which posterior_profiles refuses: the models come from to_model, so it works here."""
    mb, mc = _sampler_thermal()
    assert mb.native_descriptor() is not None and mb._native_thermal
    tr = _random_track(mb, 2, 2 * 263, seed=23, chainL=263)
    _check("thermal", mc, tr, (2.5, 5.0, 100))


def test_end_to_end_joint_data():
    mb, mc = _sampler_joint()
    n = len(T_JOINT)
    assert mc.joint.Ptot == 3 * n
    tr = _random_track(mb, 2, 2 * 263, seed=24, chainL=263)
    vlo = np.concatenate([np.full(n, 2.5), np.full(n, 2.0), np.full(n, 0.3)])          # c, U and H/V on their own scales
    vhi = np.concatenate([np.full(n, 4.5), np.full(n, 4.5), np.full(n, 2.0)])
    dev = _check("joint", mc, tr, (vlo, vhi, 60))
    assert dev["hist"].shape == (2, 3 * n, 60) and int(dev["hist"][:, 2 * n:].sum()) > 0


def test_a_planted_misfit_shows_in_misfit_dev():
    """misfit_dev is the staleness check of a loaded track: one wrong misfit planted in an accepted row that final rows sit on
    shows there (against the figure the test computes itself, inside _check), and the other point does not notice."""
    mb, mc = _sampler_cont()
    tr = _random_track(mb, 2, 2 * 263, seed=25, chainL=263)
    before = _check("before planting", mc, tr, (2.0, 5.0, 120))
    want = _sources_expected(tr)
    cand = want["weight"][1].copy()
    cand[want["imin_source"][1]] = 0
    r = int(cand.argmax())
    assert cand[r] >= 3 and tr[1, r, 2] > 0.5                            # an accepted row at least two rejected final rows sit on
    tr[1, r, 0] = 1.0e6                                                  # no longer final itself, still their source
    assert _sources_expected(tr)["weight"][1, r] >= 2
    after = _check("after planting", mc, tr, (2.0, 5.0, 120))
    assert float(after["misfit_dev"][1]) > 9.0e5 > float(before["misfit_dev"][1])
    assert float(after["misfit_dev"][0]) == float(before["misfit_dev"][0]) and _same(after["pred_mean"][0], before["pred_mean"][0])


def test_postpoint_predictive_on_the_device(tmp_path):
    from pysurfinv_amd.point import Point, PostPoint
    pt = Point(CONT, periods=list(G["trace/periods"]), vels=list(G["trace/c_obs"]), uncers=list(G["trace/uncer"]), device=DEV)
    pt.MCinvMP(outdir=str(tmp_path), pid="here", runN=600, chainL=60, seed=3)
    p = PostPoint(os.path.join(str(tmp_path), "here.npz"), device=DEV)
    a = p.predictive(hist=(2.0, 5.0, 120))
    P = len(G["trace/periods"])
    assert a["n_final"] == int(p.accFinal.sum()) and 1 <= a["n_sources"] <= a["n_final"] and a["thres"] == p.thres
    assert a["mean"].shape == (P,) and a["hist"].shape == (P, 120) and a["quantiles"].shape == (P, 3)
    assert a["n_failed"] == 0 and (a["count"] == a["n_final"]).all() and (a["min"] <= a["mean"]).all() and (a["mean"] <= a["max"]).all()
    # a track the sampler wrote itself: every source row's record is the misfit of its own parameters, up to the team the
    # lock step's batch ran with (the root search's answers differ by 1e-6 between team sizes)
    assert a["misfit_dev"] < 1e-3
    # minMod's curve reproduces minMod's misfit
    obs, un = np.asarray(G["trace/c_obs"], float), np.asarray(G["trace/uncer"], float)
    assert abs(np.sqrt((((a["min_pred"] - obs) / un) ** 2).mean()) - a["min_misfit"]) < 1e-3
