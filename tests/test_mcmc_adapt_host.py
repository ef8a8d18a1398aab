"""Adaptive proposals (csrc/surfdisp_mcmc_adapt.hip: surfdisp_mcmc_adapt_device; ``mcmc.adapt_reference``, ``MetropolisBatch.set_adaptive``,
``run_grid(proposal="adaptive")``, ``Point.MCinvMP(proposal="adaptive")``) - what needs no device: the numpy statement against
direct formulas, the entry's argument checks (invalid calls only: nothing launches) and the interface's refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_prior_redraw import _cpu_model             # noqa: E402

from pysurfinv_amd import mcmc, settings             # noqa: E402
from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402
from pysurfinv_amd.mcmc import (MetropolisBatch, PriorRules, adapt_reference, adapt_state_len, adapt_state_views,   # noqa: E402
                                cov_factor_reference)
from pysurfinv_amd.proposal import Adaptation, Factor, ReferenceSteps, fused_schedule   # noqa: E402

OFF = dict(target_accept=-1.0)


def _full(S):
    """The symmetric matrix of an upper triangle."""
    S = np.triu(S)
    return S + np.triu(S, 1).T


def _feed(xs, **kw):
    """The updates xs[t] [F, cpp, N] one after the other, no accept windows, step 0.1 -> (state, last cov)."""
    state, cov = None, None
    for x in xs:
        state, cov = adapt_reference(state, x, None, np.full(x.shape[2], 0.1), **kw)
    return state, cov


def test_state_layout():
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "surfdisp.h")).read()
    assert "#define SURFDISP_MCMC_ADAPT_HEAD 8\n" in hdr and mcmc.ADAPT_HEAD == 8
    assert adapt_state_len(13) == 8 + 13 + 169
    st = np.arange(2.0 * adapt_state_len(3)).reshape(2, -1)
    v = adapt_state_views(st, 3)
    assert v["weight"][1] == st[1, 0] and v["log_scale"][1] == st[1, 1] and v["n_updates"][0] == 2 and v["fallbacks"][0] == 3
    assert v["mean"].shape == (2, 3) and v["mean"][0, 0] == 8 and v["scatter"].shape == (2, 3, 3) and v["scatter"][0, 0, 0] == 11


@pytest.mark.parametrize("F,cpp,N,T", [(1, 1, 1, 7), (3, 5, 13, 6), (2, 100, 64, 2)])
def test_welford_is_the_sample_covariance(F, cpp, N, T):
    """forget = 1, every sample fed, no scale: S / W = np.cov(bias=True) of all samples, mean their mean, to 1e-12 relative."""
    rng = np.random.default_rng(5)
    xs = [3.5 + rng.uniform(-0.5, 0.5, (F, cpp, N)) for _ in range(T)]
    st, _ = _feed(xs, **OFF)
    v = adapt_state_views(st, N)
    X = np.concatenate(xs, axis=1)
    assert (v["weight"] == T * cpp).all() and (v["n_updates"] == 0).all() and (v["log_scale"] == 0).all()
    for f in range(F):
        ref = np.cov(X[f].T, bias=True).reshape(N, N)
        assert np.abs(_full(v["scatter"][f]) / v["weight"][f] - ref).max() <= 1e-12 * np.abs(ref).max() + 1e-300
        assert np.abs(v["mean"][f] - X[f].mean(axis=0)).max() <= 1e-12 * np.abs(X[f]).max()
        assert not np.tril(v["scatter"][f], -1).any()


def test_forgetting_is_the_weighted_covariance():
    """forget < 1: a sample of update t of T carries the weight forget^(T - 1 - t); mean and S / W against the direct weighted sums."""
    rng = np.random.default_rng(6)
    F, cpp, N, T, f = 2, 4, 5, 6, 0.9
    xs = [3.5 + rng.uniform(-0.5, 0.5, (F, cpp, N)) for _ in range(T)]
    st, _ = _feed(xs, forget=f, **OFF)
    v = adapt_state_views(st, N)
    w = np.repeat(f ** (T - 1 - np.arange(T)), cpp)
    X = np.concatenate(xs, axis=1)
    for p in range(F):
        m = (w[:, None] * X[p]).sum(axis=0) / w.sum()
        C = np.einsum("i,ij,ik->jk", w, X[p] - m, X[p] - m) / w.sum()
        assert abs(v["weight"][p] - w.sum()) <= 1e-12 * w.sum()
        assert np.abs(v["mean"][p] - m).max() <= 1e-12 * np.abs(X[p]).max()
        assert np.abs(_full(v["scatter"][p]) / v["weight"][p] - C).max() <= 1e-12 * np.abs(C).max()


def test_log_scale_follows_the_accept_rate():
    rng = np.random.default_rng(7)
    F, cpp, N, R = 3, 4, 2, 5
    x = 3.5 + rng.uniform(-0.5, 0.5, (F, cpp, N))
    flags = np.zeros((F, cpp, R))
    flags[0] = 1.0                                                     # a = 1 > target: up
    flags[2, 0, :] = 1.0                                               # a = 1 / 4 = target: stays
    kw = dict(target_accept=0.25, gain=1.0, decay=0.6, log_scale_bounds=(-0.3, 1.0))
    st, _ = adapt_reference(None, x, flags, np.full(N, 0.1), **kw)
    v = adapt_state_views(st, N)
    assert v["log_scale"].tolist() == [0.75, -0.25, 0.0] and v["n_updates"].tolist() == [1, 1, 1]
    st, _ = adapt_reference(st, x, flags, np.full(N, 0.1), **kw)       # k = 2: steps of 2^-0.6, into the clamps
    v = adapt_state_views(st, N)
    assert v["log_scale"][0] == 1.0 and v["log_scale"][1] == -0.3 and v["log_scale"][2] == 0.0 and (v["n_updates"] == 2).all()
    st3, _ = adapt_reference(st, x, flags, np.full(N, 0.1), **dict(kw, log_scale_bounds=(-3.0, 3.0)))
    assert adapt_state_views(st3, N)["log_scale"][1] == -0.3 + 3.0 ** -0.6 * (0.0 - 0.25)
    for empty in (None, np.zeros((F, cpp, 0))):                        # an empty window leaves ls and k alone, the moments move
        st2, _ = adapt_reference(st, x, empty, np.full(N, 0.1), **kw)
        v2 = adapt_state_views(st2, N)
        assert np.array_equal(v2["log_scale"], v["log_scale"]) and (v2["n_updates"] == 2).all() and (v2["weight"] == 3 * cpp).all()
    st2, _ = adapt_reference(st, x, flags, np.full(N, 0.1), **dict(kw, target_accept=-1.0))
    assert np.array_equal(adapt_state_views(st2, N)["log_scale"], v["log_scale"]) and (adapt_state_views(st2, N)["n_updates"] == 2).all()


def test_fixed_scalar_and_identical_chains():
    """A scalar that never varies with step 0: zero row and column, not counted in N_live.  Identical chains with step > 0: ridge
    step^2 on the diagonal, a matrix the factor statement takes.  Below min_weight: no covariance."""
    rng = np.random.default_rng(8)
    F, cpp, N = 2, 6, 4
    x = 3.5 + rng.uniform(-0.5, 0.5, (F, cpp, N))
    x[:, :, 2] = 3.25                                                  # constant, step 0
    x[1] = x[1, 0]                                                     # point 1: all chains identical
    step = np.array([0.1, 0.2, 0.0, 0.05])
    st, cov = adapt_reference(None, x, None, step, min_weight=cpp + 1, ridge=1e-3, **OFF)
    assert cov is None and (adapt_state_views(st, N)["ready"] == 0).all()
    st, cov = adapt_reference(None, x, None, step, min_weight=cpp, ridge=1e-3, **OFF)
    v = adapt_state_views(st, N)
    assert (v["ready"] == 1).all() and np.array_equal(cov, np.transpose(cov, (0, 2, 1)))
    assert not cov[:, 2, :].any() and not cov[:, :, 2].any()
    live = [0, 1, 3]
    c = 2.38 * 2.38 / 3                                                # N_live = 3, scale 1
    want0 = c * (np.cov(x[0][:, live].T, bias=True) + 1e-3 * np.diag(step[live] ** 2))
    assert np.allclose(cov[0][np.ix_(live, live)], want0, rtol=1e-12, atol=0)
    assert np.allclose(cov[1], c * 1e-3 * np.diag(step ** 2), rtol=1e-12, atol=0)
    L, flag = cov_factor_reference(cov, 1.0, step)
    assert flag.tolist() == [0, 0] and np.allclose(L[1], np.sqrt(c * 1e-3) * np.diag(step), rtol=1e-12)
    assert not L[:, 2, :].any() and not L[:, :, 2].any()
    # the scale enters as exp(2 ls)
    st[:, 1] = 0.5
    st2, cov2 = adapt_reference(st, x, None, step, min_weight=cpp, ridge=1e-3, **OFF)
    assert np.allclose(cov2[1], np.exp(1.0) * cov[1], rtol=1e-12)


# ------------------------------------------------------------------------------------------------------ the entry's argument checks
def test_entry_rejects_bad_arguments_before_any_device_call():
    from pysurfinv_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    some = ctypes.c_void_p(ctypes.addressof(buf))                      # never dereferenced: every call below is rejected on the host
    order = ("stream", "F", "cpp", "N", "p", "track", "chain_stride", "row_stride", "row_lo", "row_hi", "step", "forget", "target_accept",
             "gain", "decay", "ls_min", "ls_max", "min_weight", "ridge", "state", "cov_out")
    base = dict(stream=None, F=3, cpp=4, N=13, p=some, track=some, chain_stride=100, row_stride=16, row_lo=1, row_hi=6, step=some,
                forget=0.9, target_accept=0.25, gain=1.0, decay=0.6, ls_min=-3.0, ls_max=3.0, min_weight=52.0, ridge=1e-3, state=some,
                cov_out=some)
    nan = float("nan")
    bad = [dict(F=0), dict(cpp=0), dict(N=0), dict(N=65), dict(F=-1), dict(forget=0.0), dict(forget=1.0000001), dict(forget=-0.5),
           dict(forget=nan), dict(row_hi=0), dict(row_lo=-1), dict(p=None), dict(state=None), dict(step=None), dict(track=None),
           dict(ridge=-1e-9), dict(ridge=nan), dict(min_weight=0.5), dict(min_weight=nan), dict(ls_min=1.0, ls_max=0.0),
           dict(target_accept=1.5), dict(target_accept=nan), dict(gain=nan), dict(decay=nan)]
    for over in bad:
        a = dict(base)
        a.update(over)
        dbl = ("forget", "target_accept", "gain", "decay", "ls_min", "ls_max", "min_weight", "ridge")
        rc = L.surfdisp_mcmc_adapt_device(*[ctypes.c_double(a[k]) if k in dbl else a[k] for k in order])
        assert rc == _lib.ERR_INVALID, (over, rc)
        assert b"surfdisp_mcmc_adapt_device" in L.surfdisp_last_error(), over
    assert "surfdisp_mcmc_adapt_device" in _lib.EXPORTS


# ------------------------------------------------------------------------------------------------------ the interface
def _cpu_sampler(isgood=None, **kw):
    m = _cpu_model()
    P = len(settings.MCMC_PERIODS)
    return MetropolisBatch(m.spec, m.to_model, settings.MCMC_PERIODS, np.full(P, 3.5), np.full(P, 0.05), device="cpu", isgood=isgood, **kw)


def _options(mc, cpp=4):
    """What set_adaptive stores, made by hand: a sampler without a device cannot be given adaptation through the front door."""
    ad = Adaptation(mc.proposer, mc.spec.n, mc._exh, cpp, every=10, start=20, until=None, forget=1.0, target_accept=0.25, gain=1.0,
                    decay=0.6, min_weight=52.0, ridge=1e-3, log_scale_bounds=(-3.0, 3.0))
    assert (ad.cpp, ad.every, ad.start, ad.until, ad.forget, ad.target_accept, ad.gain, ad.decay, ad.min_weight, ad.ridge, ad.ls_min,
            ad.ls_max) == (cpp, 10, 20, None, 1.0, 0.25, 1.0, 0.6, 52.0, 1e-3, -3.0, 3.0)
    return ad


def test_set_adaptive_refusals():
    mc = _cpu_sampler()
    mc.set_adaptive(None)                                              # always allowed
    with pytest.raises(ValueError, match="fused"):                     # no HIP device: no fused path
        mc.set_adaptive(4)
    with pytest.raises(ValueError, match="callback"):
        _cpu_sampler(isgood=lambda p: torch.ones(p.shape[0], dtype=torch.bool)).set_adaptive(4)
    with pytest.raises(ValueError, match="local_rows"):
        _cpu_sampler(isgood=PriorRules(_cpu_model()), local_rows=np.zeros(4, np.int64)).set_adaptive(4)
    with pytest.raises(ValueError, match="chains_per_point"):
        mc.set_adaptive(0)
    with pytest.raises(ValueError, match="every"):
        mc.set_adaptive(4, every=0)
    for until in (20, 5):
        with pytest.raises(ValueError, match="until"):
            mc.set_adaptive(4, start=20, until=until)
    for kw in (dict(forget=0.0), dict(forget=1.5), dict(ridge=-1.0), dict(log_scale_bounds=(1.0, -1.0)), dict(min_weight=0.0)):
        with pytest.raises(ValueError, match="set_adaptive"):
            mc.set_adaptive(4, **kw)
    assert mc._adaptation is None and mc.adaptation() is None
    # both switches turn it off
    mc._adaptation = _options(mc)
    mc.set_adaptive(None)
    assert mc._adaptation is None
    mc._adaptation = _options(mc)
    mc.set_proposal(None)
    assert mc._adaptation is None and mc._given is None
    # ... and the proposal in force is the earlier one again; a run's working factors come before set_proposal's, and only while it lasts
    plain = mc.proposal()
    assert type(plain) is ReferenceSteps and plain.max_depth == 4
    mc._adaptation = ad = _options(mc)
    assert mc.proposal() is plain                                      # not inside a run: nothing of the adaptation is in force
    ad.working = Factor(mc.proposer, None, mc._exh, torch.zeros(2, mc.spec.n, mc.spec.n, dtype=torch.float64), 4)
    mc._given = Factor(mc.proposer, None, mc._exh, torch.zeros(1, mc.spec.n, mc.spec.n, dtype=torch.float64), 1 << 62)
    assert mc.proposal() is ad.working and mc.proposal().max_depth == 4
    ad.end()
    assert mc.proposal() is mc._given
    mc.set_adaptive(None)
    assert mc.proposal() is mc._given
    mc.set_proposal(None)
    assert mc.proposal() is plain


def test_run_points_run_and_run_graphed_refuse():
    mc = _cpu_sampler(forward=lambda *a: pytest.fail("nothing may be evaluated"))
    mc._adaptation = _options(mc, cpp=4)
    with pytest.raises(ValueError, match="chains_per_point"):
        mc.run_points(2, 3, 5)
    with pytest.raises(ValueError, match="set_adaptive"):
        mc.run_graphed(4, 5)
    with pytest.raises(ValueError, match="set_adaptive"):              # the torch loop draws no adaptive proposals
        mc.run(8, 5)
    with pytest.raises(ValueError, match="set_adaptive"):
        mc.run_points(2, 4, 5)


def test_update_instants():
    ad = Adaptation(None, 13, None, 4, start=10, every=5, until=30)
    due = [i for i in range(60) if ad.due(i, i + 1)]
    assert due == [10, 15, 20, 25]
    assert ad.due(11, 15) is False and ad.due(11, 16) and ad.due(26, 40) is False and ad.due(0, 11)
    assert not ad.due(30, 31) and not ad.due(0, 10)


@pytest.mark.parametrize("chainL", [1, 2, 5, 13])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_fused_schedule_covers_the_rows(chainL, d):
    calls = list(fused_schedule(chainL, d))
    assert calls[0] == (0, 1, True) and not any(first for _, _, first in calls[1:])
    rows = [r for i, ns, _ in calls for r in range(i, i + ns)]
    assert rows == list(range(chainL))                                 # every row once, in order
    assert all(1 <= ns <= d for _, ns, _ in calls)
    assert len(calls) == (chainL if d == 1 else 1 + -(-(chainL - 1) // d))
    if d == 1:
        assert calls == [(i, 1, i == 0) for i in range(chainL)]


def test_fused_schedule_places_the_updates():
    """start = 2, every = 3, until = 9: the instants 2, 5, 8.  An update follows the call among whose rows i .. i + ns - 1 an instant
    lies, once, with the window up to the call's last row.  Written out from that rule: (call numbers from 1, window ends)."""
    ad = Adaptation(None, 13, None, 4, start=2, every=3, until=9)
    want = {(13, 1): ([3, 6, 9], [2, 5, 8]),          # one row per call: call n is row n - 1
            (13, 2): ([2, 4, 5], [2, 6, 8]),          # calls 0 | 1-2 | 3-4 | 5-6 | 7-8 | 9-10 | 11-12
            (13, 3): ([2, 3, 4], [3, 6, 9]),          # calls 0 | 1-3 | 4-6 | 7-9 | 10-12
            (13, 4): ([2, 3], [4, 8]),                # calls 0 | 1-4 | 5-8 | 9-12: the instants 5 and 8 share a call
            (5, 1): ([3], [2]), (5, 2): ([2], [2]),   # five rows: the instant 2 alone; calls 0 | 1-2 | 3-4
            (5, 3): ([2], [3]), (5, 4): ([2], [4]),   # calls 0 | 1-3 | 4 and 0 | 1-4
            (2, 1): ([], []), (2, 4): ([], [])}       # rows 0 and 1: no instant
    for (chainL, d), (numbers, ends) in want.items():
        got = [(n, i + ns - 1) for n, (i, ns, _) in enumerate(fused_schedule(chainL, d), 1) if ad.due(i, i + ns)]
        assert got == list(zip(numbers, ends)), (chainL, d)


def test_public_routes_reach_the_sampler_on_a_thermal_model():
    """proposal="adaptive" accepts a thermal model: without a device the refusal is the sampler's, about the HIP device."""
    from pysurfinv_amd import grid
    from pysurfinv_amd.point import Point
    mb = Model1DBatch(settings.C5_SETTING, device="cpu")
    P = len(settings.MCMC_PERIODS)
    obs = np.full((3, P), 3.8)
    with pytest.raises(ValueError, match="HIP device") as e:
        grid.run_grid(mb, np.arange(3.0), np.zeros(3), settings.MCMC_PERIODS, obs, 0.01 * obs, 2, 3, device="cpu", proposal="adaptive",
                      forward=lambda *a: pytest.fail("nothing may be evaluated"))
    assert "thermal" not in str(e.value)
    with pytest.raises(ValueError, match="adaptive="):
        grid.run_grid(mb, np.arange(3.0), np.zeros(3), settings.MCMC_PERIODS, obs, 0.01 * obs, 2, 3, device="cpu", adaptive=dict(every=5))
    pt = Point(settings.C5_SETTING, periods=settings.MCMC_PERIODS, vels=[3.8] * P, uncers=[0.04] * P, device="cpu")
    with pytest.raises(ValueError, match="HIP device") as e:
        pt.MCinvMP(outdir="unused", runN=4, chainL=2, proposal="adaptive", adaptive=dict(every=5))
    assert "thermal" not in str(e.value)
    with pytest.raises(ValueError, match="adaptive="):
        pt.MCinvMP(outdir="unused", runN=4, chainL=2, adaptive=dict(every=5))
