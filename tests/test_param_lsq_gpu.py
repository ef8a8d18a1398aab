"""surfdisp_lsq_step_params_device (include/surfdisp.h section (6i)) on the GPU against paramlsq.param_lsq_reference, on synthetic inputs
built as tests/lsq_cases.py builds them (``step_case`` of tests/param_lsq_cases.py).

Bars, those of tests/test_lsq_modes_gpu.py and tests/test_lsq_resolution_gpu.py for cond(A) <= 1e4 (asserted: a condition on the
inputs): delta, cov and sigma to 1e-10 of the largest entry, stats to 1e-12 relative, logdet to 1e-10 (|logdet| + Nu), info exact; a
flagged stack all zeros, its neighbours solved."""
import numpy as np
import pytest

from lsq_cases import _case, launch
from param_lsq_cases import STEP_CASES, step_case, step_launch, step_reference
from pysurfinv_amd import _lib, linearized

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,Lmax,N,Nu", STEP_CASES)
def test_step_kernel_matches_the_reference_step(B, Lmax, N, Nu):
    c = step_case(B, Lmax, N, Nu)
    rc, o = step_launch(c)
    assert rc == _lib.SUCCESS, _lib.lib().surfdisp_last_error()
    flags, worst = [], dict(delta=0.0, cov=0.0, sigma=0.0, stats=0.0, logdet=0.0, cond=0.0)
    assert (c["free"] == 0).any() or Nu == 1                                # some fixed unknowns (a single unknown stays free)
    for b in range(B):
        tag = f"({B},{Lmax},{N},{Nu}) stack {b}"
        ref, rows = step_reference(c, b)
        free = (c["free"][b] if c["free"].ndim == 2 else c["free"]).astype(bool)
        used, dropped, flag = (int(v) for v in o["info"][b])
        assert (used, dropped, flag) == (ref["used"], N - ref["used"], ref["flag"]), (tag, o["info"][b], ref["used"], ref["flag"])
        for k in ("delta", "cov", "sigma", "logdet", "stats"):
            assert np.isfinite(o[k][b]).all(), (tag, k)
        assert not o["delta"][b][~free].any() and not o["sigma"][b][~free].any(), tag
        assert not o["cov"][b][~free].any() and not o["cov"][b][:, ~free].any(), tag
        flags.append(flag)
        for k, name in enumerate(("misfit", "prior", "predicted")):
            e = abs(o["stats"][b, k] - ref[name])
            worst["stats"] = max(worst["stats"], e / abs(ref[name]) if ref[name] else e)
            assert e <= 1e-12 * abs(ref[name]), (tag, name, o["stats"][b, k], ref[name])
        if flag != 0:
            assert not o["delta"][b].any() and not o["cov"][b].any() and not o["sigma"][b].any() and o["logdet"][b] == 0.0, tag
            continue
        cond = np.linalg.cond(ref["A"])
        worst["cond"] = max(worst["cond"], cond)
        assert cond <= 1e4, (tag, cond)                                     # the premise of the relative bars
        assert np.array_equal(o["cov"][b], o["cov"][b].T), tag
        for k in ("delta", "cov", "sigma"):
            e = np.abs(o[k][b] - ref[k]).max() / np.abs(ref[k]).max()
            worst[k] = max(worst[k], e)
            assert e <= 1e-10, (tag, k, e)
        e = abs(o["logdet"][b] - ref["logdet"]) / (abs(ref["logdet"]) + Nu)
        worst["logdet"] = max(worst["logdet"], e)
        assert e <= 1e-10, (tag, e)
        assert ref["used"] > 0 and np.abs(ref["delta"]).max() > 0
    print(f"({B},{Lmax},{N},{Nu}): worst relative errors " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    if c["obs"].ndim == 2 and B >= 3:
        assert flags[2] == 1 and flags[1] == 0 and flags[3 % B] == 0          # every row masked: flag 1, its neighbours solved
    if N > 12:                                                                # the NaN kernel row and the NaN thickness row of stack 0
        ref0, rows0 = step_reference(c, 0)
        kept = np.array(rows0)[ref0["kept"]]
        assert 5 in rows0 and 5 not in kept and 10 in rows0 and 10 not in kept
    assert (o["info"][:, 1] >= (c["cols"][:, 0] == 3).sum()).all()            # the rows of the source without part_h


def test_optional_outputs_may_be_null_and_a_failed_pivot_is_zeros():
    c = step_case(3, 17, 40, 5)
    rc, full = step_launch(c)
    rc2, o = step_launch(c, cov=True, sigma=True, logdet=True, prior_w=True, prior_ref=True, free=True, nlay=True)
    assert rc == rc2 == _lib.SUCCESS
    assert all((o[k] == 7.0).all() for k in ("cov", "sigma", "logdet")) and not (o["stats"][:, 1] != 0).any()
    rc3, o3 = step_launch(c, cov=True)                                        # sigma without cov
    assert rc3 == _lib.SUCCESS and np.array_equal(o3["sigma"], full["sigma"]) and np.array_equal(o3["delta"], full["delta"])
    neg = dict(c, lam=-1e12 * np.ones(3))                                     # a negative damping: the first pivot fails
    rc4, o4 = step_launch(neg)
    assert rc4 == _lib.SUCCESS
    flags = o4["info"][:, 2].tolist()
    assert flags == [2, 2, 1]
    for k in ("delta", "cov", "sigma", "logdet"):
        assert not o4[k].any(), k
    assert np.array_equal(o4["stats"][:, 2], o4["stats"][:, 0] + o4["stats"][:, 1]) and np.isfinite(o4["stats"]).all()


@pytest.mark.parametrize("B,Lmax,N", [(3, 17, 40), (2, 64, 100)])
def test_a_selection_jacobian_is_the_vs_step_of_the_old_entry(B, Lmax, N):
    """The inputs of ``lsq_cases._case`` through both entries: jac[vs] selects the free layers of each stack, jac[vp] and jac[rho] carry
    the slopes there, jac[h] is zero, scale 1, no prior, alpha 0 - delta of surfdisp_lsq_step_device to 1e-12 relative."""
    c = dict(_case(B, Lmax, N, seed=900 + Lmax), alpha=0.0)
    rc, old = launch("step", c)
    assert rc == _lib.SUCCESS
    fr = np.broadcast_to(c["free"].astype(bool), (B, Lmax)) & (np.arange(Lmax)[None, :] < c["nlay"][:, None])
    Nu = int(fr.sum(axis=1).max())
    assert Nu <= 64
    jac, free = np.zeros((B, 4, Lmax, Nu)), np.zeros((B, Nu), np.uint8)
    for b in range(B):
        idx = np.nonzero(fr[b])[0]
        j = np.arange(idx.size)
        jac[b, 1, idx, j], jac[b, 0, idx, j], jac[b, 2, idx, j] = 1.0, c["vp_slope"][b, idx], c["rho_slope"][b, idx]
        free[b, :idx.size] = 1
    zeros_h = [np.zeros_like(c["part"][0]) for _ in range(5)]
    p = dict(B=B, Lmax=Lmax, N=N, Nu=Nu, P=c["P"], nlay=c["nlay"], jac=jac, part=c["part"], part_h=zeros_h, pred=c["pred"], cols=c["cols"],
             weights=c["weights"], obs=c["obs"], uncer=c["uncer"], mask=c["mask"], free=free, scale=np.ones(Nu), prior_w=None, prior_ref=None,
             params=np.zeros((B, Nu)), lam=c["lam"])
    rc, new = step_launch(p)
    assert rc == _lib.SUCCESS, _lib.lib().surfdisp_last_error()
    assert np.array_equal(new["info"], old["info"]) and (old["info"][:, 2] == 0).any()
    for b in range(B):
        idx = np.nonzero(fr[b])[0]
        d_old, d_new = old["delta"][b, idx], new["delta"][b, :idx.size]
        assert np.abs(d_new - d_old).max() <= 1e-12 * np.abs(d_old).max(), (b, np.abs(d_new - d_old).max(), np.abs(d_old).max())
        assert not new["delta"][b, idx.size:].any()
        assert abs(new["stats"][b, 0] - old["stats"][b, 0]) <= 1e-12 * abs(old["stats"][b, 0])
        assert abs(new["stats"][b, 2] - old["stats"][b, 2]) <= 1e-12 * abs(old["stats"][b, 2])
