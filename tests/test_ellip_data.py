"""Rayleigh ellipticity (H/V) as joint data (pysurfinv_amd.obsdata, quantity "E"): validation, column table, the torch misfit
and failure rule, and the sampler on it with the CPU oracle standing in for the device solver (no GPU).  The oracle's
ellipticity comes from surfdisp_oracle_forward_dbg, stack by stack."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from settings import CONT                            # noqa: E402
from test_joint_data import T_R, oracle_joint_forward, synthetic_sets
from pysurfinv_amd.layers_batch import Model1DBatch
from pysurfinv_amd.mcmc import MetropolisBatch
from pysurfinv_amd.obsdata import DICT_KEYS, DispersionData, JointData, as_datasets

T_E = np.array([5.0, 8.0, 10.0, 14.0, 20.0, 25.0, 30.0])


def oracle_ratio(model, per, nlay=None):
    """Ellipticities [B, P] (float32) and phase velocities of the CPU oracle, stack by stack."""
    from oracle import cport
    O = cport.lib()
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    model = np.ascontiguousarray(model, np.float32)
    B, _, L = model.shape
    p32 = np.ascontiguousarray(per, np.float32)
    P = p32.size
    c = np.zeros((B, P), np.float32); u = np.zeros((B, P), np.float32); r = np.zeros((B, P), np.float32)
    for i in range(B):
        n = L if nlay is None else int(nlay[i])
        m = np.ascontiguousarray(model[i][:, :n])
        O.surfdisp_oracle_forward_dbg(n, 2, fp(m[0]), fp(m[1]), fp(m[2]), fp(m[3]), fp(m[4]), fp(p32), P, fp(c[i]), fp(u[i]), fp(r[i]))
    return c, r


def oracle_ellip_forward(jd):
    """test_joint_data's forward hook on the CPU oracle, plus eR of the Rayleigh solve's periods."""
    base = oracle_joint_forward(jd)

    def fwd(model, nlay):
        out = base(model, nlay)
        out["eR"] = None
        if jd.with_ratio:
            c, r = oracle_ratio(model.cpu().numpy(), jd.solve_periods["R"], None if nlay is None else nlay.cpu().numpy())
            assert np.array_equal(c.astype(np.float64), out["cR"].numpy())   # the same solve as the batch entry's
            out["eR"] = torch.from_numpy(r.astype(np.float64))
        return out
    return fwd


def ellip_set(mb, T=T_E, absolute=False, seed=11, weight=1.0):
    """An ellipticity curve observed on ONE PRIOR DRAW (chi is nearly invariant under the uniform scaling that
    synthetic_sets observes c and U on: it moves by about 1e-3), uncertainty 0.02."""
    mc = MetropolisBatch(mb.spec, mb.to_model, [10.0], [3.0], [0.1], device="cpu", seed=seed)
    model, nlay = mb.to_model(mc.reset(1))
    c, r = oracle_ratio(model.numpy(), T, None if nlay is None else nlay.numpy())
    assert (c[0] > 0.01).all() and np.isfinite(r[0]).all()
    return DispersionData("R", "E", T, r[0].astype(np.float64), np.full(len(T), 0.02), weight=weight, absolute=absolute)


def test_validation_keys_and_round_trip(tmp_path):
    T = [10.0, 20.0]
    v, u = [0.9, 1.1], [0.02, 0.02]
    with pytest.raises(ValueError):
        DispersionData("L", "E", T, v, u)                                  # Love waves have no ellipticity
    with pytest.raises(ValueError):
        DispersionData("R", "c", T, v, u, absolute=True)
    with pytest.raises(ValueError):
        DispersionData("R", "U", T, v, u, absolute=True)
    with pytest.raises(ValueError):
        DispersionData("L", "c", T, v, u, absolute=True)
    with pytest.raises(ValueError):                                        # duplicates, whatever their `absolute`
        JointData([DispersionData("R", "E", T, v, u), DispersionData("R", "E", T, v, u, absolute=True)])
    with pytest.raises(ValueError):
        JointData([DispersionData("R", "E", T, v, u), DispersionData("R", "E", T, v, u)])
    with pytest.raises(ValueError):
        as_datasets({"RayHv": (T, v, u)})
    with pytest.raises(ValueError):
        as_datasets({"LoveHV": (T, v, u)})
    assert DICT_KEYS["RayPhase"][:2] == ("R", "c") and DICT_KEYS["LoveGroup"][:2] == ("L", "U")
    hv, el = as_datasets({"RayHV": (T, v, u), "RayEllip": (T, v, u)})
    assert (hv.wave, hv.quantity, hv.absolute, hv.source) == ("R", "E", True, 5)
    assert (el.wave, el.quantity, el.absolute, el.source) == ("R", "E", False, 4)
    for d in (hv, el, DispersionData("R", "c", T, [3.0, 3.1], u)):
        dd = d.to_dict()
        assert dd["absolute"] is d.absolute
        e = DispersionData.from_dict(dd)
        assert (e.wave, e.quantity, e.absolute, e.weight) == (d.wave, d.quantity, d.absolute, d.weight)
        assert np.array_equal(e.values, d.values)
    old = hv.to_dict()
    del old["absolute"]                                                    # a file written before the key existed
    assert DispersionData.from_dict(old).absolute is False
    np.savez(tmp_path / "d.npz", obs=np.array({"data": [hv.to_dict(), el.to_dict(), old]}, dtype=object))
    back = as_datasets(np.load(tmp_path / "d.npz", allow_pickle=True)["obs"][()]["data"][:2])
    assert [(d.quantity, d.absolute) for d in back] == [("E", True), ("E", False)]
    assert np.array_equal(back[0].periods, hv.periods) and np.array_equal(back[0].uncer, hv.uncer)
    third = DispersionData.from_dict(np.load(tmp_path / "d.npz", allow_pickle=True)["obs"][()]["data"][2])
    assert third.quantity == "E" and third.absolute is False


def test_column_table_sources_and_period_lists():
    from pysurfinv_amd import _lib
    vals = lambda T: np.full(len(T), 3.5)
    T = [20.0, 10.0, 30.0]
    four = [DispersionData(w, q, T, vals(T), vals(T)) for w, q in (("R", "c"), ("R", "U"), ("L", "c"), ("L", "U"))]
    assert [d.source for d in four] == [0, 1, 2, 3]                        # the existing four do not move
    jd4 = JointData(four)
    assert jd4.col_src.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 and jd4.with_ratio is False
    # identical arrays: order kept; the E set reads the Rayleigh solve
    jd = JointData(four + [DispersionData("R", "E", T, vals(T), vals(T))])
    assert jd.with_ratio is True and jd.solve_periods["R"].tolist() == T and jd.solve_periods["L"].tolist() == T
    assert jd.col_src.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [4] * 3 and jd.col_idx[-3:].tolist() == [0, 1, 2]
    assert jd.kind("R") == jd4.kind("R") == _lib.KIND_RAYLEIGH and jd.kind("L") == _lib.KIND_LOVE
    # differing ones: the ascending union; |chi| is source 5; the kind flags of R are unchanged by the E set
    Tc, Te = [30.0, 10.0, 20.0], [5.0, 20.0, 25.0]
    rc = DispersionData("R", "c", Tc, vals(Tc), vals(Tc))
    jd = JointData([rc, DispersionData("R", "E", Te, vals(Te), vals(Te), weight=2.0, absolute=True)])
    assert jd.solve_periods["R"].tolist() == [5.0, 10.0, 20.0, 25.0, 30.0] and jd.waves == ("R",)
    assert jd.col_src.tolist() == [0, 0, 0, 5, 5, 5] and jd.col_idx.tolist() == [4, 1, 2, 0, 2, 3]
    assert jd.col_w.tolist() == [1.0, 1.0, 1.0, 2.0, 2.0, 2.0] and jd.with_ratio is True and not jd.with_group["R"]
    assert jd.kind("R") == JointData([rc]).kind("R") == _lib.KIND_RAYLEIGH | _lib.PHASE_ONLY
    assert jd.cols.dtype == torch.int32 and jd.cols.tolist() == [[0, 4], [0, 1], [0, 2], [5, 0], [5, 2], [5, 3]]
    # an E set alone is allowed, as a lone U set is
    jd = JointData([DispersionData("R", "E", Te, vals(Te), vals(Te))])
    assert jd.waves == ("R",) and jd.solve_periods["R"].tolist() == Te and jd.col_src.tolist() == [4, 4, 4] and jd.with_ratio
    assert JointData([rc]).with_ratio is False


def test_ellip_misfit_formula_and_failure_rule():
    """Weighted chi2 by hand on a fake forward; signed against absolute on a negative prediction; NaN and inf in a column a
    set reads fail the model, NaN in a column nobody reads does not, chi = 0 and chi < 0 do not."""
    mb = Model1DBatch(CONT)
    Tc, Te = [10.0, 20.0, 30.0], [5.0, 20.0]
    B = 7

    def fake(model, nlay):
        assert model.shape[0] == B
        cR = torch.full((B, 4), 3.5, dtype=torch.float64)                  # R solve: 5, 10, 20, 30
        eR = torch.full((B, 4), 0.9, dtype=torch.float64)
        eR[:, 2] = -0.8                                                    # a negative ellipticity at 20 s
        eR[1, 0] = np.nan                                                  # 1: NaN where the E set reads
        eR[2, 2] = np.inf                                                  # 2: inf where the E set reads
        eR[3, 2] = -np.inf                                                 # 3: -inf
        eR[4, 1] = np.nan                                                  # 4: NaN at 10 s, which no E column reads
        eR[5, 0] = 0.0                                                     # 5: chi = 0: a prediction, not a failure
        eR[6, 0] = -3.0                                                    # 6: chi < 0 likewise
        z = torch.zeros(B, dtype=torch.int32)
        return dict(cR=cR, uR=torch.full((B, 4), np.nan, dtype=torch.float64), cL=None, uL=None, statusR=z, statusL=None, eR=eR)

    p = torch.as_tensor(mb.spec.v0)[None, :].repeat(B, 1)
    expect = {}
    for absolute in (False, True):
        data = [DispersionData("R", "c", Tc, [3.6, np.nan, 3.6], [0.1, 0.1, 0.1]),
                DispersionData("R", "E", Te, [1.0, 0.7], [0.05, 0.1], weight=0.5, absolute=absolute)]
        mc = MetropolisBatch(mb.spec, mb.to_model, device="cpu", forward=fake, data=data)
        assert mc.joint.solve_periods["R"].tolist() == [5.0, 10.0, 20.0, 30.0] and mc.joint.with_ratio
        assert mc.mask.tolist() == [True, False, True, True, True]
        mis, chi, L = mc.misfit(p)
        e20 = 0.8 if absolute else -0.8
        raw = lambda e5: 2 * (0.1 / 0.1) ** 2 + 0.5 * (((1.0 - e5) / 0.05) ** 2 + ((0.7 - e20) / 0.1) ** 2)
        for b, e5 in ((0, 0.9), (4, 0.9), (5, 0.0), (6, 3.0 if absolute else -3.0)):
            r = raw(e5)
            clamped = r if r < 50 else np.sqrt(50 * r)
            assert abs(mis[b].item() - np.sqrt(r / 4)) < 1e-9 * np.sqrt(r / 4), (absolute, b)
            assert abs(chi[b].item() - clamped) < 1e-9 * clamped and abs(L[b].item() - np.exp(-clamped / 2)) < 1e-15, (absolute, b)
        for b in (1, 2, 3):
            assert mis[b].item() == 88888 and chi[b].item() == 88888 and L[b].item() == 0, (absolute, b)
        expect[absolute] = chi[0].item()
    assert expect[True] < expect[False]                                    # |-0.8| is closer to 0.7 than -0.8 is
    # a forward dict without eR is an error, not a silent zero
    mc = MetropolisBatch(mb.spec, mb.to_model, device="cpu", data=data,
                         forward=lambda m, n: {k: v for k, v in fake(m, n).items() if k != "eR"})
    with pytest.raises(ValueError):
        mc.misfit(p)


def test_oracle_ellipticity_of_the_prior_is_solved_and_finite():
    """What the chain test below rests on: the start model and prior draws of CONT are solved at all 19 periods with a
    finite ellipticity (no case has to be left out)."""
    mb = Model1DBatch(CONT)
    mc = MetropolisBatch(mb.spec, mb.to_model, [10.0], [3.0], [0.1], device="cpu", seed=0)
    params = torch.cat([torch.as_tensor(mb.spec.v0)[None, :], mc.reset(40)])
    model, nlay = mb.to_model(params)
    c, r = oracle_ratio(model.numpy(), T_R, None if nlay is None else nlay.numpy())
    assert (c > 0.01).all() and np.isfinite(r).all() and r.min() > 0.5 and r.max() < 2.5


@pytest.mark.parametrize("which", ["Rc_RE", "five"])
def test_short_ellip_chain_on_the_oracle(which):
    """{Rc, RE} and all five sets (per-chain rows, one masked entry per set) on the CPU oracle: every recorded row's misfit
    is the recomputed misfit of its parameters, plain and speculative lock steps."""
    mb = Model1DBatch(CONT)
    four = synthetic_sets(mb)
    if which == "Rc_RE":
        sets = [four[0], ellip_set(mb, T=T_R)]                             # identical period arrays: the order as given
    else:
        sets = four + [ellip_set(mb, T=T_E, absolute=True)]                # the union with T_R and T_U
    C = 3
    rows = []
    for k, d in enumerate(sets):
        v = np.tile(d.values, (C, 1)) * (1 + 0.01 * np.arange(C))[:, None]
        v[1, k % d.values.size] = np.nan
        rows.append(DispersionData(d.wave, d.quantity, d.periods, v, np.tile(d.uncer, (C, 1)), weight=1.0 + 0.5 * k,
                                   absolute=d.absolute))
    jd = JointData(rows)
    assert jd.with_ratio and (jd.col_src >= 4).sum() == sets[-1].periods.size
    mc = MetropolisBatch(mb.spec, mb.to_model, device="cpu", seed=3, forward=oracle_ellip_forward(jd), data=rows)
    for depth in (1, 2):
        tr = mc.run(C, 5, spec_depth=depth)
        assert tr.shape == (C, 5, 3 + mb.spec.n) and (tr[:, 0, 2] == 1).all()
        for k in range(5):
            mis, _, L = mc.misfit(tr[:, k, 3:].contiguous())
            assert torch.equal(mis, tr[:, k, 0]) and torch.equal(L, tr[:, k, 1]), (depth, k)
        assert float(tr[:, :, 0].max()) < 88888                            # every solve succeeds, every ellipticity is finite
    assert mc.n_forward == C * 5 + C * (1 + 3 * 2) + C * 10                # (stacks, not solves) + the re-evaluations


def test_point_npz_round_trip_with_ellipticity(tmp_path):
    from pysurfinv_amd.point import Point, PostPoint
    mb = Model1DBatch(CONT)
    rc, hv = synthetic_sets(mb)[0], ellip_set(mb, absolute=True)
    raw = {"RayPhase": (rc.periods, rc.values, rc.uncer), "RayHV": (hv.periods, hv.values, hv.uncer)}
    p = Point(CONT, data=raw, device="cpu")
    assert [(d.wave, d.quantity, d.absolute) for d in p.data] == [("R", "c", False), ("R", "E", True)]
    fwd = oracle_ellip_forward(JointData(p.data))
    base = p._sampler
    p._sampler = lambda seed=None, **kw: base(seed=seed, forward=fwd, **{k: v for k, v in kw.items() if k == "isgood"})
    arr = p.MCinvMP(outdir=str(tmp_path), pid="e", runN=12, chainL=4, seed=1)
    f = np.load(tmp_path / "e.npz", allow_pickle=True)
    obs = f["obs"][()]
    assert [(d["wave"], d["quantity"], d["absolute"]) for d in obs["data"]] == [("R", "c", False), ("R", "E", True)]
    assert np.array_equal(obs["T"], rc.periods) and np.array_equal(obs["data"][1]["values"], hv.values)
    assert np.array_equal(f["mcTrack"], arr) and (arr[:, 0] < 88888).all()
    q = PostPoint(str(tmp_path / "e.npz"), device=None, _forward=fwd)
    assert [(d.wave, d.quantity, d.absolute) for d in q.data] == [("R", "c", False), ("R", "E", True)]
    assert q.avgMod.misfit == p.misfit(q.avgMod.params)[0]
    p2 = Point(CONT, data={"RayEllip": (hv.periods, hv.values, hv.uncer)}, device="cpu")
    assert p2.data[0].absolute is False and list(p2.obs["T"]) == []
