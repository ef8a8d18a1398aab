"""Joint data (pysurfinv_amd.obsdata): period lists, column table, validation, the torch joint misfit and the sampler on it,
with the CPU oracle standing in for the device solver (no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from settings import CONT, PERIODS                   # noqa: E402
from pysurfinv_amd.layers_batch import Model1DBatch
from pysurfinv_amd.mcmc import MetropolisBatch
from pysurfinv_amd.obsdata import DispersionData, JointData

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_driver.npz"))
T_R = G["trace/periods"]
T_U = np.array([5.0, 6.0, 8.0, 10.0, 12.0, 16.0, 20.0, 30.0])
T_L = np.array([10.0, 15.0, 20.0, 30.0, 40.0])


def oracle_joint_forward(jd):
    """The joint forward hook on the CPU oracle: one solve per wave type with data (kind 2 Rayleigh, kind 1 Love)."""
    from oracle import cport

    def fwd(model, nlay):
        out = dict(cR=None, uR=None, cL=None, uL=None, statusR=None, statusL=None)
        for w, kind in (("R", 2), ("L", 1)):
            if w in jd.solve_periods:
                c, u, st = cport.forward_batch(model.cpu().numpy(), jd.solve_periods[w], kind,
                                               nlay=None if nlay is None else nlay.cpu().numpy(), nthreads=4)
                out["c" + w], out["u" + w] = torch.from_numpy(c.astype(np.float64)), torch.from_numpy(u.astype(np.float64))
                out["status" + w] = torch.from_numpy(st)
        return out
    return fwd


def synthetic_sets(mb, scale=1.01, seed=0):
    """Four data sets observed on the curves of a slightly faster start model (periods differ per set), 1-2 % errors."""
    from oracle import cport
    v = torch.as_tensor(mb.spec.v0)[None, :] * scale
    model, nlay = mb.to_model(v)
    model = model.numpy()
    rng = np.random.default_rng(seed)
    out = []
    for w, q, T, kind in (("R", "c", T_R, 2), ("R", "U", T_U, 2), ("L", "c", T_L, 1), ("L", "U", T_L, 1)):
        c, u, st = cport.forward_batch(model, T, kind, nthreads=2)
        val = (c if q == "c" else u)[0].astype(np.float64)
        unc = np.full(T.size, 0.02 if q == "c" else 0.04)
        out.append(DispersionData(w, q, T, val * (1 + 0.005 * rng.standard_normal(T.size)), unc))
    return out


def test_period_lists_keep_identical_order_and_union_otherwise():
    vals = lambda T: np.full(len(T), 3.5)
    # identical period arrays: that array as given, order kept (a lone Rayleigh-phase set: today's solve)
    Td = [20.0, 10.0, 30.0]
    jd = JointData([DispersionData("R", "c", Td, vals(Td), vals(Td)), DispersionData("R", "U", Td, vals(Td), vals(Td))])
    assert jd.solve_periods["R"].tolist() == Td and jd.waves == ("R",) and jd.with_group["R"]
    assert jd.col_src.tolist() == [0, 0, 0, 1, 1, 1] and jd.col_idx.tolist() == [0, 1, 2, 0, 1, 2]
    one = JointData([DispersionData("R", "c", T_R, G["trace/c_obs"], G["trace/uncer"])])
    assert np.array_equal(one.solve_periods["R"], np.asarray(T_R, np.float32)) and not one.with_group["R"]
    from pysurfinv_amd import _lib
    assert one.kind("R") == _lib.KIND_RAYLEIGH | _lib.PHASE_ONLY
    # differing ones: the ascending float32 union; the column table points at (source, index in that solve)
    Tc, Tu, Tl = [30.0, 10.0, 20.0], [5.0, 10.0, 25.0, 10.000000001], [12.0, 8.0]
    jd = JointData([DispersionData("R", "c", Tc, vals(Tc), vals(Tc), weight=2.0),
                    DispersionData("L", "c", Tl, vals(Tl), vals(Tl)),
                    DispersionData("R", "U", Tu[:3], vals(Tu[:3]), vals(Tu[:3]))])
    assert jd.solve_periods["R"].dtype == np.float32 and jd.solve_periods["R"].tolist() == [5.0, 10.0, 20.0, 25.0, 30.0]
    assert jd.solve_periods["L"].tolist() == [12.0, 8.0]                # alone in its wave type: as given
    assert jd.col_src.tolist() == [0, 0, 0, 2, 2, 1, 1, 1]
    assert jd.col_idx.tolist() == [4, 1, 2, 0, 1, 0, 1, 3]
    assert jd.col_w.tolist() == [2.0, 2.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    o = 0
    for d in jd.datasets:                                               # every column reads its own period of its set's solve
        n = d.periods.size
        assert (jd.col_src[o:o + n] == d.source).all()
        assert np.array_equal(jd.solve_periods[d.wave][jd.col_idx[o:o + n]], d.periods.astype(np.float32))
        o += n
    assert jd.cols.shape == (8, 2) and jd.cols.dtype == torch.int32
    # periods equal in float32 are one period of the union
    jd = JointData([DispersionData("R", "c", [10.0, 20.0], [3.0, 3.1], [0.1, 0.1]),
                    DispersionData("R", "U", [10.000000001, 30.0], [3.0, 3.1], [0.1, 0.1])])
    assert jd.solve_periods["R"].tolist() == [10.0, 20.0, 30.0] and jd.col_idx.tolist() == [0, 1, 0, 2]


def test_validation_errors():
    T = [10.0, 20.0]
    with pytest.raises(ValueError):
        DispersionData("X", "c", T, [3, 3], [0.1, 0.1])
    with pytest.raises(ValueError):
        DispersionData("R", "ellipticity", T, [3, 3], [0.1, 0.1])
    with pytest.raises(ValueError):
        DispersionData("R", "c", T, [3, 3, 3], [0.1, 0.1, 0.1])                  # values vs periods
    with pytest.raises(ValueError):
        DispersionData("R", "c", T, [3, 3], [0.1, 0.1, 0.1])                     # uncer vs values
    with pytest.raises(ValueError):
        DispersionData("R", "c", [0.0, 20.0], [3, 3], [0.1, 0.1])                # non-positive period
    with pytest.raises(ValueError):
        JointData([DispersionData("R", "U", T, [3, 3], [0.1, 0.1]), DispersionData("R", "U", T, [3, 3], [0.1, 0.1])])
    with pytest.raises(ValueError):
        JointData([DispersionData("R", "c", T, np.ones((3, 2)), np.ones((3, 2))),
                   DispersionData("L", "c", T, np.ones((4, 2)), np.ones((4, 2)))])   # per-chain sets of different C
    mb = Model1DBatch(CONT)
    d = [DispersionData("R", "c", T, [3, 3], [0.1, 0.1])]
    with pytest.raises(ValueError):
        MetropolisBatch(mb.spec, mb.to_model, T, [3, 3], [0.1, 0.1], device="cpu", data=d)
    with pytest.raises(ValueError):
        MetropolisBatch(mb.spec, mb.to_model, c_obs=[3, 3], device="cpu", data=d)
    with pytest.raises(ValueError):
        MetropolisBatch(mb.spec, mb.to_model, device="cpu")
    mc = MetropolisBatch(mb.spec, mb.to_model, device="cpu", data=d)
    with pytest.raises(ValueError):
        mc.run_graphed(4, 4)


def test_joint_misfit_formula_and_failure_rule():
    """Weighted chi2, N, clamp and L by hand on a fake joint forward; FAIL for a Love status, a c < 0.01 at an unmasked or a
    masked period (per wave type), a NaN group velocity a U set reads - and not for a NaN U no set reads."""
    mb = Model1DBatch(CONT)
    Tc, Tu, Tl = [10.0, 20.0, 30.0], [5.0, 10.0], [10.0, 20.0]
    cobs = np.array([3.6, np.nan, 3.6])                                   # one masked entry
    data = [DispersionData("R", "c", Tc, cobs, [0.1, 0.1, 0.1]),
            DispersionData("R", "U", Tu, [3.2, 3.2], [0.2, 0.0]),         # uncertainty 0: masked
            DispersionData("L", "c", Tl, [4.0, 4.0], [0.1, 0.1], weight=0.5)]
    B = 6

    def fake(model, nlay):
        assert model.shape[0] == B
        cR = torch.full((B, 4), 3.5, dtype=torch.float64)                # R solve: 5, 10, 20, 30
        uR = torch.full((B, 4), 3.0, dtype=torch.float64)
        cL = torch.full((B, 2), 3.9, dtype=torch.float64)
        uL = torch.full((B, 2), np.nan, dtype=torch.float64)              # no Love U set: never read
        stR, stL = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        stL[1] = 2                                                        # 1: only the Love solve fails
        cR[2, 1] = 0.001                                                  # 2: c < 0.01 at the unmasked 10 s entry
        cR[3, 2] = 0.001                                                  # 3: ... at the masked 20 s entry
        cR[4, 0] = 0.005                                                  # 4: ... at 5 s, a period of the U set only
        uR[5, 0] = np.nan                                                 # 5: a NaN group velocity the U set reads
        return dict(cR=cR, uR=uR, cL=cL, uL=uL, statusR=stR, statusL=stL)
    mc = MetropolisBatch(mb.spec, mb.to_model, device="cpu", forward=fake, data=data)
    assert mc.joint.solve_periods["R"].tolist() == [5.0, 10.0, 20.0, 30.0]
    assert mc.mask.tolist() == [True, False, True, True, False, True, True]
    p = torch.as_tensor(mb.spec.v0)[None, :].repeat(B, 1)
    mis, chi, L = mc.misfit(p)
    chi_raw = 2 * (0.1 / 0.1) ** 2 + (0.2 / 0.2) ** 2 + 0.5 * 2 * (0.1 / 0.1) ** 2        # = 4, below the clamp
    n = 5
    assert abs(mis[0].item() - np.sqrt(chi_raw / n)) < 1e-12
    assert abs(chi[0].item() - chi_raw) < 1e-12 and abs(L[0].item() - np.exp(-chi_raw / 2)) < 1e-15
    for b in range(1, B):
        assert mis[b].item() == 88888 and chi[b].item() == 88888 and L[b].item() == 0, b
    # the clamp: chi2 >= 50 -> sqrt(50 chi2)
    mc.data = [DispersionData("R", "c", Tc, [4.5, 4.5, 4.5], [0.1, 0.1, 0.1], weight=3.0)]
    mis, chi, L = mc.misfit(p[:1].repeat(B, 1))
    raw = 3.0 * 3 * (1.0 / 0.1) ** 2
    assert abs(mis[0].item() - np.sqrt(raw / 3)) < 1e-9 and abs(chi[0].item() - np.sqrt(50 * raw)) < 1e-9
    assert L[0].item() == np.exp(-0.5 * chi[0].item())


def test_short_joint_chain_on_the_oracle():
    """A joint chain (all four sets, per-chain rows with masked entries) on the CPU oracle: every recorded row's misfit is the
    recomputed misfit of its parameters, plain and speculative lock steps."""
    mb = Model1DBatch(CONT)
    sets = synthetic_sets(mb)
    C = 3
    rows = []
    for k, d in enumerate(sets):
        v = np.tile(d.values, (C, 1)) * (1 + 0.01 * np.arange(C))[:, None]
        v[1, k % d.values.size] = np.nan
        rows.append(DispersionData(d.wave, d.quantity, d.periods, v, np.tile(d.uncer, (C, 1)), weight=1.0 + 0.5 * k))
    jd = JointData(rows)
    mc = MetropolisBatch(mb.spec, mb.to_model, device="cpu", seed=3, forward=oracle_joint_forward(jd), data=rows)
    for depth in (1, 2):
        tr = mc.run(C, 5, spec_depth=depth)
        assert tr.shape == (C, 5, 3 + mb.spec.n) and (tr[:, 0, 2] == 1).all()
        for k in range(5):
            mis, _, L = mc.misfit(tr[:, k, 3:].contiguous())
            assert torch.equal(mis, tr[:, k, 0]) and torch.equal(L, tr[:, k, 1]), (depth, k)
        assert float(tr[:, :, 0].max()) < 88888                            # a sensible model: every solve succeeds
    assert mc.n_forward == C * 5 + C * (1 + 3 * 2) + C * 10                # (stacks, not solves) + the re-evaluations


def test_point_npz_round_trip_of_joint_obs(tmp_path):
    from pysurfinv_amd.point import Point, PostPoint
    mb = Model1DBatch(CONT)
    sets = synthetic_sets(mb)
    raw = {"RayPhase": (sets[0].periods, sets[0].values, sets[0].uncer), "RayGroup": (sets[1].periods, sets[1].values, sets[1].uncer),
           "LoveGroup": (sets[3].periods, sets[3].values, sets[3].uncer)}
    p = Point(CONT, data=raw, device="cpu")
    jd = JointData(p.data)
    fwd = oracle_joint_forward(jd)
    base = p._sampler
    p._sampler = lambda seed=None, **kw: base(seed=seed, forward=fwd, **{k: v for k, v in kw.items() if k == "isgood"})
    arr = p.MCinvMP(outdir=str(tmp_path), pid="j", runN=12, chainL=4, seed=1)
    f = np.load(tmp_path / "j.npz", allow_pickle=True)
    obs = f["obs"][()]
    assert set(obs) == {"T", "c", "uncer", "data"} and np.array_equal(obs["T"], sets[0].periods)
    assert [(d["wave"], d["quantity"]) for d in obs["data"]] == [("R", "c"), ("R", "U"), ("L", "U")]
    assert np.array_equal(obs["data"][1]["values"], sets[1].values) and np.array_equal(f["mcTrack"], arr)
    q = PostPoint(str(tmp_path / "j.npz"), device=None, _forward=fwd)
    assert [(d.wave, d.quantity) for d in q.data] == [("R", "c"), ("R", "U"), ("L", "U")]
    assert q.avgMod.misfit == p.misfit(q.avgMod.params)[0]
    # without the Rayleigh-phase set the reference's keys are empty
    p2 = Point(CONT, data=[sets[2]], device="cpu")
    assert list(p2.obs["T"]) == [] and list(p2.obs["c"]) == [] and len(p2.obs["data"]) == 1
    with pytest.raises(ValueError):
        Point(CONT, data=raw, periods=[10.0], vels=[3.0], uncers=[0.1], device="cpu")
