"""Posterior Vs(z) profiles, the statement (pysurfinv_amd.posterior.posterior_reference) pinned to the reference's PostPoint:
tests/golden/ref_post.npz holds its Vs at depth (37 depths x 43 final rows) for the trace of tests/golden/post_trace.npz.
No GPU here; the device entry is held against this statement in tests/test_posterior_gpu.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "golden")]
from settings import CONT, PERIODS                   # noqa: E402
from posterior_cases import POST_NPZ, _edges, _oracle_forward, _track   # noqa: E402
from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402
from pysurfinv_amd import posterior                  # noqa: E402

GP = np.load(os.path.join(HERE, "golden", "ref_post.npz"), allow_pickle=True)
G = np.load(os.path.join(HERE, "golden", "ref_driver.npz"))
HIST = (1.0, 5.0, 400)


@pytest.mark.parametrize("tmc,key", [(True, "tmc"), (False, "raw")])
def test_reference_statement_matches_reference_postpoint(tmc, key):
    mb = Model1DBatch(CONT)
    r = posterior.posterior_reference(mb, torch.from_numpy(_track()), GP["zdeps"], true_markov_chain=tmc, hist=HIST)
    vz = GP[f"{key}/values_z"]
    assert vz.shape == (37, 43) and np.isfinite(vz).all()
    assert float(r["min_misfit"][0]) == float(GP[f"{key}/min_misfit"]) and float(r["thres"][0]) == float(GP[f"{key}/thres"])
    _, _, _, final, _ = posterior.select_reference(_track(), tmc)
    assert np.array_equal(final[0], GP[f"{key}/accFinal"]) and int(r["n_final"][0]) == 43
    assert np.abs(r["pmean"][0].numpy() - GP[f"{key}/avg_params"]).max() < 1e-12
    assert np.abs(r["vs_mean"][0].numpy() - vz.mean(axis=1)).max() < 1e-9
    assert np.abs(r["vs_std"][0].numpy() - vz.std(axis=1)).max() < 1e-9
    assert (r["count"][0].numpy() == 43).all()
    assert np.abs(r["vs_min"][0].numpy() - vz.min(axis=1)).max() < 1e-9
    assert np.abs(r["vs_max"][0].numpy() - vz.max(axis=1)).max() < 1e-9
    # histogram: exact, which is fair while no value sits on an edge
    edges = _edges(HIST)
    assert np.abs(vz[:, :, None] - edges[None, None, :]).min() > 1e-9
    for d in range(37):
        assert np.array_equal(r["hist"][0, d].numpy(), np.histogram(vz[d], edges)[0])
    assert int(r["below"].sum()) == 0 and int(r["above"].sum()) == 0
    # quantiles from the histogram: inside the bin that holds the sample quantile, ordered
    q = r["quantiles"][0].numpy()
    assert q.shape == (37, 3) and (np.diff(q, axis=1) >= 0).all()
    assert np.abs(q[:, 1] - np.median(vz, axis=1)).max() < 2 * 0.01 + 1e-12


def test_depths_outside_every_model():
    mb = Model1DBatch(CONT)
    r = posterior.posterior_reference(mb, torch.from_numpy(_track()), [-1.0, 0.5, 100.0, 250.0])
    cnt = r["count"][0].numpy()
    assert list(cnt) == [0, 43, 43, 0]
    m = r["vs_mean"][0].numpy()
    assert np.isnan(m[[0, 3]]).all() and np.isfinite(m[[1, 2]]).all()
    assert np.isnan(r["vs_std"][0].numpy()[[0, 3]]).all() and np.isnan(r["vs_min"][0].numpy()[[0, 3]]).all()


def test_prefix_rule_is_a_mask_on_the_misfits():
    mb = Model1DBatch(CONT)
    tr = _track()
    a = posterior.posterior_reference(mb, torch.from_numpy(tr), GP["zdeps"], chainL=80, prefix=40, hist=HIST)
    masked = tr.copy()
    masked[0, np.arange(240) % 80 >= 40, 0] = np.inf
    b = posterior.posterior_reference(mb, torch.from_numpy(masked), GP["zdeps"], hist=HIST)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(torch.nan_to_num(a[k].double(), nan=-7.0), torch.nan_to_num(b[k].double(), nan=-7.0)), k
    assert 1 <= int(a["n_final"][0]) < 240
    with pytest.raises(ValueError):
        posterior.posterior_reference(mb, torch.from_numpy(tr), GP["zdeps"], chainL=80, prefix=81)
    with pytest.raises(ValueError):
        posterior.posterior_reference(mb, torch.from_numpy(tr), GP["zdeps"], chainL=70, prefix=10)


def test_postpoint_profile_on_the_host():
    from pysurfinv_amd.point import PostPoint
    for tmc, key in ((True, "tmc"), (False, "raw")):
        p = PostPoint(POST_NPZ, trueMarkovChain=tmc, device=None)
        pr = p.profile(GP["zdeps"], hist=HIST)
        vz = GP[f"{key}/values_z"]
        assert np.abs(pr["std"] - vz.std(axis=1)).max() < 1e-9
        assert np.abs(pr["std"] - p._loadValues(zdeps=GP["zdeps"]).std(axis=1)).max() < 1e-9
        assert np.abs(pr["mean"] - vz.mean(axis=1)).max() < 1e-9 and pr["n_final"] == 43 and pr["thres"] == p.thres
        assert pr["hist"].shape == (37, 400) and pr["quantiles"].shape == (37, 3)


def test_device_route_refuses_without_a_device_or_descriptor():
    from pysurfinv_amd import _lib
    from settings import OCEAN
    from settings_therm import HYBRID_STATIC
    mb = Model1DBatch(CONT)
    with pytest.raises(_lib.SurfdispError):                               # a supported model, but no device
        posterior.posterior_profiles(mb, torch.from_numpy(_track()), GP["zdeps"])
    for bad in (OCEAN, HYBRID_STATIC):                                    # no static structure; a thermal layer: said before the device is looked at
        mbb = Model1DBatch(bad)
        with pytest.raises(ValueError):
            posterior.posterior_profiles(mbb, torch.zeros((1, 4, 3 + mbb.spec.n), dtype=torch.float64), GP["zdeps"])


def test_quantile_formula():
    h = torch.tensor([[0, 2, 2, 0], [0, 0, 0, 0]], dtype=torch.int32)
    q = posterior.quantiles_from_hist(h, 1.0, 3.0, (0.0, 0.25, 0.5, 1.0)).numpy()
    # bins of width 0.5 on [1, 3): the two middle ones hold 2 each
    assert np.allclose(q[0], [1.5, 1.75, 2.0, 2.5]) and np.isnan(q[1]).all()


# ------------------------------------------------------------------ run_grid(..., profile_depths=...), 2 gloo ranks on CPU
NPTS, CHAINS, CHAINL = 5, 2, 4
ZD = [0.5, 3.0, 20.0, 60.0, 150.0, 400.0]


def _obs():
    c = np.tile(G["trace/c_obs"], (NPTS, 1)) * (1 + 0.002 * np.arange(NPTS)[:, None])
    c[3, 5] = np.nan
    return c, np.tile(G["trace/uncer"], (NPTS, 1))


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pysurfinv_amd import grid
    per = G["trace/periods"].astype(np.float32)
    c, u = _obs()
    out = []
    for zd in (ZD, None):
        r = grid.run_grid(Model1DBatch(CONT), np.arange(NPTS) * 0.5 + 230, np.arange(NPTS) * 0.25 + 44, per, c, u,
                          CHAINS, CHAINL, outdir=None, rank=rank, world=world, device="cpu", seed=1,
                          forward=_oracle_forward(per), profile_depths=zd)
        out.append((sorted(r.keys()), r["points"], r["mcTrack"], r.get("profiles"), r["summaries"]))
    q.put((rank, out))
    dist.barrier(); dist.destroy_process_group()


def test_two_rank_grid_carries_every_points_profile():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn"); q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs: p.start()
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda t: t[0])
    for p in procs: p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    parent_keys = sorted(["points", "mcTrack", "summaries", "columns", "elapsed", "elapsed_write", "report"])
    mb = Model1DBatch(CONT)
    for rank, (with_p, without) in res:
        keys, (lo, hi), tracks, prof, summ = with_p
        assert keys == sorted(parent_keys + ["profiles"])
        assert without[0] == parent_keys and without[3] is None
        assert np.array_equal(without[4], summ, equal_nan=True)            # the same chains, the same summaries
        assert sorted(prof) == ["count", "max", "mean", "min", "std", "zdeps"]
        for k in ("count", "mean", "std", "min", "max"):
            assert prof[k].shape == (NPTS, len(ZD))                         # every rank holds all points
        ref = posterior.posterior_reference(mb, torch.from_numpy(tracks), ZD)
        for k, rk in (("mean", "vs_mean"), ("std", "vs_std"), ("min", "vs_min"), ("max", "vs_max")):
            a, b = prof[k][lo:hi], ref[rk].numpy()
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(a - b)) < 1e-12
        assert np.array_equal(prof["count"][lo:hi], ref["count"].numpy())
        assert (prof["count"][:, -1] == 0).all() and (prof["count"][:, 1] >= 1).all()
    assert np.array_equal(res[0][1][0][3]["mean"], res[1][1][0][3]["mean"], equal_nan=True)
