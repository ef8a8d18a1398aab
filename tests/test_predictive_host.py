"""Posterior predictive curves, the statement (pysurfinv_amd.posterior.predictive_reference) on the reference's own fixture track
(tests/golden/post_trace.npz, setting CONT, its obs): the predicted Rayleigh phase velocities of the 43 final rows' models, with
the CPU oracle as the forward solve through the sampler's ``forward=`` hook.  No GPU here; the device route is held against this
statement in tests/test_predictive_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "golden")]
from settings import CONT                            # noqa: E402
from posterior_cases import POST_NPZ, _oracle_forward, _track   # noqa: E402
from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402
from pysurfinv_amd.mcmc import MetropolisBatch       # noqa: E402
from pysurfinv_amd import posterior, _lib            # noqa: E402

GP = np.load(os.path.join(HERE, "golden", "ref_post.npz"), allow_pickle=True)
SRC = np.load(POST_NPZ, allow_pickle=True)
OBS = SRC["obs"][()]
PERIODS = np.asarray(OBS["T"], np.float32)
HIST = (2.5, 4.5, 200)


def _sampler(c_obs=None, uncer=None):
    mb = Model1DBatch(CONT)
    return mb, MetropolisBatch(mb.spec, mb.to_model, OBS["T"], OBS["c"] if c_obs is None else c_obs,
                               OBS["uncer"] if uncer is None else uncer, device="cpu", forward=_oracle_forward(PERIODS))


def _curve(mb, params):
    """The oracle's curve of ONE parameter vector, solved alone."""
    model, nlay = mb.to_model(torch.as_tensor(np.asarray(params, float)[None]))
    c, st = _oracle_forward(PERIODS)(model, nlay)
    assert int(st[0]) == 0
    return c[0].numpy()


@pytest.mark.parametrize("tmc,key", [(True, "tmc"), (False, "raw")])
def test_reference_statement_on_the_fixture_track(tmc, key):
    mb, mc = _sampler()
    tr = _track()
    r = posterior.predictive_reference(mc, torch.from_numpy(tr), true_markov_chain=tmc, hist=HIST)
    P = PERIODS.size
    assert int(r["n_final"][0]) == 43 and int(r["n_failed"][0]) == 0 and (r["count"][0].numpy() == 43).all()
    assert float(r["min_misfit"][0]) == float(GP[f"{key}/min_misfit"]) and float(r["thres"][0]) == float(GP[f"{key}/thres"])
    paras = GP[f"{key}/MCparas"]                                         # the reference PostPoint's parameters, row by row
    imin = int(r["imin"][0])
    assert np.array_equal(r["min_pred"][0].numpy(), _curve(mb, paras[imin]))
    # brute force: one solve per final row, no batching
    final = np.asarray(GP[f"{key}/accFinal"], bool)
    curves = np.array([_curve(mb, paras[i]) for i in np.nonzero(final)[0]])
    assert curves.shape == (43, P)
    for k, want in (("pred_mean", curves.mean(axis=0)), ("pred_std", curves.std(axis=0)), ("pred_min", curves.min(axis=0)),
                    ("pred_max", curves.max(axis=0))):
        assert np.abs(r[k][0].numpy() - want).max() < 1e-12, k
    fit = (curves.mean(axis=0) - np.asarray(OBS["c"], float)) / np.asarray(OBS["uncer"], float)
    assert np.abs(r["fit"][0].numpy() - fit).max() < 1e-9
    # weights, derived here from the selection: they sum to n_final, and the weighted figures of the distinct rows are the same
    _, _, _, fin, src = posterior.select_reference(tr, tmc)
    assert np.array_equal(fin[0], final)
    weight = np.bincount(src[0][fin[0]], minlength=tr.shape[1])
    assert weight.sum() == 43 and int(r["n_sources"][0]) == int((weight > 0).sum())
    assert (int(r["n_sources"][0]) < 43) == tmc                          # rejected final rows share their source
    rows = np.nonzero(weight)[0]
    distinct = np.array([_curve(mb, tr[0, i, 3:]) for i in rows])
    wmean = (weight[rows, None] * distinct).sum(axis=0) / 43
    assert np.abs(wmean - r["pred_mean"][0].numpy()).max() < 1e-12
    wstd = np.sqrt((weight[rows, None] * (distinct - wmean) ** 2).sum(axis=0) / 43)
    assert np.abs(wstd - r["pred_std"][0].numpy()).max() < 1e-12
    # the recorded misfits are the reference solver's: the oracle reproduces them to its parity bar
    assert 0.0 <= float(r["misfit_dev"][0]) < 1e-3
    # histogram per column
    edges = np.arange(HIST[2] + 1) * ((HIST[1] - HIST[0]) / HIST[2]) + HIST[0]
    assert np.abs(curves[:, :, None] - edges[None, None, :]).min() > 1e-9
    for c in range(P):
        assert np.array_equal(r["hist"][0, c].numpy(), np.histogram(curves[:, c], edges)[0])
    assert int(r["below"].sum()) == 0 and int(r["above"].sum()) == 0
    q = r["quantiles"][0].numpy()
    assert q.shape == (P, 3) and (np.diff(q, axis=1) >= 0).all()
    assert np.abs(q[:, 1] - np.median(curves, axis=0)).max() < 2 * 0.01 + 1e-12


def test_failed_rows_masked_observations_and_ranges_per_column():
    mb = Model1DBatch(CONT)
    P = PERIODS.size
    oracle = _oracle_forward(PERIODS)

    def fwd(model, nlay):                                                # every stack faster than 3.17 km/s at the first period fails:
        c, st = oracle(model, nlay)                                      # about half of the final rows (3.148 .. 3.192, mean 3.170)
        st = st.clone(); st[c[:, 0] > 3.17] = 1
        return c, st
    c_obs = np.asarray(OBS["c"], float).copy(); c_obs[2] = np.nan        # a masked observation
    mc = MetropolisBatch(mb.spec, mb.to_model, OBS["T"], c_obs, OBS["uncer"], device="cpu", forward=fwd)
    tr = _track()
    vlo, vhi = np.linspace(2.0, 3.0, P), np.linspace(4.0, 5.0, P)
    r = posterior.predictive_reference(mc, torch.from_numpy(tr), hist=(vlo, vhi, 50), max_batch=7)
    one = posterior.predictive_reference(mc, torch.from_numpy(tr), hist=(vlo, vhi, 50))
    for k in r:                                                          # the slices of max_batch rows do not show
        assert torch.equal(torch.nan_to_num(r[k].double(), nan=-7.0), torch.nan_to_num(one[k].double(), nan=-7.0)), k
    nf = int(r["n_failed"][0])
    assert 0 < nf < 43 and (r["count"][0].numpy() == 43 - nf).all()
    assert np.isnan(r["fit"][0, 2].item()) and np.isfinite(np.delete(r["fit"][0].numpy(), 2)).all()
    h = r["hist"][0].numpy()
    assert h.shape == (P, 50) and ((h.sum(axis=1) + r["below"][0].numpy() + r["above"][0].numpy()) == 43 - nf).all()
    assert float(r["misfit_dev"][0]) > 1e4                               # a failed source row: 88888 against its record


def test_postpoint_predictive_on_the_host():
    from pysurfinv_amd.point import PostPoint
    p = PostPoint(POST_NPZ, device=None, _forward=_oracle_forward(PERIODS))
    pr = p.predictive(hist=HIST)
    _, mc = _sampler()
    r = posterior.predictive_reference(mc, torch.from_numpy(_track()), hist=HIST)
    assert pr["n_final"] == 43 and pr["thres"] == p.thres and pr["n_sources"] == int(r["n_sources"][0])
    for k, rk in (("mean", "pred_mean"), ("std", "pred_std"), ("min", "pred_min"), ("max", "pred_max"), ("min_pred", "min_pred"),
                  ("fit", "fit"), ("hist", "hist"), ("quantiles", "quantiles")):
        assert np.array_equal(pr[k], r[rk][0].numpy()), k
    with pytest.raises(ValueError):
        PostPoint(POST_NPZ, device=None).predictive()                    # neither a device nor a forward hook


def test_device_route_refuses_without_a_device():
    _, mc = _sampler()
    tr = torch.from_numpy(_track())
    with pytest.raises(ValueError, match="forward"):                     # the hook has no device solve
        posterior.posterior_predictive(mc, tr)
    mb = Model1DBatch(CONT)
    plain = MetropolisBatch(mb.spec, mb.to_model, OBS["T"], OBS["c"], OBS["uncer"], device="cpu")
    with pytest.raises(_lib.SurfdispError):                              # a sampler that could solve, but no device track
        posterior.posterior_predictive(plain, tr)
    with pytest.raises(ValueError):
        posterior.posterior_predictive(plain, tr.numpy())


@pytest.mark.parametrize("fn", [posterior.predictive_reference, posterior.posterior_predictive])
def test_shape_checks(fn):
    mb = Model1DBatch(CONT)
    N, P = mb.spec.n, PERIODS.size
    mc = MetropolisBatch(mb.spec, mb.to_model, OBS["T"], OBS["c"], OBS["uncer"], device="cpu")
    tr = torch.from_numpy(_track())
    per_point = MetropolisBatch(mb.spec, mb.to_model, OBS["T"], np.tile(OBS["c"], (3, 1)), np.tile(OBS["uncer"], (3, 1)), device="cpu")
    bad = [dict(track=tr[0]), dict(track=tr[:, :, :-1]), dict(track=torch.zeros((1, 0, 3 + N), dtype=torch.float64)),
           dict(obs_rows=[0, 0]), dict(sampler=per_point), dict(sampler=per_point, obs_rows=[3]),
           dict(sampler=per_point, obs_rows=[-1]),
           dict(chainL=80, prefix=81), dict(chainL=70, prefix=10), dict(prefix=10), dict(max_batch=0),
           dict(hist=(3.0, 3.0, 10)), dict(hist=(2.0, 4.0, 0)), dict(hist=(np.zeros(P + 1), 5.0, 10)),
           dict(hist=(np.full(P, np.nan), 5.0, 10))]
    for kw in bad:
        a = dict(sampler=mc, track=tr)
        a.update(kw)
        with pytest.raises(ValueError):
            fn(a.pop("sampler"), a.pop("track"), **a)
