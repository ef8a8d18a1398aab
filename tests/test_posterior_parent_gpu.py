"""The posterior device code (csrc/surfdisp_post.hip, csrc/surfdisp_pred.hip, their shared pieces in csrc/surfdisp_post_common.h,
the three C entries and their Python wrappers) after its consolidation must compute, BYTE FOR BYTE, what the commit before it
computed: the results are fp64 sums in an order the input alone fixes, plus integer atomics, so a differing byte is changed
arithmetic.

tests/golden/posterior_parent.npz holds every tensor of every returned dict of ``run_parent_cases`` below (inputs:
tests/posterior_cases.py), recorded on the GPU from a checkout of the parent commit with its own library
(scripts/record_posterior_parent.py ROOT) - never from the code under test.  The cases are the smallest that reach every shared
piece: profiles of the carry track (a tile boundary, NaN and 88888 misfits) under three selections, of a track one row past a
slab at 65 depths (two slabs x two depth chunks, a one-lane tail), without a histogram, and of the ocean model with per-point
constants (aux slots, a BottomDepth layer); the sources of the carry track and of the slab-boundary track under three
selections each; the statistics of 70 columns (two chunks, the second ragged) over lists of 0, 5 and a slab + 300 rows with
per-column ranges, the same without failed array and histogram, and an empty list."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import posterior_cases as pc                         # noqa: E402
from pysurfinv_amd import posterior                  # noqa: E402
from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402

HIST = (1.0, 5.0, 40)
CASES = ([f"profiles_carry_{s}" for s in pc.SELECTIONS] + ["profiles_slab_plus_one", "profiles_one_depth", "profiles_ocean"]
         + [f"sources_carry_{s}" for s in pc.SELECTIONS] + [f"sources_slab_{s}" for s in pc.SELECTIONS]
         + ["statistics", "statistics_plain", "statistics_empty"])


def run_parent_cases():
    """Every case of CASES through the ``pysurfinv_amd`` this process imported, on the GPU.  Returns {"<case>/<key>": numpy array}
    of every tensor of every returned dict."""
    mbc = Model1DBatch(pc.CONT)
    mb = Model1DBatch(pc.CONT, device=pc.DEV)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(pc.DEV)
    carry, res = dev(pc._carry_track(mbc)), {}
    for s, sel in pc.SELECTIONS.items():
        res[f"profiles_carry_{s}"] = posterior.posterior_profiles(mb, carry, pc.DEPTHS, hist=HIST, **sel)
        res[f"sources_carry_{s}"] = posterior.posterior_sources(carry, **sel)
    res["profiles_slab_plus_one"] = posterior.posterior_profiles(mb, dev(pc._slab_plus_one_track(mbc)), pc.CHUNK_DEPTHS[65], hist=HIST)
    res["profiles_one_depth"] = posterior.posterior_profiles(mb, carry, [20.3], hist=None)
    setting, keys, table, rows, zd = pc._local_case("ocean")
    ocean = Model1DBatch(setting, device=pc.DEV, local_keys=keys).set_local_info(table)
    track = pc._random_track(Model1DBatch(setting, local_keys=keys), 3, 300, seed=14)
    res["profiles_ocean"] = posterior.posterior_profiles(ocean, dev(track), zd, rows=rows, hist=HIST)
    slab = dev(pc._slab_boundary_track(mbc))
    for s, sel in zip(pc.SELECTIONS, pc.SLAB_BOUNDARY_SELECTIONS):
        res[f"sources_slab_{s}"] = posterior.posterior_sources(slab, **sel)
    pred, failed, w, offsets, hist = pc._stats_inputs()
    res["statistics"] = posterior.predictive_statistics(dev(pred), dev(failed), dev(w), dev(offsets), hist=hist)
    res["statistics_plain"] = posterior.predictive_statistics(dev(pred), None, dev(w), dev(offsets))
    pred, failed, w, offsets, hist = pc._empty_list_inputs()
    res["statistics_empty"] = posterior.predictive_statistics(pred, failed, w, offsets, hist=hist)
    torch.cuda.synchronize()
    assert sorted(res) == sorted(CASES)
    return {f"{case}/{k}": v.cpu().numpy() for case, r in res.items() for k, v in r.items()}


@pytest.fixture(scope="module")
def parent():
    return dict(np.load(os.path.join(HERE, "golden", "posterior_parent.npz")))


@pytest.fixture(scope="module")
def here():
    return run_parent_cases()


def test_cases_are_the_recorded_ones(parent):
    assert sorted({k.split("/")[0] for k in parent}) == sorted(CASES)
    # the comparison below is about real figures: final rows in every selection, counted values, filled bins, quantiles
    for case in CASES:
        if not case.startswith("statistics"):
            assert (parent[case + "/n_final"] >= 1).all(), case
    for s in pc.SELECTIONS:
        assert parent[f"profiles_carry_{s}/hist"].sum() > 0 and np.isfinite(parent[f"profiles_carry_{s}/quantiles"]).any()
        assert parent[f"sources_slab_{s}/weight"].sum() == parent[f"sources_slab_{s}/n_final"].sum()
    assert "hist" not in {k.split("/")[1] for k in parent if k.startswith(("profiles_one_depth/", "statistics_plain/"))}
    assert parent["statistics/hist"].shape == (3, pc.P_A, pc.NBINS_A) and parent["statistics/count"][2].max() > 5000
    assert parent["statistics_empty/count"].sum() == 0 and np.isnan(parent["statistics_empty/pred_mean"]).all()


@pytest.mark.parametrize("case", CASES)
def test_bytes_equal_the_parent_commit(parent, here, case):
    want = {k: v for k, v in parent.items() if k.startswith(case + "/")}
    got = {k: v for k, v in here.items() if k.startswith(case + "/")}
    assert sorted(got) == sorted(want)
    bad = []
    for k, w in want.items():
        g = got[k]
        if g.dtype != w.dtype or g.shape != w.shape:
            bad.append(f"{k}: {g.dtype} {g.shape} against {w.dtype} {w.shape}")
        elif g.tobytes() != w.tobytes():
            words = lambda a: np.frombuffer(a.tobytes(), np.uint8).reshape(-1, a.itemsize)
            bad.append(f"{k}: {int((words(g) != words(w)).any(axis=1).sum())} of {g.size} words differ")
    assert not bad, "differs from the parent commit's bytes: " + "; ".join(bad)
