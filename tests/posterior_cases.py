"""What the tests of the posterior code (tests/test_posterior_*.py, tests/test_predictive_*.py) share: their tracks and depths, the
inputs of the statistics entry, the comparisons, the host files' fixture track and oracle forward hook.  A plain module, not a
conftest."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from settings import CONT                            # noqa: E402
from pysurfinv_amd import posterior                  # noqa: E402
from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402

POST_NPZ = os.path.join(HERE, "golden", "post_trace.npz")
DEV = "cuda:0"
DEPTHS = [0.0, 0.3, 1.7, 5.0, 20.3, 33.3, 47.0, 100.0, 180.0, 197.7, 260.0]
# D > 64 launches a second grid dimension of the profile kernel (a workgroup per slab, point and chunk of 64 depths); only chunk 0
# keeps the parameters' figures and the count of final rows.  65: a one-lane tail in chunk 1.  200: the reference's own use
# (plotVsProfileShaded: 200 depths), here from above the surface to below every model's bottom, a partly filled last chunk.
CHUNK_DEPTHS = {65: np.linspace(0.0, 186.0, 65), 200: np.linspace(-4.0, 261.0, 200), 256: np.linspace(0.05, 199.0, 256)}
# a static ocean structure (water, constant sediment, two-point crust, BottomDepth mantle): the layer kinds CONT lacks
OCEAN_STATIC = {"OceanWater": {"H": 2.5}, "OceanSediment": {"H": [0.4, "abs", 0.2, 0.05], "Vs": [1.0, 0.5, 1.6, 0.05]},
                "OceanCrust": {"H": [6.0, "abs", 0.9, 0.2], "Vs": [[3.25, "abs", 0.3, 0.02], [3.94, "abs", 0.3, 0.02]]},
                "OceanMantle": {"BottomDepth": [200.0, "abs", 30.0, 2.0],
                                "Vs": [[4.4, "abs", 0.4, 0.02], [4.2, "abs", 0.4, 0.02], [4.3, "abs", 0.4, 0.02], [4.5, "abs", 0.4, 0.02]]},
                "Info": {"modelType": "MCInv", "refLayer": False}}


# ------------------------------------------------------------------ comparisons
def _edges(hist):
    vlo, vhi, nb = hist
    return np.arange(nb + 1) * ((vhi - vlo) / nb) + vlo


def _same(a, b):
    return torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0))


def _close(name, a, b, tol):
    a, b = a.detach().cpu().numpy().astype(float), b.detach().cpu().numpy().astype(float)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), name
    both = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(a[~both & ~np.isnan(a)], b[~both & ~np.isnan(b)]), name          # (infinities: the same ones)
    err = float(np.abs(a[both] - b[both]).max()) if both.any() else 0.0
    print(f"PARITY {name}: max |device - reference| = {err:.3e} (bar {tol:g})")
    assert err < tol, (name, err)


# ------------------------------------------------------------------ tracks
def _fixture_track():
    """The reference PostPoint's own trace, [R, 3 + N]."""
    return np.array(np.load(POST_NPZ, allow_pickle=True)["mcTrack"], float)


def _track():
    """The same as a track of one point (the host files)."""
    return _fixture_track()[None]


def _oracle_forward(periods):
    """The CPU oracle as the ``forward=`` hook of a sampler or of run_grid."""
    from oracle import cport

    def fwd(model, nlay):
        c, u, st = cport.forward_batch(model.cpu().numpy(), periods, 2,
                                       nlay=None if nlay is None else nlay.cpu().numpy(), nthreads=2)
        return torch.from_numpy(c.astype(np.float64)), torch.from_numpy(st)
    return fwd


def _random_track(mb, npnt, R, seed, chainL=None):
    """Parameters uniform in the prior box, misfits in 0.5..3 (about a fifth of the rows final), a random accept column."""
    rng = np.random.default_rng(seed)
    N = mb.spec.n
    lo, hi = np.asarray(mb.spec.vmin, float), np.asarray(mb.spec.vmax, float)
    tr = np.zeros((npnt, R, 3 + N))
    tr[:, :, 0] = rng.uniform(0.5, 3.0, (npnt, R))
    tr[:, :, 1] = np.exp(-tr[:, :, 0])
    tr[:, :, 2] = rng.random((npnt, R)) < 0.4
    tr[:, :, 3:] = lo + (hi - lo) * rng.random((npnt, R, N))
    if chainL:
        tr[:, ::chainL, 2] = 1.0
    return tr


def _carry_track(mb):
    """2 points x 2 * 263 rows: a rejected run across the 256-row tile boundary, a chain with nothing accepted but its first row,
    NaN and 88888 misfits."""
    tr = _random_track(mb, 2, 2 * 263, seed=11, chainL=263)
    tr[:, 200:301, 2] = 0.0                       # chain 0: a rejected run across the 256-row tile boundary
    tr[:, 264:, 2] = 0.0                          # chain 1: nothing accepted but its first row
    tr[0, [5, 250, 300], 0] = np.nan
    tr[1, [0, 17, 400], 0] = 88888.0
    tr[0, 255, 0] = 0.45; tr[0, 256, 0] = 0.46    # final rows on either side of the boundary, both inside the rejected run
    return tr


def _slab_plus_one_track(mb):
    """1 point x SLAB_ROWS + 1 rows: the lone row of the second slab is rejected, final, and holds the minimum."""
    R = posterior.SLAB_ROWS + 1
    tr = _random_track(mb, 1, R, seed=12)
    tr[0, R - 60:, 2] = 0.0                       # the last row of the first slab and the lone row of the second: rejected
    tr[0, R - 1, 0] = 0.4                         # ... and that lone row is final, and holds the minimum
    return tr


SELECTIONS = {"tmc": dict(), "raw": dict(true_markov_chain=False), "prefix": dict(chainL=263, prefix=100)}
SLAB_BOUNDARY_SELECTIONS = [dict(), dict(true_markov_chain=False), dict(chainL=posterior.SLAB_ROWS + 300, prefix=posterior.SLAB_ROWS + 200)]


def _slab_boundary_track(mb):
    """1 point x SLAB_ROWS + 300 rows: a rejected run across the slab boundary, final rows on either side, the minimum behind it."""
    S = posterior.SLAB_ROWS
    tr = _random_track(mb, 1, S + 300, seed=21)
    tr[0, 0, 2] = 1.0
    tr[0, S - 40:S + 50, 2] = 0.0                                        # a rejected run across the slab boundary
    tr[0, S - 1, 0] = 0.45; tr[0, S, 0] = 0.46; tr[0, S + 7, 0] = 0.4    # final rows on either side, the minimum behind it
    return tr


def _local_case(name):
    """(setting, local keys, local-information table, rows, depths) of the per-point-constants cases "cont" and "ocean"."""
    setting, keys, table = ((CONT, ["topo", "Mantle.H"], [[-1.0, 152.0], [0.7, 160.0], [2.2, 171.5]]) if name == "cont" else
                            (OCEAN_STATIC, ["topo"], [[-3.0], [0.0], [1.5]]))
    return setting, keys, table, np.array([2, 0, 1]), [-2.0, -1.4, 0.0, 0.8, 2.6, 3.4, 9.0, 12.0, 60.0, 155.0, 172.0, 199.0, 228.0]


# ------------------------------------------------------------------ the statistics entry
SLAB = posterior.PRED_SLAB_ROWS
P_A, NBINS_A = 70, 37                 # two chunks of 64 columns, the second ragged
LENS_A = [0, 5, SLAB + 300]           # an empty point, one wavefront's worth, a slab boundary (two workgroups per point and chunk)


def _stats_inputs(seed=3):
    rng = np.random.default_rng(seed)
    total = sum(LENS_A)
    centre = np.linspace(0.5, 4.5, P_A)                                  # the columns live on different scales
    pred = (centre[None, :] + 0.2 * rng.standard_normal((total, P_A))).astype(np.float32)
    w = rng.integers(0, 6, total).astype(np.int32)
    failed = (rng.random(total) < 0.1).astype(np.uint8)
    bad = rng.random((total, P_A))
    pred[bad < 0.01] = np.nan
    pred[(bad >= 0.01) & (bad < 0.015)] = np.inf
    pred[(bad >= 0.015) & (bad < 0.02)] = -np.inf
    pred[:, P_A - 1] = np.nan                                            # a column in which no row counts
    w[:5] = [2, 0, 1, 5, 3]; failed[:5] = [0, 0, 1, 0, 0]                # the five rows of point 1
    pred[3, 6] = np.nan
    offsets = np.concatenate([[0], np.cumsum(LENS_A)]).astype(np.int32)
    return pred, failed, w, offsets, (centre - 0.3, centre + 0.35, NBINS_A)


def _empty_list_inputs():
    """(pred, failed, w, offsets, hist) of two points with an empty list, device tensors."""
    return (torch.empty((0, 4), dtype=torch.float32, device=DEV), None, torch.empty(0, dtype=torch.int32, device=DEV),
            torch.zeros(3, dtype=torch.int32, device=DEV), (np.zeros(4), np.ones(4), 3))
