"""The ragged batch of tests/test_eigen_gpu.py: B = 130, Lmax = 70, P = 8, nlay from 3 to 70 - more than two 64-unit tiles
and more than one 64-layer tile, both with a partial last tile - with one water-top stack, one stack that fails validation
and a last period (800 s) that the Love search leaves unsolved on the thin stacks (the Rayleigh fundamental exists at every period here: its unsolved units are the bad stack's).  Layers beyond nlay hold plausible garbage."""
import numpy as np

from pysurfinv_amd import synth

B, LMAX = 130, 70
PERIODS = np.array([6.0, 10.0, 16.0, 25.0, 40.0, 60.0, 100.0, 800.0], np.float32)
WATER, BAD = 5, 77


def ragged_batch():
    m = np.empty((B, 5, LMAX), np.float32)
    m[:] = np.array([7.0, 4.0, 3.0, 5.0, 0.002], np.float32)[None, :, None]      # beyond nlay: never read
    nlay = np.empty(B, np.int32)
    for b in range(B):
        n = 3 + (b * 67) // (B - 1)
        nlay[b] = n
        m[b, :, :n] = synth.synth_models(1, n, seed=100 + b, noise=0.04, monotone=(b % 3 != 0),
                                         total_thickness=60.0 + 2.0 * b)[0]
    w = synth.water_models(1, seed=9)[0]
    nlay[WATER] = w.shape[1]
    m[WATER, :, :w.shape[1]] = w
    m[BAD, 0, 1] = -1.0                                                           # Vp < 0: BADMODEL
    assert nlay.min() == 3 and nlay.max() == LMAX
    return m, nlay, PERIODS
