"""The host statement of the damped least-squares step (pysurfinv_amd.linearized.lsq_step_reference) against an augmented
least-squares problem, and the argument errors of the linearised inversion.  CPU only."""
import numpy as np
import pytest

from lsq_cases import _problem
from pysurfinv_amd import _lib, linearized, synth
from pysurfinv_amd.obsdata import DispersionData


@pytest.mark.parametrize("N,n", [(1, 1), (7, 3), (40, 17), (100, 64)])
def test_reference_step_solves_the_augmented_least_squares_problem(N, n):
    """min ||W^1/2 (G d - r)||^2 + alpha ||Q^1/2 D (x0 + d)||^2 + lam ||d||^2 as one stacked lstsq problem: both sides
    float64, cond(A) <= 1e4 (asserted), so the normal equations lose at most cond(A) eps ~ 1e-12 against the QR-based
    lstsq: the bar of relative 1e-9 leaves three digits."""
    G, r, w, x0, alpha, Q, lam = _problem(N, n, seed=100 + n)
    A, g = linearized.normal_equations(G, r, w, x0, alpha, Q, lam)
    assert np.linalg.cond(A) <= 1e4
    D = np.zeros((max(n - 1, 0), n))
    for k in range(n - 1):
        D[k, k], D[k, k + 1] = -1.0, 1.0
    sq = np.sqrt(alpha * Q)[:, None] * D
    lhs = np.vstack([np.sqrt(w)[:, None] * G, sq, np.sqrt(lam) * np.eye(n)])
    rhs = np.concatenate([np.sqrt(w) * r, -sq @ x0, np.zeros(n)])
    want = np.linalg.lstsq(lhs, rhs, rcond=None)[0]
    got = linearized.lsq_step_reference(G, r, w, x0, alpha, Q, lam)
    assert got["flag"] == 0
    assert np.abs(got["delta"] - want).max() <= 1e-9 * np.abs(want).max()
    assert got["misfit"] == pytest.approx((w * r * r).sum(), rel=1e-14)
    assert got["roughness"] == pytest.approx((Q * np.diff(x0) ** 2).sum(), rel=1e-14, abs=0)
    # the predicted objective is the stacked problem's residual without the damping rows
    t = lhs[:N + max(n - 1, 0)] @ want - rhs[:N + max(n - 1, 0)]
    assert got["predicted"] == pytest.approx(t @ t, rel=1e-9)


def test_reference_step_flags():
    G, r, w, x0, alpha, Q, lam = _problem(5, 8, seed=3)
    out = linearized.lsq_step_reference(G[:0], r[:0], w[:0], x0, alpha, Q, lam)
    assert out["flag"] == 1 and not out["delta"].any()
    out = linearized.lsq_step_reference(G, r, w, x0, 0.0, Q, 0.0)            # N < n, no regularisation: singular
    assert out["flag"] == 2 and not out["delta"].any() and np.isfinite(out["predicted"])


def test_consecutive_weights_run_over_free_layers():
    free = np.array([0, 1, 1, 0, 0, 1, 1], bool)
    Q = np.array([9.0, 2.0, 3.0, 0.5, 4.0, 7.0])
    idx, w = linearized.consecutive_weights(free, Q)
    assert idx.tolist() == [1, 2, 5, 6] and w.tolist() == [2.0, 0.5, 7.0]
    vp, rho = linearized.group_slopes(["water", "sediment", "crust", "mantle"])
    assert vp.tolist() == [0.0, 1.23, 1.8, 1.76] and rho[3] == pytest.approx(1 / 4.5)


def _data(per, **kw):
    v = np.full(per.size, 3.5)
    return DispersionData(kw.get("wave", "R"), kw.get("quantity", "c"), per, v, 0.01 * v)


def test_argument_errors_need_no_gpu():
    per = synth.default_periods(6)
    model = synth.synth_models(3, 8, seed=1)
    big = np.repeat(synth.synth_models(2, 10, seed=1), 20, axis=2)           # 200 layers, every one free
    with pytest.raises(ValueError, match="at most 128"):
        linearized.LinearizedBatch(big, [_data(per)])
    with pytest.raises(ValueError, match="vp_slope"):
        linearized.LinearizedBatch(model, [_data(per)], vp_slope=np.zeros(7))
    with pytest.raises(ValueError, match="rho_slope"):
        linearized.LinearizedBatch(model, [_data(per)], rho_slope=np.zeros((2, 8)))
    with pytest.raises(ValueError, match="Q"):
        linearized.LinearizedBatch(model, [_data(per)], Q=np.ones(8))
    with pytest.raises(ValueError, match="ellipticity"):
        linearized.LinearizedBatch(model, [dict(wave="L", quantity="E", periods=per, values=per, uncer=per)])
    with pytest.raises(ValueError, match="duplicate"):
        linearized.LinearizedBatch(model, [_data(per), _data(per)])
    with pytest.raises(ValueError, match="free"):
        linearized.LinearizedBatch(model, [_data(per)], free=np.ones(5, bool))
    # a well-formed problem on a device that is not a HIP device: an error, never a CPU fallback
    with pytest.raises((ValueError, _lib.SurfdispError)):
        linearized.LinearizedBatch(model, [_data(per)], device="cpu")
