"""Thickness modes of the linearised inversion on the host: the shape helpers (pysurfinv_amd.linearized.thickness_mode,
interface_mode), the numpy statements of the two mode entries (lsq_modes_step_reference, lsq_modes_resolution_reference) and the
argument errors.  CPU only."""
import numpy as np
import pytest

from lsq_cases import _problem
from pysurfinv_amd import linearized, synth
from pysurfinv_amd.obsdata import DispersionData

H = np.array([0.5, 1.5, 2.0, 6.0, 10.0, 12.0, 8.0, 0.0])                    # the last layer is the half space


def test_thickness_mode_thickens_its_group_by_one():
    T = linearized.thickness_mode(H, [1, 2, 3])
    assert T.dtype == np.float64 and T.shape == H.shape
    assert T[[1, 2, 3]].sum() == pytest.approx(1.0, rel=1e-15)
    assert not T[[0, 4, 5, 6, 7]].any()
    assert np.allclose(T[[1, 2, 3]], H[[1, 2, 3]] / 9.5, rtol=1e-15)        # the layers keep their proportions
    assert linearized.thickness_mode(H, 4)[4] == 1.0                          # a single layer


def test_interface_mode_moves_the_interface_and_keeps_the_total_depth():
    above, below = [0, 1, 2, 3], [4, 5, 6]
    T = linearized.interface_mode(H, above, below)
    assert T[above].sum() == pytest.approx(1.0, rel=1e-15) and T[below].sum() == pytest.approx(-1.0, rel=1e-15)
    assert T[7] == 0.0
    assert abs(T.sum()) <= 4e-16
    y = 0.8
    h = H + T * y
    assert h.sum() == pytest.approx(H.sum(), rel=1e-15)                     # the total depth
    assert h[above].sum() == pytest.approx(H[above].sum() + y, rel=1e-15)   # the interface went down by y
    assert (h[:7] > 0).all()


@pytest.mark.parametrize("call", [
    lambda: linearized.thickness_mode(H, []),
    lambda: linearized.thickness_mode(H, [6, 7]),                             # contains the last layer
    lambda: linearized.thickness_mode(H, [-1]),
    lambda: linearized.thickness_mode(np.array([0.0, 0.0, 1.0, 0.0]), [0, 1]),   # group thickness 0
    lambda: linearized.thickness_mode(np.array([1.0, -2.0, 1.0, 0.0]), [0, 1]),  # ... negative
    lambda: linearized.interface_mode(H, [], [4]),
    lambda: linearized.interface_mode(H, [0, 1], []),
    lambda: linearized.interface_mode(H, [0, 1], [6, 7]),
    lambda: linearized.interface_mode(H, [0, 1, 2], [2, 3]),                  # a shared layer
    lambda: linearized.interface_mode(np.array([1.0, 0.0, 0.0, 0.0]), [0], [1, 2]),
])
def test_shape_helpers_refuse_bad_groups(call):
    with pytest.raises(ValueError):
        call()


def test_mode_columns_ignore_the_half_space_and_beyond():
    rng = np.random.default_rng(4)
    kh = rng.normal(0, 0.1, (5, 8)).astype(np.float32)
    T = rng.normal(0, 1, (2, 8))
    want = kh[:, :5].astype(np.float64) @ T[:, :5].T
    kh[:, 5:] = np.nan                                                      # never read with nlay = 6
    assert np.array_equal(linearized.mode_columns(kh, T, nlay=6), want)


@pytest.mark.parametrize("N,n", [(1, 1), (7, 3), (40, 17)])
def test_references_without_modes_are_the_existing_references(N, n):
    G, r, w, x0, alpha, Q, lam = _problem(N, n, seed=100 + n)
    for Gy in (None, np.zeros((N, 0))):
        a, b = linearized.lsq_modes_step_reference(G, r, w, x0, alpha, Q, lam, Gy), linearized.lsq_step_reference(G, r, w, x0, alpha, Q, lam)
        assert a["delta_y"].shape == (0,)
        for k in b:
            assert np.array_equal(a[k], b[k]), k
        a = linearized.lsq_modes_resolution_reference(G, w, n, alpha, Q, lam, Gy)
        b = linearized.lsq_resolution_reference(G, w, n, alpha, Q, lam)
        assert set(a) == set(b)
        for k in b:
            assert np.array_equal(a[k], b[k]), k


def _hand_built(G, Gy, r, w, x0, alpha, Q, lam, ms, beta, y):
    """The augmented system written out entry by entry: [G | Gy]^T W [G | Gy], the band of alpha D^T Q D and lam on the Vs block,
    lam ms_k + beta_k on the mode diagonal, -beta_k y_k on the modes' right-hand side."""
    n, K = G.shape[1], Gy.shape[1]
    Ga = np.concatenate([G, Gy], axis=1)
    A, g = np.zeros((n + K, n + K)), np.zeros(n + K)
    for i in range(n + K):
        g[i] = sum(w[q] * Ga[q, i] * r[q] for q in range(len(r)))
        for j in range(n + K):
            A[i, j] = sum(w[q] * Ga[q, i] * Ga[q, j] for q in range(len(r)))
    for j in range(n):
        A[j, j] += lam
    for j in range(n - 1):                                                  # Q_j (x_{j+1} - x_j)^2
        A[j, j] += alpha * Q[j]; A[j + 1, j + 1] += alpha * Q[j]
        A[j, j + 1] -= alpha * Q[j]; A[j + 1, j] -= alpha * Q[j]
        d = x0[j + 1] - x0[j]
        g[j] += alpha * Q[j] * d; g[j + 1] -= alpha * Q[j] * d
    for k in range(K):
        A[n + k, n + k] += lam * ms[k] + beta[k]
        g[n + k] -= beta[k] * y[k]
    return A, g


def test_reference_step_with_modes_solves_the_hand_built_system():
    """N = 9 rows, n = 4 Vs unknowns, K = 2 modes: A delta = g for the system built entry by entry, to 1e-12 of its scale (cond(A)
    below 1e3, asserted); the predicted objective is the objective of the quadratic model at the solution."""
    N, n, K = 9, 4, 2
    G, r, w, x0, alpha, Q, lam = _problem(N, n, seed=11)
    rng = np.random.default_rng(12)
    Gy = rng.standard_normal((N, K)) * 0.1
    ms, beta, y = np.array([25.0, 4.0]), np.array([0.0, 0.6]), np.array([0.3, -1.2])
    A, g = _hand_built(G, Gy, r, w, x0, alpha, Q, lam, ms, beta, y)
    assert np.linalg.cond(A) < 1e3
    A2, g2 = linearized.modes_normal_equations(G, Gy, r, w, x0, alpha, Q, lam, ms, beta, y)
    assert np.allclose(A2, A, rtol=1e-13, atol=1e-13) and np.allclose(g2, g, rtol=1e-13, atol=1e-13)
    out = linearized.lsq_modes_step_reference(G, r, w, x0, alpha, Q, lam, Gy, ms, beta, y)
    assert out["flag"] == 0 and out["delta"].shape == (n,) and out["delta_y"].shape == (K,)
    d = np.concatenate([out["delta"], out["delta_y"]])
    assert np.abs(A @ d - g).max() <= 1e-12 * (np.abs(A).sum(axis=1).max() * np.abs(d).max() + np.abs(g).max())
    t = r - G @ out["delta"] - Gy @ out["delta_y"]
    x1, y1 = x0 + out["delta"], y + out["delta_y"]
    want = (w * t * t).sum() + alpha * (Q * np.diff(x1) ** 2).sum() + (beta * y1 * y1).sum()
    assert out["predicted"] == pytest.approx(want, rel=1e-13)
    assert out["misfit"] == pytest.approx((w * r * r).sum(), rel=1e-14)
    # the step minimises objective + lam |delta|^2 + lam ms delta_y^2: a nudge in any direction costs more
    full = lambda dd: ((w * (r - G @ dd[:n] - Gy @ dd[n:]) ** 2).sum() + alpha * (Q * np.diff(x0 + dd[:n]) ** 2).sum()
                       + (beta * (y + dd[n:]) ** 2).sum() + lam * (dd[:n] ** 2).sum() + (lam * ms * dd[n:] ** 2).sum())
    for j in range(n + K):
        e = np.zeros(n + K); e[j] = 1e-3
        assert full(d) < full(d + e) and full(d) < full(d - e)
    # resolution: cov = A^-1 and res = cov H of the same matrix
    res = linearized.lsq_modes_resolution_reference(G, w, n, alpha, Q, lam, Gy, ms, beta)
    Ga = np.concatenate([G, Gy], axis=1)
    Hm = Ga.T @ (w[:, None] * Ga)
    assert np.abs(A @ res["cov"] - np.eye(n + K)).max() <= 1e-12
    assert np.abs(A @ res["res"] - Hm).max() <= 1e-12 * np.abs(Hm).max()
    assert res["dof"] == pytest.approx(np.trace(np.linalg.solve(A, Hm)), rel=1e-12)
    assert res["logdet"] == pytest.approx(np.linalg.slogdet(A)[1], rel=1e-12)
    assert res["sigma_post"].shape == (n + K,) and (res["sigma_data"] <= res["sigma_post"]).all()


def test_reference_step_with_modes_flags():
    G, r, w, x0, alpha, Q, lam = _problem(5, 3, seed=3)
    Gy = np.ones((5, 2))
    beta, y = np.array([2.0, 0.0]), np.array([0.5, 9.0])
    out = linearized.lsq_modes_step_reference(G[:0], r[:0], w[:0], x0, alpha, Q, lam, Gy[:0], None, beta, y)
    rough = (Q * np.diff(x0) ** 2).sum()
    assert out["flag"] == 1 and not out["delta"].any() and not out["delta_y"].any() and out["delta_y"].shape == (2,)
    assert out["predicted"] == pytest.approx(alpha * rough + 2.0 * 0.25, rel=1e-14)
    out = linearized.lsq_modes_step_reference(G, r, w, x0, 0.0, Q, 0.0, Gy)     # two equal columns, no damping: singular
    assert out["flag"] == 2 and not out["delta_y"].any()
    assert linearized.lsq_modes_resolution_reference(G, w, 3, 0.0, Q, 0.0, Gy)["flag"] == 2


def test_mode_argument_errors_need_no_gpu():
    per = synth.default_periods(6)
    model = synth.synth_models(3, 8, seed=1)
    v = np.full(per.size, 3.5)
    c = DispersionData("R", "c", per, v, 0.01 * v)
    u = DispersionData("R", "U", per, v, 0.01 * v)
    T = linearized.interface_mode(model[0, 3], [0, 1, 2], [3, 4])
    with pytest.raises(ValueError, match="thickness modes need phase-velocity data only: the library has no dU/dh or dchi/dh yet"):
        linearized.LinearizedBatch(model, [c, u], modes=T[None])
    with pytest.raises(ValueError, match="modes"):
        linearized.LinearizedBatch(model, [c], modes=np.zeros((9, 8)))
    with pytest.raises(ValueError, match="modes"):
        linearized.LinearizedBatch(model, [c], modes=np.zeros((1, 7)))
    with pytest.raises(ValueError, match="mode_scale"):
        linearized.LinearizedBatch(model, [c], modes=T[None], mode_scale=0.0)
    with pytest.raises(ValueError, match="mode_scale"):
        linearized.LinearizedBatch(model, [c], modes=T[None], mode_scale=np.ones((3, 1)))   # per stack against shared modes
    with pytest.raises(ValueError, match="mode_prior"):
        linearized.LinearizedBatch(model, [c], modes=T[None], mode_prior=-1.0)
