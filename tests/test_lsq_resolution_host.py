"""The host statement of the posterior covariance and resolution of the damped least-squares problem
(pysurfinv_amd.linearized.lsq_resolution_reference): its algebraic identities, its limits and its flags.  CPU only.

Bars.  The problems are those of tests/test_lsq_host.py (cond(A) <= 1e4, asserted there), so an inverse formed through the
Cholesky factor carries cond(A) eps ~ 1e-12 of relative error: the identities are asked to 1e-9 of the matrices' scale."""
import numpy as np
import pytest

from pysurfinv_amd import linearized


def _problem(N, n, seed):
    """Random G times a modest spectrum (cond(A) <= 1e4 whatever (N, n)), weights, interface weights with a cut."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, n))
    w = rng.uniform(0.5, 2.0, N)
    Q = rng.uniform(0.5, 1.5, max(n - 1, 0))
    if n > 2:
        Q[n // 2] = 0.0
    return G, w, Q, 0.7, 0.3


CASES = [(1, 1), (7, 3), (40, 17), (100, 64), (5, 8)]


@pytest.mark.parametrize("N,n", CASES)
def test_reference_identities(N, n):
    G, w, Q, alpha, lam = _problem(N, n, seed=200 + n)
    ref = linearized.lsq_resolution_reference(G, w, n, alpha, Q, lam)
    assert ref["flag"] == 0
    x0 = np.linspace(2.0, 4.0, n)
    A, _ = linearized.normal_equations(G, np.ones(N), w, x0, alpha, Q, lam)          # A depends on neither r nor x0
    H = G.T @ (w[:, None] * G)
    cov, res = ref["cov"], ref["res"]
    assert cov.shape == (n, n) and res.shape == (n, n)
    assert np.array_equal(cov, cov.T)
    scale = np.abs(A).sum(axis=1).max() * np.abs(cov).max()
    assert np.abs(cov @ A - np.eye(n)).max() <= 1e-9 * (scale + 1)                    # the reference's A is normal_equations' A
    assert np.abs(A @ res - H).max() <= 1e-9 * (np.abs(A).sum(axis=1).max() * np.abs(res).max() + np.abs(H).max())
    assert ref["dof"] == pytest.approx(np.trace(res), rel=1e-14, abs=1e-14)
    assert -1e-12 <= ref["dof"] <= n + 1e-12
    assert np.allclose(ref["rdiag"], np.diag(res), rtol=0, atol=0)
    assert np.allclose(ref["sigma_post"] ** 2, np.diag(cov), rtol=1e-14, atol=0)
    assert np.allclose(ref["sigma_data"] ** 2, np.diag(res @ cov), rtol=1e-9, atol=1e-12 * np.abs(np.diag(cov)).max())
    # Cd = C - C (alpha S + lam I) C with a positive semi-definite bracket: the data part never exceeds the whole
    assert (ref["sigma_data"] <= ref["sigma_post"]).all()
    assert ref["logdet"] == pytest.approx(np.linalg.slogdet(A)[1], rel=1e-12, abs=1e-12)
    # the same with the unknowns' vector in place of their number
    again = linearized.lsq_resolution_reference(G, w, x0, alpha, Q, lam)
    assert all(np.array_equal(ref[k], again[k]) for k in ref)


@pytest.mark.parametrize("N,n", [(7, 3), (40, 17), (100, 64)])
def test_resolution_limits_of_the_damping(N, n):
    """Full column rank, alpha = 0: lam -> 1e-12 ||H|| leaves res = I to 1e-6 (cond(H) lam / ||H|| <= 1e4 1e-12 is far below),
    lam -> 1e12 ||H|| leaves res = H / lam -> 0."""
    G, w, Q, _, _ = _problem(N, n, seed=300 + n)
    H = G.T @ (w[:, None] * G)
    norm = np.linalg.norm(H, 2)
    assert np.linalg.matrix_rank(G) == n
    lo = linearized.lsq_resolution_reference(G, w, n, 0.0, Q, 1e-12 * norm)
    assert lo["flag"] == 0 and np.abs(lo["res"] - np.eye(n)).max() <= 1e-6
    assert lo["dof"] == pytest.approx(n, abs=1e-6 * n)
    hi = linearized.lsq_resolution_reference(G, w, n, 0.0, Q, 1e12 * norm)
    assert hi["flag"] == 0 and np.abs(hi["res"]).max() <= 1e-11 and 0.0 <= hi["dof"] <= 1e-11 * n
    assert (hi["sigma_data"] <= hi["sigma_post"]).all()


def test_reference_flags_leave_zeros():
    G, w, Q, alpha, lam = _problem(5, 8, seed=3)
    keys = ("cov", "res", "sigma_post", "sigma_data", "rdiag")
    out = linearized.lsq_resolution_reference(G[:0], w[:0], 8, alpha, Q, lam)
    assert out["flag"] == 1 and out["cov"].shape == (8, 8) and out["rdiag"].shape == (8,)
    assert not any(out[k].any() for k in keys) and out["dof"] == 0.0 and out["logdet"] == 0.0
    H = G.T @ (w[:, None] * G)
    out = linearized.lsq_resolution_reference(G, w, 8, 0.0, Q, -2.0 * np.linalg.norm(H, 2))      # A = H + lam I: indefinite
    assert out["flag"] == 2
    assert not any(out[k].any() for k in keys) and out["dof"] == 0.0 and out["logdet"] == 0.0
    Gn = G.copy(); Gn[0, 0] = np.inf                                                            # A not finite
    with np.errstate(invalid="ignore"):
        out = linearized.lsq_resolution_reference(Gn, w, 8, alpha, Q, lam)
    assert out["flag"] == 2 and not any(out[k].any() for k in keys)
