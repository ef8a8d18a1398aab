#!/usr/bin/env python3
"""CPU, one-off: the numpy statements of pysurfinv_amd/linearized.py against those of another revision of the same file
(``python scripts/lsq_host_parity.py PATH/TO/OTHER/linearized.py``), on the problems of tests/lsq_cases.py ``_problem`` with K = 0, 1, 2,
8 mode columns of scale 0.1.  Without modes every output must be equal; with modes g and the off-diagonal of A must be equal, the
diagonal of A within 2 ulp (three non-negative terms summed in another order), and the solved quantities within (n + K) eps cond(A)
of their largest magnitude (scalars: of max(|value|, 1)).  Not a test: BLAS summation order differs between hosts."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from lsq_cases import _problem  # noqa: E402
from pysurfinv_amd import linearized as new  # noqa: E402

spec = importlib.util.spec_from_file_location("pysurfinv_amd._other_linearized", sys.argv[1])
old = importlib.util.module_from_spec(spec)
spec.loader.exec_module(old)
EPS = np.finfo(np.float64).eps
bad = []


def same(tag, a, b):
    for k in a:
        if not np.array_equal(a[k], b[k]):
            bad.append(f"{tag}: {k} differs")
    if set(a) != set(b):
        bad.append(f"{tag}: keys {sorted(set(a) ^ set(b))}")


def worst(tag, a, b, keys, bound):
    """max over ``keys`` of |a - b| / (largest magnitude) / bound."""
    m = 0.0
    for k in keys:
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        scale = max(np.abs(y).max(), 1.0) if y.ndim == 0 else np.abs(y).max()
        m = max(m, float(np.abs(x - y).max() / scale / bound) if scale > 0 else float(np.abs(x - y).max() > 0))
    if m > 1.0:
        bad.append(f"{tag}: {m:.2f} x the bound")
    return m


print("   N    n  K    cond(A)  diag A (ulp)  step / bound  resolution / bound")
for N, n in ((1, 1), (7, 3), (40, 17), (100, 64), (256, 128)):
    G, r, w, x0, alpha, Q, lam = _problem(N, n, seed=100 + n)
    tag = f"({N},{n})"
    same(tag + " normal_equations", dict(zip("Ag", new.normal_equations(G, r, w, x0, alpha, Q, lam))),
         dict(zip("Ag", old.normal_equations(G, r, w, x0, alpha, Q, lam))))
    same(tag + " step", new.lsq_step_reference(G, r, w, x0, alpha, Q, lam), old.lsq_step_reference(G, r, w, x0, alpha, Q, lam))
    same(tag + " resolution", new.lsq_resolution_reference(G, w, n, alpha, Q, lam), old.lsq_resolution_reference(G, w, n, alpha, Q, lam))
    condA = np.linalg.cond(new.normal_equations(G, r, w, x0, alpha, Q, lam)[0])
    print(f"{N:4d} {n:4d}  0  {condA:9.2e}  every output of normal_equations and of the two Vs-only references equal")
    for K in (1, 2, 8):
        rng = np.random.default_rng(77 + n + K)
        Gy = rng.standard_normal((N, K)) * 0.1
        ms, beta, y = rng.uniform(0.5, 30.0, K), rng.uniform(0.0, 2.0, K), rng.normal(0.0, 1.0, K)
        beta[K - 1] = 0.0
        tag = f"({N},{n},{K})"
        (A, g), (Ao, go) = (m.modes_normal_equations(G, Gy, r, w, x0, alpha, Q, lam, ms, beta, y) for m in (new, old))
        off = ~np.eye(n + K, dtype=bool)
        if not (np.array_equal(g, go) and np.array_equal(A[off], Ao[off])):
            bad.append(f"{tag}: g or the off-diagonal of A differs")
        ulp = np.abs(np.diag(A) - np.diag(Ao)) / np.spacing(np.abs(np.diag(Ao)))
        if ulp.max() > 2:
            bad.append(f"{tag}: diag A {ulp.max()} ulp")
        condA = np.linalg.cond(Ao)
        bound = (n + K) * EPS * condA
        s, so = (m.lsq_modes_step_reference(G, r, w, x0, alpha, Q, lam, Gy, ms, beta, y) for m in (new, old))
        v, vo = (m.lsq_modes_resolution_reference(G, w, n, alpha, Q, lam, Gy, ms, beta) for m in (new, old))
        if (s["flag"], v["flag"]) != (so["flag"], vo["flag"]) or s["flag"] != 0:
            bad.append(f"{tag}: flags")
        ws = worst(tag + " step", s, so, ("delta", "delta_y", "misfit", "roughness", "predicted"), bound)
        wv = worst(tag + " resolution", v, vo, ("cov", "res", "sigma_post", "sigma_data", "rdiag", "dof", "logdet"), bound)
        print(f"{N:4d} {n:4d} {K:2d}  {condA:9.2e}  {ulp.max():12.1f}  {ws:12.2e}  {wv:18.2e}")

# flags: no rows; singular with alpha = lam = 0 (N < n without modes, two equal mode columns with)
G, r, w, x0, alpha, Q, lam = _problem(5, 8, seed=3)
G3, r3, w3, x3, _, Q3, _ = _problem(5, 3, seed=3)
Gy = np.ones((5, 2))
for tag, call in (
        ("step, no rows", lambda m: m.lsq_step_reference(G[:0], r[:0], w[:0], x0, alpha, Q, lam)),
        ("step, singular", lambda m: m.lsq_step_reference(G, r, w, x0, 0.0, Q, 0.0)),
        ("resolution, no rows", lambda m: m.lsq_resolution_reference(G[:0], w[:0], 8, alpha, Q, lam)),
        ("resolution, singular", lambda m: m.lsq_resolution_reference(G, w, 8, 0.0, Q, 0.0)),
        ("modes step, no rows", lambda m: m.lsq_modes_step_reference(G3[:0], r3[:0], w3[:0], x3, alpha, Q3, lam, Gy[:0], None, [2.0, 0.0], [0.5, 9.0])),
        ("modes step, singular", lambda m: m.lsq_modes_step_reference(G3, r3, w3, x3, 0.0, Q3, 0.0, Gy)),
        ("modes resolution, no rows", lambda m: m.lsq_modes_resolution_reference(G3[:0], w3[:0], 3, alpha, Q3, lam, Gy[:0])),
        ("modes resolution, singular", lambda m: m.lsq_modes_resolution_reference(G3, w3, 3, 0.0, Q3, 0.0, Gy))):
    a, b = call(new), call(old)
    same(tag, a, b)
    print(f"{tag}: flag {a['flag']} (other revision {b['flag']}), every output equal: {not any(x.startswith(tag) for x in bad)}")
print("FAILED:\n  " + "\n  ".join(bad) if bad else "all within the stated bounds")
sys.exit(1 if bad else 0)
