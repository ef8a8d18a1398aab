"""CPU check of tests/secular64.py, the float64 secular functions the GPU tests compare the kernel with: their roots must be
the roots of the equations of motion themselves, propagated through every layer with a matrix exponential (no
compound matrices, no closed-form layer coefficients), on random stacks and on stacks built so that a root sits within
a few float32 ulps of a layer velocity - where the closed forms switch between sin and sinh and divide by a vanishing
vertical wavenumber."""
import numpy as np
import pytest
from scipy.linalg import expm
from scipy.optimize import brentq

import secular64 as s64

RTOL = 1e-9


def _rayleigh_matrix(k, om, a, b, rho):
    # y = (ur, uz, tz, tr): dy/dz = A y for an isotropic layer
    mu = rho * b * b; lam = rho * (a * a - 2 * b * b); l2m = lam + 2 * mu
    A = np.zeros((4, 4))
    A[0, 1] = -k; A[0, 3] = 1.0 / mu
    A[1, 2] = 1.0 / l2m; A[1, 0] = k * lam / l2m
    A[2, 1] = -om * om * rho; A[2, 3] = k
    A[3, 2] = -k * lam / l2m; A[3, 0] = -om * om * rho + 4 * k * k * mu * (lam + mu) / l2m
    return A


def brute_rayleigh(a, b, rho, d, c, T):
    """det of the surface tractions of the half space's two decaying solutions, propagated up layer by layer (up to a
    positive factor: the pair is re-orthonormalised with det R > 0)."""
    om = 2 * np.pi / T; k = om / c
    A = _rayleigh_matrix(k, om, a[-1], b[-1], rho[-1])
    w, V = np.linalg.eig(A)
    Y = np.real(V[:, np.argsort(w.real)[:2]])              # the two solutions that decay with depth,
    Y = Y @ np.linalg.inv(Y[:2])                            # as the pair with displacements I (continuous in c)
    for i in range(len(d) - 2, -1, -1):
        nsub = 1 + int(k * d[i] / 0.5)                      # re-orthonormalised every half wavelength / e-fold
        P = expm(-_rayleigh_matrix(k, om, a[i], b[i], rho[i]) * (d[i] / nsub))
        for _ in range(nsub):
            q, r = np.linalg.qr(P @ Y)
            if np.linalg.det(r) < 0:
                q[:, 0] = -q[:, 0]
            Y = q
    return np.linalg.det(Y[2:])


def brute_love(b, rho, d, c, T):
    """surface stress of the half space's decaying SH solution, propagated up layer by layer."""
    om = 2 * np.pi / T; k = om / c
    mu = rho[-1] * b[-1] ** 2
    y = np.array([1.0, -mu * k * np.sqrt(1 - (c / b[-1]) ** 2)])
    for i in range(len(d) - 2, -1, -1):
        mu = rho[i] * b[i] ** 2
        A = np.array([[0.0, 1.0 / mu], [k * k * mu - om * om * rho[i], 0.0]])
        y = expm(-A * d[i]) @ y
        y /= np.abs(y).max()
    return y[1]


def f64_rayleigh(a, b, rho, d, c, T):
    return s64.delta_rayleigh(a, b, rho, d, len(d), c, T)[0]


def f64_love(b, rho, d, c, T):
    return s64.delta_love(b, rho, d, len(d), c, T)[0]


def roots(f, lo, hi, n=700):
    cs = np.linspace(lo, hi, n)
    v = np.array([f(c) for c in cs])
    out = []
    for i in range(n - 1):
        if np.sign(v[i]) != np.sign(v[i + 1]) and v[i] != 0:
            out.append(brentq(f, cs[i], cs[i + 1], xtol=1e-15, rtol=1e-15))
    return np.array(out)


def random_stack(rng, kind):
    L = int(rng.integers(3, 7))
    b = np.sort(rng.uniform(0.6, 4.2, L)); b[-1] = max(b[-1], b[-2] + 0.2)
    if rng.random() < 0.3:                                  # a low-velocity layer
        j = int(rng.integers(1, L - 1)); b[j] *= 0.8
    a = b * rng.uniform(1.6, 2.0, L)
    rho = 1.7 + 0.3 * b
    d = rng.uniform(0.5, 15.0, L); d[-1] = 0.0
    T = float(rng.uniform(2.0, 40.0))
    return [np.float32(x).astype(np.float64) for x in (a, b, rho, d)], np.float64(np.float32(T))


def check_roots(kind, stack, T):
    a, b, rho, d = stack
    if kind == 2:
        f, g = (lambda c: f64_rayleigh(a, b, rho, d, c, T)), (lambda c: brute_rayleigh(a, b, rho, d, c, T))
    else:
        f, g = (lambda c: f64_love(b, rho, d, c, T)), (lambda c: brute_love(b, rho, d, c, T))
    lo, hi = 0.8 * b.min(), b[-1] * (1 - 1e-6)
    r = roots(f, lo, hi)
    assert len(r) >= 1
    for x in r:
        w = 1e-7 * x
        assert np.sign(g(x - w)) != np.sign(g(x + w)), (kind, x)
        y = brentq(g, x - w, x + w, xtol=1e-15, rtol=1e-15)
        assert abs(y / x - 1) < RTOL, (kind, x, y)
    rg = roots(g, lo, hi)
    assert len(rg) == len(r), (r, rg)
    return r


@pytest.mark.parametrize("kind", [2, 1])
def test_secular64_roots_random_stacks(kind):
    rng = np.random.default_rng(17 + kind)
    for _ in range(15):
        check_roots(kind, *random_stack(rng, kind))


@pytest.mark.parametrize("kind", [2, 1])
def test_secular64_roots_at_a_layer_velocity(kind):
    """A root moved onto a layer velocity by fixed-point iteration (Rayleigh: the top layer's P velocity, the #290
    construction; Love: a layer's S velocity): the float32 velocity ends within a few ulps of the root."""
    rng = np.random.default_rng(29 + kind)
    near = 0
    for _ in range(6):
        (a, b, rho, d), T = random_stack(rng, kind)
        T = np.float64(np.float32(2.0 * d.sum() / b.min()))   # long period: the fundamental root well above the top layer's S
        if kind == 2:                                         # the top layer's P velocity, its S velocity well below
            j, vel = 0, a
            b[0] = np.float64(np.float32(0.5 * check_roots(kind, (a, b, rho, d), T)[0]))
        else:                                                 # the first layer whose S velocity is above the root
            c0 = check_roots(kind, (a, b, rho, d), T)[0]
            j, vel = (int(np.argmax(b[:-1] > c0)) if (b[:-1] > c0).any() else len(b) - 2), b

        def gap(v):                                           # root with the layer's velocity at v, minus v
            vel[j] = np.float64(np.float32(v))
            return check_roots(kind, (a, b, rho, d), T)[0] - vel[j]
        v0 = check_roots(kind, (a, b, rho, d), T)[0]; g0 = gap(v0)
        v1 = v0 + g0; g1 = gap(v1)
        for it in range(8):                                   # secant steps onto root == velocity
            if g1 == g0 or abs(g1) < 2.0 ** -24 * v1:
                break
            v0, g0, v1 = v1, g1, v1 - g1 * (v1 - v0) / (g1 - g0)
            g1 = gap(v1)
        v = vel[j]
        r = check_roots(kind, (a, b, rho, d), T)
        near += int(np.abs(r / v - 1).min() < 4 * 2.0 ** -24)
    assert near >= 4
