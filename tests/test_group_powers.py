"""CPU checks of the group kernel's fast fit: the closed-form powers P^(4 nreg) of the RK4 step (make_base / pow_sublayers /
pow_expand in surfdisp_kernels.hip, compiled for the host by tests/hostcheck/powcheck.hip) against the repeated
prop_sq / prop_apply products they replace and against a long double reference, and the whole group velocity of the
host-compiled group_rayleigh against the oracle on random stacks, fed with the oracle's own c and ellipticity.
No GPU needed; skipped if hipcc is absent."""
import ctypes
import os
import sys

import numpy as np
import pytest

import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcheck")


@pytest.fixture(scope="module")
def powlib():
    return ctypes.CDLL(hostbuild.build(os.path.join(HC, "powcheck.hip"), os.path.join(HC, "libpowcheck.so")))


def _layers(rng, n):
    """n random layers in four families -> (q9 float32 [N, 9] in RCoef order, nreg, traction scale mu k, family)."""
    f32 = np.float32
    fam = np.repeat(np.arange(4), n // 4)
    b = rng.uniform(0.5, 4.5, fam.size).astype(f32)
    a = (b * rng.uniform(1.6, 2.0, fam.size)).astype(f32)
    rho = rng.uniform(1.8, 3.4, fam.size).astype(f32)
    T = np.exp(rng.uniform(np.log(0.5), np.log(200.0), fam.size)).astype(f32)
    u = rng.uniform(0.0, 1.0, fam.size)
    c = np.where(fam == 0, a * (1.02 + 1.5 * u),                # oscillatory: c > a
        np.where(fam == 1, b * (0.2 + 0.78 * u),                # evanescent: c < b
        np.where(fam == 2, b + (a - b) * (0.02 + 0.96 * u),     # mixed: b < c < a
                 b * 10.0 ** rng.uniform(-4, -1.5, fam.size)))).astype(f32)   # near-degenerate: c << b, r_a ~ r_b ~ k
    near = (fam == 3) & (rng.uniform(size=fam.size) < 0.5)
    a = np.where(near, b * (1.0 + 10.0 ** rng.uniform(-6, -3, fam.size)), a).astype(f32)   # ... and r_a ~ r_b from a ~ b
    k = 2 * np.pi / (c.astype(np.float64) * T)
    ra = k * np.sqrt(np.abs(1 - (c / a.astype(np.float64)) ** 2))
    rmax = np.maximum(ra, k * np.sqrt(np.abs(1 - (c / b.astype(np.float64)) ** 2)))
    kdr = np.where(fam == 0, rng.uniform(0.1, 15.0, fam.size), rng.uniform(0.5, 30.0, fam.size))   # k d r over the layer
    d = (kdr / rmax).astype(f32)
    nreg = np.where(rng.uniform(size=fam.size) < 0.7, 5, rng.integers(1, 6, fam.size)).astype(np.int32)
    q = np.zeros((fam.size, 9), f32)
    for i in range(fam.size):                                  # rayleigh_sweep's coefficients, in fp32
        wvno = f32(6.2831853072) / (c[i] * T[i]); wvnosq = wvno * wvno
        omega = f32(6.2831853072) / T[i]; omegsq = omega * omega
        dsub = d[i] / f32(5.0)
        xmu = rho[i] * b[i] * b[i]
        xlamb = rho[i] * (a[i] * a[i] - f32(2.0) * b[i] * b[i])
        a12 = f32(1.0) / (xlamb + f32(2.0) * xmu)
        a13 = wvno * xlamb * a12
        a21 = -omegsq * rho[i]
        a43 = a21 + f32(4.0) * wvnosq * xmu * (xlamb + xmu) * a12
        q[i] = (a12, a13, a21, wvno, -wvno, f32(1.0) / xmu, -a13, a43, -dsub / f32(4.0))
    return q, nreg, (rho * b * b).astype(np.float64) * k, fam


def _scaled(blocks, s):
    """16 block-ordered entries -> 4x4 in (ur, tz, uz, tr), displacements and tractions brought to one scale."""
    m = np.empty((blocks.shape[0], 4, 4))
    for bi in range(4):
        r, cc = 2 * (bi // 2), 2 * (bi % 2)
        m[:, r:r + 2, cc:cc + 2] = blocks[:, 4 * bi:4 * bi + 4].reshape(-1, 2, 2)
    dsc = np.stack([np.ones_like(s), s, np.ones_like(s), s], 1)
    return m * dsc[:, None, :] / dsc[:, :, None]


def test_closed_form_powers(powlib):
    rng = np.random.default_rng(20261015)
    q, nreg, s, fam = _layers(rng, 4000)
    N = q.shape[0]
    out = {k: np.zeros((N, 16)) for k in ("closed", "stepped", "ref")}
    dp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    powlib.sd_powcheck(N, dp(q), dp(nreg), dp(out["closed"]), dp(out["stepped"]), dp(out["ref"]))
    ref = _scaled(out["ref"], s)
    assert np.isfinite(ref).all()
    norm = np.abs(ref).max(axis=(1, 2))
    err = {k: np.abs(_scaled(out[k], s) - ref).max(axis=(1, 2)) / norm for k in ("closed", "stepped")}
    # relative to |P^m|: fp64 rounding, grown by the cancellation of the fastest and slowest solutions in a layer (k d r <= 30);
    # per family, no worse than the repeated products (measured: 0.6 .. 1.9 x their largest error, at most 2.5e-14)
    assert err["closed"].max() < 1e-13
    for f in range(4):
        sel = fam == f
        print(f"family {f}: closed {err['closed'][sel].max():.2e}  stepped {err['stepped'][sel].max():.2e}")
        assert err["closed"][sel].max() < 3 * err["stepped"][sel].max()


@pytest.fixture(scope="module")
def hostlib():
    """tests/hostcheck/run_hostcheck.py on the group-velocity host build (the library test_hostcheck.py builds)."""
    hostbuild.build(os.path.join(HC, "hostcheck.hip"), os.path.join(HC, "libhostcheck.so"))
    sys.path.insert(0, HC)
    import run_hostcheck
    return run_hostcheck


@pytest.mark.parametrize("water", [False, True])
def test_group_velocity_random_stacks(hostlib, water):
    """6 000 stacks x 20 periods (1.2e5 units) per case: the fit's powers and restart feed the whole U."""
    from pysurfinv_amd import synth
    model = synth.synth_models(6000, 10, seed=7 + water)
    if water:                                                  # a water layer on top (vs = 0)
        model[:, 0, 0] = 1.5; model[:, 1, 0] = 0.0; model[:, 2, 0] = 1.03
    per = np.ascontiguousarray(synth.default_periods(20), np.float32)
    c, u, r = hostlib.oracle_dbg(model, per, 2)
    uh = hostlib.host_group(model, per, 2, c, r)
    ok = u != 0
    assert ok.mean() > 0.9
    err = np.abs(uh[ok] / u[ok] - 1)
    print(f"water={water}: {ok.sum()} units, max {err.max():.2e}, mean {err.mean():.2e}")
    assert err.max() < 5e-6
