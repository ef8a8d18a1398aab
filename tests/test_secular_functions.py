"""GPU: the fp32 secular functions of the root search (surfdisp_kernels.hip: layer_coef, ray_step, ray_close,
delta_rayleigh, delta_love) against their float64 restatement (tests/secular64.py), at the trial velocities where they go
wrong - within a few float32 ulps of a layer velocity, where the evanescent branch divides sinh(x) by a vertical wavenumber
that goes to zero.  The output tests cannot see such a defect except where a team's subdivision happens to converge onto
the jump it makes (third soak, #290: one team size, one stack in 10^7); these see it on every run.

tests/probe/secular_probe.hip is compiled here (hipcc --offload-arch=gfx950) into tests/probe/; it #includes the kernel
source and runs its functions one thread per case.  Bounds marked "measured" were measured on this build; the comment next
to each gives the figure the build before the small-argument sinh fix produced on the same cases."""
import ctypes
import os

import numpy as np
import pytest

import hostbuild
import secular64 as s64

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.path.join(HERE, "probe")
ULP = 2.0 ** -24
fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


@pytest.fixture(scope="module")
def probe():
    return ctypes.CDLL(hostbuild.build(os.path.join(PROBE, "secular_probe.hip"), os.path.join(PROBE, "libsecular_probe.so"),
                                       extra=["-fno-slp-vectorize"], opt="-O3", quiet=False))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def run_coef(P, arg, wd):
    arg, wd = _f32(arg), _f32(wd)
    out = np.zeros((arg.size, 5), np.float32)
    assert P.sp_coef(arg.size, fp(arg), fp(wd), fp(out)) == 0
    return out


def run_step(P, st, trial, lyr, flags):
    st, trial, lyr = _f32(st), _f32(trial), _f32(lyr)
    flags = np.ascontiguousarray(flags, np.int32)
    n = len(flags)
    assert st.shape == (n, 5) and trial.shape == (n, 2) and lyr.shape == (n, 5)
    out = np.zeros((n, 6), np.float32)
    assert P.sp_step(n, fp(st), fp(trial), fp(lyr), ip(flags), fp(out)) == 0
    return out


def run_close(P, st, trial, lyr, start):
    st, trial, lyr = _f32(st), _f32(trial), _f32(lyr)
    start = np.ascontiguousarray(start, np.int32)
    n = len(start)
    out = np.zeros((n, 2), np.float32)
    assert P.sp_close(n, fp(st), fp(trial), fp(lyr), ip(start), fp(out)) == 0
    return out


def run_secular(P, stacks, mmax, tst, c, T, kind, mode):
    """stacks float32 [nstk, 4, L] (a, b, rho, d) -> [ntr, 3] (value, mag, phi)"""
    stacks = _f32(stacks); mmax = np.ascontiguousarray(mmax, np.int32); tst = np.ascontiguousarray(tst, np.int32)
    c, T = _f32(c), _f32(T)
    nstk, four, L = stacks.shape
    out = np.zeros((len(c), 3), np.float32)
    assert P.sp_secular(nstk, L, fp(stacks), ip(mmax), len(c), ip(tst), fp(c), fp(T), kind, mode, fp(out)) == 0
    return out


def ulp_offsets():
    return np.array(sorted(set(range(0, 65)) | {2 ** e for e in range(7, 21)}), np.float64)


# ------------------------------------------------------------------------------------------------- 1. layer coefficients
def coef_cases(seed=3):
    ks = ulp_offsets()
    vs = np.array([1.0, 1.475, 2.45, 4.2995994, 8.1])
    wds = np.array([1e-4, 1e-3, 0.014, 0.1, 1.0, 10.0, 60.0])
    K, V, W, S = np.meshgrid(ks, vs, wds, [-1.0, 1.0], indexing="ij")
    c = np.float32(V) * (1.0 + S * K * ULP)
    c = c.astype(np.float32).astype(np.float64)
    v = np.float32(V).astype(np.float64)
    arg = (1.0 - (c / v) ** 2).ravel()
    wd = W.ravel()
    rng = np.random.default_rng(seed)
    n = 100000
    arg_r = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-9, 1, n)
    wd_r = 10.0 ** rng.uniform(-4, np.log10(60.0), n)
    arg = np.concatenate([arg, arg_r]).astype(np.float32)
    wd = np.concatenate([wd, wd_r]).astype(np.float32)
    return arg, wd


def coef_errors(P):
    """normalised errors of (rsin, sinr, cs) and of sinh/cosh for |x| > 1, and the bound each must meet:
    2^-20 + 2e-7 |x|.  Evanescent side: relative to the value (sinh, cosh have no zeros).  Oscillatory side: relative to the
    functions' envelopes |r| min(1, |x|), wd min(1, 1/|x|) and 1 (relative to the value itself is meaningless at a zero
    of sin x or cos x)."""
    arg, wd = coef_cases()
    o = run_coef(P, arg, wd).astype(np.float64)
    rsin, sinr, cs, x, ph = s64.coef(arg.astype(np.float64), wd.astype(np.float64))
    ev = arg.astype(np.float64) > 0
    r = np.sqrt(np.abs(arg.astype(np.float64)))
    ax = np.abs(x)
    with np.errstate(all="ignore"):
        keep = np.isfinite(o).all(axis=1) & (np.abs(cs) < 1e37) & (np.abs(o[:, 2]) < 1e37)   # fp32 overflow: not this code's trials
    env_rs = np.where(ev, np.abs(rsin), r * np.minimum(1.0, ax))
    env_sr = np.where(ev, np.abs(sinr), wd * np.minimum(1.0, 1.0 / np.maximum(ax, 1e-300)))
    env_cs = np.where(ev, np.abs(cs), 1.0)
    floor = 1e-20 * wd                                        # c == v exactly: r = 1e-15 gives rsin ~ 1e-30 wd against 0
    with np.errstate(all="ignore"):
        e_rs = np.abs(o[:, 0] - rsin) / np.maximum(env_rs, floor)
        e_sr = np.abs(o[:, 1] - sinr) / env_sr
        e_cs = np.abs(o[:, 2] - cs) / env_cs
        ratio = np.where(ev & (ax > 1), np.abs((o[:, 1] * r * np.sign(x)) / o[:, 2] - np.tanh(ax) * np.sign(x)) / np.tanh(ax), 0.0)
    bound = 2.0 ** -20 + 2e-7 * ax                            # 1e-7 |x|: the uncorrected exp2's common scale error; another
                                                              # 1e-7 |x|: x = k d r is itself an fp32 product (r to 1.5 ulp)
    return dict(keep=keep, ev=ev, ax=ax, e_rs=e_rs, e_sr=e_sr, e_cs=e_cs, ratio=ratio, bound=bound)


def test_layer_coefficients_against_float64(probe):
    E = coef_errors(probe)
    k = E["keep"]
    assert k.sum() > 100000
    worst = {n: float(np.max((E[n] / E["bound"])[k])) for n in ("e_rs", "e_sr", "e_cs")}
    worst["ratio"] = float(np.max(E["ratio"][k & E["ev"] & (E["ax"] > 1)]) / 2.0 ** -20)
    print("layer_coef: worst error / bound", worst)
    # measured on this build: 0.86 of the bound for rsin, sinr, cos and 0.20 for the ratio; before the fix: rsin and sinr
    # 1e6 x the bound (sinh came out 0 one float off a layer velocity)
    for n, w in worst.items():
        assert w <= 1.0, (n, worst)


def test_layer_coefficients_exact_at_the_velocity(probe):
    """arg == 0 (c == v to the last bit) and the smallest arguments on either side: the degenerate limits
    rsin = 0, sinr = k d, cos = 1 to a few ulps, on both sides alike."""
    wd = np.array([1e-4, 0.014, 1.0, 60.0], np.float32)
    for a in (0.0, 1e-30, -1e-30, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -23, -(2.0 ** -23)):
        o = run_coef(probe, np.full(wd.size, a, np.float32), wd).astype(np.float64)
        assert np.all(np.abs(o[:, 1] / wd - 1) < 4 * ULP * (1 + wd * wd)), (a, o[:, 1], wd)
        assert np.all(np.abs(o[:, 2] - 1) < 4 * ULP * (1 + wd * wd)), (a, o[:, 2])
        assert np.all(np.abs(o[:, 0]) <= 2 * abs(a) * wd + 1e-28), (a, o[:, 0])


# ------------------------------------------------------------------------------------------------- 2. one layer step
STEP_BOUND = 1e-5      # measured on this build: 2.6e-6; before the small-argument sinh fix: 6.5e-3


def step_cases(seed=5):
    rng = np.random.default_rng(seed)
    rows = []
    units = [np.eye(5)[i] for i in range(5)]
    for (a, b, rho, d, T) in [(4.2995994, 2.45, 2.7, 1.36, 141.6), (6.3, 3.6, 2.9, 5.0, 20.0), (2.5, 1.2, 2.1, 0.3, 8.0),
                              (8.1, 4.6, 3.3, 20.0, 60.0), (1.8, 0.4, 1.9, 0.05, 3.0)]:
        for vel in (a, b):
            for k in ulp_offsets():
                for sgn in (-1.0, 1.0):
                    c = np.float32(np.float32(vel) * (1.0 + sgn * k * ULP))
                    for s in units + [rng.normal(size=5) for _ in range(2)]:
                        rows.append((s, c, T, (a, b, rho, d, rho * rng.uniform(0.8, 1.2)), 1 | (int(rng.random() < 0.5) << 2)))
    # liquid top layer near c = 1.475 (start 1, first)
    for k in ulp_offsets():
        for sgn in (-1.0, 1.0):
            c = np.float32(np.float32(1.475) * (1.0 + sgn * k * ULP))
            for d in (0.05, 1.0, 4.0):
                for s in units + [rng.normal(size=5)]:
                    rows.append((s, c, 15.0, (1.475, 0.0, 1.027, d, 0.0), 1 | 4))
    st = np.array([r[0] for r in rows]); trial = np.array([(r[1], r[2]) for r in rows]); lyr = np.array([r[3] for r in rows])
    flags = np.array([r[4] for r in rows])
    return _f32(st), _f32(trial), _f32(lyr), flags


def step_errors(P):
    st, trial, lyr, flags = step_cases()
    o = run_step(P, st, trial, lyr, flags).astype(np.float64)
    err = np.zeros(len(flags))
    for i in range(len(flags)):
        a, b, rho, d, rp = (float(v) for v in lyr[i])
        ref, _ = s64.ray_step(st[i], trial[i, 0], trial[i, 1], a, b, d, rho, rp, flags[i] & 3, bool(flags[i] & 4))
        ref = np.array(ref)
        scale = np.abs(ref).max()
        # (a liquid layer maps some unit states to zero: the kernel must give exactly zero there)
        err[i] = np.abs(o[i, :5] - ref).max() / scale if scale > 0 else (0.0 if not o[i, :5].any() else np.inf)
    return err


def test_one_layer_step_against_float64(probe):
    err = step_errors(probe)
    print(f"ray_step: worst |f32 - f64| / max|f64| = {err.max():.3e} over {err.size} steps (bound {STEP_BOUND:.1e})")
    assert np.isfinite(err).all()
    assert err.max() < STEP_BOUND


def test_closure_against_float64(probe):
    rng = np.random.default_rng(9)
    n = 4000
    st = rng.normal(size=(n, 5)); a = rng.uniform(6.0, 8.5, n); b = a / rng.uniform(1.65, 1.9, n)
    c = b * rng.uniform(0.3, 0.999, n); T = rng.uniform(2.0, 150.0, n)
    lyr = np.stack([a, b, rng.uniform(3.0, 3.5, n), rng.uniform(2.5, 3.2, n)], 1)
    start = rng.integers(1, 4, n)
    st, lyr, trial = _f32(st), _f32(lyr), _f32(np.stack([c, T], 1))
    o = run_close(probe, st, trial, lyr, start).astype(np.float64)
    for i in range(n):
        v, mag = s64.ray_close(st[i], trial[i, 0], trial[i, 1], *lyr[i], int(start[i]))
        assert abs(o[i, 0] - v) <= 1e-5 * mag, (i, o[i], v, mag)
        assert abs(o[i, 1] / mag - 1) < 1e-5


# ------------------------------------------------------------------------------------------------- 3. whole functions
# measured: |f32 - f64| / mag, worst over every battery: Rayleigh 1.3e-4, Love 8.9e-6 (before the fix: 4.7e-4, 2.0e-4 - but
# the flat bound is not what separates them, the continuity criterion is: worst near / far 1.9 here, 32..58 before the fix)
FLAT_BOUND = {2: 3e-4, 1: 2e-5}


def near_velocity_battery(kind, water=False):
    """stacks [nstk, 4, L] and trials: c within 1..4096 ulps of each layer's alpha (Rayleigh) or beta (both) in turn, and
    10^3..10^4 ulps away (the same stack's 'far' reference for the continuity criterion)."""
    from pysurfinv_amd import synth
    if water:
        m = synth.sediment_models(6, 9, seed=21, water=True)
    else:
        m = np.concatenate([synth.synth_models(4, 8, seed=22, total_thickness=40.0),
                            synth.sediment_models(4, 8, seed=23)])
    stacks = np.stack([m[:, 0], m[:, 1], m[:, 2], m[:, 3]], 1).astype(np.float32)     # (a, b, rho, d); last layer = half space
    nstk, _, L = stacks.shape
    rng = np.random.default_rng(31 + kind + 2 * water)
    near = np.concatenate([np.arange(1, 65), [128, 256, 512, 1024, 2048, 4096]])
    far = np.unique(np.geomspace(1000, 10000, 40).astype(int))
    tst, c, T, tag = [], [], [], []                          # tag: (stack, layer-velocity id, far?, ulps)
    for s in range(nstk):
        vels = []
        for j in range(L - 1):
            if stacks[s, 1, j] > 0:
                vels.append(stacks[s, 1, j])
            if kind == 2:
                vels.append(stacks[s, 0, j])
        for vid, v in enumerate(vels):
            Tp = float(np.float32(rng.uniform(3.0, 150.0)))
            for k, isfar in [(k, 0) for k in near] + [(k, 1) for k in far]:
                for sgn in (-1.0, 1.0):
                    tst.append(s); c.append(np.float32(v * (1.0 + sgn * k * ULP))); T.append(Tp); tag.append((s, vid, isfar, k))
    return stacks, np.full(nstk, L), np.array(tst), _f32(c), _f32(T), np.array(tag)


def whole_errors(P, kind, mode, water=False):
    stacks, mmax, tst, c, T, tag = near_velocity_battery(kind, water)
    o = run_secular(P, stacks, mmax, tst, c, T, kind, mode).astype(np.float64)
    sd = stacks.astype(np.float64)
    e = np.full(len(c), np.nan)
    for i in range(len(c)):
        a, b, rho, d = sd[tst[i]]
        if kind == 2:
            v, mag, _ = s64.delta_rayleigh(a, b, rho, d, int(mmax[tst[i]]), float(c[i]), float(T[i]))
        else:
            v, mag, _ = s64.delta_love(b, rho, d, int(mmax[tst[i]]), float(c[i]), float(T[i]))
        if np.isfinite(o[i]).all() and np.isfinite(mag) and mag > 0 and o[i, 1] < 1e37:
            e[i] = abs(o[i, 0] - v) / mag
    return e, tag


def continuity(e, tag):
    """per (stack, layer velocity): worst error within +-64 ulps against the worst 10^3..10^4 ulps away"""
    out = []
    for key in {(int(t[0]), int(t[1])) for t in tag}:
        sel = (tag[:, 0] == key[0]) & (tag[:, 1] == key[1]) & np.isfinite(e)
        near, far = e[sel & (tag[:, 2] == 0) & (tag[:, 3] <= 64)], e[sel & (tag[:, 2] == 1)]
        if near.size and far.size:
            out.append((near.max(), far.max(), key))
    return out


@pytest.mark.parametrize("kind,mode,water", [(2, 0, False), (2, 1, False), (1, 2, False), (2, 0, True), (1, 2, True)])
def test_secular_function_continuous_at_layer_velocities(probe, kind, mode, water):
    e, tag = whole_errors(probe, kind, mode, water)
    assert np.isfinite(e).sum() > 0.5 * e.size
    flat = float(np.nanmax(e))
    cont = continuity(e, tag)
    worst = max(cont, key=lambda t: t[0] / max(t[1], 1e-30))
    print(f"kind {kind} mode {mode} water {water}: worst |f32 - f64|/mag {flat:.3e} (bound {FLAT_BOUND[kind]:.0e}); "
          f"worst near/far {worst[0]:.3e} / {worst[1]:.3e} = {worst[0] / max(worst[1], 1e-30):.2f} at {worst[2]}")
    assert flat < FLAT_BOUND[kind]
    for near, far, key in cont:
        assert near <= 3.0 * far + 1e-7, (key, near, far)


# measured: Rayleigh 7.9e-3 (the same before the fix: u1 = g^2 b1 + 2 g h3 - h5 cancels where c is far below a rock layer's S
# velocity, g = 2 b^2 / c^2 in the hundreds - soft sediments over rock, the case the ellipticity kernel hands to the exact path),
# Love 1.3e-5
RANDOM_BOUND = {2: 2e-2, 1: 3e-5}


def test_secular_function_random_stacks(probe):
    from pysurfinv_amd import synth
    worsts = []
    for kind, mode in ((2, 0), (2, 1), (1, 2)):
        m = np.concatenate([synth.synth_models(64, 10, seed=41), synth.sediment_models(64, 10, seed=42)])
        stacks = np.stack([m[:, 0], m[:, 1], m[:, 2], m[:, 3]], 1).astype(np.float32)
        rng = np.random.default_rng(43)
        n = 4096
        tst = rng.integers(0, len(m), n)
        c = _f32(stacks[tst, 1, :].min(1) * rng.uniform(0.9, 1.3, n)); T = _f32(rng.uniform(3.0, 150.0, n))
        o = run_secular(probe, stacks, np.full(len(m), 10), tst, c, T, kind, mode).astype(np.float64)
        sd = stacks.astype(np.float64)
        worst = 0.0
        for i in range(n):
            a, b, rho, d = sd[tst[i]]
            if kind == 2:
                v, mag, _ = s64.delta_rayleigh(a, b, rho, d, 10, float(c[i]), float(T[i]))
            else:
                v, mag, _ = s64.delta_love(b, rho, d, 10, float(c[i]), float(T[i]))
            if np.isfinite(o[i]).all() and np.isfinite(mag) and mag > 0 and o[i, 1] < 1e37:
                worst = max(worst, abs(o[i, 0] - v) / mag)
        print(f"random stacks kind {kind} mode {mode}: worst |f32 - f64|/mag {worst:.3e}")
        worsts.append((worst, kind))
    for worst, kind in worsts:
        assert worst < RANDOM_BOUND[kind]


# ------------------------------------------------------------------------------------------------- 4. the forward path
TEAMS = (0, 1, 2, 4, 8, 16, 64)


def _dif(h, i):
    """earth-flattening velocity factor of regular layer i (prep_stack): the working stack's velocity / the model's"""
    R0 = 6371.0
    r_i = R0 - float(np.sum(h[:i], dtype=np.float64)); r_n = r_i - float(h[i])
    return (1.0 / r_n - 1.0 / r_i) * R0 / np.log(r_i / r_n)


def _oracle_c(model, per, kind, variant=0):
    from oracle import cport
    cport.lib().surfdisp_oracle_set_variant(variant)
    try:
        c, _, _ = cport.forward_batch(model[None], per, kind)
    finally:
        cport.lib().surfdisp_oracle_set_variant(0)
    return c[0]


def velocity_on_root_stack(kind):
    """Rayleigh: 43 layers of 1.36 km over a half space, T = 141.6 s, the top layer's (working-stack) P velocity moved onto
    the oracle's root (#290); Love: a 10-layer stack whose fifth layer's S velocity sits on the root of its longest period."""
    if kind == 2:
        L = 44
        vs = np.concatenate([np.linspace(2.45, 3.95, L - 1), [4.6]])
        vp = 1.75 * vs; vp[0] = 4.3
        h = np.full(L, 1.36); h[-1] = 0.0
        per = np.array([40.0, 80.0, 141.6], np.float32)
        j, row = 0, 0
    else:
        L = 10
        vs = np.array([2.6, 2.9, 3.1, 3.3, 3.55, 3.7, 3.9, 4.1, 4.3, 4.7])
        vp = 1.75 * vs
        h = np.array([3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0, 15.0, 20.0, 0.0])
        per = np.array([10.0, 20.0, 30.0], np.float32)
        j, row = 4, 1
    rho = 0.541 + 0.3601 * vp
    model = np.stack([vp, vs, rho, h, np.zeros(L)]).astype(np.float32)
    f = _dif(model[3], j)

    def gap(v):                                               # the last period's root with the layer's working velocity v, - v
        model[row, j] = np.float32(v / f)
        if kind == 1:
            model[0, j] = np.float32(1.75 * model[1, j]); model[2, j] = np.float32(0.541 + 0.3601 * model[0, j])
        return float(_oracle_c(model, per, kind)[-1]) - float(model[row, j]) * f
    v0 = float(_oracle_c(model, per, kind)[-1]); g0 = gap(v0)
    v1 = v0 + g0; g1 = gap(v1)
    for _ in range(8):                                        # secant steps onto root == velocity
        if g1 == g0 or abs(g1) < 2.0 ** -24 * v1:
            break
        v0, g0, v1 = v1, g1, v1 - g1 * (v1 - v0) / (g1 - g0)
        g1 = gap(v1)
    return model, per, float(model[row, j]) * f


@pytest.mark.parametrize("kind", [2, 1])
def test_forward_with_a_layer_velocity_on_the_root(probe, kind):
    """Every team size must return the oracle's roots (1e-4, same zero pattern) where the oracle's variants 1-3 agree to
    2e-5 - a regression test of the forward path at the construction that exposed the defect.  It passed on the build
    before the small-argument sinh fix too (no team size converged onto the jump here): not a detector of that defect."""
    from pysurfinv_amd import _lib, forward
    model, per, vel = velocity_on_root_stack(kind)
    co = _oracle_c(model, per, kind)
    print(f"kind {kind}: layer velocity {vel:.7f}, oracle root {co[-1]:.7f}")
    assert abs(co[-1] / vel - 1) < 1e-6
    var = np.array([_oracle_c(model, per, kind, v) for v in (1, 2, 3)])
    with np.errstate(all="ignore"):
        defined = np.all(np.abs(var / co - 1) < 2e-5, axis=0) & (co > 0)
    assert defined[-1]
    for team in TEAMS:
        _lib.lib().surfdisp_set_team(team)
        try:
            c, _, _ = forward.forward_batch(model[None], per, kind)
        finally:
            _lib.lib().surfdisp_set_team(0)
        c = c[0]
        print(f"  team {team}: c {c}  oracle {co}")
        assert np.array_equal(c > 0, co > 0), (team, c, co)
        assert np.all(np.abs(c[defined] / co[defined] - 1) < 1e-4), (team, c, co)
