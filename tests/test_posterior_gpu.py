"""surfdisp_posterior_profile_device (csrc/surfdisp_post.hip) against the numpy statement posterior.posterior_reference and the
reference PostPoint's fixture (tests/golden/ref_post.npz).  Bars: 1e-9 for the Vs statistics (the project's bar for
Model1D.value against that fixture; mean, std, min and max are 1-Lipschitz in the values), 1e-12 for the parameter means (the bar
of avg_params in tests/test_mcmc.py); the selection, the counts and the histograms exactly - the latter while no value lies within
1e-9 of a bin edge, which every test asserts.  The measured maxima of an MI355X run are in profiles/posterior/parity.txt."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "golden")]
from settings import CONT, OCEAN                     # noqa: E402
from settings_therm import HYBRID_STATIC             # noqa: E402
from posterior_cases import (CHUNK_DEPTHS, DEPTHS, DEV, _carry_track, _close, _edges, _fixture_track, _local_case, _random_track,   # noqa: E402
                             _same, _slab_plus_one_track)
from pysurfinv_amd.layers_batch import Model1DBatch  # noqa: E402
from pysurfinv_amd import posterior, _lib            # noqa: E402

pytestmark = pytest.mark.gpu

GP = np.load(os.path.join(HERE, "golden", "ref_post.npz"), allow_pickle=True)
G = np.load(os.path.join(HERE, "golden", "ref_driver.npz"))
HIST = (1.0, 5.0, 400)


def _final_values(mb, track, zdeps, rows=None, **sel):
    """Vs at depth of every final row, per point (what the histograms count): list of [n_final, D]."""
    _, _, _, final, src = posterior.select_reference(track, sel.get("true_markov_chain", True), sel.get("chainL"), sel.get("prefix"))
    out = []
    if rows is None and mb.n_aux:
        rows = np.arange(track.shape[0])
    for p in range(track.shape[0]):
        par = track[p, src[p][final[p]], 3:]
        out.append(mb.value(torch.as_tensor(par), zdeps, rows=None if rows is None else np.full(par.shape[0], rows[p]))
                   if par.shape[0] else np.zeros((0, len(zdeps))))
    return out


def _check(label, mb_dev, mb_cpu, track, zdeps, hist=HIST, rows=None, **sel):
    """One device call against the statement on the same track; returns the device result."""
    dev = posterior.posterior_profiles(mb_dev, torch.from_numpy(track).to(DEV), zdeps, rows=rows, hist=hist, **sel)
    torch.cuda.synchronize()
    ref = posterior.posterior_reference(mb_cpu, torch.from_numpy(track), zdeps, rows=rows, hist=hist, **sel)
    assert set(dev) == set(ref)
    for k in ("min_misfit", "thres", "imin", "n_final", "count"):
        assert torch.equal(dev[k].cpu(), ref[k]), (label, k)
    _close(f"{label} pmean", dev["pmean"], ref["pmean"], 1e-12)
    _close(f"{label} pstd", dev["pstd"], ref["pstd"], 1e-9)
    for k in ("vs_mean", "vs_std", "vs_min", "vs_max"):
        _close(f"{label} {k}", dev[k], ref[k], 1e-9)
    if hist is not None:
        edges = _edges(hist)
        for v in _final_values(mb_cpu, track, zdeps, rows=rows, **sel):
            v = v[np.isfinite(v)]
            if v.size:
                assert np.abs(v[:, None] - edges[None, :]).min() > 1e-9, label      # exactness is a fair demand
        for k in ("hist", "below", "above"):
            assert torch.equal(dev[k].cpu(), ref[k]), (label, k)
        _close(f"{label} quantiles", dev["quantiles"], ref["quantiles"], 1e-9)
    return dev


# ------------------------------------------------------------------ 1. the reference PostPoint's fixture
def test_fixture_parity_from_the_device_entry():
    mb, mbc = Model1DBatch(CONT, device=DEV), Model1DBatch(CONT)
    fx = _fixture_track()
    p1 = np.concatenate([fx[160:240], fx[0:80], fx[80:160]])             # its three chains in the order 2, 0, 1
    p2 = fx.copy(); p2[:80, 0] = 88888.0
    track = np.stack([fx, p1, p2])
    for tmc, key in ((True, "tmc"), (False, "raw")):
        dev = _check(f"fixture {key}", mb, mbc, track, GP["zdeps"], true_markov_chain=tmc)
        vz = GP[f"{key}/values_z"]
        edges = _edges(HIST)
        assert np.abs(vz[:, :, None] - edges[None, None, :]).min() > 1e-9
        assert float(dev["min_misfit"][0]) == float(GP[f"{key}/min_misfit"]) and float(dev["thres"][0]) == float(GP[f"{key}/thres"])
        assert int(dev["n_final"][0]) == 43 and (dev["count"][0].cpu().numpy() == 43).all()
        assert np.abs(dev["pmean"][0].cpu().numpy() - GP[f"{key}/avg_params"]).max() < 1e-12
        for k, want in (("vs_mean", vz.mean(axis=1)), ("vs_std", vz.std(axis=1)), ("vs_min", vz.min(axis=1)), ("vs_max", vz.max(axis=1))):
            err = np.abs(dev[k][0].cpu().numpy() - want).max()
            print(f"PARITY fixture {key} {k} against the reference PostPoint: {err:.3e} (bar 1e-09)")
            assert err < 1e-9, (k, err)
        h = dev["hist"][0].cpu().numpy()
        for d in range(37):
            assert np.array_equal(h[d], np.histogram(vz[d], edges)[0]), d


# ------------------------------------------------------------------ 2. the carry across tile and slab boundaries
@pytest.mark.parametrize("sel", [dict(), dict(true_markov_chain=False), dict(chainL=263, prefix=100)], ids=["tmc", "raw", "prefix"])
def test_boundary_carry(sel):
    mb, mbc = Model1DBatch(CONT, device=DEV), Model1DBatch(CONT)
    _check(f"carry {sel}", mb, mbc, _carry_track(mbc), DEPTHS, **sel)


def test_one_row_past_a_slab():
    mb, mbc = Model1DBatch(CONT, device=DEV), Model1DBatch(CONT)
    R = posterior.SLAB_ROWS + 1
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "surfdisp.h")).read()
    assert f"#define SURFDISP_POST_SLAB_ROWS {posterior.SLAB_ROWS}\n" in hdr
    tr = _slab_plus_one_track(mbc)
    dev = _check("slab + 1", mb, mbc, tr, DEPTHS)
    assert int(dev["imin"][0]) == R - 1
    two = _check("slab + 1, two depth chunks", mb, mbc, tr, CHUNK_DEPTHS[65])     # two slabs x two chunks of partials
    assert int(two["n_final"][0]) == int(dev["n_final"][0]) and torch.equal(two["pmean"], dev["pmean"])


# ------------------------------------------------------------------ 2b. more than one chunk of 64 depths (CHUNK_DEPTHS)
@pytest.mark.parametrize("D", [65, 200, 256])
def test_more_than_one_depth_chunk(D):
    mb, mbc = Model1DBatch(CONT, device=DEV), Model1DBatch(CONT)
    zd = CHUNK_DEPTHS[D]
    assert zd.size == D <= posterior.DEPTHS_MAX
    tr = _carry_track(mbc)
    dev = _check(f"{D} depths", mb, mbc, tr, zd)
    few = _check(f"{D} depths, every 8th alone", mb, mbc, tr, zd[::8], hist=None)
    for k in ("count", "vs_mean", "vs_std", "vs_min", "vs_max"):             # a depth's figures do not depend on its chunk or lane
        assert torch.equal(torch.nan_to_num(dev[k][:, ::8].double(), nan=-7.0), torch.nan_to_num(few[k].double(), nan=-7.0)), k
    for k in ("pmean", "pstd", "n_final"):
        assert torch.equal(dev[k], few[k]), k
    if D == 200:
        assert bool((dev["count"][:, :3] == 0).all()) and bool((dev["count"][:, -40:] == 0).all())    # above 0 km, below 208 km
        assert bool((dev["count"][:, 60:70] == dev["n_final"][:, None]).all())                        # chunk 0 / chunk 1, inside
    _check(f"{D} depths, prefix", mb, mbc, tr, zd, chainL=263, prefix=100)


# ------------------------------------------------------------------ 3. degenerate sets
def test_degenerate_sets():
    mb, mbc = Model1DBatch(CONT, device=DEV), Model1DBatch(CONT)
    tr = _random_track(mbc, 2, 300, seed=13)
    tr[0, :, 0] = 5.0; tr[0, 123, 0] = 1.0        # point 0: exactly one final row
    dev = _check("one final row", mb, mbc, tr, DEPTHS)
    assert int(dev["n_final"][0]) == 1
    inside = dev["count"][0] == 1
    assert bool(inside[:9].all()) and int(dev["count"][0, -1]) == 0      # down to 180 km every model has a value
    assert bool((dev["vs_std"][0][inside] == 0).all())
    assert torch.equal(dev["vs_min"][0][inside], dev["vs_max"][0][inside]) and torch.equal(dev["vs_min"][0][inside], dev["vs_mean"][0][inside])
    assert bool((dev["pstd"][0] == 0).all())
    # D = 1, and no histogram: the three arrays and the quantiles are absent
    one = _check("D = 1", mb, mbc, tr, [20.3], hist=None)
    assert "hist" not in one and "quantiles" not in one and one["count"].shape == (2, 1)
    assert torch.equal(one["vs_mean"][:, 0], dev["vs_mean"][:, 4])          # the same bits in another lane
    # depths outside every model: count 0 and NaN there, the others as before
    out = _check("outside", mb, mbc, tr, [-1.0, 20.3, 100.0, 250.0])
    assert bool((out["count"][:, [0, 3]] == 0).all()) and bool(torch.isnan(out["vs_mean"][:, [0, 3]]).all())
    assert torch.equal(out["vs_mean"][:, 1], dev["vs_mean"][:, 4]) and torch.equal(out["vs_mean"][:, 2], dev["vs_mean"][:, 7])
    # a final row whose crust coefficient is NaN: its crust depths drop out, the other depths and rows do not notice
    bad = tr.copy()
    fin1 = np.where(bad[1, :, 0] < 1.0)[0]
    bad[1, fin1[2], 2] = 1.0; bad[1, fin1[2], 3 + 5] = np.nan             # (an accepted row keeps its own parameters)
    res = _check("NaN parameter", mb, mbc, bad, DEPTHS)
    crust = [4]                                    # 20.3 km lies in every model's crust (sediment <= 3.5 km, Moho >= 25.5 km)
    ok = _check("NaN parameter, clean twin", mb, mbc, tr, DEPTHS)
    assert bool((res["count"][1, crust] < ok["count"][1, crust]).all()) and torch.equal(res["count"][1, 7:9], ok["count"][1, 7:9])
    assert torch.equal(res["vs_mean"][0, :9], ok["vs_mean"][0, :9])


# ------------------------------------------------------------------ 4. reproducibility
@pytest.mark.parametrize("depths", [DEPTHS, CHUNK_DEPTHS[200]], ids=["one chunk", "four chunks"])
def test_two_calls_give_the_same_bits(depths):
    mb = Model1DBatch(CONT, device=DEV)
    tr = torch.from_numpy(_carry_track(Model1DBatch(CONT))).to(DEV)
    a = posterior.posterior_profiles(mb, tr, depths, hist=HIST)
    b = posterior.posterior_profiles(mb, tr, depths, hist=HIST)
    torch.cuda.synchronize()
    c = posterior.posterior_profiles(mb, tr.flip(0).contiguous(), depths, hist=HIST)
    torch.cuda.synchronize()
    for k in a:
        assert _same(a[k], b[k]), k
        assert _same(a[k], c[k].flip(0)), k


# ------------------------------------------------------------------ 5. per-point constants
@pytest.mark.parametrize("name", ["cont", "ocean"])
def test_per_point_constants(name):
    """The settings of tests/test_local_info.py are thermal, non-static or carry the Gaussian crust term - none has a native
    descriptor the entry supports -, so: CONT with a per-point topography and mantle thickness, and a static ocean structure
    (water layer, BottomDepth mantle) with a per-point topography."""
    setting, keys, table, rows, zd = _local_case(name)
    mb = Model1DBatch(setting, device=DEV, local_keys=keys).set_local_info(table)
    mbc = Model1DBatch(setting, local_keys=keys).set_local_info(table)
    assert mb.native_descriptor() is not None and not mb._native_thermal
    tr = _random_track(mbc, 3, 300, seed=14)
    dev = _check(f"local {name}", mb, mbc, tr, zd, rows=rows)
    assert not torch.equal(dev["count"][0], dev["count"][1])             # the points' tops differ, and it shows
    _check(f"local {name}, rows = None", mb, mbc, tr, zd)                        # point p reads table row p


# ------------------------------------------------------------------ 5b. the descriptor zoo
ZOO_HIST = (1.003, 5.003, 400)        # the zoo's constant velocities (2.4, 3.9, 4.05, ...) would sit on the edges of HIST
ZOO_DEPTHS = [-0.7, 0.5, 1.2, 2.2, 2.7, 3.5, 4.6, 8.0, 15.0, 25.0, 31.0, 50.0, 100.0, 179.0, 185.0, 205.0]


@pytest.mark.parametrize("name", ["ten", "pairs", "moho"])
def test_descriptor_zoo_settings(name):
    """tests/descriptor_zoo.py: the cap of ten input layers (SURFDISP_POST_MAX_LAYERS), two layers per group with an 8-slot mantle,
    and a BottomDepth on a middle layer under a per-point topography.  The bars of _check."""
    import descriptor_zoo as Z
    mb, mbc = Z.zoo_model(name, DEV), Z.cpu_model(name)
    assert mb.native_descriptor() is not None and not mb._native_thermal
    npnt = 4 if name == "moho" else 3
    tr = _random_track(mbc, npnt, 300, seed=16)
    dev = _check(f"zoo {name}", mb, mbc, tr, ZOO_DEPTHS, hist=ZOO_HIST, rows=np.array([2, 0, 3, 1]) if name == "moho" else None)
    assert int(dev["count"].max()) > 0 and bool((dev["count"][:, 0] == 0).all())   # -0.7 km lies above every stack



def test_argument_errors_return_before_launch():
    mb = Model1DBatch(CONT, device=DEV)
    idesc, fdesc = posterior._host_descriptor(mb)
    L = _lib.lib()
    npnt, R, N, D = 2, 120, mb.spec.n, 3
    track = torch.from_numpy(_random_track(Model1DBatch(CONT), npnt, R, seed=15)).to(DEV)
    f64, i32 = dict(dtype=torch.float64, device=DEV), dict(dtype=torch.int32, device=DEV)
    outs = ([torch.full((npnt,), -5.0, **f64) for _ in range(2)] + [torch.full((npnt,), -5, **i32) for _ in range(2)]
            + [torch.full((npnt, N), -5.0, **f64) for _ in range(2)] + [torch.full((npnt, D), -5, **i32)]
            + [torch.full((npnt, D), -5.0, **f64) for _ in range(4)]
            + [torch.full((npnt, D, 8), -5, **i32), torch.full((npnt, D), -5, **i32), torch.full((npnt, D), -5, **i32)])
    ws = torch.zeros(int(L.surfdisp_posterior_workspace_bytes(npnt, R, N, D)), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0 and L.surfdisp_posterior_workspace_bytes(0, R, N, D) == 0
    zd = np.array([1.0, 20.0, 100.0])
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(npoints=npnt, R=R, N=N, track=track.data_ptr(), stride=3 + N, idesc=idesc, fdesc=fdesc.data_ptr(), aux=None, K=0,
                 D=D, zd=zd, tmc=1, chainL=0, prefix=0, nbins=8, vlo=1.0, vhi=5.0, outs=[o.data_ptr() for o in outs],
                 ws=ws.data_ptr(), ws_bytes=ws.numel())
        a.update(kw)
        ide = None if a["idesc"] is None else np.ascontiguousarray(a["idesc"], np.int32)
        z = None if a["zd"] is None else np.ascontiguousarray(a["zd"], np.float64)
        return L.surfdisp_posterior_profile_device(
            ctypes.c_void_p(stream), a["npoints"], a["R"], a["N"], ctypes.c_void_p(a["track"]), a["stride"],
            None if ide is None else ide.ctypes.data_as(ctypes.c_void_p), idesc.size if ide is None else ide.size,
            ctypes.c_void_p(a["fdesc"]), ctypes.c_void_p(a["aux"]), a["K"], None,
            a["D"], None if z is None else z.ctypes.data_as(ctypes.c_void_p), a["tmc"], a["chainL"], a["prefix"], a["nbins"],
            a["vlo"], a["vhi"], *[ctypes.c_void_p(p) for p in a["outs"]], ctypes.c_void_p(a["ws"]), a["ws_bytes"])

    def desc_with(at, value):
        d = idesc.copy(); d[at] = value
        return d

    def outs_without(i):
        p = [o.data_ptr() for o in outs]; p[i] = None
        return p

    nin = int(idesc[0])
    assert nin == 3 and idesc.size >= 4 + 16 * nin
    lay = lambda l, field: 4 + 8 * l + field          # layer l's ints: kind, thickness slot, BottomDepth, coefficients, grid begin, end
    cases = dict(npoints=dict(npoints=0), R=dict(R=0), N=dict(N=0), stride=dict(stride=2 + N), D0=dict(D=0),
                 Dcap=dict(D=posterior.DEPTHS_MAX + 1, zd=np.arange(posterior.DEPTHS_MAX + 1.0)),
                 N_big=dict(N=129, stride=3 + 129), R_big=dict(R=2**30 + 1), slabs_big=dict(npoints=2**31 - 1, R=posterior.SLAB_ROWS + 1),
                 K_negative=dict(K=-1),
                 descending=dict(zd=[1.0, 100.0, 20.0]), equal=dict(zd=[1.0, 20.0, 20.0]), nan_depth=dict(zd=[1.0, np.nan, 100.0]),
                 inf_depth=dict(zd=[1.0, 20.0, np.inf]),
                 vhi=dict(vhi=1.0), nbins=dict(nbins=0), vlo_nan=dict(vlo=np.nan), vhi_nan=dict(vhi=np.nan), vhi_inf=dict(vhi=np.inf),
                 vlo_inf=dict(vlo=-np.inf),
                 prefix0=dict(chainL=60, prefix=0), prefix_big=dict(chainL=60, prefix=61), not_multiple=dict(chainL=50, prefix=10),
                 thermal=dict(idesc=desc_with(lay(2, 0), 6)),                 # the mantle's kind
                 kind_unknown=dict(idesc=desc_with(lay(1, 0), 8)), kind_negative=dict(idesc=desc_with(lay(1, 0), -1)),
                 no_layer=dict(idesc=desc_with(0, 0)), eleven_layers=dict(idesc=desc_with(0, 11)),
                 slot=dict(idesc=desc_with(lay(0, 1), N)),                    # a thickness slot behind the row, with no aux table
                 slot_negative=dict(idesc=desc_with(lay(0, 1), -2)),
                 coef_count=dict(idesc=desc_with(lay(1, 3), 9)),
                 coef_slot=dict(idesc=desc_with(4 + 8 * nin + 8 * 1, N)),     # the crust's first coefficient, behind the row
                 topo_slot=dict(idesc=desc_with(lay(0, 6), N + 1)),
                 grid_gap=dict(idesc=desc_with(lay(1, 4), int(idesc[lay(1, 4)]) + 1)),
                 grid_one_point=dict(idesc=desc_with(lay(2, 5), int(idesc[lay(2, 4)]) + 1)),
                 grid_short=dict(idesc=desc_with(1, int(idesc[1]) + 1)),      # the ranges end before ngrid
                 short_desc=dict(idesc=idesc[:20]), tiny_desc=dict(idesc=idesc[:3]),
                 no_track=dict(track=None), no_idesc=dict(idesc=None), no_fdesc=dict(fdesc=None), no_zdeps=dict(zd=None),
                 no_workspace=dict(ws=None), aux_missing=dict(K=1), small_ws=dict(ws_bytes=ws.numel() - 1),
                 pmean_alone=dict(outs=outs_without(5)), pstd_alone=dict(outs=outs_without(4)),
                 no_below=dict(outs=outs_without(12)), no_above=dict(outs=outs_without(13)))
    for i, nm in ((0, "min_misfit"), (1, "thres"), (2, "imin"), (3, "n_final"), (6, "count"), (7, "vs_mean"), (8, "vs_std"),
                  (9, "vs_min"), (10, "vs_max")):
        cases[f"no_{nm}"] = dict(outs=outs_without(i))
    for name, kw in cases.items():
        assert call(**kw) == _lib.ERR_INVALID, name
        assert b"invalid" in L.surfdisp_last_error(), name
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == -5).all())                                    # nothing was written
    assert call() == _lib.SUCCESS and call(chainL=60, prefix=60) == _lib.SUCCESS
    torch.cuda.synchronize()
    assert bool((outs[6] >= 0).all()) and int(outs[11].sum() + outs[12].sum() + outs[13].sum()) == int(outs[6].sum())
    for bad in (HYBRID_STATIC, OCEAN):
        with pytest.raises(ValueError):
            posterior.posterior_profiles(Model1DBatch(bad, device=DEV), torch.zeros((1, 4, 3 + Model1DBatch(bad).spec.n),
                                                                                  dtype=torch.float64, device=DEV), zd)


def test_model_and_track_on_different_devices():
    """The kernel reads the descriptor's float part through a device pointer: a model built on the host (Model1DBatch's default)
    with a device track is an error of the caller, said as one."""
    mbc = Model1DBatch(CONT)
    track = torch.from_numpy(_random_track(mbc, 1, 60, seed=16)).to(DEV)
    with pytest.raises(ValueError, match="device"):
        posterior.posterior_profiles(mbc, track, DEPTHS)
    torch.cuda.synchronize()
    assert int(posterior.posterior_profiles(Model1DBatch(CONT, device=DEV), track, DEPTHS)["n_final"][0]) >= 1


# ------------------------------------------------------------------ 7. end to end
def test_point_to_profile_end_to_end(tmp_path):
    from pysurfinv_amd.point import Point, PostPoint
    pt = Point(CONT, periods=list(G["trace/periods"]), vels=list(G["trace/c_obs"]), uncers=list(G["trace/uncer"]), device=DEV)
    pt.MCinvMP(outdir=str(tmp_path), pid="here", runN=600, chainL=60, seed=3)
    f = os.path.join(str(tmp_path), "here.npz")
    z = GP["zdeps"]
    a = PostPoint(f, device=DEV).profile(z, hist=HIST)
    b = PostPoint(f, device=None).profile(z, hist=HIST)
    assert set(a) == set(b) and a["n_final"] == b["n_final"] >= 1 and a["thres"] == b["thres"]
    assert np.array_equal(a["count"], b["count"])
    for k in ("mean", "std", "min", "max", "pstd"):
        err = np.nanmax(np.abs(a[k] - b[k]))
        print(f"PARITY end to end {k}: {err:.3e} (bar 1e-09)")
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])) and err < 1e-9, k
    assert np.abs(a["pmean"] - b["pmean"]).max() < 1e-12
    # convergence: the last prefix is the whole chain
    p = PostPoint(f, device=DEV)
    mb = p.initMod
    track = torch.as_tensor(p.MC[None], dtype=torch.float64, device=DEV)
    cv = posterior.convergence(mb, track, z, chainL=60)
    full = posterior.posterior_profiles(mb, track, z)
    assert cv["prefixes"][0] == 6 and cv["prefixes"][-1] == 60 and cv["mean"].shape == (20, 1, len(z))
    assert torch.equal(cv["mean"][-1], full["vs_mean"]) and torch.equal(cv["std"][-1], full["vs_std"])
    host = posterior.convergence(Model1DBatch(p.setting), torch.from_numpy(p.MC[None]), z, chainL=60)
    _close("convergence mean", cv["mean"], host["mean"], 1e-9)
    _close("convergence std", cv["std"], host["std"], 1e-9)


# ------------------------------------------------------------------ 8. run_grid(..., profile_depths=...) on the device
@pytest.mark.parametrize("local", [False, True], ids=["plain", "local info"])
def test_grid_profiles_on_the_device(local, monkeypatch):
    """One rank on the GPU: the profiles come from the device entry on the tracks while they are on the device (with local
    information: point p reads row p of the rank's table) and equal the statement on the returned tracks."""
    from pysurfinv_amd import grid
    npts, zd = 5, [-0.5, 0.5, 3.0, 20.0, 60.0, 150.0, 400.0]
    c = np.tile(G["trace/c_obs"], (npts, 1)) * (1 + 0.002 * np.arange(npts)[:, None])
    u = np.tile(G["trace/uncer"], (npts, 1))
    keys = ["topo", "Mantle.H"] if local else None
    table = np.array([[-1.0, 152.0], [0.7, 160.0], [2.2, 171.5], [0.0, 155.0], [1.1, 165.0]]) if local else None
    calls, entry = [], posterior.posterior_profiles
    monkeypatch.setattr(posterior, "posterior_profiles", lambda *a, **k: calls.append(a[1].device.type) or entry(*a, **k))
    r = grid.run_grid(Model1DBatch(CONT, device=DEV, local_keys=keys), np.arange(npts), np.arange(npts), G["trace/periods"], c, u,
                      8, 20, outdir=None, device=DEV, seed=2, local_info=table, profile_depths=zd)
    assert calls == ["cuda"]
    prof = r["profiles"]
    assert sorted(prof) == ["count", "max", "mean", "min", "std", "zdeps"] and prof["count"].dtype == np.int64
    mbc = Model1DBatch(CONT, local_keys=keys)
    if local:
        mbc.set_local_info(table)
    ref = posterior.posterior_reference(mbc, torch.from_numpy(r["mcTrack"]), zd, rows=np.arange(npts) if local else None)
    assert np.array_equal(prof["count"], ref["count"].numpy())
    assert (prof["count"][:, 0] > 0).any() == local                          # -0.5 km: inside a model only where the point has topography
    assert (prof["count"][:, -1] == 0).all() and (prof["count"][:, 3] >= 1).all()
    for k, rk in (("mean", "vs_mean"), ("std", "vs_std"), ("min", "vs_min"), ("max", "vs_max")):
        a, b = prof[k], ref[rk].numpy()
        assert a.shape == (npts, len(zd)) and np.array_equal(np.isnan(a), np.isnan(b))
        err = float(np.nanmax(np.abs(a - b)))
        print(f"PARITY grid {'local' if local else 'plain'} {k}: {err:.3e} (bar 1e-09)")
        assert err < 1e-9, (k, err)
