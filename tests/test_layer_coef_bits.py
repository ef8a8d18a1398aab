"""CPU checks that layer_coef (one wave type's coefficients in one layer of the Rayleigh and Love recursions) and sincos_cw
give, bit for bit, what the form they replace gave: r and 1/r signed by copysignf before the evanescent / oscillatory branch,
and the quadrant signs of sin and cos applied by selects.  Both forms are compiled for the host by
tests/hostcheck/lcoefcheck.hip, the old one as a copy in that file.  NaN compares equal to NaN.
No GPU needed; skipped if hipcc is absent."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcheck")
FIELDS = ("r", "rsin", "sinr", "cs", "x", "ph")
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(hostbuild.build(os.path.join(HC, "lcoefcheck.hip"), os.path.join(HC, "liblcoefcheck.so")))
    L.lc_pairs.restype = ctypes.c_int
    L.lc_pairs.argtypes = [ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    L.lc_random.restype = ctypes.c_long
    L.lc_random.argtypes = [ctypes.c_uint64, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    L.sincos_sweep.restype = None
    L.sincos_sweep.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_uint32),
                               ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_uint32)]
    return L


def _pairs(L, arg, wd):
    arg, wd = np.broadcast_arrays(np.asarray(arg, f32), np.asarray(wd, f32))
    arg, wd = np.ascontiguousarray(arg.ravel()), np.ascontiguousarray(wd.ravel())
    idx = np.zeros(8, np.int64); mask = np.zeros(8, np.int32)
    nd = L.lc_pairs(arg.size, arg.ctypes.data, wd.ctypes.data, 8, idx.ctypes.data, mask.ctypes.data)
    rows = [(float(arg[i]), float(wd[i]), [FIELDS[b] for b in range(6) if m >> b & 1]) for i, m in zip(idx[:nd], mask[:nd])]
    return nd, rows


def _sweep(L, lo, hi, parts=32):
    """sincos_sweep over the float bit patterns [lo, hi), in parts on threads (ctypes drops the GIL) ->
    ((count, first offender) old vs new, (count, first offender) not odd)."""
    edges = np.linspace(lo, hi, parts + 1).astype(np.int64)

    def one(k):
        ns, fs, no, fo = ctypes.c_long(0), ctypes.c_uint32(0), ctypes.c_long(0), ctypes.c_uint32(0)
        L.sincos_sweep(int(edges[k]), int(edges[k + 1]), ctypes.byref(ns), ctypes.byref(fs), ctypes.byref(no), ctypes.byref(fo))
        return ns.value, fs.value, no.value, fo.value

    with ThreadPoolExecutor(max_workers=min(parts, os.cpu_count() or 1)) as ex:
        res = list(ex.map(one, range(parts)))
    first = lambda vals: np.uint32(vals[0]).view(f32) if vals else None
    return ((sum(r[0] for r in res), first([r[1] for r in res if r[0]])),
            (sum(r[2] for r in res), first([r[3] for r in res if r[2]])))


def _hi_bits(v):
    return int(np.array(v, f32).view(np.uint32))


def test_sincos_every_float_up_to_1e4(lib):
    """Every float x with 0 < |x| <= 1e4 (all quadrants, both signs, denormals), and +-inf and a NaN: the new sign
    handling of sincos_cw gives what the old selects gave, and sincos_cw(-x) == (-sin, cos) to the bit - what lets
    layer_coef evaluate the oscillatory coefficients at k d |r| whatever the sign of r."""
    (ns, fs), (no, fo) = _sweep(lib, 1, _hi_bits(1.0e4) + 1)
    assert ns == 0, f"{ns} arguments differ from the old form, first {fs!r}"
    assert no == 0, f"{no} arguments are not odd, first {fo!r}"
    (ns, fs), _ = _sweep(lib, _hi_bits(np.inf), _hi_bits(np.inf) + 2, parts=1)   # +-inf and a NaN
    assert ns == 0


def test_special_args(lib):
    """+-0, the 1e-30 clamp and around it, denormals, +-inf and NaNs of both signs, against k d over 1e-6 .. 1e4 (and the
    extremes of the float range)."""
    nan = np.float32(np.nan)
    neg_nan = np.array(0xFFC00000, np.uint32).view(f32)
    special = np.array([0.0, -0.0, 1e-30, -1e-30, np.nextafter(f32(1e-30), f32(0)), np.nextafter(f32(1e-30), f32(1)),
                        -np.nextafter(f32(1e-30), f32(1)), 1e-38, -1e-38, 1e-40, -1e-40, 1.4e-45, -1.4e-45,
                        np.inf, -np.inf, 1e38, -1e38, 3.4e38, -3.4e38, 1.0, -1.0], f32)
    special = np.concatenate([special, [nan, neg_nan]]).astype(f32)
    wd = np.concatenate([np.logspace(-6, 4, 2001), [1e-30, 1e-20, 1e10, 3e38, np.inf, np.nan]]).astype(f32)
    n, rows = _pairs(lib, special[:, None], wd[None, :])
    assert n == 0, rows


def test_every_quadrant(lib):
    """x = k d |r| across every quadrant up to |x| = 1e4, on the oscillatory side with r > 0 (arg = -1, |r| = 1: x = k d)
    and with r < 0 (arg = +0 and a NaN with a clear sign bit: |r| = 1e-15 from the clamp), each multiple of pi/2 with its
    neighbouring floats."""
    rng = np.random.default_rng(5)
    k = np.arange(0, 6367)
    centres = (k * (np.pi / 2)).astype(f32)
    near = [centres]
    for _ in range(3):
        near.append(np.nextafter(near[-1], f32(np.inf)))
    lo = [centres]
    for _ in range(3):
        lo.append(np.nextafter(lo[-1], f32(0)))
    x = np.concatenate(near + lo + [rng.uniform(0, 1e4, 200000).astype(f32)])
    x = x[(x > 0) & (x <= 1e4)]
    n, rows = _pairs(lib, f32(-1.0), x)
    assert n == 0, rows
    ra = f32(f32(1e-30) * (f32(1) / np.sqrt(f32(1e-30))))             # |r| at the clamp (host rsq_hw)
    for arg in (f32(0.0), np.float32(np.nan)):
        n, rows = _pairs(lib, arg, (x / ra).astype(f32))
        assert n == 0, rows
    # a random |r| on the oscillatory side, x spread over the same quadrants
    arg = -(10.0 ** rng.uniform(-8, 3, x.size)).astype(f32)
    ra = np.sqrt(np.abs(arg)).astype(f32)
    n, rows = _pairs(lib, arg, (x / ra).astype(f32))
    assert n == 0, rows


def test_series_edge(lib):
    """The evanescent side around |x| = 1/4, where sinh switches to the series, with |r| from arg = 1 (x = -k d) and
    from random arg > 0."""
    q = f32(0.25)
    wd = [q]
    for _ in range(64):
        wd.append(np.nextafter(wd[-1], f32(1)))
    w2 = [q]
    for _ in range(64):
        w2.append(np.nextafter(w2[-1], f32(0)))
    wd = np.array(wd + w2, f32)
    n, rows = _pairs(lib, f32(1.0), wd)
    assert n == 0, rows
    rng = np.random.default_rng(6)
    arg = (10.0 ** rng.uniform(-6, 3, 100000)).astype(f32)
    x = rng.uniform(0.2499, 0.2501, arg.size)
    n, rows = _pairs(lib, arg, (x / np.sqrt(arg.astype(np.float64))).astype(f32))
    assert n == 0, rows


def test_random_pairs(lib):
    """1e8 random (arg, k d) pairs, in 16 seeded streams."""
    def one(seed):
        out_a = np.zeros(4, f32); out_w = np.zeros(4, f32)
        nd = lib.lc_random(seed, 6_250_000, 4, out_a.ctypes.data, out_w.ctypes.data)
        return nd, list(zip(out_a[:min(nd, 4)].tolist(), out_w[:min(nd, 4)].tolist()))

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        res = list(ex.map(one, range(1, 17)))
    assert sum(n for n, _ in res) == 0, [r for n, r in res if n]


def test_zero_phase_differs_only_in_the_sign_of_zero(lib):
    """The one place the forms part: k d |r| == 0 with r < 0 (arg = +0 or a NaN with a clear sign bit), where sincos_cw(+-0)
    gives +0 and the old form's rsin = r * 0 and sinr = 0 / r came out as -0.  It needs a layer of zero thickness, which the
    prep kernel rejects (BADMODEL), so no accepted stack reaches it; pinned here so that it stays the only exception."""
    arg = np.array([0.0, np.nan, -0.0, -1.0, 1.0, 0.0], f32)
    wd = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1e-40], f32)
    n, rows = _pairs(lib, arg, wd)
    assert n == 3 and all(r[2] == ["rsin", "sinr"] for r in rows), rows
    assert [r[0] == 0.0 or r[0] != r[0] for r in rows] == [True] * 3
