"""CPU check of the scan's team decision (pysurfinv_amd/csrc/surfdisp_k_scan.h): the four-point form, which a two-lane
team's double lean pass takes once, must give what two two-point decisions in sequence give - the second one starting from
the first one's carry, as two consecutive single passes do - FIELD FOR FIELD: event index, crossing or guard, and the
bracket / carry words (value and trial velocity to the bit, mm).  tests/hostcheck/scancheck.hip compiles the header for the
host and runs both.  The event index and kind are also compared with the rule written out here, point by point.

Every pattern of: the four points' values from {-1, +1, NaN, -NaN, -0, +0} (a NaN of either sign bit counts as positive,
-0 as negative), the value before them from {-1, +1, NaN}, the four guard flags, a period's first pass or a later one,
and mm equal everywhere / different at every point / changing between a lane's two points.
No GPU needed; skipped if hipcc is absent."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcheck")
f32 = np.float32
FIELDS = ("event", "cross", "lo_value", "lo_c", "lo_mm", "hi_value", "hi_c", "hi_mm")


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(hostbuild.build(os.path.join(HC, "scancheck.hip"), os.path.join(HC, "libscancheck.so")))
    L.sc_run.restype = None
    L.sc_run.argtypes = [ctypes.c_long] + [ctypes.c_void_p] * 7
    return L


def _cases():
    neg_nan = np.array(0xFFC00000, np.uint32).view(f32)
    vals = np.array([-1.0, 1.0, np.nan, neg_nan, -0.0, 0.0], f32)
    v4 = np.array(list(itertools.product(range(6), repeat=4)))                     # [1296, 4]
    v0 = np.array([0, 1, 2])
    g4 = np.array(list(itertools.product((0, 1), repeat=4)))                       # [16, 4]
    mms = np.array([[7, 7, 7, 7, 7], [9, 8, 7, 6, 5], [7, 7, 7, 6, 6], [7, 8, 7, 8, 7]])
    iv, i0, ig, fi, im = np.meshgrid(np.arange(len(v4)), v0, np.arange(16), (0, 1), np.arange(len(mms)), indexing="ij")
    iv, i0, ig, fi, im = (a.ravel() for a in (iv, i0, ig, fi, im))
    v = np.concatenate([vals[i0][:, None], vals[v4[iv]]], axis=1).astype(f32)
    # a grid as the scan's: the point before, then four steps of 0.005 (distinct words, so that a swapped point shows)
    c = np.tile((f32(3.2) + f32(0.005) * np.arange(5, dtype=f32)).astype(f32), (v.shape[0], 1))
    return (np.ascontiguousarray(v), np.ascontiguousarray(c), np.ascontiguousarray(mms[im].astype(np.int32)),
            np.ascontiguousarray(g4[ig].astype(np.int32)), np.ascontiguousarray(fi.astype(np.int32)))


@pytest.fixture(scope="module")
def ran(lib):
    v, c, mm, g, first = _cases()
    four = np.zeros((v.shape[0], 8), np.int32)
    seq = np.zeros_like(four)
    lib.sc_run(v.shape[0], v.ctypes.data, c.ctypes.data, mm.ctypes.data, g.ctypes.data, first.ctypes.data,
               four.ctypes.data, seq.ctypes.data)
    return v, c, mm, g, first, four, seq


def test_every_pattern_is_there(ran):
    v, _, mm, g, first, _, _ = ran
    assert v.shape[0] == 6 ** 4 * 3 * 16 * 2 * 4
    assert np.isnan(v).any() and (mm[:, 1] != mm[:, 3]).any() and (mm.min(axis=1) == mm.max(axis=1)).any()
    assert set(first.tolist()) == {0, 1} and len(np.unique(g, axis=0)) == 16


def test_four_points_equal_two_passes_of_two(ran):
    four, seq = ran[5], ran[6]
    bad = np.nonzero((four != seq).any(axis=1))[0]
    msg = ""
    if bad.size:
        i = bad[0]
        msg = (f"{bad.size} cases differ; first: values {ran[0][i]}, mm {ran[2][i]}, guards {ran[3][i]}, first {ran[4][i]}: "
               f"four-point {dict(zip(FIELDS, four[i]))}, two passes {dict(zip(FIELDS, seq[i]))}")
    assert not bad.size, msg


def test_event_is_the_rule_point_by_point(ran):
    """calcul.f:157-170 one point at a time: a sign change against the point before it (NaN positive) is a bracket, else a
    failed guard ends the search; the period's first trial has no point before it and is never an event."""
    v, c, mm, g, first, four, _ = ran
    neg = np.signbit(v) & ~np.isnan(v)
    e = np.full(v.shape[0], -1)
    cross = np.zeros(v.shape[0], bool)
    for i in (3, 2, 1, 0):
        has_prev = (first == 0) if i == 0 else np.ones(v.shape[0], bool)
        cr = has_prev & (neg[:, i + 1] != neg[:, i])
        ev = cr | (has_prev & (g[:, i] != 0))
        e = np.where(ev, i, e)
        cross = np.where(ev, cr, cross)
    assert np.array_equal(four[:, 0], e) and np.array_equal(four[:, 1] != 0, cross)
    # the bracket: the point before the event and the event, each with its own mm; without an event the last point
    rows = np.arange(v.shape[0])
    lo = np.where(e >= 0, e, 4)
    hi = np.where(e >= 0, e + 1, 4)
    assert np.array_equal(four[:, 2], v.view(np.int32)[rows, lo]) and np.array_equal(four[:, 5], v.view(np.int32)[rows, hi])
    assert np.array_equal(four[:, 3], c.view(np.int32)[rows, lo]) and np.array_equal(four[:, 6], c.view(np.int32)[rows, hi])
    assert np.array_equal(four[:, 4], mm[rows, lo]) and np.array_equal(four[:, 7], mm[rows, hi])
