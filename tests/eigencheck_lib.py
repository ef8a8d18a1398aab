"""The ``eigenlib`` fixture of the eigenfunction tests: tests/hostcheck/eigencheck.hip (the EIG instantiations of
group_rayleigh / group_love of surfdisp_kernels.hip compiled for the host with hipcc).  Skipped if hipcc is absent."""
import ctypes
import os

import numpy as np
import pytest

import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcheck")


class EigenHost:
    def __init__(self, so):
        self.H = ctypes.CDLL(so)

    def group(self, model, per, kind, c, ratio, nlay=None):
        """(u [B, P]; vals [B, P, 4, L] float32 as the lane stores them, undivided, NaN where the lane wrote nothing;
        div [B, P]; hs [B, P] int (-1: none); I [B, P, 3] float32)."""
        model = np.ascontiguousarray(model, np.float32)
        model = model[None] if model.ndim == 2 else model
        per = np.ascontiguousarray(per, np.float32)
        B, _, L = model.shape; P = per.size
        c = np.ascontiguousarray(np.asarray(c, np.float32).reshape(B, P))
        ratio = np.ascontiguousarray(np.asarray(ratio, np.float32).reshape(B, P))
        u = np.zeros((B, P), np.float32)
        out = np.full((B, P, 4, L), np.nan, np.float32)
        unit = np.zeros((B, P, 5), np.float64)
        fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        nl = None if nlay is None else np.ascontiguousarray(nlay, np.int32)
        self.H.sd_eigencheck_group(B, L, None if nl is None else nl.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), fp(model), P, fp(per),
                                   int(kind), fp(c), fp(ratio), fp(u), fp(out), unit.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return u, out, unit[..., 0].astype(np.float32), unit[..., 1].astype(np.int64), unit[..., 2:].astype(np.float32)


def finish(vals, div, hs, kind):
    """What surfdisp_eigen_transpose_kernel makes of a unit's stores (not the code under test: the GPU tests run that): the
    fp32 quotient by the unit's divisor down to its deepest layer, zeros below and for units without one.  Love's
    low-amplitude exclusion never triggers on the fixture stacks (asserted by the caller).  -> [B, P, 4, L]; Love: rows
    0 (ut) and 3 (tq), rows 1, 2 zeros."""
    B, P, _, L = vals.shape
    out = np.zeros((B, P, 4, L), np.float32)
    idx = np.arange(L)
    for b in range(B):
        for k in range(P):
            m = idx <= hs[b, k]
            rows = ((0, 0), (1, 1), (2, 2), (3, 3)) if int(kind) == 2 else ((0, 0), (3, 1))
            for dst, src in rows:
                out[b, k, dst, m] = (vals[b, k, src, m] / np.float32(div[b, k])).astype(np.float32)
    return out


@pytest.fixture(scope="module")
def eigenlib():
    return EigenHost(hostbuild.build(os.path.join(HC, "eigencheck.hip"), os.path.join(HC, "libeigencheck.so")))
