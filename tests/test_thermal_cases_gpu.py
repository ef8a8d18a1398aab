"""surfdisp_thermal_kernel + surfdisp_layers_kernel on the case set of tests/thermal_cases.py against the float64
torch mirror evaluated ON THE CPU (an independent libm): every layout, every grid size, every branch the host test
shows the rows to reach, and - tests/test_thermal_cases_host.py - no row near a decision boundary."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import thermal_cases as tc                                              # noqa: E402

NAMES = list(tc.CASES)
VS_BAR, QS_BAR = 1e-10, 1e-9                               # the bars of test_native_thermal_kernel_matches_torch_mirror
_CPU = {}


def cpu_statement(name):
    """(grid Vs, grid Qs) float64 [B, npts] and the fp32 stack [B, 5, L] of the CPU mirror; computed once, read-only."""
    if name not in _CPU:
        p, r, _ = tc.rows(name)
        mb = tc.model(name, "cpu")
        model, nlay = mb.to_model_torch(p, r)
        vs, qs = mb.layers[-1]["grid_last"]
        assert int((nlay != model.shape[2]).sum()) == 0
        _CPU[name] = tuple(a.numpy().copy() for a in (vs, qs, model))
        for a in _CPU[name]:
            a.setflags(write=False)
    return _CPU[name]


def native(name, mb=None):
    """(thermal scratch float64 [B, npts, 2], fp32 stack) of the HIP kernels for the case's rows, as numpy."""
    p, r, _ = tc.rows(name)
    mb = mb or tc.model(name, "cuda:0")
    assert mb.native_descriptor() is not None and mb._native_thermal
    model, nlay = mb.to_model(p.to("cuda:0"), None if r is None else r.to("cuda:0"))
    assert nlay is None                                    # the native path, not the torch one
    torch.cuda.synchronize()
    npts = tc.CASES[name]["npts"]
    return mb._thermal_scratch[:, :npts].cpu().numpy().copy(), model.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_thermal_grid_values_match_cpu_float64(name):
    """Vs and Qs on the thermal layer's grid in float64: relative 1e-10 and 1e-9, the bars the project already holds
    the kernel to against the mirror on the device - here against the mirror on the CPU.  (Measured worst over the ten
    cases: Vs 5.6e-14, Qs 4.0e-14; profiles/thermal_cases/parity.txt.)"""
    vs, qs, _ = cpu_statement(name)
    sc, _ = native(name)
    assert sc.shape == vs.shape + (2,)
    assert np.isfinite(sc).all()
    e_vs = np.abs(sc[:, :, 0] - vs) / np.abs(vs)
    e_qs = np.abs(sc[:, :, 1] - qs) / np.abs(qs)
    rv, rq = np.unravel_index(np.argmax(e_vs), e_vs.shape), np.unravel_index(np.argmax(e_qs), e_qs.shape)
    print(f"{name}: {vs.shape[0]} rows x {vs.shape[1]} points  worst Vs {e_vs.max():.3e} = {e_vs.max() / VS_BAR:.2e} x bar "
          f"(row {rv[0]}, point {rv[1]})  worst Qs {e_qs.max():.3e} = {e_qs.max() / QS_BAR:.2e} x bar (row {rq[0]}, point {rq[1]})")
    assert e_vs.max() < VS_BAR, (rv, e_vs.max())
    assert e_qs.max() < QS_BAR, (rq, e_qs.max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_fp32_stack_is_the_rounded_float64_stack(name):
    """vp, vs, rho, h and 1/Qs of every output layer are float32(float64 value) of the CPU mirror or a neighbouring
    float: two doubles that agree to 1e-9 round to the same or to adjacent floats (one float32 ulp is 6e-8)."""
    _, _, want = cpu_statement(name)
    _, got = native(name)
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32
    up, down = np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))
    ok = (got == want) | (got == up) | (got == down)
    print(f"{name}: {int((got != want).sum())} of {got.size} entries differ, {int((~ok).sum())} by more than one ulp")
    for k, nm in enumerate(("vp", "vs", "rho", "h", "1/Qs")):
        bad = np.argwhere(~ok[:, k])
        assert bad.size == 0, (nm, bad[:5].tolist(), got[:, k][~ok[:, k]][:5], want[:, k][~ok[:, k]][:5])


@pytest.mark.gpu
def test_short_knot_rows_do_not_depend_on_the_launch():
    """The 3 km layer (rows with no knot and one knot) twice in one process, another setting's batch in between:
    the scratch is bit-identical - nothing the kernel reads was left in LDS by another workgroup."""
    mb = tc.model("bd13_yama", "cuda:0")
    first, m1 = native("bd13_yama", mb)
    other, _ = native("bd200_yama")
    assert np.isfinite(other).all()
    second, m2 = native("bd13_yama", mb)
    assert np.array_equal(first.view(np.int64), second.view(np.int64))
    assert np.array_equal(m1.view(np.int32), m2.view(np.int32))
