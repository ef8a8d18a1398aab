"""The Jacobian of the params -> stack map (csrc/surfdisp_layers_dual.h, include/surfdisp.h section (6i)) on the HOST: the dual-number
functions the kernel surfdisp_params_jacobian_kernel runs, compiled for the host (tests/hostcheck/jaccheck.hip), against central
differences of Model1DBatch.seis_prop_layers in float64 (paramlsq.jacobian_reference).

Bar: |jac - fd| <= 1e-6 max(1, max |column|).  With a central step of 1e-5 of the parameter's width the difference quotient's own
error is orders below: truncation h^2 f''' / 6 with h <= 2e-4 and the quartic / rational closed forms, rounding 1e-16 x 200 km / h <=
5e-9 at the narrowest width (h = 4e-6).  Largest error seen: 9.5e-10 (MCMC_SETTING), 4.9e-9 (the oceanic setting) -
profiles/param_lsq/parity.txt."""
import ctypes
import os

import numpy as np
import pytest

import hostbuild
from param_lsq_cases import JAC_BAR, REL_STEP, SETTINGS, host_descriptor, jac_error, param_rows
from pysurfinv_amd import paramlsq

HC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")


def load_jaccheck():
    L = ctypes.CDLL(hostbuild.build(os.path.join(HC, "jaccheck.hip"), os.path.join(HC, "libjaccheck.so")))
    L.sd_jaccheck.restype = ctypes.c_int
    L.sd_jaccheck.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5
    return L


@pytest.fixture(scope="module")
def lib():
    return load_jaccheck()


def host_jacobian(lib, mb, idesc, fdesc, L, p_full, Nu):
    p_full = np.ascontiguousarray(p_full, np.float64)
    C, N = p_full.shape
    layer, jac = np.full((C, 4, L), 7.0), np.full((C, 4, L, Nu), 7.0)
    rc = lib.sd_jaccheck(C, N, Nu, L, p_full.ctypes.data, idesc.ctypes.data, fdesc.ctypes.data, layer.ctypes.data, jac.ctypes.data)
    assert rc == 0
    return layer, jac


@pytest.fixture(scope="module")
def both(lib):
    """name -> (mb, params [3, Nu], layer, jac of the host run, layer, jac of the finite differences)"""
    out = {}
    for name, setting in SETTINGS.items():
        mb, idesc, fdesc, L = host_descriptor(setting)
        p = param_rows(mb)
        out[name] = (mb, p, *host_jacobian(lib, mb, idesc, fdesc, L, p, mb.spec.n), *paramlsq.jacobian_reference(mb, p, REL_STEP))
    return out


@pytest.mark.parametrize("name", list(SETTINGS))
def test_dual_numbers_match_central_differences(both, name):
    mb, p, layer, jac, layer_fd, fd = both[name]
    assert jac.shape == fd.shape == (3, 4, layer.shape[2], mb.spec.n) and (layer.shape[2], mb.spec.n) == {"mcmc": (96, 13), "ocean": (85, 7)}[name]
    assert np.isfinite(jac).all()
    assert np.abs(layer - layer_fd).max() <= 1e-12 * np.abs(layer_fd).max()          # the value part is the torch statement's
    ratio, worst = jac_error(jac, fd)
    print(f"{name}: largest |jac - fd| {worst:.2e}, worst error / bar {ratio:.2e}")
    assert ratio <= 1.0, (name, ratio, worst)
    assert (np.abs(jac).max(axis=(1, 2)) > 0).all()                                  # every unknown has a non-zero column


def test_signs_and_zeros_of_the_continental_setting(both):
    """MCMC_SETTING: Sediment.H (an abs_pos H), two sediment coefficients, Crust.H, four crust coefficients, five mantle coefficients
    over a constant mantle thickness, the reference mantle.  Output layers: 1 sediment, 15 crust, 60 mantle, 20 reference."""
    mb, p, layer, jac, _, _ = both["mcmc"]
    names = mb.spec.names
    sed_h, crust_h = names.index("Sediment.H"), names.index("Crust.H")
    VP, VS, RHO, H = 0, 1, 2, 3
    # thickening the sediment: its own layer by as much, the crust's h unchanged, nothing in h below shifts
    assert np.array_equal(jac[:, H, 0, sed_h], np.ones(3)) and not jac[:, H, 1:, sed_h].any()
    assert not jac[:, :3, :, sed_h].any() and not jac[:, :3, :, crust_h].any()       # Vs is a function of relative depth: no H in it
    assert np.allclose(jac[:, H, 1:16, crust_h], 1.0 / 15, rtol=1e-14) and not jac[:, H, 16:, crust_h].any() and not jac[:, H, 0, crust_h].any()
    for j, n in enumerate(names):
        if ".Vs" not in n:
            continue
        lay = slice(0, 1) if n.startswith("Sediment") else (slice(1, 16) if n.startswith("Crust") else slice(16, 96))
        inside = np.zeros(96, bool); inside[lay] = True
        assert not jac[:, :, ~inside, j].any(), n                                     # a coefficient moves its own group only
        assert not jac[:, H, :, j].any(), n
        assert (jac[:, VS, inside, j] >= 0).all() and (jac[:, VP, inside, j] >= 0).all() and jac[:, VS, inside, j].max() > 0, n
        assert (np.sign(jac[:, RHO, inside, j]) == np.sign(jac[:, VS, inside, j])).all(), n   # rho rises with Vs in every class here
    last = names.index("Mantle.Vs[4]")
    # the reference mantle hangs off the last grid point: its 20 layers move rigidly with the last coefficient (basis value 1 there)
    assert np.allclose(jac[:, VS, 76:, last], 1.0, rtol=1e-12) and np.allclose(jac[:, VP, 76:, last], 1.76, rtol=1e-12)
    assert np.allclose(jac[:, RHO, 76:, last], 1 / 4.5, rtol=1e-12)
    assert np.allclose(jac[:, VP, 0, :3], 2.0 * jac[:, VS, 0, :3], rtol=1e-14) and np.allclose(jac[:, VP, 1:16], 1.8 * jac[:, VS, 1:16], rtol=1e-14)


def test_signs_and_zeros_of_the_oceanic_setting(both):
    """Water (1 layer), Cascadia sediment (1), crust (3), mantle on a BottomDepth (60), reference mantle (20)."""
    mb, p, layer, jac, _, _ = both["ocean"]
    names = mb.spec.names
    sed_h, bottom = names.index("OceanSedimentCascadia.H"), names.index("OceanMantle.BottomDepth")
    VP, VS, RHO, H = 0, 1, 2, 3
    assert not jac[:, :, 0, :].any() and not layer[:, VS, 0].any()                    # nothing moves the water layer
    assert np.array_equal(jac[:, H, 1, sed_h], np.ones(3)) and not jac[:, H, 2:5, sed_h].any()
    assert np.allclose(jac[:, H, 5:65, sed_h], -1.0 / 60, rtol=1e-13)                 # BottomDepth: the mantle thins by as much
    assert not jac[:, H, 65:, sed_h].any()                                            # ... and its bottom stays: no shift below
    assert (jac[:, VS, 1, sed_h] > 0).all() and np.allclose(jac[:, VP, 1, sed_h], 1.23 * jac[:, VS, 1, sed_h], rtol=1e-14)
    assert np.allclose(jac[:, RHO, 1, sed_h], 0.3601 * 1.23 * jac[:, VS, 1, sed_h], rtol=1e-14)
    assert not jac[:, :3, 2:, sed_h].any()
    assert np.allclose(jac[:, H, 5:65, bottom], 1.0 / 60, rtol=1e-13) and not jac[:, H, :5, bottom].any() and not jac[:, H, 65:, bottom].any()
    assert not jac[:, :3, :, bottom].any()
    crust0 = names.index("OceanCrust.Vs[0]")
    assert (jac[:, VS, 2:5, crust0] > 0).all() and not jac[:, :, 5:, crust0].any() and not jac[:, :, :2, crust0].any()
    # the mantle's last coefficient is a constant: the reference mantle's Vs moves with no unknown but through the basis row of
    # the last grid point, which is 1 at that constant alone
    assert np.abs(jac[:, :3, 65:, :]).max() <= 1e-12


def test_a_per_point_topo_shifts_no_derivative(lib):
    """Info.topo as a per-point local constant behind the unknowns (Nu < N): -max(topo, 0) is a constant of the row."""
    setting = dict(SETTINGS["mcmc"], Info=dict(SETTINGS["mcmc"]["Info"], topo=0.0))
    table = np.array([[-1.0], [0.8], [2.5]])
    mb, idesc, fdesc, L = host_descriptor(setting, ["topo"], table)
    p = param_rows(mb)
    layer, jac = host_jacobian(lib, mb, idesc, fdesc, L, np.concatenate([p, table], axis=1), mb.spec.n)
    layer_fd, fd = paramlsq.jacobian_reference(mb, p, REL_STEP)
    ratio, worst = jac_error(jac, fd)
    print(f"topo: largest |jac - fd| {worst:.2e}, worst error / bar {ratio:.2e}")
    assert ratio <= 1.0 and np.abs(layer - layer_fd).max() <= 1e-12 * np.abs(layer_fd).max()
    mb0, idesc0, fdesc0, L0 = host_descriptor(SETTINGS["mcmc"])
    plain = host_jacobian(lib, mb0, idesc0, fdesc0, L0, p, mb.spec.n)[1]
    assert np.array_equal(jac, plain)                                                 # the stack moves rigidly: the same derivatives
