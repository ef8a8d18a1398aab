"""surfdisp_params_jacobian_device (include/surfdisp.h section (6i)) through Model1DBatch.jacobian on the GPU: the derivative against
central differences of the torch statement in float64 (the bar of tests/test_param_jacobian_host.py), and the value part against the
stack kernel - float32(layer) is rows 0..3 of to_model_native's model bit for bit, so the statement that is differentiated cannot
drift off the map."""
import numpy as np
import pytest

from param_lsq_cases import REL_STEP, SETTINGS, jac_error, param_rows
from pysurfinv_amd import paramlsq, settings
from pysurfinv_amd.layers_batch import Model1DBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(mb, p, rows=None):
    import torch
    pt = torch.as_tensor(p, device=DEV)
    layer, jac = mb.jacobian(pt, rows)
    model, _ = mb.to_model_native(pt, rows)
    C, Nu, L = p.shape[0], mb.spec.n, model.shape[2]
    assert tuple(layer.shape) == (C, 4, L) and tuple(jac.shape) == (C, 4, L, Nu) and layer.dtype == jac.dtype == torch.float64
    assert torch.equal(layer.to(torch.float32), model[:, :4, :])                      # bit for bit
    layer_fd, fd = paramlsq.jacobian_reference(mb, p, REL_STEP, rows=rows)
    jac = jac.cpu().numpy()
    assert np.isfinite(jac).all()
    assert np.abs(layer.cpu().numpy() - layer_fd).max() <= 1e-12 * np.abs(layer_fd).max()
    ratio, worst = jac_error(jac, fd)
    assert (np.abs(jac).max(axis=(1, 2)) > 0).all()
    return ratio, worst, jac


@pytest.mark.parametrize("name", list(SETTINGS))
def test_jacobian_kernel_matches_central_differences_and_the_stack_kernel(name):
    mb = Model1DBatch(SETTINGS[name], device=DEV)
    ratio, worst, _ = _check(mb, param_rows(mb))
    print(f"{name}: largest |jac - fd| {worst:.2e}, worst error / bar {ratio:.2e}")
    assert ratio <= 1.0, (name, ratio, worst)


def test_a_per_point_topo_is_a_constant_behind_the_unknowns():
    """Info.topo per point (Nu = 13 < N = 14), rows given out of order: the same derivatives as without it, another stack top."""
    setting = dict(SETTINGS["mcmc"], Info=dict(SETTINGS["mcmc"]["Info"], topo=0.0))
    mb = Model1DBatch(setting, device=DEV, local_keys=["topo"]).set_local_info(np.array([[-1.0], [0.8], [2.5], [0.3]]))
    p = param_rows(mb)
    ratio, worst, jac = _check(mb, p, rows=[3, 0, 2])
    print(f"topo: largest |jac - fd| {worst:.2e}, worst error / bar {ratio:.2e}")
    assert ratio <= 1.0
    plain = Model1DBatch(SETTINGS["mcmc"], device=DEV)
    assert np.array_equal(jac, _check(plain, p)[2])


def test_a_thermal_setting_is_refused():
    import torch
    mb = Model1DBatch(settings.C5_SETTING, device=DEV)
    with pytest.raises(ValueError, match="thermal"):
        mb.jacobian(torch.as_tensor(mb.spec.v0[None, :], device=DEV))
    # the entry itself: NaN for the whole chain (it reads no scratch array: none is passed)
    import ctypes
    from pysurfinv_amd import _lib
    idesc, fdesc, L = mb.native_descriptor()
    p = torch.as_tensor(np.tile(mb.spec.v0, (2, 1)), device=DEV).contiguous()
    Nu = mb.spec.n
    layer, jac = torch.full((2, 4, L), 7.0, dtype=torch.float64, device=DEV), torch.full((2, 4, L, Nu), 7.0, dtype=torch.float64, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib().surfdisp_params_jacobian_device(None, 2, Nu, Nu, L, ptr(p), ptr(idesc), ptr(fdesc), ptr(layer), ptr(jac))
    torch.cuda.synchronize()
    assert rc == _lib.SUCCESS and bool(torch.isnan(layer).all()) and bool(torch.isnan(jac).all())
