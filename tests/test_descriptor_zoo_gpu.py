"""Every kernel that reads a params -> stack descriptor (csrc/surfdisp_layers_grid.h and its copies), on the settings of
tests/descriptor_zoo.py, against the float64 torch statement on the CPU (pinned to the modelled project by
tests/test_descriptor_zoo.py).  The posterior-profile kernel's zoo cases are in tests/test_posterior_gpu.py.

C = 301 rows per setting: C L is above 256 and no multiple of 256 or 64 for L = 85, 35, 68.  `moho` runs with K = 1 (a per-point
topography behind the unknowns), its rows given out of order.  The measured figures of an MI355X run are in
profiles/descriptor_zoo/parity.txt."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import descriptor_zoo as Z
import mcmc_prior_replay as PR
from pysurfinv_amd import _lib
from pysurfinv_amd.mcmc import PriorRules

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 301
MAX_EXCLUDED = 0.005                  # tests/test_prior_redraw.py


@functools.lru_cache(maxsize=None)
def _gpu_model(name):
    return Z.zoo_model(name, DEV)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


@functools.lru_cache(maxsize=None)
def _stack64(name):
    """(params [C, Nu], rows, float64 [C, 5, L] rows vp, vs, rho, h, 1/Qs of the torch statement on the CPU): computed once."""
    mb = Z.cpu_model(name)
    p = Z.zoo_params(mb, C, seed=31)
    rows = Z.zoo_rows(mb, C)
    (h, vs, vp, rho, qs, qp), nlay = mb.seis_prop_layers(torch.from_numpy(p), rows)
    assert h.shape[1] == Z.LAYERS[name] and bool((nlay == Z.LAYERS[name]).all())
    ref = torch.stack([vp, vs, rho, h, 1.0 / qs], dim=1).numpy()
    for a in (p, ref):
        a.setflags(write=False)
    return p, rows, ref


@pytest.mark.parametrize("name", list(Z.ZOO))
def test_stack_kernel_against_the_float64_statement(name):
    """surfdisp_params_to_model_device.  vp, vs, rho, h: within one fp32 ulp of float32(reference) - both sides evaluate the same
    formulas in fp64 in another order and differ by about 1e-11 relative at worst (h, a difference of depths near 200 km), so their
    fp32 roundings differ only where the two fp64 values straddle a rounding boundary, and then by one ulp.  1/Qs comes from
    closed-form constants: bit-equal."""
    assert (C * Z.LAYERS[name]) % 64 and C * Z.LAYERS[name] > 256
    p, rows, ref64 = _stack64(name)
    mb = _gpu_model(name)
    model, nl = mb.to_model_native(torch.as_tensor(p, device=DEV), rows)
    torch.cuda.synchronize()
    assert nl is None and model.dtype == torch.float32 and tuple(model.shape) == ref64.shape
    dev = model.cpu().numpy()
    ref = ref64.astype(np.float32)
    differ = dev.view(np.uint32) != ref.view(np.uint32)
    ulp = np.spacing(np.abs(ref))
    worst = float((np.abs(dev.astype(np.float64) - ref.astype(np.float64)) / ulp).max())
    rel64 = float((np.abs(dev.astype(np.float64) - ref64) / np.maximum(np.abs(ref64), 1e-30))[:, :4].max())
    print(f"PARITY zoo stack {name}: {int(differ.sum())} of {differ.size} words differ from float32(float64 statement), "
          f"{int(differ[:, 4].sum())} of them in 1/Qs, largest difference {worst:.1f} ulp, largest |dev - fp64| / |fp64| {rel64:.2e}")
    assert np.isfinite(dev).all()
    assert not differ[:, 4].any()
    assert worst <= 1.0
    if name != "pairs":                                     # a water top: Vs exactly zero, and nothing else is
        assert not dev[:, 1, 0].any() and (dev[:, 1, 1:] > 0).all()


@pytest.mark.parametrize("name", list(Z.ZOO))
def test_jacobian_kernel_on_the_zoo(name):
    """surfdisp_params_jacobian_device through the checks of tests/test_param_jacobian_gpu.py: float32(layer) is the stack kernel's
    rows bit for bit, the value part is the torch statement's, the derivative within JAC_BAR of central differences, no zero column."""
    from test_param_jacobian_gpu import _check
    p, rows, _ = _stack64(name)
    ratio, worst, _ = _check(_gpu_model(name), np.array(p), rows)
    print(f"PARITY zoo jacobian {name}: largest |jac - fd| {worst:.2e}, worst error / bar {ratio:.2e}")
    assert ratio <= 1.0, (name, ratio, worst)


def _prior_call(mb, rules, q, only_tag, mark_tag, tags):
    idesc, fdesc, L = mb.native_descriptor()
    _lib.check(_lib.lib().surfdisp_prior_device(None, q.shape[0], q.shape[1], int(L), _ptr(q), _ptr(idesc), _ptr(fdesc), _ptr(rules.device_flags()),
                                                ctypes.c_double(-1.0 if rules.vs_max is None else rules.vs_max), only_tag, mark_tag, _ptr(tags)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", list(Z.ZOO))
def test_prior_kernel_on_the_zoo(name):
    """surfdisp_prior_device against prior_good on 5000 uniform draws, three rule sets per setting, on the rows whose smallest rule
    slack is at least SLACK_BAND; then only_tag."""
    n = 5000
    mbc, mb = Z.cpu_model(name), _gpu_model(name)
    p = Z.zoo_params(mbc, n, seed=37)
    rows = Z.zoo_rows(mbc, n)
    q = mb._full(torch.as_tensor(p, device=DEV), rows).contiguous()          # [n, Nu + K]
    assert q.shape[1] == mbc.spec.n + (1 if name == "moho" else 0)
    for i, kw in enumerate(Z.RULES[name]):
        rules = PriorRules(mb, **kw)
        want, slack = PR.rule_margins(PriorRules(mbc, **kw), p, rows)
        keep = slack >= PR.SLACK_BAND
        tags = torch.zeros(n, dtype=torch.uint8, device=DEV)
        _prior_call(mb, rules, q, -1, 1, tags)
        got = tags.cpu().numpy()
        assert set(np.unique(got)) <= {0, 1}
        wrong = int(((got == 0) != want)[keep].sum())
        share = float(want.mean())
        print(f"PARITY zoo prior {name} {kw}: accept share {share:.3f}, {wrong} of {int(keep.sum())} decisions differ, "
              f"{int((~keep).sum())} rows left out, smallest slack {slack.min():.2e}")
        assert 0.05 <= share <= 0.95, (name, kw, share)
        assert (~keep).sum() <= MAX_EXCLUDED * n, (name, kw)
        assert wrong == 0, (name, kw, wrong)
        if i == 0:
            # only_tag = 1, mark_tag = 3 on tags 0, 1, 2: a chain below 1 is not looked at, the others carry 3 exactly where the rules fail
            pre = (np.arange(n) % 3).astype(np.uint8)
            tags = torch.from_numpy(pre).to(DEV)
            _prior_call(mb, rules, q, 1, 3, tags)
            got = tags.cpu().numpy()
            assert np.array_equal(got[pre == 0], pre[pre == 0])
            sel = keep & (pre > 0)
            assert np.array_equal(got[sel], np.where(want, pre, 3)[sel]) and (got[sel] == 3).any() and (got[sel] != 3).any()


REDRAW = dict(step=4.0, G=1000, U=10000)


@pytest.mark.parametrize("name,depth", [("pairs", 2), ("pairs", 4), ("moho", 2)])
def test_redraw_kernel_on_the_zoo(name, depth):
    """surfdisp_mcmc_propose_prior_device against the host replay (tests/test_prior_redraw.py::_against_replay): `pairs` under
    (crust monotone, jumps) - the rule walker's bit 1 and bit 2 on adjacent layers of one group - and `moho` with K = 1.  C = 67."""
    from test_prior_redraw import _against_replay
    from test_mcmc_replay import SEEDS
    mbc = Z.cpu_model(name)
    kw = Z.RULES[name][2 if name == "pairs" else 0]
    rows = Z.zoo_rows(mbc, 67)
    out, tries, ref, tol, keep = _against_replay(dict(kw=kw, **REDRAW), None, 67, depth, 0, SEEDS[1], 17, 0.05, f"zoo {name} depth {depth}",
                                                 model=(mbc, _gpu_model(name), rows))
    assert tries.max() < REDRAW["G"] + REDRAW["U"]
    assert ((out > mbc.spec.vmin) & (out < mbc.spec.vmax)).all()
