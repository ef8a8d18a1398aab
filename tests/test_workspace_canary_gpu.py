"""Every forward entry on a workspace of exactly the size its ``*_workspace_bytes`` function states, with a canary behind it: the
entry's carving must stay inside that size, and its results must be those of the plan's ordinary workspace, word for word.
The workspace is the first half of one allocation filled with 0xA5, so a wrong offset lands in the second half instead of
faulting.  This ties the size functions to the carving (csrc/surfdisp_capi.hip: one layout for both)."""
import numpy as np
import pytest

B, L, P = 3, 6, 4
NLAY = (6, 4, 2)                    # ragged: a full stack, a shorter one, the smallest
RAYLEIGH, LOVE = 2, 1

# (plan method, workspace entry, keyword arguments, wave types)
CASES = [
    ("run", "forward", {}, (RAYLEIGH, LOVE)),
    ("run", "forward", dict(want_ratio=True), (RAYLEIGH, LOVE)),
    ("run_kernels", "kernels", {}, (RAYLEIGH, LOVE)),
    ("run_kernels", "forward", dict(small_workspace=True), (RAYLEIGH, LOVE)),
    ("run_group_kernels", "group", {}, (RAYLEIGH, LOVE)),
    ("run_ellip_kernels", "ellip", {}, (RAYLEIGH,)),
    ("run_atten", "atten", {}, (RAYLEIGH, LOVE)),
    ("run_eigen", "eigen", {}, (RAYLEIGH, LOVE)),
    ("run_thickness_kernels", "thickness", {}, (RAYLEIGH, LOVE)),
]


def _inputs():
    import torch
    from pysurfinv_amd import synth
    model = torch.from_numpy(synth.synth_models(B, L, seed=5)).cuda()
    per = torch.from_numpy(synth.default_periods(P)).cuda()
    return model, per, torch.tensor(NLAY, dtype=torch.int32).cuda()


def _words(x):
    """A result as raw 32-bit words (tensors), or itself (counts, None)."""
    import torch
    return x.contiguous().view(torch.int32).cpu().numpy() if isinstance(x, torch.Tensor) else x


@pytest.mark.gpu
@pytest.mark.parametrize("method,entry,kw,kinds", CASES, ids=[c[0] + ("_" + "_".join(c[2]) if c[2] else "") for c in CASES])
def test_exact_size_workspace_keeps_its_canary_and_the_results(method, entry, kw, kinds):
    import torch
    from pysurfinv_amd import _lib, forward
    model, per, nlay = _inputs()
    n = int(getattr(_lib.lib(), forward.BatchPlan._WS_BYTES[entry])(B, L, P))
    assert n > 0
    for kind in kinds:
        buf = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device="cuda")
        plan, ordinary = forward.BatchPlan(B, L, P), forward.BatchPlan(B, L, P)
        ws, nbytes = plan.workspace(entry, buf[:n])
        assert nbytes == n and ws.data_ptr() == buf.data_ptr()
        got = [_words(x) for x in getattr(plan, method)(model, per, kind=kind, nlay=nlay, **kw)]
        torch.cuda.synchronize()
        assert plan._last_ws.data_ptr() == buf.data_ptr()                      # the call ran on the installed workspace
        assert bool((buf[n:] == 0xA5).all()), (method, kind, "the entry wrote behind its workspace")
        assert not bool((buf[:n] == 0xA5).all())                               # ... and did use it
        ref = [_words(x) for x in getattr(ordinary, method)(model, per, kind=kind, nlay=nlay, **kw)]
        assert len(got) == len(ref)
        for i, (a, b) in enumerate(zip(got, ref)):
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, b), (method, kind, i)
            else:
                assert a == b, (method, kind, i)
        assert (got[0] != 0).any()                                             # some period was solved: the comparison is not of zeros
