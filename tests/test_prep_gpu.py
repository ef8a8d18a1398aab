"""The working stack the prep kernel writes (K0, surfdisp_prep_kernel<KIND, TL>, csrc/surfdisp_k_prep.h), read where it is written:
one forward solve on a workspace filled with 0xA5, then the SoA copy mdl [9][Lmax][B], the row copy rows [B][9][Lmax], nl, fsafe and
ovf are read at the offsets surfdisp_workspace_prep_offsets states and compared with the numpy statement of prep_stack
(tests/kernel_rows_ref.py: prep_factors32, prep_stats; pinned to the oracle's flat1 and to prep_stack on the host by
tests/test_prep_oracle.py and tests/test_kernel_rows_host.py).  Batches and shapes: tests/prep_cases.py.

Bars.  vp, vs, rho, 1/Qs, hsf, nl, fsafe, ovf[0]: bit-equal.  dif, qqq, dfl, hsr pass through the device's fp64 log / pow: inside the
derived fp32 bounds against float64 unconditionally (prep_cases.compare_copy), and bit-equal to prep_factors32 - two correctly
working fp64 libraries round to different fp32 values with a chance of about 3e-9 per call.  ovf[1], ovf[2] = 2 logf, 4 logf of
statistics compared above: within 4 fp32 ulp of the float64 logarithm (the 3 ulp the device library's logf is specified to, and the
multiply).  A copy the launch does not write (use_rows / need_soa of forward_device_impl) still holds the fill pattern.
The measured figures of an MI355X run are in profiles/prep_stack/parity.txt."""
import ctypes

import numpy as np
import pytest

import prep_cases as pc

pytestmark = pytest.mark.gpu

# (id, (TL, Lmax, B, P), forced root-search team or 0, phase-only)
CASES = [(f"TL{s[0]}_L{s[1]}_B{s[2]}", s, 0, False) for s in pc.SHAPES] + [
    ("team4_soa_only", pc.SHAPES[2], 4, False), ("team8_both", pc.SHAPES[2], 8, False), ("phase_only_rows_only", pc.SHAPES[5], 0, True)]


def _solve(Lmax, B, P, kind, team, phase_only):
    """One forward solve on a 0xA5-filled workspace -> (the workspace's bytes, status, lanes per stack of the root search)."""
    import torch
    from pysurfinv_amd import _lib, forward, synth
    L = _lib.lib()
    m, nlay, bad = pc.batch(Lmax, B)
    n = int(L.surfdisp_workspace_bytes(B, Lmax, P))
    buf = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    plan = forward.BatchPlan(B, Lmax, P)
    plan.workspace("forward", buf)
    flags = kind | (_lib.PHASE_ONLY if phase_only else 0)
    assert L.surfdisp_set_team(team) == 0
    try:
        G = int(L.surfdisp_get_team2(B, Lmax, P, flags))
        _, _, st = plan.run(torch.from_numpy(m).cuda(), torch.from_numpy(synth.default_periods(P)).cuda(), kind=flags,
                            nlay=torch.from_numpy(nlay).cuda())
        torch.cuda.synchronize()
    finally:
        L.surfdisp_set_team(0)
    assert plan._last_ws.data_ptr() == buf.data_ptr()
    return m, nlay, bad, buf.cpu().numpy(), st.cpu().numpy(), G


@pytest.mark.parametrize("kind", [2, 1], ids=["rayleigh", "love"])
@pytest.mark.parametrize("name,shape,team,phase_only", CASES, ids=[c[0] for c in CASES])
def test_working_stack_is_prep_stack(name, shape, team, phase_only, kind):
    from pysurfinv_amd import _lib
    TL, Lmax, B, P = shape
    assert pc.prep_lanes(B, Lmax) == TL and (B % (256 // TL) or B >= 20000)       # (a ragged last block in every small shape)
    m, nlay, bad, ws, st, G = _solve(Lmax, B, P, kind, team, phase_only)
    off = (ctypes.c_size_t * 5)()
    assert _lib.lib().surfdisp_workspace_prep_offsets(B, Lmax, P, off) == 0
    words = lambda o, count, dt: ws[o:o + 4 * count].view(dt)
    nw = 9 * Lmax * B
    soa = np.ascontiguousarray(words(off[0], nw, np.float32).reshape(9, Lmax, B).transpose(2, 0, 1))     # -> [B, 9, Lmax]
    rows = words(off[1], nw, np.float32).reshape(B, 9, Lmax)
    nl, fsafe, ovf = words(off[2], B, np.int32), words(off[3], B, np.float32), words(off[4], 3 * B, np.float32).reshape(3, B)
    e = pc.expected(m, nlay, kind)
    g = e["good"]
    assert bad and not g[list(bad)].any() and g.sum() == B - len(bad)
    assert (st[list(bad)] == _lib.BADMODEL).all() and (st[g] != _lib.BADMODEL).all()

    # which copies this launch writes (forward_device_impl): rows for teams of at least 8 lanes; the SoA copy unless a phase-only
    # call has rows (the group-velocity kernel and narrow teams read it)
    use_rows = G >= 8
    need_soa = (not use_rows) or (not phase_only)
    if team:
        assert G == team
    assert (use_rows, need_soa) == {"team4_soa_only": (False, True), "team8_both": (True, True),
                                    "phase_only_rows_only": (True, False)}.get(name, (use_rows, True))
    ndiff, worst, frac, nwords = 0, 0.0, 0.0, 0
    for label, copy, written in (("SoA", soa, need_soa), ("rows", rows, use_rows)):
        if not written:
            assert (copy.view(np.uint32) == pc.FILL).all(), (name, label, "a copy this launch does not need was written")
            continue
        d, w, f = pc.compare_copy(copy, e, f"{name} {label}")
        ndiff, worst, frac = ndiff + d, max(worst, w), max(frac, f)
        nwords += 4 * int(e["written"][g].sum())

    # the verdict and the statistics
    assert np.array_equal(nl, e["nl"]), name
    assert np.array_equal(fsafe.view(np.uint32), e["fsafe"].view(np.uint32)), name
    assert np.array_equal(ovf[0][g].view(np.uint32), e["hthick"][g].view(np.uint32)), name
    ulp_log = 0.0
    for row, arg in ((1, e["rhomax"]), (2, (np.float32(2.0) * e["bmax"] * e["bmax"]).astype(np.float32))):
        ref = (2.0 * row) * np.log(arg[g].astype(np.float64))
        ulp_log = max(ulp_log, float((np.abs(ovf[row][g] - ref) / np.spacing(np.abs(ref).astype(np.float32))).max()))
    print(f"PARITY prep {name} kind {kind}: teams of {G}, {ndiff} of {nwords} words of dif, qqq, dfl, hsr differ from prep_factors32 "
          f"(largest {worst:.1f} ulp), worst error against float64 {frac:.2f} of the derived bound, ovf[1..2] within {ulp_log:.2f} ulp of "
          f"the float64 logarithm; fsafe = 1e30 on {int((e['fsafe'][g] > 1e29).sum())}, hthick = 1e30 on {int((e['hthick'][g] > 1e29).sum())} good stacks")
    assert ulp_log <= 4.0, (name, ulp_log)
    assert ndiff == 0, (name, ndiff, worst)
