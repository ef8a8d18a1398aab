"""The working stack's reference on the CPU: kernel_rows_ref.prep_factors32 - what tests/test_prep_gpu.py holds the prep kernel to -
against the factors the oracle's own flat1 applies (surfdisp_oracle_flatten: flat1 on unit vp and rho for every prefix length), and
kernel_rows_ref.prep_stats against prep_stack compiled for the host, on the batches of tests/prep_cases.py.

With surfdisp_oracle_set_variant(2) the oracle forms log / pow in double precision rounded once, as prep_stack does: bit for bit.
With variant 0 - logf / powf of the C library, the modelled project's own arithmetic - the factors stay inside the derived fp32
bounds of tests/test_kernel_rows_host.py against float64."""
import numpy as np
import pytest

import kernel_rows_ref as kr
import prep_cases as pc
from hostcheck_lib import hostlib  # noqa: F401
from oracle import cport
from test_kernel_rows_host import _inputs


def _random_layers():
    """1000 stacks of 20 layers, 0.05 .. 60 km log-uniform, a stack at most 251 km thick (the bounds' depths stay below 256 km)."""
    rng = np.random.default_rng(77)
    h = np.exp(rng.uniform(np.log(0.05), np.log(60.0), (1000, 20)))
    h = np.maximum(h * np.minimum(1.0, 250.0 / h.sum(axis=1, keepdims=True)), 0.05)
    m = np.ones((1000, 5, 20), np.float32)
    m[:, 3, :] = h
    return m


def _batches():
    return list(_inputs()) + [("random_20000", _random_layers(), None)]


@pytest.mark.parametrize("kind", [2, 1])
def test_flat1_with_double_precision_log_and_pow_is_prep_factors32(kind):
    for name, m, nlay in _batches():
        got = cport.flatten(m[:, 3, :], kind, nlay, variant=2)
        f32 = kr.prep_factors32(m, kind, nlay)
        for k in kr.FIELDS:
            assert np.array_equal(got[k].view(np.uint32), f32[k].view(np.uint32)), (name, kind, k)


@pytest.mark.parametrize("kind", [2, 1])
def test_flat1_with_the_c_librarys_logf_and_powf_stays_inside_the_derived_bounds(kind):
    worst = {k: 0.0 for k in kr.FIELDS}
    ndiff = 0
    for name, m, nlay in _batches():
        got = cport.flatten(m[:, 3, :], kind, nlay, variant=0)
        f32, f64 = kr.prep_factors32(m, kind, nlay), kr.prep_factors64(m, kind, nlay)
        bound, sels = kr.prep_bounds(m, kind, nlay)
        for k in kr.FIELDS:
            sel = sels[k]
            assert not got[k][~sel].any(), (name, k)
            rel = np.abs(got[k].astype(np.float64)[sel] / f64[k][sel] - 1.0) / bound[k][sel]
            worst[k] = max(worst[k], float(rel.max()))
            ndiff += int((got[k].view(np.uint32) != f32[k].view(np.uint32)).sum())
            assert rel.max() <= 1.0, (name, kind, k, float(rel.max()))
    print(f"flat1 (logf / powf) vs float64, kind {kind}: worst fraction of the bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f"; {ndiff} words differ from prep_factors32")


def test_flatten_rejects_a_bad_layer_count():
    h = np.ones(4, np.float32)
    out = [np.zeros(4, np.float32) for _ in range(5)]
    assert cport.lib().surfdisp_oracle_flatten(0, 2, cport._fp(h), *[cport._fp(a) for a in out]) == -1


@pytest.mark.parametrize("kind", [2, 1])
def test_prep_stats_is_prep_stack_on_the_host(hostlib, kind):
    """nl, fsafe and ovf[0] of prep_stack compiled for the host equal the numpy statement bit for bit on the batches the GPU test
    uses (bad stacks, liquid layers, non-monotone stacks included); ovf[1], ovf[2] are 2 logf and 4 logf of its rhomax and 2 bmax^2
    within 1 fp32 ulp (the C library's logf)."""
    seen = set()
    for TL, Lmax, B, P in pc.SHAPES:
        m, nlay, bad = pc.batch(Lmax, min(B, 600))
        e = pc.expected(m, nlay, kind)
        nl, fsafe, ovf = hostlib.host_prep_stats(m, kind, nlay)
        rows, _ = hostlib.host_prep_rows(m, kind, nlay)
        g = e["good"]
        assert np.array_equal(nl, e["nl"]) and not g[list(bad)].any() and g.sum() == len(g) - len(bad), (Lmax, bad)
        assert np.array_equal(fsafe.view(np.uint32), e["fsafe"].view(np.uint32))
        assert np.array_equal(ovf[0][g].view(np.uint32), e["hthick"][g].view(np.uint32))
        assert np.array_equal(rows[g].view(np.uint32), e["rows"][g].view(np.uint32))
        for row, arg in ((1, e["rhomax"]), (2, (np.float32(2.0) * e["bmax"] * e["bmax"]).astype(np.float32))):
            ref = (2.0 * row) * np.log(arg[g].astype(np.float64))
            assert (np.abs(ovf[row][g] - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all(), (Lmax, row)
        seen |= {("bad", k) for k in bad.values()}
        seen |= {("liquid", bool((e["hthick"][g] == np.float32(1e30)).any())), ("nonmono", bool((e["fsafe"][g] == np.float32(1e30)).any())),
                 ("n2", bool((nlay[g] == 2).any())), ("full", bool((nlay[g] == Lmax).any()))}
    assert seen >= {("bad", k) for k in pc.BAD_KINDS} | {("liquid", True), ("nonmono", True), ("n2", True), ("full", True)}, seen
