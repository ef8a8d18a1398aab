"""CPU tests of tests/kernel_rows_ref.py, the host statement of prep_stack's flattening factors and of the chain factors
(no GPU): fp32 replay against float64 at a derived cancellation bound, bit-exact against prep_stack itself compiled for the
host, and the closed forms of the chain factors at T = 1 s and 1/Qs = 0."""
import numpy as np
import pytest

import kernel_rows_ref as kr
from hostcheck_lib import hostlib  # noqa: F401  (fixture: the kernel's SD_HD code compiled for the host)

EPS = 2.0 ** -24


def _inputs():
    """(name, model [B, 5, L], nlay): thick and thin layers, a water top, 68 and 70 layers, ragged nlay."""
    import os
    from pysurfinv_amd import synth
    eus = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test1_eus.npz"))["model"].astype(np.float32)
    deep, nlay = kr.deep_batch()
    ok = np.isfinite(deep).all(axis=(1, 2))
    return (("synth_L12", synth.synth_models(2, 12, seed=3, noise=0.05), None), ("eus_L68", eus, None),
            ("water_L9", synth.water_models(2), None),
            ("sediment_L10", synth.sediment_models(3, 10, seed=7, total_thickness=120.0), None),
            ("deep_L70", deep[ok], nlay[ok]))


@pytest.mark.parametrize("kind", [2, 1])
def test_prep_factors32_within_the_cancellation_bound_of_float64(kind):
    """prep_factors32 (fp32, the kernel's operation order) against prep_factors64.  The bounds, with e = 2^-24, R0 = 6371,
    h the layer's thickness, p the exponent, L the layer count and r >= R0 - sum h the radii:
      dif : 1/r_n and 1/r_i are each rounded (e/r) and subtracted (the difference is h/r^2): 2 e r/h; the quotient r_i/r_n
            is rounded next to 1 (e) before its log (h/r): e r/h.  Errors of the radii themselves cancel in the ratio.
            |d dif / dif| <= 3 e R0/h + 8 e   (8 e: the remaining roundings of single operations)
      qqq : r_i^p and r_n^p each rounded (e r^p), the difference is p r^(p-1) h: (2/p) e r/h, and the same log: the same
            bound holds (p > 1).
      dfl : z = R0 log(R0/r): the quotient is rounded in [1, 2) (e) -> R0 e, z itself to 2^-17 (z < 256), the radius to
            2^-12 (r in [4096, 8192)), the fp32 thickness sum above layer i's bottom to (i + 1) 2^-17 (sum < 256): each of
            the two depths is off by at most a = R0 e + 2^-17 + 2^-12 + (i + 1) 2^-17, the difference is rounded again:
            |d dfl| <= 2 a + 2^-17.
      hsf : |d r| / r + 2 e at the layer's own top radius r, |d r| <= 2^-12 + i 2^-17;   hsr = (1/hsf)^p: p times that + 2 e.
    Measured: dif 0.70, qqq 0.45 (Love 0.38), dfl 0.62, hsf 0.49, hsr 0.46 (Love 0.52) of these bounds at worst."""
    worst = {k: 0.0 for k in kr.FIELDS}
    for name, m, nlay in _inputs():
        f32, f64 = kr.prep_factors32(m, kind, nlay), kr.prep_factors64(m, kind, nlay)
        bound, sels = kr.prep_bounds(m, kind, nlay)                    # (the formulas above, shared with the tests of the prep kernel)
        for k in kr.FIELDS:
            sel = sels[k]
            assert not f32[k][~sel].any() and not f64[k][~sel].any(), (name, k)
            rel = np.abs(f32[k].astype(np.float64)[sel] / f64[k][sel] - 1.0) / bound[k][sel]
            worst[k] = max(worst[k], float(rel.max()))
            assert rel.max() <= 1.0, (name, kind, k, float(rel.max()))
    print(f"prep_factors32 vs float64, kind {kind}: worst fraction of the bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert all(v > 0.02 for v in worst.values())                       # (a bound a hundred times too wide says nothing)


@pytest.mark.parametrize("kind", [2, 1])
def test_prep_factors32_is_prep_stack_bit_for_bit(hostlib, kind):
    """prep_stack itself (SD_HD, compiled for the host by tests/hostcheck) returns the same bits as the numpy statement for
    dif, qqq, dfl, hsf, hsr of every layer, ragged nlay and a water top included; a non-finite stack gets nl = 0."""
    for name, m, nlay in _inputs():
        rows, nl = hostlib.host_prep_rows(m, kind, nlay)
        f32 = kr.prep_factors32(m, kind, nlay)
        assert (nl == (m.shape[2] if nlay is None else nlay)).all(), name
        for j, k in enumerate(kr.FIELDS):
            assert np.array_equal(rows[:, 4 + j, :].view(np.int32), f32[k].view(np.int32)), (name, kind, k)
    deep, nlay = kr.deep_batch()
    _, nl = hostlib.host_prep_rows(deep, kind, nlay)
    assert nl[31] == 0 and (np.delete(nl, 31) == np.delete(nlay, 31)).all()


def test_chain64_closed_forms():
    """T = 1 s: ln(1/T) = 0, so dadb = 0 and dbdb = dada = f exactly; 1/Qs = 0: the same at every period; Love: dadb = 0;
    at Qs = 20, T = 100 s qsq = -7.3e-2 and the factors follow their definitions."""
    from pysurfinv_amd import synth
    m = synth.sediment_models(1, 10, seed=7, total_thickness=120.0)
    m[0, 4, 0] = 1.0 / 20.0
    per = np.array([1.0, 100.0], np.float32)
    f = kr.prep_factors32(m, 2)
    ch = kr.chain64(m, per, 2, f)
    for tag, fk, rk in (("", "dif", "qqq"), ("_hs", "hsf", "hsr")):
        assert np.array_equal(ch["dbdb" + tag][0, 0], f[fk][0].astype(np.float64))
        assert np.array_equal(ch["dada" + tag][0, 0], f[fk][0].astype(np.float64))
        assert not ch["dadb" + tag][0, 0].any()
        assert np.array_equal(ch["rfac" + tag][0, 1], f[rk][0].astype(np.float64))
    qsq = float(m[0, 4, 0]) * np.log(1.0 / 100.0) / np.pi
    assert abs(qsq + 7.33e-2) < 1e-4
    vs, vp = float(m[0, 1, 0]), float(m[0, 0, 0])
    assert ch["dbdb"][0, 1, 0] == (1.0 + qsq) * float(f["dif"][0, 0])
    assert np.isclose(ch["dadb"][0, 1, 0], (8.0 / 3.0) * qsq * vs / vp * float(f["dif"][0, 0]), rtol=1e-15)
    assert np.isclose(ch["dada_hs"][0, 1, 0], (1.0 - qsq * (4.0 / 3.0) * vs * vs / (vp * vp)) * float(f["hsf"][0, 0]), rtol=1e-15)
    m0 = m.copy(); m0[:, 4, :] = 0.0
    c0 = kr.chain64(m0, per, 2, f)
    assert np.array_equal(c0["dbdb"][0, 0], c0["dbdb"][0, 1]) and not c0["dadb"].any()
    assert not kr.chain64(m, per, 1, kr.prep_factors32(m, 1))["dadb"].any()


@pytest.mark.parametrize("kind", [2, 1])
def test_chain_factors_on_the_host_compiled_kernel(hostlib, kind):
    """The KERN instantiation of group_rayleigh / group_love compiled for the host (the code the device runs: kern_coef,
    chain_of, the sweep, the unit's factor), plain and with unit chain factors, at the oracle's roots of one-period solves:
    at every solved unit, for every solid layer above the unit's deepest non-zero layer, dcdb = dbdb rawb + dadb rawa,
    dcda = dada rawa, dcdr = rfac rawr with the regular-role factors of chain64 on prep_factors32; the deepest non-zero
    layer with the half-space-role factors where it is the stack's last layer, else between the two roles' predictions.
    Bar (derived): 16 x 2^-24 of the sum of the magnitudes of the terms - the two paths differ by fewer than eight fp32
    roundings (1 + qsq, x f, the layer's coefficient, the share's rounding to fp32, the unit's factor on either side).
    Inputs of kernel_rows_ref.chain_inputs (the deep batch: twelve of its stacks, 64, 65 and 70 layers among them).
    Measured: 4.4 roundings (Rayleigh), 3.6 (Love) at worst.  With dada = (1 + qpq) f planted the Rayleigh rows miss by
    1.4e5 .. 3.0e5 roundings on every input; with dif in place of hsf the last layer's row is zero."""
    total = 0.0
    for name, (m, nlay, per) in kr.chain_inputs().items():
        per = np.asarray(per, np.float32)
        if name == "deep_L70":
            pick = list(kr.DEEP_PICKS) + [5, 33, 62, 90]
            m, nlay = np.ascontiguousarray(m[pick]), nlay[pick]
        B, _, L = m.shape
        c, ratio = np.zeros((B, per.size), np.float32), np.zeros((B, per.size), np.float32)
        for b in range(B):
            n = L if nlay is None else int(nlay[b])
            for k in range(per.size):                                  # one-period solves, as SURFDISP_INDEPENDENT
                cc, _, rr = hostlib.oracle_dbg(np.ascontiguousarray(m[b:b + 1, :, :n]), per[k:k + 1], kind)
                if not cc[0, 0] > 0:
                    break                                              # (later periods stay unsolved: the failure cascade)
                c[b, k], ratio[b, k] = cc[0, 0], rr[0, 0]
        plain = hostlib.host_kernels(m, per, kind, c, ratio, nlay)
        raw = hostlib.host_kernels(m, per, kind, c, ratio, nlay, refcoord=True)
        assert np.array_equal(plain[0], raw[0])
        worst, cnt = kr.chain_errors(m, nlay, per, kind, (c, plain[0], None) + plain[1:], (c, raw[0], None) + raw[1:])
        print(f"chain factors (host) {name} kind {kind}: units {cnt[0]} (half space in the last layer {cnt[1]}, higher {cnt[2]}); "
              f"worst above {worst[0] * kr.CHAIN_ULPS:.2f} last-layer {worst[1] * kr.CHAIN_ULPS:.2f} between "
              f"{worst[2] * kr.CHAIN_ULPS:.2f} roundings (bar {kr.CHAIN_ULPS:.0f})")
        assert cnt[0] > 0 and cnt[1] > 0 and cnt[2] > 0, cnt
        assert max(worst) <= 1.0, (name, worst)
        total = max(total, max(worst))
    assert total > 0
