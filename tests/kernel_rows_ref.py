"""Host statements of what the sensitivity-kernel entries do AFTER the eigenproblem (csrc/surfdisp_kernels.hip): the
per-layer flattening factors of ``prep_stack`` and the chain factors of ``chain_of`` / ``kern_coef`` that turn the
partials with respect to the flattened, attenuated layer values (SURFDISP_KERN_REFCOORD) into the caller's dc/dVs,
dc/dVp, dc/drho.  Plain numpy; in the style of tests/secular64.py and tests/mcmc_replay.py.

    regular layer i   : dif_i = (1/r_n - 1/r_i) R0 / ln(r_i/r_n),  qqq_i = (r_i^p - r_n^p) / (ln(r_i/r_n) R0^p p),
                        dfl_i = R0 ln(R0/r_n) - R0 ln(R0/r_i)                               (flat1.f:44-56, 65-68)
    layer i as half space: hsf_i = R0 / r_i,  hsr_i = (1/hsf_i)^p                            (flat1.f:58-62)
    r_i = R0 - sum_{j<i} h_j,  r_n = r_i - h_i,  p = 2.275 (Rayleigh) | 5 (Love),  R0 = 6371

    qsq = qsinv ln(1/T) / pi,  qpq = qsq (4/3) Vs^2 / Vp^2                                   (calcul.f:122-126)
    dbdb = (1 + qsq) f,  dadb = (8/3) qsq (Vs/Vp) f,  dada = (1 - qpq) f,  rfac
    with f = dif, rfac = qqq for a regular layer and f = hsf, rfac = hsr for the layer used as half space, so that
    dc/dVs = dbdb rawb + dadb rawa,  dc/dVp = dada rawa,  dc/drho = rfac rawr."""
import functools
import os

import numpy as np

EUS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test1_eus.npz"))
R0 = 6371.0
FIELDS = ("dif", "qqq", "dfl", "hsf", "hsr")


def pwr_of(kind):
    """The flattening exponent as the kernel holds it: an fp32 constant (2.275 is not representable)."""
    return np.float32(5.0 if int(kind) & 3 == 1 else 2.275)


def _stacks(model, nlay):
    m = np.asarray(model)
    m = m[None] if m.ndim == 2 else m
    B, _, L = m.shape
    n = np.full(B, L, np.int64) if nlay is None else np.asarray(nlay, np.int64).ravel()
    return m, n


def _log32(x):
    return np.log(x.astype(np.float64)).astype(np.float32)          # log32: fp64 log, rounded once


def _pow32(x, p):
    return np.power(x.astype(np.float64), np.float64(p)).astype(np.float32)      # powr32


def prep_factors32(model, kind, nlay=None):
    """dif, qqq, dfl, hsf, hsr float32 [B, L] of model [B, 5, L] (or [5, L] -> [1, L]) exactly as ``prep_stack`` forms
    them: fp32 in the kernel's operation order, log / pow in fp64 rounded once.  The last layer of a stack (index
    nlay - 1) has dif = qqq = dfl = 0; entries at and beyond nlay are 0."""
    m, n = _stacks(model, nlay)
    B, _, L = m.shape
    f32 = np.float32
    r0, pwr = f32(R0), pwr_of(kind)
    apw = _pow32(np.full(1, r0), pwr)[0]
    h = m[:, 3, :].astype(f32)
    out = {k: np.zeros((B, L), f32) for k in FIELDS}
    hs = np.zeros(B, f32)
    r_i = np.full(B, r0, f32)
    z_i = np.zeros(B, f32)
    with np.errstate(all="ignore"):
        for i in range(L):
            live, reg = i < n, i < n - 1
            hs = (hs + h[:, i]).astype(f32)
            r_n = (r0 - hs).astype(f32)
            fltd = _log32(r_i / r_n)
            dif = (f32(1.0) / r_n - f32(1.0) / r_i) * r0 / fltd
            difr = _pow32(r_i, pwr) - _pow32(r_n, pwr)
            qqq = difr / (fltd * apw * pwr)
            z_n = r0 * _log32(r0 / r_n)
            dfl = z_n - z_i
            hsf = r0 / r_i
            hsr = _pow32(f32(1.0) / hsf, pwr)
            for k, v, sel in (("dif", dif, reg), ("qqq", qqq, reg), ("dfl", dfl, reg), ("hsf", hsf, live), ("hsr", hsr, live)):
                assert v.dtype == f32
                out[k][:, i] = np.where(sel, v, f32(0.0))
            z_i = np.where(reg, z_n, z_i)
            r_i = r_n
    return out


def prep_factors64(model, kind, nlay=None):
    """The same formulas in float64 on the fp32 inputs (thickness sums included)."""
    m, n = _stacks(model, nlay)
    B, _, L = m.shape
    p = np.float64(pwr_of(kind))
    h = m[:, 3, :].astype(np.float64)
    bot = np.cumsum(h, axis=1)
    r_n = R0 - bot
    r_i = R0 - (bot - h)
    idx = np.arange(L)[None, :]
    live, reg = idx < n[:, None], idx < n[:, None] - 1
    with np.errstate(all="ignore"):
        fltd = np.log(r_i / r_n)
        dif = (1.0 / r_n - 1.0 / r_i) * R0 / fltd
        qqq = (r_i ** p - r_n ** p) / (fltd * R0 ** p * p)
        dfl = R0 * np.log(R0 / r_n) - R0 * np.log(R0 / r_i)
        hsf = R0 / r_i
        hsr = (1.0 / hsf) ** p
    z = np.zeros((B, L))
    return dict(dif=np.where(reg, dif, z), qqq=np.where(reg, qqq, z), dfl=np.where(reg, dfl, z),
                hsf=np.where(live, hsf, z), hsr=np.where(live, hsr, z))


def prep_bounds(model, kind, nlay=None):
    """(bound, sel): per field the relative bound [B, L] of an fp32 evaluation in the kernel's operation order against
    prep_factors64 - derived in tests/test_kernel_rows_host.py::test_prep_factors32_within_the_cancellation_bound_of_float64 - and
    the entries it holds for (regular layers for dif, qqq, dfl; live layers for hsf, hsr).  Regular layers must be thicker than
    0.05 km: the bound is for layers far above the radii's ulp."""
    m, n = _stacks(model, nlay)
    B, _, L = m.shape
    p = float(pwr_of(kind))
    h = np.maximum(m[:, 3, :].astype(np.float64), 1e-30)            # (the half space's 0 is never selected)
    reg = np.arange(L)[None, :] < n[:, None] - 1
    live = np.arange(L)[None, :] < n[:, None]
    assert (h[reg] > 0.05).all()
    hl = np.where(live, m[:, 3, :].astype(np.float64), 0.0)
    r_top = R0 - (np.cumsum(hl, axis=1) - hl)                       # radius of the layer's top
    dr_top = 2.0 ** -12 + np.arange(L)[None, :] * 2.0 ** -17       # ... its fp32 error: i additions and the subtraction
    dr = dr_top + 2.0 ** -17                                       # (a depth below layer i: one more addition)
    e = 2.0 ** -24
    bound = dict(dif=3 * e * R0 / h + 8 * e, qqq=3 * e * R0 / h + 8 * e,
                 dfl=(2 * (R0 * e + 2.0 ** -17 + dr) + 2.0 ** -17) / h,
                 hsf=dr_top / r_top + 2 * e, hsr=p * (dr_top / r_top + 2 * e) + 2 * e)
    return bound, {k: (live if k in ("hsf", "hsr") else reg) for k in FIELDS}


ACCUR = np.float32(1.0e-8)           # csrc/surfdisp_k_common.h


def prep_stats(model, kind, nlay=None, factors=None):
    """The per-stack verdict and statistics of ``prep_stack`` restated in numpy, fp32 in its operation order, on the factors of
    ``prep_factors32``: dict of nl int32 [B] (0: a bad stack), fsafe float32 [B] (the thickest regular layer of a good, monotone
    stack, else 1e30), hthick (ovf[0]: the thickest flattened layer, 1e30 with a liquid layer below the top), rhomax and bmax
    (float32: the arguments of the two logarithms, ovf[1] = 2 logf(rhomax), ovf[2] = 4 logf(2 bmax^2)).  hthick, rhomax and bmax
    are meaningful for good stacks only."""
    m, n = _stacks(model, nlay)
    B, _, L = m.shape
    f32 = np.float32
    f = prep_factors32(m, kind, np.clip(n, 0, L)) if factors is None else factors
    idx = np.arange(L)[None, :]
    ok_n = (n >= 2) & (n <= L)
    live, reg = (idx < n[:, None]) & ok_n[:, None], (idx < n[:, None] - 1) & ok_n[:, None]
    vp, vs, rho, h, qs = (m[:, k, :].astype(f32) for k in range(5))
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(vp) & np.isfinite(vs) & np.isfinite(rho) & np.isfinite(h) & np.isfinite(qs)) | ~(vp > 0) | ~(rho > 0) | (vs < 0) | (h < 0)
        r_n = (f32(R0) - np.cumsum(h, axis=1, dtype=f32)).astype(f32)           # (numpy sums a row of fp32 in order)
        bad_reg = ~(r_n > 0) | ~np.isfinite(f["dif"]) | ~np.isfinite(f["qqq"])
        ok = ok_n & ~(bad & live).any(axis=1) & ~(bad_reg & reg).any(axis=1)
        hmax = np.where(reg, h, f32(0)).max(axis=1).astype(f32)
        drop = np.zeros((B, L), bool)
        drop[:, 1:] = (vs[:, 1:] < vs[:, :-1]) | (vp[:, 1:] < vp[:, :-1])
        mono = ~(drop & live).any(axis=1)
        hthick = np.where(live, f["dfl"], f32(0)).max(axis=1).astype(f32)
        liquid = (~(np.abs(vs) > ACCUR) & live & (idx > 0)).any(axis=1)
        hthick = np.where(liquid, f32(1.0e30), hthick).astype(f32)
        rhomax = np.where(live, rho * np.maximum(f["qqq"], f["hsr"]), f32(0)).max(axis=1).astype(f32)
        bmax = np.where(live, (f32(1.06) * vs) * np.maximum(f["dif"], f["hsf"]), f32(0)).max(axis=1).astype(f32)
    return dict(nl=np.where(ok, n, 0).astype(np.int32), fsafe=np.where(ok & mono, hmax, f32(1.0e30)).astype(f32),
                hthick=hthick, rhomax=rhomax, bmax=bmax)


def chain64(model, periods, kind, factors):
    """Chain factors float64 [B, P, L] per (stack, period, layer) from the fp32 inputs and the per-layer ``factors``
    (``prep_factors32`` for what the kernel multiplies with, ``prep_factors64`` for the exact ones): dbdb, dadb, dada,
    rfac for the regular role and dbdb_hs, dadb_hs, dada_hs, rfac_hs for the half-space role.  The attenuation part is
    float64.  Love has no Vp dependence: its dadb is 0 and dada is not used.  Water layers (Vs <= 0): dadb = 0."""
    m, _ = _stacks(model, None)
    T = np.asarray(periods, np.float32).astype(np.float64).ravel()
    vp, vs, qs = (m[:, r, None, :].astype(np.float64) for r in (0, 1, 4))
    lnT = np.log(1.0 / T)[None, :, None]
    qsq = qs * lnT / np.pi
    with np.errstate(all="ignore"):
        qpq = qsq * (4.0 / 3.0) * vs * vs / (vp * vp)
        dadb = (8.0 / 3.0) * qsq * (vs / vp)
    if int(kind) & 3 == 1:
        dadb = np.zeros_like(dadb)
    out = {}
    for tag, fk, rk in (("", "dif", "qqq"), ("_hs", "hsf", "hsr")):
        f = np.asarray(factors[fk], np.float64)[:, None, :]
        out["dbdb" + tag] = (1.0 + qsq) * f
        out["dadb" + tag] = dadb * f
        out["dada" + tag] = (1.0 - qpq) * f
        out["rfac" + tag] = np.broadcast_to(np.asarray(factors[rk], np.float64)[:, None, :], out["dbdb" + tag].shape).copy()
    return out


def predict_rows(ch, rawb, rawa, rawr, role=""):
    """Caller-coordinate rows from REFCOORD rows: (dcdb, dcda, dcdr) and, for each, the sum of the magnitudes of its
    terms (what a rounding bound is relative to).  ``rawa`` None: Love."""
    rb, rr = np.asarray(rawb, np.float64), np.asarray(rawr, np.float64)
    ra = np.zeros_like(rb) if rawa is None else np.asarray(rawa, np.float64)
    t1, t2 = ch["dbdb" + role] * rb, ch["dadb" + role] * ra
    ka, kr = ch["dada" + role] * ra, ch["rfac" + role] * rr
    return (t1 + t2, ka, kr), (np.abs(t1) + np.abs(t2), np.abs(ka), np.abs(kr))


EPS = 2.0 ** -24
CHAIN_ULPS = 16.0                  # the plain and the REFCOORD code path differ by fewer than eight fp32 roundings
CHAIN_FLOOR = 16.0 * 2.0 ** -126   # below the smallest normal fp32 number a rounding is absolute (2^-126 at most), not relative


def chain_errors(m, nlay, per, kind, plain, raw):
    """Worst |row - prediction| in units of the bar (16 x 2^-24 of the sum of the magnitudes of the terms) for (layers
    above the unit's deepest non-zero layer, that layer where it is the stack's last, that layer elsewhere), and the
    counts of units compared."""
    c, u, st, kb, ka, krho = plain
    _, _, _, rb, ra, rr = raw
    B, P, L = kb.shape
    n = np.full(B, L) if nlay is None else np.asarray(nlay, np.int64)
    ch = chain64(m, per, kind, prep_factors32(m, kind, nlay))
    solved = c > 0
    nzrow = (kb != 0).any(axis=2)
    assert solved.sum() > 0 and not (nzrow & ~solved).any()
    assert nzrow.sum() >= 0.9 * solved.sum(), (int(nzrow.sum()), int(solved.sum()))
    assert np.array_equal(kb != 0, rb != 0)                            # the same layers carry a share in both calls
    last = L - 1 - np.argmax((kb != 0)[:, :, ::-1], axis=2)            # [B, P]: the unit's deepest non-zero layer
    idx = np.arange(L)[None, None, :]
    with np.errstate(invalid="ignore"):
        solid = (m[:, 1, :] > 0)[:, None, :]
    above = nzrow[:, :, None] & (idx < last[:, :, None]) & solid
    at = nzrow[:, :, None] & (idx == last[:, :, None]) & solid
    at_end = at & (last == (n[:, None] - 1))[:, :, None]
    at_mid = at & ~at_end
    below = idx > np.where(nzrow, last, -1)[:, :, None]
    reg, mag = predict_rows(ch, rb, ra, rr, "")
    hsp, hmag = predict_rows(ch, rb, ra, rr, "_hs")
    worst = [0.0, 0.0, 0.0]
    for q, (got, rawrow) in enumerate(((kb, rb), (ka, ra), (krho, rr))):
        if got is None:
            assert kind & 3 == 1 and q == 1
            continue
        assert not got[below].any() and not rawrow[below].any()
        g = got.astype(np.float64)
        bar, hbar = CHAIN_ULPS * EPS * mag[q] + CHAIN_FLOOR, CHAIN_ULPS * EPS * hmag[q] + CHAIN_FLOOR
        e_above = np.abs(g - reg[q]) / bar
        e_end = np.abs(g - hsp[q]) / hbar
        lo, hi = np.minimum(reg[q], hsp[q]), np.maximum(reg[q], hsp[q])
        e_mid = np.maximum(np.maximum(lo - g, g - hi), 0.0) / np.maximum(bar, hbar)
        for j, (e, sel) in enumerate(((e_above, above), (e_end, at_end), (e_mid, at_mid))):
            if sel.any():
                worst[j] = max(worst[j], float(e[sel].max()))
    return worst, (int(nzrow.sum()), int(at_end.any(axis=2).sum()), int(at_mid.any(axis=2).sum()))


DEEP_PICKS = (0, 63, 64, 127, 128, 129, 7, 100)      # both sides of every 64-stack tile edge + two shallow stacks


@functools.lru_cache(maxsize=None)
def _deep_batch():
    """The deep, ragged batch: B = 130 (three 64-stack tiles, the last with two stacks), Lmax = 70 (two 64-layer tiles,
    the second with six layers) -> (model [130, 5, 70], nlay int32 [130]).  Monotone stacks, nlay ragged in 3 .. 70 with
    stacks 0, 63, 64, 127, 128, 129 at 64, 65, 70, 70, 64, 65 layers and stacks 7, 100 at 3 and 9; water tops on stacks 5,
    62, 128; stack 31 not finite; the half space of stack 33 (3.2 km/s) slower than the mode at long periods."""
    from pysurfinv_amd import synth
    m = synth.synth_models(130, 70, seed=29, noise=0.03, monotone=True)
    nlay = np.random.default_rng(5).integers(3, 71, 130).astype(np.int32)
    for s, n in zip(DEEP_PICKS, (64, 65, 70, 70, 64, 65, 3, 9)):
        nlay[s] = n
    for s in (5, 62, 128):
        m[s, 1, 0] = 0.0; m[s, 0, 0] = 1.475; m[s, 2, 0] = 1.027; m[s, 4, 0] = 1e-4; m[s, 3, 0] = 2.0
    nlay[31] = nlay[33] = 70
    m[31, 1, 3] = np.nan
    m[33, 1, -1] = 3.2; m[33, 0, -1] = 1.76 * 3.2
    return m, nlay


def deep_batch():
    m, nlay = _deep_batch()
    return m.copy(), nlay.copy()


TALL_PICKS = (0, 1, 63, 64, 65, 7, 20, 21)           # both sides of the 64-stack tile edge, of layers 64 and 128, a shallow stack


@functools.lru_cache(maxsize=None)
def _tall_batch():
    """Three 64-layer tiles, the last with ONE row: B = 66 (a full 64-stack tile and one with two stacks), Lmax = 129 ->
    (model [66, 5, 129], nlay int32 [66]).  Monotone stacks, nlay ragged in 3 .. 129 with stacks 0, 1, 63, 64, 65, 7, 20, 21
    at 129, 128, 129, 65, 64, 3, 127, 66 layers."""
    from pysurfinv_amd import synth
    m = synth.synth_models(66, 129, seed=31, noise=0.03, monotone=True)
    nlay = np.random.default_rng(9).integers(3, 130, 66).astype(np.int32)
    for s, n in zip(TALL_PICKS, (129, 128, 129, 65, 64, 3, 127, 66)):
        nlay[s] = n
    return m, nlay


def tall_batch():
    m, nlay = _tall_batch()
    return m.copy(), nlay.copy()


CHAIN_PERIODS = (6.0, 10.0, 25.0, 60.0, 100.0)


def chain_inputs():
    """name -> (model, nlay, periods) of the chain-factor tests: a 12-layer stack, the TEST1 model (68 layers), a water top,
    a sediment stack whose sediment layers have Qs 20 .. 80 (qsq reaches 7e-2; also run at T = 1 s, where ln(1/T) = 0),
    the deep ragged batch."""
    from pysurfinv_amd import synth
    sed = synth.sediment_models(1, 10, seed=7, total_thickness=120.0)
    soft = sed[0, 1] < 1.5
    assert 1 <= soft.sum() <= 4
    sed[0, 4, soft] = 1.0 / np.linspace(20.0, 80.0, int(soft.sum()))
    dm, dn = deep_batch()
    return {"synth_L12": (synth.synth_models(1, 12, seed=3, noise=0.05), None, CHAIN_PERIODS),
            "eus_L68": (EUS["model"].astype(np.float32), None, CHAIN_PERIODS),
            "water_L9": (synth.water_models(1), None, CHAIN_PERIODS),
            "sediment_L10": (sed, None, (1.0,) + CHAIN_PERIODS),
            "deep_L70": (dm, dn, CHAIN_PERIODS)}
