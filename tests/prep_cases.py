"""What the tests of the working stack (K0, csrc/surfdisp_k_prep.h) share: the batches, and what prep_stack must write for them
according to tests/kernel_rows_ref.py.  A plain module, not a conftest.

A batch mixes ragged nlay (2 and Lmax included), a water top, Vs = 0 below the top (hthick = 1e30), a non-monotone stack (fsafe =
1e30), sub-kilometre layers deep in the stack and the bad stacks of test_gpu_parity.test_bad_models_are_flagged_not_crashing
(nl = 0), each between good neighbours: at stack 1 (inside the first wavefront), at the last stack of the first block of the prep
launch, just behind it, and at stack 5.  Regular layers are thicker than 0.05 km and a stack is thinner than 256 km, which the
derived fp32 bounds of kernel_rows_ref.prep_bounds assume."""
import numpy as np

import kernel_rows_ref as kr

# (lanes per stack of the prep launch, Lmax, B, P): the smallest shapes that reach each of the seven instantiations per wave type,
# B no multiple of 256 / TL there; four passes of a lane over the layers; the cap of 262 144 lanes binding; one lane per stack
SHAPES = [(2, 2, 259, 1), (4, 3, 131, 2), (8, 5, 67, 3), (16, 9, 35, 1), (32, 17, 19, 2), (64, 33, 11, 3), (64, 200, 3, 1),
          (16, 33, 20000, 1), (1, 2, 262144, 1)]
FILL = np.uint32(0xA5A5A5A5)
BAD_KINDS = ("nan_vp", "negative_h", "nlay_1", "nlay_over")


def prep_lanes(B, Lmax):
    """launch_prep's rule (csrc/surfdisp_kernels.hip): about 262 144 lanes, never more lanes than layers (rounded up to a power of two)."""
    TL = 1
    while TL < 64 and B * TL < 262144 and TL < Lmax:
        TL *= 2
    return TL


def batch(Lmax, B, seed=0):
    """(model float32 [B, 5, Lmax], nlay int32 [B], {stack: bad kind})."""
    nb = min(B, 4096)                                       # (a large batch repeats 4096 distinct stacks)
    rng = np.random.default_rng(1000 + 7 * Lmax + seed)
    n = rng.integers(2, Lmax + 1, nb)
    n[0] = Lmax
    if nb > 2:
        n[2] = 2
    w = rng.uniform(0.2, 1.0, (nb, Lmax))
    total = rng.uniform(100.0 if Lmax > 20 else 20.0, 240.0, (nb, 1))
    h = total * w / w.sum(axis=1, keepdims=True)
    z = np.linspace(0.0, 1.0, Lmax)
    vs = np.sort(3.0 + 1.6 * z + rng.normal(0.0, 0.05, (nb, Lmax)), axis=1)
    vp = 1.76 * vs
    rho = 0.541 + 0.3601 * vp
    qs = np.where(vs < 4.0, 1.0 / 600.0, 1.0 / 150.0)
    b = np.arange(nb)
    deep = (b % 4 == 1) & (n >= 6)
    h[deep, n[deep] - 3] = 0.3                              # a sub-kilometre layer deep in the stack
    water = (b % 5 == 0) & (n >= 3)
    vs[water, 0], vp[water, 0], rho[water, 0], h[water, 0], qs[water, 0] = 0.0, 1.475, 1.027, 2.0, 1.0e-4
    liquid = (b % 7 == 3) & (n >= 4)
    vs[liquid, min(2, Lmax - 1)] = 0.0                      # Vs = 0 below the top
    dip = (b % 7 == 5) & (n >= 3) & ~water
    vs[dip, 1] = vs[dip, 0] - 0.2                           # a non-monotone stack
    h[b, n - 1] = 0.0                                       # the half space
    m = np.stack([vp, vs, rho, h, qs], axis=1).astype(np.float32)
    reps = -(-B // nb)
    m, n = np.tile(m, (reps, 1, 1))[:B].copy(), np.tile(n, reps)[:B].astype(np.int32)
    per_block = 256 // prep_lanes(B, Lmax)
    bad = {}
    for k, pos in enumerate(sorted({1, per_block - 1, per_block + 1, 5})):
        if pos % 2 == 0 or pos >= B - 1:
            continue
        kind = BAD_KINDS[(k + Lmax + seed) % 4]
        bad[pos] = kind
        if kind == "nan_vp":
            m[pos, 0, min(2, n[pos] - 1)] = np.nan
        elif kind == "negative_h":
            m[pos, 3, 0] = -1.0
        else:
            n[pos] = 1 if kind == "nlay_1" else Lmax + 1
    return m, n, bad


def expected(model, nlay, kind):
    """What prep_stack must leave for `model`: dict of
      rows float32 [B, 9, Lmax] (vp, vs, rho, 1/Qs, dif, qqq, dfl, hsf, hsr; zero where nothing is written),
      written bool [B, Lmax] (layers i < nlay of a stack with 2 <= nlay <= Lmax: the kernel writes them whatever they hold),
      good bool [B], nl, fsafe, hthick, rhomax, bmax (kernel_rows_ref.prep_stats),
      f64 / bound / sel: prep_factors64 and the derived relative fp32 bounds per field, on the good stacks (ones elsewhere)."""
    B, _, L = model.shape
    n = np.asarray(nlay, np.int64)
    valid_n = (n >= 2) & (n <= L)
    nc = np.where(valid_n, n, 0)
    f = kr.prep_factors32(model, kind, nc)
    st = kr.prep_stats(model, kind, n, factors=f)
    good = st["nl"] > 0
    rows = np.zeros((B, 9, L), np.float32)
    written = np.arange(L)[None, :] < nc[:, None]
    for j, src in enumerate((0, 1, 2, 4)):
        rows[:, j, :] = np.where(written, model[:, src, :], 0.0)
    for j, k in enumerate(kr.FIELDS):
        rows[:, 4 + j, :] = f[k]
    clean = np.where(good[:, None, None], model, model[np.argmax(good)][None]).astype(np.float32)   # (bounds of good stacks only)
    ng = np.where(good, n, n[np.argmax(good)])
    bound, sel = kr.prep_bounds(clean, kind, ng)
    return dict(rows=rows, written=written, good=good, f64=kr.prep_factors64(clean, kind, ng), bound=bound,
                sel={k: v & good[:, None] for k, v in sel.items()}, **st)


def ulps(a, b):
    """|a - b| in units of the fp32 spacing at |b| (float32 arrays)."""
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)


def compare_copy(got, exp, what):
    """One copy of the working stack, got float32 [B, 9, Lmax] (the words as read from the workspace), against `exp`: returns
    (number of words of dif, qqq, dfl, hsr that differ from prep_factors32, their largest difference in fp32 ulp, the largest
    error of those fields against prep_factors64 as a fraction of the derived bound).  Asserted here: nothing is written beyond
    nlay or for a stack without a valid nlay; vp, vs, rho, 1/Qs, hsf are bit-equal; dif, qqq, dfl, hsr lie inside the derived fp32
    bounds of tests/test_kernel_rows_host.py against prep_factors64."""
    gw, ew = got.view(np.uint32), exp["rows"].view(np.uint32)
    W = np.broadcast_to(exp["written"][:, None, :], got.shape)
    assert (gw[~W] == FILL).all(), (what, "words beyond nlay were written")
    G = W & exp["good"][:, None, None]
    for j in (0, 1, 2, 3, 7):
        assert np.array_equal(gw[:, j][G[:, j]], ew[:, j][G[:, j]]), (what, "field", j)
    frac = 0.0
    for j, k in ((4, "dif"), (5, "qqq"), (6, "dfl"), (8, "hsr")):
        s = exp["sel"][k]
        rel = np.abs(got[:, j][s].astype(np.float64) / exp["f64"][k][s] - 1.0) / exp["bound"][k][s]
        frac = max(frac, float(rel.max()))
        assert rel.max() <= 1.0, (what, k, float(rel.max()))
        dead = G[:, j] & ~s                                # the last layer's dif, qqq, dfl: zero
        assert not got[:, j][dead].any(), (what, k)
    idx = np.array([4, 5, 6, 8])
    diff = (gw[:, idx] != ew[:, idx]) & G[:, idx]
    worst = float(ulps(got[:, idx][diff], exp["rows"][:, idx][diff]).max()) if diff.any() else 0.0
    return int(diff.sum()), worst, frac
