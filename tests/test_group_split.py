"""CPU checks of the fast path's own sublayer split in the Rayleigh group kernel (fast_sublayers in surfdisp_kernels.hip):
group_rayleigh compiled for the host (tests/hostcheck/splitcheck.hip) with the default step bound and with
-DSD_GROUP_LAMH=0 (the reference's split everywhere), fed with the oracle's own c and ellipticity.  U from the two splits
agrees within a few fp32 ulps, the new split is no further from the oracle than the reference's split, and the saving
survives the wavefront-level maximum (64 stacks at one period step the largest count among their lanes).
The split bar is set by rounding, not by the step: the knot integrands are fp32, so ANY change of the knots moves U by up
to ~4e-7 on rock stacks (a bound of 0.02, which saves 3 % of the sublayers, already gives 3.1e-7 on the bench stacks).
On sediment stacks (slow, thin layers: the largest lambda h) the step's own error adds up to ~2e-6, against their
~3e-5 distance from the oracle that the reference's split has too.  The high-contrast family (random, non-monotone
velocities, thick layers, periods from 2 s) reaches fit cancellations up to 1e7 on the fast path: there the fit and the
sweep must step the same split, and above SD_GROUP_OWN_CANCEL both step the reference's.
No GPU needed; skipped if hipcc is absent."""
import ctypes
import os

import numpy as np
import pytest

import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcheck")
SRC = os.path.join(HC, "splitcheck.hip")

U_SPLIT_BAR = {"rock": 1e-6, "sediment": 4e-6}   # U, new split vs the reference's split (8 fp32 ulps; sediment: below
                                                 # the rock stacks' oracle bar, a tenth of their own distance from the oracle)
U_ORACLE_BAR = 5e-6      # U vs the oracle on rock stacks (tests/test_group_powers.py)


@pytest.fixture(scope="module")
def libs():
    return {"new": ctypes.CDLL(hostbuild.build(SRC, os.path.join(HC, "libsplitcheck.so"))),
            "ref": ctypes.CDLL(hostbuild.build(SRC, os.path.join(HC, "libsplitcheck_ref.so"), extra=["-DSD_GROUP_LAMH=0.0f"]))}


@pytest.fixture(scope="module")
def oracle():
    from oracle import cport
    return cport.lib()


def _fp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _oracle(O, model, nlay, per):
    """the oracle's c, U and ellipticity per stack (each stack its own layer count)"""
    B = model.shape[0]; P = len(per)
    c = np.zeros((B, P), np.float32); u = np.zeros((B, P), np.float32); r = np.zeros((B, P), np.float32)
    fpf = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for i in range(B):
        m = np.ascontiguousarray(model[i, :, :nlay[i]])
        O.surfdisp_oracle_forward_dbg(int(nlay[i]), 2, fpf(m[0]), fpf(m[1]), fpf(m[2]), fpf(m[3]), fpf(m[4]),
                                      fpf(per), P, fpf(c[i]), fpf(u[i]), fpf(r[i]))
    return c, u, r


def _host(lib, model, nlay, per, c, r):
    B, _, L = model.shape; P = len(per)
    u = np.zeros((B, P), np.float32); hs = np.zeros((B, P), np.int32); rec = np.zeros((B, P, L, 2), np.int32)
    cancel = np.zeros((B, P))
    lib.sd_splitcheck_group(B, L, _fp(nlay), _fp(model), P, _fp(per), _fp(c), _fp(r), _fp(u), _fp(hs), _fp(rec),
                            _fp(cancel))
    return u, hs, rec, cancel


def _wave_cost(hs, rec, key):
    """sublayers stepped per wavefront (64 consecutive stacks, one period), the lanes' layer loops aligned from each
    lane's half-space layer: sum over loop iterations of the largest count among the lanes"""
    B, P, L, _ = rec.shape
    tot = 0
    for w0 in range(0, B, 64):
        for k in range(P):
            it = np.zeros(L, np.int64)
            for b in range(w0, min(w0 + 64, B)):
                h = hs[b, k]
                if h < 0:
                    continue
                n = rec[b, k, h::-1, key]                    # iteration i visits layer h - i
                it[:n.size] = np.maximum(it[:n.size], np.maximum(n, 0))
            tot += it.sum()
    return int(tot)


def _cases():
    from pysurfinv_amd import synth
    from pysurfinv_amd.settings import MCMC_PERIODS
    dper = synth.default_periods(20)
    mper = np.asarray(MCMC_PERIODS, np.float32)
    bench = synth.synth_models(1024, 10, seed=11)
    wet = synth.synth_models(512, 10, seed=12)
    wet[:, 0, 0] = 1.5; wet[:, 1, 0] = 0.0; wet[:, 2, 0] = 1.03
    sed = synth.sediment_models(512, 10, seed=13)
    rng = np.random.default_rng(14)
    nl = rng.integers(3, 21, 1024).astype(np.int32)          # ragged: 3 .. 20 layers, mixed within every wavefront
    rag = np.zeros((1024, 5, 20), np.float32)
    for n in range(3, 21):
        sel = np.nonzero(nl == n)[0]
        m = synth.synth_models(sel.size, n, seed=100 + n)
        rag[sel, :, :n] = m
        rag[sel, :, n:] = m[:, :, -1:]
    rng = np.random.default_rng(15)
    B, L = 1024, 12                                          # high contrast: Vs in random order, thick layers
    vs = rng.uniform(1.5, 4.8, (B, L)); vp = vs * rng.uniform(1.6, 2.2, (B, L)); h = rng.uniform(2.0, 60.0, (B, L))
    hc = np.stack([vp, vs, 0.541 + 0.3601 * vp, h, 1.0 / np.where(vs < 4.0, 600.0, 150.0)], axis=1).astype(np.float32)
    hper = np.geomspace(2.0, 100.0, 20).astype(np.float32)
    sed8 = synth.sediment_models(512, 12, seed=16, max_layers=8)
    full = lambda m: np.full(m.shape[0], m.shape[2], np.int32)
    return {"bench": (bench, full(bench), dper), "bench_mcmc_periods": (bench, full(bench), mper),
            "water": (wet, full(wet), dper), "sediment": (sed, full(sed), dper),
            "sediment_mcmc_periods": (sed, full(sed), mper), "ragged_3_20": (rag, nl, dper),
            "sediment_8_layers": (sed8, full(sed8), dper), "high_contrast": (hc, full(hc), hper)}


CASES = ["bench", "bench_mcmc_periods", "water", "sediment", "sediment_mcmc_periods", "ragged_3_20", "sediment_8_layers",
         "high_contrast"]


@pytest.mark.parametrize("case", CASES)
def test_split_u(libs, oracle, case):
    model, nlay, per = _cases()[case]
    model = np.ascontiguousarray(model, np.float32); nlay = np.ascontiguousarray(nlay); per = np.ascontiguousarray(per)
    c, uo, r = _oracle(oracle, model, nlay, per)
    un, hs, rn, can = _host(libs["new"], model, nlay, per, c, r)
    ur, hs_r, rr, can_r = _host(libs["ref"], model, nlay, per, c, r)
    assert (hs == hs_r).all()
    assert (rr[..., 0] == rr[..., 1]).all()                 # the B build steps the reference's split
    fast_n, fast_r = (rn[..., 0] >= 0).any(axis=2), (rr[..., 0] >= 0).any(axis=2)   # units on the fast path
    both = fast_n & fast_r
    assert (rn[both][..., 0] == rr[both][..., 0]).all()
    assert (fast_n != fast_r).mean() < 0.01                  # (the fit's cancellation decides the path: a few flip)
    ok = (uo != 0) & (ur != 0)
    assert ok.mean() > (0.25 if case == "high_contrast" else 0.9)
    if case == "high_contrast":                              # fast-path units where the fit's cancellation is large
        assert ((can_r > 1e5) & (can_r <= 1e7) & ok).sum() > 1000
        ok &= (np.abs(ur.astype(np.float64) / np.where(uo != 0, uo, 1) - 1) < U_ORACLE_BAR)   # (the rest is off already)
    d_split = np.abs(un[ok].astype(np.float64) / ur[ok] - 1)
    d_new = np.abs(un[ok].astype(np.float64) / uo[ok] - 1)
    d_ref = np.abs(ur[ok].astype(np.float64) / uo[ok] - 1)
    lay = rn[..., 0] > 0                                     # (unit, layer) the fast sweep stepped
    fewer = (rn[..., 1] < rn[..., 0])[lay].mean()
    ndiv = np.where(nlay > 1, np.minimum(5, 99 // np.maximum(nlay - 1, 1)), 1)
    unit_fewer = ((rn[..., 1] < ndiv[:, None, None]) & lay).any(axis=2)[hs >= 0].mean()
    steps = rn[..., 1][lay].sum() / rn[..., 0][lay].sum()
    wave = _wave_cost(hs, rn, 1) / _wave_cost(hs, rn, 0)
    print(f"{case}: {ok.sum()} units; U new vs ref split max {d_split.max():.2e} (bit-identical {np.mean(d_split == 0):.4f}); "
          f"vs oracle new {d_new.max():.2e} ref {d_ref.max():.2e}; layers with n' < nreg {fewer:.3f}, units with a layer "
          f"n' < ndiv {unit_fewer:.3f}; sublayers stepped {steps:.3f} of the reference's, wavefront max {wave:.3f}; "
          f"fast-path units above the cancellation bound {((can > 1e5) & (can <= 1e7)).sum()}")
    assert d_split.max() < U_SPLIT_BAR["sediment" if case.startswith("sediment") else "rock"]
    assert d_new.max() <= max(U_ORACLE_BAR, d_ref.max()) + U_SPLIT_BAR["rock"]
    if not case.startswith("sediment") and case != "high_contrast":
        assert d_new.max() < U_ORACLE_BAR
    assert wave <= (0.8 if case in ("bench", "water", "ragged_3_20") else 1.0)
    if case == "high_contrast":
        assert d_new.max() < U_ORACLE_BAR
