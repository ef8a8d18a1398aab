"""The least-squares step in parameter space (include/surfdisp.h section (6i)) on the host: the numpy statement
paramlsq.param_lsq_reference against the statement of the Vs step it is written on (linearized.lsq_step_reference) and against a direct
numpy.linalg.solve, and the argument errors of ParamLsqPlan / ParamLsqBatch and of the two C entries (refused before any launch: no
device is needed)."""
import ctypes

import numpy as np
import pytest

from lsq_cases import _problem
from pysurfinv_amd import _lib, linearized, paramlsq, settings
from pysurfinv_amd.layers_batch import Model1DBatch
from pysurfinv_amd.obsdata import DispersionData


@pytest.mark.parametrize("N,n,L", [(1, 1, 2), (7, 3, 5), (40, 14, 17), (100, 52, 64), (100, 64, 96), (12, 8, 9)])
def test_a_selection_jacobian_is_the_vs_step_without_smoothing(N, n, L):
    """jac[vs] a selection matrix of the free layers, the other jac rows zero, scale 1, no prior: the step of
    linearized.lsq_step_reference with alpha = 0, to 1e-12 relative."""
    G, r, w, x0, _, Q, lam = _problem(N, n, seed=100 + N + n)
    rng = np.random.default_rng(N)
    idx = np.sort(rng.choice(L, n, replace=False))
    Kb = rng.standard_normal((N, L)); Kb[:, idx] = G
    fixed = np.ones(L, bool); fixed[idx] = False
    Kb[:, np.nonzero(fixed)[0][::2]] = np.nan
    Kb[0, fixed] = np.nan                                                # a NaN kernel entry where jac is zero: skipped, not multiplied
    jac = np.zeros((4, L, n))
    jac[1, idx, np.arange(n)] = 1.0
    Ka, Kr, Kh = (rng.standard_normal((N, L)) for _ in range(3))          # multiplied by zero columns of jac: skipped
    Kh[:, 0] = np.nan
    ref = linearized.lsq_step_reference(G, r, w, x0, 0.0, Q, lam)
    got = paramlsq.param_lsq_reference(Kb, Ka, Kr, Kh, jac, r, w, lam, np.ones(n))
    assert got["flag"] == ref["flag"] == 0 and got["used"] == N and got["prior"] == 0.0
    assert np.array_equal(got["G"], G)
    assert np.abs(got["delta"] - ref["delta"]).max() <= 1e-12 * np.abs(ref["delta"]).max()
    for k in ("misfit", "predicted"):
        assert abs(got[k] - ref[k]) <= 1e-12 * abs(ref[k]), k
    res = linearized.lsq_resolution_reference(G, w, n, 0.0, Q, lam)
    assert np.abs(got["cov"] - res["cov"]).max() <= 1e-12 * np.abs(res["cov"]).max() and abs(got["logdet"] - res["logdet"]) <= 1e-12 * n


def test_prior_damping_and_predicted_objective_against_a_direct_solve():
    rng = np.random.default_rng(3)
    N, L, Nu = 30, 11, 6
    Kb, Ka, Kr, Kh = (rng.standard_normal((N, L)) for _ in range(4))
    jac = rng.standard_normal((4, L, Nu)) * (rng.random((4, L, Nu)) > 0.3)
    jac[:3, 0, :] = 0.0; Kb[:, 0] = np.nan                                # a water layer: NaN d/dVs meets zero jac entries
    Kb[4, 3] = np.nan                                                     # a row with a column that is not finite: dropped
    r, w = rng.standard_normal(N), rng.uniform(0.5, 2.0, N)
    sign = np.where(np.arange(N) % 5 == 0, -1.0, 1.0)
    scale, beta = rng.uniform(0.5, 2.0, Nu), rng.uniform(0.0, 3.0, Nu)
    ref_, p = rng.standard_normal(Nu), rng.standard_normal(Nu + 2)        # (two local constants behind the unknowns)
    free = np.array([1, 1, 0, 1, 1, 0], bool)
    lam, nlay = 0.7, 9
    got = paramlsq.param_lsq_reference(Kb, Ka, Kr, Kh, jac, r, w, lam, scale, beta, ref_, p, free, nlay, sign)
    # the same from the definitions
    Gf = np.zeros((N, Nu))
    for K, q, m in ((Kb, 1, nlay), (Ka, 0, nlay), (Kr, 2, nlay), (Kh, 3, nlay - 1)):
        for i in range(m):
            for j in range(Nu):
                if jac[q, i, j] != 0.0:
                    Gf[:, j] += K[:, i] * jac[q, i, j]
    Gf *= sign[:, None]
    keep = np.arange(N) != 4
    assert np.array_equal(got["kept"], keep) and got["used"] == N - 1
    G = Gf[keep][:, free]
    rk, wk = r[keep], w[keep]
    b, y = beta[free], (p[:Nu] - ref_)[free]
    A = G.T @ (wk[:, None] * G) + np.diag(lam / scale[free] ** 2 + b)
    d = np.linalg.solve(A, G.T @ (wk * rk) - b * y)
    assert got["flag"] == 0 and not got["delta"][~free].any()
    assert np.abs(got["delta"][free] - d).max() <= 1e-12 * np.abs(d).max()
    assert got["misfit"] == pytest.approx(float((wk * rk * rk).sum()), rel=1e-13)
    assert got["prior"] == pytest.approx(float((b * y * y).sum()), rel=1e-13)
    t = rk - G @ d
    assert got["predicted"] == pytest.approx(float((wk * t * t).sum() + (b * (y + d) ** 2).sum()), rel=1e-12)
    cov = np.linalg.inv(A)
    assert np.abs(got["cov"][np.ix_(free, free)] - cov).max() <= 1e-12 * np.abs(cov).max()
    assert not got["cov"][~free].any() and not got["cov"][:, ~free].any() and np.array_equal(got["cov"], got["cov"].T)
    assert np.allclose(got["sigma"][free], np.sqrt(np.diag(cov)), rtol=1e-12) and not got["sigma"][~free].any()
    assert got["logdet"] == pytest.approx(np.linalg.slogdet(A)[1], rel=1e-12)
    # no usable row: flag 1, zeros, the objective at p
    none = paramlsq.param_lsq_reference(Kb[:0], Ka[:0], Kr[:0], Kh[:0], jac, r[:0], w[:0], lam, scale, beta, ref_, p, free, nlay)
    assert none["flag"] == 1 and not none["delta"].any() and not none["cov"].any() and none["predicted"] == none["prior"] > 0
    # a matrix that is not positive definite (no rows cannot reach here; a negative damping does): flag 2, zeros
    bad = paramlsq.param_lsq_reference(Kb, Ka, Kr, Kh, jac, r, w, -1e9, scale, None, None, None, free, nlay, sign)
    assert bad["flag"] == 2 and not bad["delta"].any() and not bad["sigma"].any() and bad["logdet"] == 0.0


def _data(quantity="c", M=3):
    per = np.asarray(settings.MCMC_PERIODS, np.float64)
    v = np.tile(np.linspace(3.2, 4.0, per.size), (M, 1))
    return [DispersionData("R", quantity, per, v, 0.01 * v)]


def test_python_layers_refuse_bad_arguments_without_a_device():
    mb = Model1DBatch(settings.MCMC_SETTING, device="cpu")
    Nu = mb.spec.n
    ok = dict(model_batch=mb, datasets=_data())
    for kw, exc, match in ((dict(params0=np.zeros((3, Nu + 1))), ValueError, "params0"),
                           (dict(params0=np.tile(mb.spec.vmax, (3, 1))), ValueError, "strictly inside"),
                           (dict(free=np.ones(Nu + 1, bool)), ValueError, "free"),
                           (dict(free=np.zeros(Nu, bool)), ValueError, "no free parameter"),
                           (dict(scale=np.zeros(Nu)), ValueError, "scale > 0"),
                           (dict(prior_w=-1.0), ValueError, "prior_w >= 0"),
                           (dict(prior_ref=np.zeros(3)), ValueError, "prior_ref"),
                           (dict(lam0=0.0), ValueError, "lam0 > 0"),
                           (dict(nu=1.0), ValueError, "nu > 1"),
                           (dict(rules=object()), ValueError, "rules"),
                           (dict(datasets=_data("E")), ValueError, linearized.MODES_NEED_NO_ELLIPTICITY[:40]),
                           (dict(device="cpu"), _lib.SurfdispError, "HIP device")):
        with pytest.raises(exc, match=match):
            paramlsq.ParamLsqBatch(**{**ok, **kw})
    shared = [DispersionData("R", "c", settings.MCMC_PERIODS, np.linspace(3.2, 4.0, 19), np.full(19, 0.03))]
    with pytest.raises(ValueError, match="give params0"):
        paramlsq.ParamLsqBatch(mb, shared)
    with pytest.raises(ValueError, match="the library has no dchi/dh"):
        paramlsq.ParamLsqPlan(mb, 3, _data("E"), device="cpu")
    with pytest.raises(_lib.SurfdispError, match="HIP device"):
        paramlsq.ParamLsqPlan(mb, 3, _data(), device="cpu")
    hybrid = Model1DBatch(settings.C5_SETTING, device="cpu")
    with pytest.raises(ValueError, match="thermal"):
        paramlsq.ParamLsqPlan(hybrid, 3, _data(), device="cpu")
    import torch
    with pytest.raises(ValueError, match="thermal"):
        hybrid.jacobian(torch.zeros(2, hybrid.spec.n, dtype=torch.float64))
    with pytest.raises(_lib.SurfdispError, match="HIP device"):
        mb.jacobian(torch.zeros(2, Nu, dtype=torch.float64))               # a CPU tensor
    gauss = dict(settings.MCMC_SETTING, Crust=dict(settings.MCMC_SETTING["Crust"], Gauss=[0.1, 10.0, 3.0]))
    with pytest.raises(_lib.SurfdispError, match="static layer structure"):
        Model1DBatch(gauss, device="cpu").jacobian(torch.zeros(2, Nu, dtype=torch.float64))


def test_c_entries_refuse_bad_arguments_before_launching():
    """SURFDISP_ERR_INVALID with stand-in pointers that are never read: nothing is launched, so no device is needed."""
    L = _lib.lib()
    x = ctypes.c_void_p(64)                                               # a non-NULL stand-in
    jac_ok = dict(C=3, N=15, Nu=13, L=96, params=x, idesc=x, fdesc=x, layer=None, jac=x)
    jac_call = lambda **kw: (lambda a: L.surfdisp_params_jacobian_device(None, a["C"], a["N"], a["Nu"], a["L"], a["params"], a["idesc"],
                                                                         a["fdesc"], a["layer"], a["jac"]))({**jac_ok, **kw})
    for kw in (dict(C=0), dict(N=0), dict(Nu=0), dict(Nu=16), dict(Nu=65, N=70), dict(L=1), dict(L=201), dict(params=None), dict(idesc=None),
               dict(fdesc=None), dict(jac=None)):
        assert jac_call(**kw) == _lib.ERR_INVALID, kw
        assert b"surfdisp_params_jacobian_device" in L.surfdisp_last_error()

    ptrs = lambda n, on: (ctypes.c_void_p * n)(*[64 if k in on else None for k in range(n)])
    ok = dict(B=2, Lmax=96, nlay=None, Nu=13, jac=x, part=ptrs(15, (0, 1, 2)), part_h=ptrs(5, (0,)), pred=ptrs(5, (0,)),
              strides=(ctypes.c_long * 5)(19, 0, 0, 0, 0), nper=(ctypes.c_int * 2)(19, 0), N=19, cols=x, weights=x, obs=x, uncer=x, mask=x,
              obs_per_stack=1, free=None, free_per_stack=0, scale=x, prior_w=None, prior_ref=None, params=x, Np=13, lam=x, delta=x, stats=x,
              info=x, cov=None, sigma=None, logdet=None)
    order = list(ok)
    step_call = lambda **kw: L.surfdisp_lsq_step_params_device(None, *[{**ok, **kw}[k] for k in order])
    bad = [dict(B=0), dict(Lmax=0), dict(Lmax=201), dict(N=0), dict(N=801), dict(Nu=0), dict(Nu=65, Np=65), dict(Np=12), dict(prior_w=x)]
    bad += [{k: None} for k in ("jac", "part", "part_h", "pred", "strides", "nper", "cols", "weights", "obs", "uncer", "mask", "scale", "params",
                                "lam", "delta", "stats", "info")]
    bad += [dict(pred=ptrs(5, ())),                                        # no phase array at all
            dict(pred=ptrs(5, (1,))),                                      # a group array without the phase array of its solve
            dict(pred=ptrs(5, (0, 4)), strides=(ctypes.c_long * 5)(19, 0, 0, 0, 5)),   # chi with a stride below nper
            dict(nper=(ctypes.c_int * 2)(0, 0)), dict(nper=(ctypes.c_int * 2)(201, 0)), dict(strides=(ctypes.c_long * 5)(18, 0, 0, 0, 0)),
            dict(part=ptrs(15, (0, 6))),                                   # partials of a source without predictions
            dict(part_h=ptrs(5, (0, 2)))]                                  # ... and thickness kernels of one
    for kw in bad:
        assert step_call(**kw) == _lib.ERR_INVALID, kw
        assert b"surfdisp_lsq_step_params_device" in L.surfdisp_last_error()
