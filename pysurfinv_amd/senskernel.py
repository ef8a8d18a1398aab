"""Finite-difference sensitivity kernels: the batched counterpart of ``SensKernelPert``
(``/root/reference/senskernel.py:129-158``).

The reference calls ``fast_surf`` 2L(+L) times, one perturbed stack at a time: layer i's Vs (or Vp)
scaled by 0.999 and 1.001, ``kernel[:, i] = (v(1.001) - v(0.999)) / 0.2 / H[i]`` (``:147-150``).
Here the 2L perturbed stacks (plus the unperturbed one) are ONE batch through the HIP solver.

Differences from the reference, on purpose:
* ``wtype='L'``: the reference reads ``cr0`` even for Love (``senskernel.py:188-192``, SURVEY.md
  section 4 defect 7) so its Love kernels are ``None``; here Love uses the Love phase velocities.
* group-velocity kernels (``ytype='grv'``) come for free from the same batch.
* analytic Rayleigh ellipticity (H/V) kernels (``analytic_kernels(ellipticity=True)``, ``ytype='ell'``) differentiate the
  reference's own recursion (DLTAR4) at the root: dchi/dm = dchi/dm|_c + (dchi/dc) dc/dm, with dc/dm from the same recursion.
* analytic group-velocity kernels (``analytic_kernels(group=True)``, ``SensKernel``) follow the toolkit's construction
  (GRV_SENS_KERNEL.f:99-108: phase partials at T x 0.99 and T x 1.01, their mean and central difference), but with the
  derived sign for all three columns: the toolkit's ``dudrho`` (GRV_SENS_KERNEL.f:107) adds the frequency term where
  ``dudb`` / ``duda`` (lines 106, 108) subtract it, and central differences of U itself side with the subtraction.
"""
from __future__ import annotations

import numpy as np

from . import forward as _forward

GROUP_RULES = {            # sensModel._convert, senskernel.py:104-124
    "water": lambda vs: (np.full_like(vs, 1.475), np.full_like(vs, 1.027), np.full_like(vs, 10000.)),
    "sediment": lambda vs: (vs * 1.23 + 1.28, 0.541 + 0.3601 * (vs * 1.23 + 1.28), np.full_like(vs, 80.)),
    "crust": lambda vs: (vs * 1.8, 0.541 + 0.3601 * (vs * 1.8), np.full_like(vs, 350.)),
    "mantle": lambda vs: (vs * 1.76, 3.4268 + (vs - 4.5) / 4.5, np.full_like(vs, 150.)),
}


def _derive(vs, grp):
    vp, rho, qs = np.zeros_like(vs), np.zeros_like(vs), np.zeros_like(vs)
    for g in set(grp):
        I = np.array([x == g for x in grp])
        vp[I], rho[I], qs[I] = GROUP_RULES[g](vs[I])
    return vp, rho, qs


def perturbed_batch(H, Vs, Vp=None, Rho=None, Qs=None, Grp=None, xtype="Vs", lo=0.999, hi=1.001):
    """model float32 [1+2L', 5, L'] : row 0 unperturbed, rows 1..L' layer i x lo, then x hi
    (layers with h <= 1e-3 dropped as ``_forward`` does, senskernel.py:182-183)."""
    H, Vs = np.asarray(H, float), np.asarray(Vs, float)
    L = H.size
    stacks = []
    for scale, i in [(1.0, -1)] + [(lo, i) for i in range(L)] + [(hi, i) for i in range(L)]:
        vs = Vs.copy()
        vp = None if Vp is None else np.asarray(Vp, float).copy()
        if i >= 0:
            if xtype == "Vs":
                vs[i] *= scale
            elif xtype == "Vp":
                if vp is None:
                    raise ValueError("xtype='Vp' needs an explicit Vp column (senskernel.py:152)")
                vp[i] *= scale
            else:
                raise ValueError(xtype)
        if vp is None or Rho is None or Qs is None:
            dvp, drho, dqs = _derive(vs, Grp)
        vp_ = vp if vp is not None else dvp
        rho_ = np.asarray(Rho, float) if Rho is not None else drho
        qs_ = np.asarray(Qs, float) if Qs is not None else dqs
        keep = H > 1e-3
        stacks.append(np.stack([vp_[keep], vs[keep], rho_[keep], H[keep], 1.0 / qs_[keep]]))
    return np.stack(stacks).astype(np.float32), np.nonzero(H > 1e-3)[0]


def sens_kernel_pert(H, Vs, Vp=None, Rho=None, Qs=None, Grp=None, periods=range(20, 101, 10),
                     wtype="R", xtype="Vs", device=0, ellipticity=False):
    """dict(phv=[P, L], grv=[P, L], c0=[P], u0=[P]); NaN columns where a perturbed solve failed.
    ``ellipticity=True`` (Rayleigh): the batch is solved on the device with the ellipticity (``BatchPlan.run(want_ratio=True)``)
    and ell=[P, L] holds the same differences of chi."""
    kind = {"R": 2, "L": 1}[wtype]
    if ellipticity and kind != 2:
        raise ValueError("ellipticity kernels are Rayleigh only (wtype='R')")
    model, kept = perturbed_batch(H, Vs, Vp, Rho, Qs, Grp, xtype)
    per = np.asarray(list(periods), np.float32)
    curves = []
    if ellipticity:
        import torch
        dev = torch.device(f"cuda:{device}")
        plan = _forward.BatchPlan(model.shape[0], model.shape[2], per.size, device=dev)
        c, u, st, ratio = plan.run(torch.from_numpy(model).to(dev), torch.from_numpy(per).to(dev), kind=kind, want_ratio=True)
        c, u, st, ratio = (t.cpu().numpy() for t in (c, u, st, ratio))
        curves = [("ell", ratio)]
    else:
        c, u, st = _forward.forward_batch(model, per, kind=kind, device=device)
    Lk = kept.size
    Hk = np.asarray(H, float)[kept]
    out = {}
    for name, v in [("phv", c), ("grv", u)] + curves:
        vL, vH = v[1:1 + Lk].astype(np.float64), v[1 + Lk:1 + 2 * Lk].astype(np.float64)
        k = (vH - vL) / 0.2 / Hk[:, None]                      # senskernel.py:150
        bad = (st[1:1 + Lk] != 0) | (st[1 + Lk:] != 0)
        k[bad] = np.nan
        full = np.zeros((per.size, np.asarray(H).size))
        full[:, kept] = k.T
        out[name] = full
    out["c0"], out["u0"], out["status"] = c[0], u[0], st
    return out


def sens_kernel_pert_batch(model, periods, wtype="R", nlay=None, lo=0.999, hi=1.001, chunk=256):
    """Finite-difference Vs kernels of MANY stacks on the device (BASELINE configs[4]: "senskernel
    sensitivity evaluation" of every model of a batch).

    model: torch float32 [M, 5, L] rows (vp, vs, rho, h, 1/Qs) on a HIP device - explicit columns,
    so only Vs is scaled (``_perturb`` with explicit Vp/Rho/Qs columns, senskernel.py:160-166);
    periods: torch float32 [P] ascending.  Each stack contributes its unperturbed solve and 2L
    perturbed ones, ``chunk`` stacks (= chunk*(2L+1) solves) per launch.
    Returns dict(phv, grv: float32 [M, P, L] = (v(hi) - v(lo)) / 0.2 / h_i (senskernel.py:150), NaN
    where a perturbed solve failed; c0, u0: [M, P]; status [M])."""
    import torch
    kind = {"R": 2, "L": 1}[wtype]
    M, _, L = model.shape
    P = periods.numel()
    dev = model.device
    # scale[j, i]: factor on layer i of variant j (0: none, 1..L: lo, L+1..2L: hi)
    scale = torch.ones((2 * L + 1, L), dtype=torch.float32, device=dev)
    ar = torch.arange(L, device=dev)
    scale[1 + ar, ar] = lo
    scale[1 + L + ar, ar] = hi
    out = {k: torch.empty((M, P, L), dtype=torch.float32, device=dev) for k in ("phv", "grv")}
    out["c0"] = torch.empty((M, P), dtype=torch.float32, device=dev)
    out["u0"] = torch.empty((M, P), dtype=torch.float32, device=dev)
    out["status"] = torch.empty(M, dtype=torch.int32, device=dev)
    V = 2 * L + 1
    plan = None
    for a in range(0, M, chunk):
        m = model[a:a + chunk]
        n = m.shape[0]
        big = m[:, None].expand(n, V, 5, L).clone()
        big[:, :, 1, :] *= scale[None]
        nl = None if nlay is None else nlay[a:a + chunk].repeat_interleave(V)
        if plan is None or plan.B != n * V:
            plan = _forward.BatchPlan(n * V, L, P, device=dev)
        c, u, st = plan.run(big.reshape(n * V, 5, L), periods, kind=kind, nlay=nl)
        c, u, st = c.view(n, V, P), u.view(n, V, P), st.view(n, V)
        bad = ((st[:, 1:1 + L] != 0) | (st[:, 1 + L:] != 0))[:, None, :]           # [n, 1, L]
        h = m[:, 3, :][:, None, :]
        for name, v in (("phv", c), ("grv", u)):
            k = (v[:, 1 + L:] - v[:, 1:1 + L]).transpose(1, 2) / 0.2 / h         # [n, P, L]
            out[name][a:a + n] = torch.where(bad | (h <= 0), torch.full_like(k, float("nan")), k)
        out["c0"][a:a + n], out["u0"][a:a + n], out["status"][a:a + n] = c[:, 0], u[:, 0], st[:, 0]
    return out


def group_from_phase_partials(c, u, k_minus, k_plus, dlnT):
    """The combination rule of the group-velocity kernels in float64 (the host statement of what the HIP combine kernel
    computes): differentiating U = d omega / dk at fixed omega (Rodi et al. 1975),

        dU/dm = (U/c) (2 - U/c) dc/dm - (U/c)^2 d(dc/dm)/d ln T,

    with dc/dm the mean of the phase partials ``k_minus`` / ``k_plus`` at T (1 - d) and T (1 + d) and the derivative their
    central difference over ``dlnT`` = ln((1 + d) / (1 - d)).  c, u broadcast against the partials (e.g. [P, 1] against
    [P, L])."""
    c = np.asarray(c, np.float64)
    u = np.asarray(u, np.float64)
    km = np.asarray(k_minus, np.float64)
    kp = np.asarray(k_plus, np.float64)
    r = u / c
    return r * (2.0 - r) * 0.5 * (km + kp) - r * r * (kp - km) / float(dlnT)


def group_thickness_reference(c, u, h_minus, h_plus, dlnT):
    """dU/dh (or dU/dz) in float64 from the thickness rows ``h_minus`` / ``h_plus`` of the phase velocity (dcdh or dcdz of
    ``thickness_kernels_reference`` / ``run_thickness_kernels``) at T (1 - d) and T (1 + d): Rodi's rule holds for any model
    parameter, so this is ``group_from_phase_partials`` on those rows - the host statement of what
    ``surfdisp_forward_group_thickness_kernels_device`` combines (include/surfdisp.h section (5h)).  c, u: the unit's own values
    at T, broadcast against the rows; ``dlnT`` = ln((1 + d) / (1 - d))."""
    return group_from_phase_partials(c, u, h_minus, h_plus, dlnT)


def attenuation_from_kernels(model, periods, c, u, kb, ka=None):
    """Apparent attenuation of the mode from its phase-velocity kernels, in float64 (the host statement of what the HIP
    attenuation kernel computes; the reference forms the same numbers after REIGEN / LEIGEN, calcul.f:256-265, 341-349,
    and never returns them).  With W_i = b_i (dc/db_i + 4/3 (b_i/a_i) dc/da_i) in the reference's coordinates
    (surfa.f:1207 ``dwx``; Love: b_i dc/db_i), rewritten for the caller-coordinate kernels ``kb`` = dc/dVs and ``ka`` =
    dc/dVp (``None``: Love) - the flattening factor cancels, qsq = qsinv ln(1/T)/pi, qpq = qsq (4/3) Vs^2/Vp^2:

        W_i = Vs kb - Vs ka (8/3) qsq (Vs/Vp) / (1 - qpq) + (4/3) ka Vs^2 (1 + qsq)^2 / (Vp (1 + qpq)(1 - qpq)),

        dqdq_i = W_i U / c^2,   qinv = sum_i dqdq_i qsinv_i  (= 1/Q_apparent),   gamma = pi qinv / (U T)  (1/km).

    model [B, 5, L] (vp, vs, rho, h, 1/Qs) or [5, L]; periods [P]; c, u [B, P]; kb, ka [B, P, L].  Returns (qinv [B, P],
    gamma [B, P], dqdq [B, P, L]); zeros at unsolved periods (c or U not > 0), water layers (Vs <= 0) and wherever the
    kernels are zero (layers below the effective half space)."""
    m = np.asarray(model, np.float64)
    m = m[None] if m.ndim == 2 else m
    T = np.asarray(periods, np.float64).ravel()
    c = np.asarray(c, np.float64).reshape(m.shape[0], T.size)
    u = np.asarray(u, np.float64).reshape(m.shape[0], T.size)
    kb = np.asarray(kb, np.float64).reshape(m.shape[0], T.size, m.shape[2])
    vp, vs, qs = m[:, 0, None, :], m[:, 1, None, :], m[:, 4, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):            # (a non-finite stack gives zeros: its c is 0)
        solid = (vs > 0) & (vp > 0)
        vs = np.where(solid, vs, 0.0)
        vp = np.where(solid, vp, 1.0)
        W = vs * kb
        if ka is not None:
            ka = np.asarray(ka, np.float64).reshape(kb.shape)
            qsq = qs * np.log(1.0 / T)[None, :, None] / np.pi
            qpq = qsq * (4.0 / 3.0) * vs * vs / (vp * vp)
            W = (W - vs * ka * (8.0 / 3.0) * qsq * (vs / vp) / (1.0 - qpq)
                 + (4.0 / 3.0) * ka * vs * vs * (1.0 + qsq) ** 2 / (vp * (1.0 + qpq) * (1.0 - qpq)))
        ok = (c > 0) & (u > 0)
        uc2 = np.where(ok, u / np.where(ok, c * c, 1.0), 0.0)
        dqdq = np.where(solid & ok[:, :, None] & (W != 0), W * uc2[:, :, None], 0.0)
        qinv = np.where(dqdq != 0, dqdq * qs, 0.0).sum(axis=2)
        gamma = np.where(ok, np.pi * qinv / np.where(ok, u * T[None, :], 1.0), 0.0)
    return qinv, gamma, dqdq


_R0 = 6371.0
_TWOPI32 = float(np.float32(6.2831853072))          # the wavenumber's constant as the solver holds it (surfa.f:871, 874)


def flattened_layers(model, period, wtype="R", nlay=None):
    """The earth-flattened, attenuation-corrected values of every layer of ONE stack at ``period``, float64, from the
    library's documented formulas (flat1.f:44-68; calcul.f:122-126) on the fp32 inputs: dict(a, b, rho, d) [L] in the
    regular role - layer i between r_i = R0 - sum_{j<i} h_j and r_n = r_i - h_i:

        dif = (1/r_n - 1/r_i) R0 / ln(r_i/r_n),  qqq = (r_i^p - r_n^p) / (ln(r_i/r_n) R0^p p),  d = R0 ln(r_i / r_n),
        qsq = qsinv ln(1/T) / pi,  b = Vs (1 + qsq) dif,  a = Vp (1 + qsq (4/3) Vs^2 / Vp^2) dif,  rho = rho qqq,

    p = 2.275 (Rayleigh) | 5 (Love), R0 = 6371; the last layer (index nlay - 1, the half space) has d = 0 and the factors
    R0 / r_i and (r_i / R0)^p.  model [5, L] (vp, vs, rho, h, 1/Qs)."""
    m = np.asarray(model, np.float32).astype(np.float64)
    L = m.shape[1]
    n = L if nlay is None else int(nlay)
    p = float(np.float32(5.0 if wtype == "L" else 2.275))
    vp, vs, rho, h, qs = m
    bot = np.cumsum(h)
    r_i, r_n = _R0 - (bot - h), _R0 - bot
    idx = np.arange(L)
    with np.errstate(all="ignore"):
        fltd = np.log(r_i / r_n)
        dif = np.where(idx < n - 1, (1.0 / r_n - 1.0 / r_i) * _R0 / fltd, _R0 / r_i)
        qqq = np.where(idx < n - 1, (r_i ** p - r_n ** p) / (fltd * _R0 ** p * p), (r_i / _R0) ** p)
        d = np.where(idx < n - 1, _R0 * fltd, 0.0)
        qsq = qs * np.log(1.0 / float(np.float32(period))) / np.pi
        qpq = qsq * (4.0 / 3.0) * vs * vs / (vp * vp)
    live = idx < n
    z = np.zeros(L)
    return dict(a=np.where(live, vp * (1.0 + qpq) * dif, z), b=np.where(live, vs * (1.0 + qsq) * dif, z),
                rho=np.where(live, rho * qqq, z), d=np.where(live, d, z))


def _expm(A):
    """exp(A) of a small real matrix: scaling and squaring around a Taylor series, float64."""
    A = np.asarray(A, np.float64)
    nrm = np.abs(A).sum(axis=1).max()
    s = max(0, int(np.ceil(np.log2(max(nrm, 1e-300)))) + 2)
    X = A / (2.0 ** s)
    E = np.eye(A.shape[0]); term = np.eye(A.shape[0])
    for k in range(1, 25):
        term = term @ X / k
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


def eigen_layer_matrix(lay, i, period, c, wtype="R", frac=1.0, rk4_steps=0, fp32_inputs=True):
    """The exact propagator of layer ``i`` of ``flattened_layers``' dict ``lay``: the matrix that carries the
    displacement-stress vector of the mode with phase velocity ``c`` at ``period`` UPWARD through ``frac`` of the layer's
    (flattened) thickness H, exp(-frac H A), float64.  Rayleigh, v = (ur, uz, tz, tr), the system REIGEN integrates
    (surfa.f:933-940, 960-963; k = omega / c):

        ur' = -k uz + tr / mu,   uz' = k lam ur / (lam + 2 mu) + tz / (lam + 2 mu),
        tz' = -omega^2 rho uz + k tr,   tr' = (4 k^2 mu (lam + mu) / (lam + 2 mu) - omega^2 rho) ur - k lam tz / (lam + 2 mu);

    Love, v = (ut, tq) (surfa.f:549-550):  ut' = tq / mu,  tq' = (k^2 mu - omega^2 rho) ut.

    ``rk4_steps`` > 0: not the exact map but the one REIGEN itself applies over that distance - that many classical
    Runge-Kutta steps (surfa.f:955-968: the polynomial I + X + X^2/2 + X^3/6 + X^4/24 of X = -h A per step).
    ``fp32_inputs=False``: ``period`` and ``c`` are not rounded to the solver's float32 first."""
    a, b, rho, H = (float(lay[k][i]) for k in ("a", "b", "rho", "d"))
    if not fp32_inputs:                                # (float64 checkers: period and c as they are given)
        om = _TWOPI32 / float(period)
        k = om / float(c)
    else:
        om = _TWOPI32 / float(np.float32(period))
        k = _TWOPI32 / (float(np.float32(c)) * float(np.float32(period)))
    mu = rho * b * b
    if wtype == "L":
        A = np.array([[0.0, 1.0 / mu], [k * k * mu - om * om * rho, 0.0]])
    else:
        lam = rho * (a * a - 2.0 * b * b)
        a12 = 1.0 / (lam + 2.0 * mu)
        a13 = k * lam * a12
        a21 = -om * om * rho
        a43 = a21 + 4.0 * k * k * mu * (lam + mu) * a12
        A = np.array([[0.0, -k, 0.0, 1.0 / mu], [a13, 0.0, a12, 0.0], [0.0, a21, 0.0, k], [a43, 0.0, -a13, 0.0]])
    if rk4_steps:
        X = -float(frac) * H / int(rk4_steps) * A
        I = np.eye(A.shape[0])
        return np.linalg.matrix_power(I + X @ (I + X @ (I + X @ (I + X / 4.0) / 3.0) / 2.0), int(rk4_steps))
    return _expm(-float(frac) * H * A)


def eigen_layer_propagate(model, period, c, layer, v, wtype="R", nlay=None, frac=1.0):
    """Carry the displacement-stress vector ``v`` ((ur, uz, tz, tr); Love (ut, tq)) given at a depth inside or at the bottom
    of input layer ``layer`` upward through ``frac`` of that layer's thickness, with the exact propagator of the
    earth-flattened, attenuation-corrected layer (``flattened_layers``, ``eigen_layer_matrix``), in float64: with
    ``frac=1`` from the top of layer ``layer + 1`` to the top of layer ``layer`` - what relates consecutive entries of
    ``eigenfunctions``.  Returns the vector at the upper depth."""
    lay = flattened_layers(model, period, wtype, nlay)
    return eigen_layer_matrix(lay, int(layer), period, c, wtype, frac) @ np.asarray(v, np.float64)


def interface_energy(v, a, b, rho, k, omega, wtype="R", liquid=False):
    """E(v; m): the Hamiltonian of the depth ODE of ``eigen_layer_matrix`` for the displacement-stress vector ``v`` ((ur, uz,
    tz, tr); Love (ut, tq)) in the material (a, b, rho) - constant through a homogeneous layer; its jump across an
    interface is that interface's depth kernel (``thickness_kernels_reference``).  lam = rho (a^2 - 2 b^2), mu = rho b^2.

        Love:      E = rho omega^2 ut^2 - mu k^2 ut^2 + tq^2 / mu
        Rayleigh:  uz' = (tz + k lam ur) / (lam + 2 mu),  ur' = tr / mu - k uz,
                   W2 = lam (uz' - k ur)^2 + 2 mu (k^2 ur^2 + uz'^2) + mu (ur' + k uz)^2,
                   E = rho omega^2 (ur^2 + uz^2) - W2 + 2 tr ur' + 2 tz uz'
        ``liquid`` (the water layer above the sea floor, lam = rho a^2; of v only uz and tz are read):
                   urw = -k tz / (rho omega^2),  uz' = tz / lam + k urw,
                   E = rho omega^2 (urw^2 + uz^2) - tz^2 / lam + 2 tz uz';      Love: E = 0 (the sea floor is its free surface)."""
    a, b, rho, k, om2 = float(a), float(b), float(rho), float(k), float(omega) ** 2
    v = np.asarray(v, np.float64)
    if wtype == "L":
        if liquid:
            return 0.0
        mu = rho * b * b
        return rho * om2 * v[0] ** 2 - mu * k * k * v[0] ** 2 + v[1] ** 2 / mu
    ur, uz, tz, tr = v
    if liquid:
        lam = rho * a * a
        urw = -k * tz / (rho * om2)
        duz = tz / lam + k * urw
        return rho * om2 * (urw * urw + uz * uz) - tz * tz / lam + 2.0 * tz * duz
    mu = rho * b * b
    lam = rho * (a * a - 2.0 * b * b)
    duz = (tz + k * lam * ur) / (lam + 2.0 * mu)
    dur = tr / mu - k * uz
    w2 = lam * (duz - k * ur) ** 2 + 2.0 * mu * (k * k * ur * ur + duz * duz) + mu * (dur + k * uz) ** 2
    return rho * om2 * (ur * ur + uz * uz) - w2 + 2.0 * tr * dur + 2.0 * tz * duz


def thickness_kernels_reference(layers, model, period, c, u, I0, v_tops, dcdb, dcda, dcdr, wtype, nlay=None, hs=None):
    """The derivatives of the phase velocity of ONE (stack, period) unit with respect to the layer thicknesses and the
    interface depths, in numpy float64: the host statement of what ``surfdisp_forward_thickness_kernels_device`` computes
    (include/surfdisp.h section (5g)).  ``layers``: the dict of ``flattened_layers`` (the values the mode was computed on;
    the layer used as half space in that role); ``model`` [5, L]; ``c``, ``u`` (the structural group velocity), ``I0`` and
    ``v_tops`` [4 | 2][L] (the vector at the top of every layer, section (5f)) as ``eigenfunctions`` returns them; ``dcdb``,
    ``dcda`` (``None``: Love), ``dcdr`` [L] the unit's rows of ``analytic_kernels``.  ``hs``: the unit's effective half space
    (default: the deepest layer with a non-zero entry in v_tops, dcdb or dcdr).

        K_j = -amp (c^3 / omega^2) [E(v_j; j-1) - E(v_j; j)],  amp = 1 / (2 c U I0),  1 <= j <= hs

    (``interface_energy``; the layer above a sea floor in its liquid form) is dc / d(flattened depth of interface j).  In the
    caller's coordinates (flat1.f; r_j = R0 - sum_{m<j} h_m, rt / rb the top / bottom radius of a layer, x = ln(rt/rb),
    p = 2.275 | 5, Sv_m = Vs dcdb + Vp dcda, Sr_m = rho dcdr):

        d ln dif/d rt =  1 / (rt^2 (1/rb - 1/rt)) - 1/(x rt),      d ln dif/d rb = -1 / (rb^2 (1/rb - 1/rt)) + 1/(x rb),
        d ln qqq/d rt =  p rt^(p-1) / (rt^p - rb^p) - 1/(x rt),    d ln qqq/d rb = -p rb^(p-1) / (rt^p - rb^p) + 1/(x rb),
        (half-space role, layer nlay - 1: d ln dif/d rt = -1/rt, d ln qqq/d rt = p/rt)
        dcdz_j = K_j R0 / r_j - [Sv_{j-1} d ln dif_{j-1}/d rb + Sr_{j-1} d ln qqq_{j-1}/d rb]
                              - [Sv_j d ln dif_j/d rt + Sr_j d ln qqq_j/d rt],
        dcdh_i = sum_{j>i} dcdz_j.

    Returns (dcdh [L], dcdz [L], K [L]); K alone is the result for a flat stack.  A water layer's own flattening-factor term
    is left out (the rows of a liquid layer are not read), and so is the dependence of the layer dropping on the thicknesses."""
    m = np.asarray(model, np.float64)
    L = m.shape[1]
    n = L if nlay is None else int(nlay)
    vt = np.asarray(v_tops, np.float64)
    kb = np.asarray(dcdb, np.float64).ravel()
    kr = np.asarray(dcdr, np.float64).ravel()
    ka = np.zeros(L) if dcda is None else np.asarray(dcda, np.float64).ravel()
    if hs is None:
        nz = np.flatnonzero((vt != 0).any(axis=0) | (kb != 0) | (kr != 0))
        hs = int(nz.max()) if nz.size else -1
    hs = min(int(hs), n - 1)
    dcdh, dcdz, K = np.zeros(L), np.zeros(L), np.zeros(L)
    c, u, I0, T = float(c), float(u), float(I0), float(period)
    if hs < 1 or not (c > 0):
        return dcdh, dcdz, K
    om = _TWOPI32 / T
    k = om / c
    fac = -(1.0 / (2.0 * c * u * I0)) * c ** 3 / (om * om)
    p = float(np.float32(5.0 if wtype == "L" else 2.275))
    vp, vs, rho, h = m[0], m[1], m[2], m[3]
    wet = not (vs[0] > 0)
    r = _R0 - np.concatenate([[0.0], np.cumsum(h)[:-1]])
    solid = vs > 0                                          # (a water layer's own factor term is left out)
    Sv = np.where(solid, vs * kb + vp * ka, 0.0)
    Sr = np.where(solid, rho * kr, 0.0)
    mat = lambda i: (layers["a"][i], layers["b"][i], layers["rho"][i])
    for j in range(1, hs + 1):
        v = vt[:, j]
        K[j] = fac * (interface_energy(v, *mat(j - 1), k, om, wtype, liquid=(wet and j == 1)) - interface_energy(v, *mat(j), k, om, wtype))
        # the layer above, regular role: its bottom radius moves
        rt, rb = r[j - 1], r[j]
        chain = 0.0
        if h[j - 1] > 0:                                    # (a layer without thickness holds no energy: no share)
            x = np.log(rt / rb)
            dif_rb = -1.0 / (rb * rb * (1.0 / rb - 1.0 / rt)) + 1.0 / (x * rb)
            qqq_rb = -p * rb ** (p - 1.0) / (rt ** p - rb ** p) + 1.0 / (x * rb)
            chain = Sv[j - 1] * dif_rb + Sr[j - 1] * qqq_rb
        # the layer below: its top radius moves
        rt = r[j]
        if j == n - 1:
            dif_rt, qqq_rt = -1.0 / rt, p / rt
        elif not h[j] > 0:
            dif_rt = qqq_rt = 0.0
        else:
            rb = r[j + 1]
            x = np.log(rt / rb)
            dif_rt = 1.0 / (rt * rt * (1.0 / rb - 1.0 / rt)) - 1.0 / (x * rt)
            qqq_rt = p * rt ** (p - 1.0) / (rt ** p - rb ** p) - 1.0 / (x * rt)
        chain += Sv[j] * dif_rt + Sr[j] * qqq_rt
        dcdz[j] = K[j] * _R0 / r[j] - chain
    dcdh[:-1] = np.cumsum(dcdz[::-1])[::-1][1:]
    return dcdh, dcdz, K


def eigenfunctions(model, periods, wtype="R", nlay=None):
    """The mode's eigenfunction at the top of every input layer and its energy integrals, for a whole batch, from ONE
    forward solve (``surfdisp_forward_eigen_device``): what REIGEN / LEIGEN leave in COMMON /rar/, /rco1/ and /rco/ and
    the reference never returns.  model: torch float32 [M, 5, L] on a HIP device; periods float32 [P].  Returns a dict:
    c, u [M, P]; status [M]; Rayleigh ur, uz, tz, tr [M, P, L] (horizontal / vertical displacement, normal / shear traction,
    uz = 1 at the top of the first solid layer), Love ut, tt (transverse displacement, shear traction, ut = 1 there);
    I0, I1, I2, amp [M, P] (the energy integrals U is formed from and the amplification factor 1 / (2 c U I0));
    ztop [M, L] the cumulative depth of every layer's top.  Values are those of the earth-flattened, attenuation-corrected
    stack at the period; zeros below a unit's effective half space, for unsolved periods and bad stacks."""
    kind = {"R": 2, "L": 1}[wtype]
    M, _, L = model.shape
    plan = _forward.BatchPlan(M, L, periods.numel(), device=model.device)
    c, u, st, ur, uz, tz, tr, en = plan.run_eigen(model, periods, kind=kind, nlay=nlay,
                                                  want_uz=(kind == 2), want_tz=(kind == 2))
    return _eigen_dict(model, kind, c, u, st, ur, uz, tz, tr, en)


def _eigen_dict(model, kind, c, u, st, ur, uz, tz, tr, en):
    import torch
    h = model[:, 3, :]
    out = dict(c=c, u=u, status=st, I0=en[..., 0], I1=en[..., 1], I2=en[..., 2], amp=en[..., 3],
               ztop=torch.cumsum(h, dim=1) - h)
    if kind == 2:
        out.update(ur=ur, uz=uz, tz=tz, tr=tr)
    else:
        out.update(ut=ur, tt=tr)
    return out


def _per_km(model, k):
    """A row of partials in the reference's ``SensKernelPert`` units: k * Vs / 100 / h (zeros where a layer has no thickness)."""
    import torch
    h = model[:, 3, :][:, None, :]
    vs = model[:, 1, :][:, None, :]
    return torch.where(h > 0, k * vs / 100.0 / torch.where(h > 0, h, torch.ones_like(h)), torch.zeros_like(k))


def group_thickness_kernels(model, periods, wtype="R", nlay=None, want_vp=True, want_rho=True, dlnT_frac=0.01):
    """``analytic_kernels(group=True)`` and ``analytic_kernels(thickness=True)`` from ONE forward solve, and the derivatives of
    the GROUP velocity with respect to the layer thicknesses and the interface depths on top of them
    (``surfdisp_forward_group_thickness_kernels_device``, both wave types).  Returns the keys of both calls with the same
    numbers - dcdb, dcda, dcdr, c0, u0, status, phv, dudb, duda, dudr, grv, dcdh, dcdz - plus dudh [M, P, L] = d U / d (thickness
    of layer i), everything below shifted rigidly, dudz [M, P, L] = d U / d (depth of the top of layer j) alone, n_failed
    (units whose shifted root failed: NaN rows in dudb .. dudz) and n_nonfinite (units whose thickness rows are not finite:
    NaN rows in dudh, dudz); see ``group_thickness_reference``.  A function of its own: ``analytic_kernels`` refuses
    ``thickness=True`` together with ``group=True`` (each of its flags names one entry of the library;
    tests/test_thickness_host.py pins the refusal)."""
    kind = {"R": 2, "L": 1}[wtype]
    M, _, L = model.shape
    plan = _forward.BatchPlan(M, L, periods.numel(), device=model.device)
    c, u, st, kb, ka, kr, ub, ua, ur, kh, kz, uh, uz, nf, nnf = plan.run_group_thickness_kernels(
        model, periods, kind=kind, nlay=nlay, dlnT_frac=dlnT_frac, want_vp=want_vp, want_rho=want_rho)
    return dict(dcdb=kb, dcda=ka, dcdr=kr, c0=c, u0=u, status=st, phv=_per_km(model, kb), dudb=ub, duda=ua, dudr=ur,
                grv=_per_km(model, ub), dcdh=kh, dcdz=kz, dudh=uh, dudz=uz, n_failed=nf, n_nonfinite=nnf)


def analytic_kernels(model, periods, wtype="R", nlay=None, want_vp=True, want_rho=True, group=False, dlnT_frac=0.01,
                     ellipticity=False, attenuation=False, eigen=False, thickness=False):
    """Sensitivity kernels of a whole batch from ONE forward solve (``surfdisp_forward_kernels_device``):
    the partial derivatives REIGEN / LEIGEN form from their energy integrals and never return
    (surfa.f:1130-1135, 1204-1207; 561-565, 584-585), with the chain factors of the attenuation
    correction and the earth flattening applied so that they refer to the caller's layer values.

    model: torch float32 [M, 5, L] (vp, vs, rho, h, 1/Qs) on a HIP device; periods float32 [P].
    Returns dict(dcdb, dcda, dcdr: float32 [M, P, L] = d c / d (Vs | Vp | rho) per layer (dcda only for
    Rayleigh); c0, u0 [M, P]; status [M]; phv = dcdb * Vs / 100 / h, the reference's ``SensKernelPert``
    units ((v(1.001 Vs) - v(0.999 Vs)) / 0.2 / H, senskernel.py:150)).
    ``group=True`` (``surfdisp_forward_group_kernels_device``): also dudb, duda, dudr [M, P, L] = d U / d (Vs | Vp | rho)
    from the phase partials at T (1 -+ dlnT_frac) (see ``group_from_phase_partials``; NaN rows where a shifted root
    failed), grv = dudb * Vs / 100 / h in phv's units, and n_failed.
    ``ellipticity=True`` (``surfdisp_forward_ellip_kernels_device``, Rayleigh only): also ratio [M, P] (the ellipticity chi),
    dedb, deda, dedr [M, P, L] = d chi / d (Vs | Vp | rho), ell = dedb * Vs / 100 / h in phv's units, and n_nonfinite (units
    whose rows are NaN).  It is one entry of its own: combined with ``group=True`` it is refused (call twice).
    ``attenuation=True`` (``surfdisp_forward_atten_device``, both wave types): also qinv [M, P] = 1 / Q_apparent of the mode
    (0 for a stack without attenuation and at unsolved periods), gamma [M, P] its attenuation coefficient in 1/km, dqdq
    [M, P, L] = d qinv / d (1/Qs of layer i) at fixed eigenfunction (qinv = sum_i dqdq_i qsinv_i, see
    ``attenuation_from_kernels``) and Qapp = 1 / qinv (inf where qinv is 0).  One entry of its own as well: refused
    together with ``group=True`` or ``ellipticity=True``.
    ``thickness=True`` (``surfdisp_forward_thickness_kernels_device``, both wave types): also dcdh [M, P, L] = d c / d (thickness
    of layer i), everything below shifted rigidly (what a change of ``model[:, 3, i]`` does), dcdz [M, P, L] = d c / d (depth of
    the top of layer j) with the other interfaces fixed, and n_nonfinite (units whose rows are NaN); see
    ``thickness_kernels_reference``.  One entry of its own as well: refused together with ``group=True``, ``ellipticity=True``
    or ``attenuation=True``; ``group_thickness_kernels`` is the call that returns the rows of group and thickness and dU/dh.
    ``eigen=True`` (``surfdisp_forward_eigen_device``, one more solve on the same plan): also the keys of
    ``eigenfunctions`` - ur, uz, tz, tr (Love ut, tt), I0, I1, I2, amp, ztop."""
    import torch
    kind = {"R": 2, "L": 1}[wtype]
    if ellipticity and kind != 2:
        raise ValueError("analytic_kernels: ellipticity kernels are Rayleigh only (wtype='R')")
    if ellipticity and group:
        raise ValueError("analytic_kernels: ellipticity=True and group=True are separate entries; call once for each")
    if attenuation and (group or ellipticity):
        raise ValueError("analytic_kernels: attenuation=True is an entry of its own; call once more for group / ellipticity")
    if thickness and (group or ellipticity or attenuation):
        raise ValueError("analytic_kernels: thickness=True is an entry of its own; call once more for group / ellipticity / attenuation")
    M, _, L = model.shape
    plan = _forward.BatchPlan(M, L, periods.numel(), device=model.device)
    if thickness:
        c, u, st, kb, ka, kr, kh, kz, nnf = plan.run_thickness_kernels(model, periods, kind=kind, nlay=nlay,
                                                                       want_vp=want_vp, want_rho=want_rho)
    elif ellipticity:
        c, u, st, ratio, kb, ka, kr, eb, ea, er, nnf = plan.run_ellip_kernels(model, periods, kind=kind, nlay=nlay,
                                                                             want_vp=want_vp, want_rho=want_rho)
    elif attenuation:
        c, u, st, kb, ka, kr, qinv, gamma, dqdq = plan.run_atten(model, periods, kind=kind, nlay=nlay,
                                                                 want_vp=want_vp, want_rho=want_rho)
    elif group:
        c, u, st, kb, ka, kr, ub, ua, ur, nf = plan.run_group_kernels(model, periods, kind=kind, nlay=nlay, dlnT_frac=dlnT_frac,
                                                                      want_vp=want_vp, want_rho=want_rho)
    else:
        c, u, st, kb, ka, kr = plan.run_kernels(model, periods, kind=kind, nlay=nlay, want_vp=want_vp, want_rho=want_rho)
    per_km = lambda k: _per_km(model, k)
    out = dict(dcdb=kb, dcda=ka, dcdr=kr, c0=c, u0=u, status=st, phv=per_km(kb))
    if group:
        out.update(dudb=ub, duda=ua, dudr=ur, grv=per_km(ub), n_failed=nf)
    if ellipticity:
        out.update(ratio=ratio, dedb=eb, deda=ea, dedr=er, ell=per_km(eb), n_nonfinite=nnf)
    if attenuation:
        out.update(qinv=qinv, gamma=gamma, dqdq=dqdq,
                   Qapp=torch.where(qinv != 0, 1.0 / qinv, torch.full_like(qinv, float("inf"))))
    if thickness:
        out.update(dcdh=kh, dcdz=kz, n_nonfinite=nnf)
    if eigen:
        c0, u0 = c.clone(), u.clone()                       # (the plan's c, u are rewritten by the second solve: same bits)
        out.update(c0=c0, u0=u0)
        e = plan.run_eigen(model, periods, kind=kind, nlay=nlay, want_uz=(kind == 2), want_tz=(kind == 2))
        ed = _eigen_dict(model, kind, *e)
        out.update({k: v for k, v in ed.items() if k not in ("c", "u", "status")})
    return out


class SensKernelPert:
    """Drop-in for the reference class of the same name (``senskernel.py:129-158``): ``model`` is a CSV
    path or a pandas DataFrame with columns ``H``, ``Vs`` and either ``Vp``/``Rho``/``Qs`` or ``Grp``
    (water / sediment / crust / mantle rules of ``sensModel._convert``, ``:104-124``).  After
    construction ``kernel['Vs']`` (and ``kernel['Vp']`` when the frame has a ``Vp`` column) hold
    float64 [n_periods, n_layers] arrays in the reference's units, (v(1.001 x) - v(0.999 x)) / 0.2 / H;
    ``periods = range(Tmin, Tmax + Tstep//2, Tstep)``.

    ``method='fd'`` reproduces the reference's finite differences (one batched solve of 2L+1 stacks per
    column); ``method='analytic'`` takes the partials of one solve (``surfdisp_forward_kernels_device``)
    and converts them, dc/dx * x / 100 / H - the same quantity without the fp32 differencing noise
    (for a layer whose Vp/Rho/Qs follow from Vs through ``Grp``, the reference's Vs perturbation also moves
    them; the analytic route applies that chain rule).  Love kernels use Love velocities (the reference
    reads ``cr0`` for both wave types and returns ``None`` for Love, SURVEY.md section 4 defect 7).
    ``kernel_grv`` holds the same for the group velocity: ``fd`` from the U of the same perturbed batch, ``analytic`` from
    ``surfdisp_forward_group_kernels_device`` with the same chain rule; ``plot(per, ytype='phv' | 'grv' | 'ell', xtype)``.
    ``ellipticity=True`` (Rayleigh) also fills ``kernel_ell`` for the ellipticity chi: ``fd`` from the ratio of the same
    perturbed batch (solved with the ellipticity), ``analytic`` from ``surfdisp_forward_ellip_kernels_device``."""

    def __init__(self, model, wtype="R", Tmin=20, Tmax=100, Tstep=10, dz=2, method="fd", device=0, ellipticity=False):
        import pandas as pd
        if isinstance(model, str):
            df = pd.read_csv(model)
        elif isinstance(model, pd.DataFrame):
            df = model.copy()
        else:
            raise ValueError(f"Wrong model input: {model}")
        self.df = df
        self.wtype = wtype
        self.periods = range(Tmin, Tmax + Tstep // 2, Tstep)
        H = df["H"].to_numpy(float)
        Vs = df["Vs"].to_numpy(float)
        grp = list(df["Grp"]) if "Grp" in df else None
        col = lambda k: df[k].to_numpy(float) if k in df else None
        Vp, Rho, Qs = col("Vp"), col("Rho"), col("Qs")
        self.H, self.Vs = H, Vs
        self.kernel, self.kernel_grv, self.kernel_ell = {}, {}, {}
        ell = bool(ellipticity) and wtype == "R"
        if method == "fd":
            for x in ("Vs", "Vp"):
                if x == "Vp" and Vp is None:
                    continue
                if ell:
                    out = sens_kernel_pert(H, Vs, Vp, Rho, Qs, grp, self.periods, wtype, x, device, ellipticity=True)
                    self.kernel_ell[x] = out["ell"]
                else:
                    out = sens_kernel_pert(H, Vs, Vp, Rho, Qs, grp, self.periods, wtype, x, device)
                self.kernel[x], self.kernel_grv[x] = out["phv"], out["grv"]
        elif method == "analytic":
            import torch
            dVp, dRho, dQs = (None, None, None) if grp is None else _derive(Vs, grp)
            vp = Vp if Vp is not None else dVp
            rho = Rho if Rho is not None else dRho
            qs = Qs if Qs is not None else dQs
            keep = H > 1e-3
            m = np.stack([vp[keep], Vs[keep], rho[keep], H[keep], 1.0 / qs[keep]])[None].astype(np.float32)
            dev = torch.device(f"cuda:{device}")
            per = torch.as_tensor(np.asarray(list(self.periods), np.float32), device=dev)
            out = analytic_kernels(torch.from_numpy(m).to(dev), per, wtype=wtype, group=True)
            Hk, vsk, vpk = H[keep], Vs[keep], vp[keep]
            dvp = np.zeros_like(vsk); drho = np.zeros_like(vsk)      # d(Vp, Rho)/dVs through the Grp rules
            if grp is not None:
                g = np.asarray(grp)[keep]
                if Vp is None:
                    dvp = np.select([g == "sediment", g == "crust", g == "mantle"], [1.23, 1.8, 1.76], 0.0)
                if Rho is None:
                    drho = np.select([g == "sediment", g == "crust", g == "mantle"],
                                     [0.3601 * 1.23, 0.3601 * 1.8, 1.0 / 4.5], 0.0)
            dsts = [(self.kernel, ("dcdb", "dcda", "dcdr"), out), (self.kernel_grv, ("dudb", "duda", "dudr"), out)]
            if ell:
                oe = analytic_kernels(torch.from_numpy(m).to(dev), per, wtype=wtype, ellipticity=True)
                dsts.append((self.kernel_ell, ("dedb", "deda", "dedr"), oe))
            for dst, (b, a, r), out in dsts:
                kb = out[b][0].double().cpu().numpy()
                ka = out[a][0].double().cpu().numpy() if out[a] is not None else np.zeros_like(kb)
                kr = out[r][0].double().cpu().numpy()
                full = np.zeros((len(list(self.periods)), H.size))
                full[:, keep] = (kb + ka * dvp[None, :] + kr * drho[None, :]) * vsk[None, :] / 100.0 / Hk[None, :]
                dst["Vs"] = full
                if Vp is not None:
                    fullp = np.zeros_like(full)
                    fullp[:, keep] = ka * vpk[None, :] / 100.0 / Hk[None, :]
                    dst["Vp"] = fullp
        else:
            raise ValueError("method must be 'fd' or 'analytic'")

    def plot(self, per=None, ytype="phv", xtype="Vs"):
        """The reference's ``SensKernelPert.plot`` (senskernel.py:193-206), with the ``grv`` branch it leaves commented out:
        one curve per period against the layers' mid depths."""
        import matplotlib.pyplot as plt
        if ytype == "phv":
            kernel = self.kernel
        elif ytype == "grv":
            kernel = self.kernel_grv
        elif ytype == "ell" and self.kernel_ell:
            kernel = self.kernel_ell
        else:
            raise ValueError(ytype if ytype != "ell" else "ytype='ell' needs ellipticity=True (Rayleigh)")
        fig, ax = plt.subplots(1, 1, figsize=[6, 8])
        zdeps = np.cumsum(self.H) - self.H / 2
        for iper, p in enumerate(self.periods):
            if per is None or p == per:
                ax.plot(kernel[xtype][iper, :], zdeps, label=f"{p}s")
        ax.invert_yaxis()
        ax.legend()
        return fig


class SensKernel:
    """Drop-in for the reference's ``SensKernel`` (``senskernel.py:8-86``), which runs the senskernel-1.0 toolkit
    (SURF_PERTURB, PHV_SENS_KERNEL, GRV_SENS_KERNEL) on a temporary copy of the model.  Here the kernels come from one
    batched call of ``surfdisp_forward_group_kernels_device`` (analytic phase partials at T and at T x (1 -+ 0.01)).

    ``model``: CSV path or DataFrame with columns H, Vp, Vs, Rho, Qs (the toolkit's model file, one row per layer, the last
    row the half space; layers with H <= 1e-3 are dropped as ``SensKernelPert`` does).  ``model=None`` -> ValueError: the
    reference's default PREM file belongs to the reference's tree.  Fundamental mode only: ``endmode != 0`` -> ValueError.

    After construction ``kernel_phv`` / ``kernel_grv`` are float [1, nCol, P, nz] on ``zdeps = arange(0, sum(H), dz)`` in the
    toolkit's units, (dc/c)/(dx/x) resp. (dU/U)/(dx/x) per km, columns (Vs, Vp, Rho) for 'R' and (Vs, Rho) for 'L'.  Each
    depth sample carries the per-km value of the LAYER that contains it (layer partial x value / velocity / thickness): the
    toolkit splits the model into dz sublayers and samples inside layers, so its curves vary within a thick layer where these
    are flat - their layer means agree.  Differences from the toolkit: its ``dudrho`` has the wrong sign on the frequency
    term (see the module docstring); NaN where a shifted root failed.
    ``ellipticity=True`` (Rayleigh) also fills ``kernel_ell`` [1, nCol, P, nz] = (dchi/chi)/(dx/x) per km for the ellipticity
    chi (H/V), in ``kernel_phv``'s convention, from ``surfdisp_forward_ellip_kernels_device``; ``plot(ytype='ell')``."""

    def __init__(self, model=None, wtype="R", Tmin=20, Tmax=100, Tstep=10, endmode=0, dz=2, device=0, ellipticity=False):
        import pandas as pd
        import torch
        if model is None:
            raise ValueError("SensKernel needs a model: the reference's default PREM file is not part of this package")
        if isinstance(model, str):
            self.model = pd.read_csv(model)
        elif isinstance(model, pd.DataFrame):
            self.model = model.copy()
        else:
            raise ValueError(f"Wrong model input: {model}")
        if endmode != 0:
            raise ValueError("SensKernel: fundamental mode only (endmode=0); overtones are not supported")
        if wtype == "R":
            self.xtype = ["Vs", "Vp", "Rho"]
        elif wtype == "L":
            self.xtype = ["Vs", "Rho"]
        else:
            raise ValueError("Wrong surface wave type!")
        self.wtype = wtype
        self.zdeps = np.arange(0, self.model["H"].sum(), dz)
        self.periods = range(Tmin, Tmax + Tstep // 2, Tstep)
        col = lambda k: self.model[k].to_numpy(float)
        H, Vp, Vs, Rho, Qs = col("H"), col("Vp"), col("Vs"), col("Rho"), col("Qs")
        keep = H > 1e-3
        H, Vp, Vs, Rho, Qs = H[keep], Vp[keep], Vs[keep], Rho[keep], Qs[keep]
        m = np.stack([Vp, Vs, Rho, H, 1.0 / Qs])[None].astype(np.float32)
        dev = torch.device(f"cuda:{device}")
        per = torch.as_tensor(np.asarray(list(self.periods), np.float32), device=dev)
        out = analytic_kernels(torch.from_numpy(m).to(dev), per, wtype=wtype, group=True)
        c = out["c0"][0].double().cpu().numpy()[:, None]
        u = out["u0"][0].double().cpu().numpy()[:, None]
        vals = {"Vs": Vs, "Vp": Vp, "Rho": Rho}
        keys = {"Vs": ("dcdb", "dudb"), "Vp": ("dcda", "duda"), "Rho": ("dcdr", "dudr")}
        # layer of each depth sample: top <= z < bottom
        lay = np.minimum(np.searchsorted(np.cumsum(H), self.zdeps, side="right"), H.size - 1)
        nCol = len(self.xtype)
        self.kernel_phv = np.full((1, nCol, len(self.periods), self.zdeps.size), np.nan)
        self.kernel_grv = np.full_like(self.kernel_phv, np.nan)
        self.layer_phv, self.layer_grv = {}, {}
        for ic, x in enumerate(self.xtype):
            for dst, lay_dst, key, v in ((self.kernel_phv, self.layer_phv, keys[x][0], c),
                                         (self.kernel_grv, self.layer_grv, keys[x][1], u)):
                k = out[key][0].double().cpu().numpy()
                per_km = k * vals[x][None, :] / v / H[None, :]
                per_km[v[:, 0] <= 0, :] = np.nan                     # unsolved periods
                lay_dst[x] = per_km                                  # [P, L] per layer
                dst[0, ic] = per_km[:, lay]
        self.kernel_ell, self.layer_ell = None, {}
        if ellipticity and wtype == "R":
            oe = analytic_kernels(torch.from_numpy(m).to(dev), per, wtype=wtype, ellipticity=True)
            chi = oe["ratio"][0].double().cpu().numpy()[:, None]
            self.kernel_ell = np.full_like(self.kernel_phv, np.nan)
            for ic, x in enumerate(self.xtype):
                k = oe[{"Vs": "dedb", "Vp": "deda", "Rho": "dedr"}[x]][0].double().cpu().numpy()
                with np.errstate(divide="ignore", invalid="ignore"):
                    per_km = k * vals[x][None, :] / chi / H[None, :]
                per_km[chi[:, 0] == 0, :] = np.nan                   # unsolved periods
                self.layer_ell[x] = per_km
                self.kernel_ell[0, ic] = per_km[:, lay]

    def plot(self, mode=0, per=None, ytype="phv", xtype="Vs"):
        """The reference's ``SensKernel.plot`` (senskernel.py:72-85): one curve per period against depth."""
        import matplotlib.pyplot as plt
        if ytype == "phv":
            kernel = self.kernel_phv
        elif ytype == "grv":
            kernel = self.kernel_grv
        elif ytype == "ell" and self.kernel_ell is not None:
            kernel = self.kernel_ell
        else:
            raise ValueError(ytype if ytype != "ell" else "ytype='ell' needs ellipticity=True (Rayleigh)")
        ix = self.xtype.index(xtype)
        fig, ax = plt.subplots(1, 1, figsize=[6, 8])
        for iper, p in enumerate(self.periods):
            if per is None or p == per:
                ax.plot(kernel[mode, ix, iper, :], self.zdeps, label=f"{p}s")
        ax.invert_yaxis()
        ax.legend()
        return fig
