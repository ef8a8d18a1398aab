#!/usr/bin/env python3
"""Central differences of the phase velocity with respect to every layer thickness, in float64 -> tests/golden/thickness_fd.npz.

The project's own float64 checker (tests/secular64.py, pysurfinv_amd.senskernel): nothing of the reference runs here.  For
the stacks synth_L5, synth_L12_s3, water_L9, sediment_L10 and eus_L68 of tests/golden/ref_eigen.npz at 6, 16, 40 and
100 s, both wave types, one unit = one (stack, period, wave type):

    c        the fundamental-mode root of secular64.delta_rayleigh / delta_love (bisection, then Illinois steps to
             machine precision) over the whole stack, flattened and attenuation-corrected with the float64 formulas of
             senskernel.flattened_layers WITHOUT its float32 cast (a thickness step of 1e-4 km must not be quantised);
             omega = 6.2831853072f / T as the solver holds it;
    u        the structural group velocity: d omega / dk of the stack with its layer values FROZEN at the period (not
             of a stack whose attenuation correction moves with T), from roots at omega exp(-+e), exp(-+2e), e = 1e-3,
             Richardson-extrapolated;
    fd_h     central differences of c with respect to every h_i (step 1e-4 km; all layers below shift rigidly);
    fd_vs, fd_vp, fd_rho   central differences with respect to every Vs_i, Vp_i, rho_i (relative step 1e-5): the
             caller-coordinate shares the flattening chain needs, and the yardstick of the 4 x rule;
    v        the eigenfunction at the top of every layer from the exact propagator (senskernel.eigen_layer_matrix),
             carried upward from the decaying half-space solutions with a re-orthonormalisation at every knot (Rayleigh),
             normalised as include/surfdisp.h section (5f) says; I0 its energy integral, exact per sublayer (Van Loan's
             block exponential), the half space in closed form, the water layer included;
    a, b, rho, d   the layer values the unit was computed on.

A stack much deeper than the mode (eus_L68: 1460 km) is cut, as the library's layer dropping cuts it: the first layer whose
top lies below 36 km x T/s (twelve wavelengths at 3 km/s; the mode's amplitude there is below 1e-9, its effect on c below
1e-18) takes the half-space role with its regular-layer values, at a layer index that stays fixed while the inputs are
stepped - without it the float64 secular function overflows at 6 s.  The entries below it are zeros.

The water layer of water_L9: its rows dcdb, dcda, dcdr are zero in the library, so its own flattening factors are frozen
while a thickness is stepped and its fd_vs, fd_vp, fd_rho entries are stored as zeros (the stated omission of (5g)).

    python tests/golden/make_golden_thickness.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import secular64 as S                                      # noqa: E402
from pysurfinv_amd import senskernel                       # noqa: E402

R0 = 6371.0
TWOPI32 = float(np.float32(6.2831853072))
NAMES = ("synth_L5", "synth_L12_s3", "water_L9", "sediment_L10", "eus_L68")
PERIODS = (6.0, 16.0, 40.0, 100.0)
DH, DREL, EU = 1.0e-4, 1.0e-5, 1.0e-3
NSUB = 16


def flatten64(m, T, w, frozen0=None):
    """senskernel.flattened_layers on a float64 model, no float32 cast.  frozen0: (dif, qqq) of layer 0 to keep."""
    vp, vs, rho, h, qs = m
    L = m.shape[1]
    p = float(np.float32(5.0 if w == "L" else 2.275))
    bot = np.cumsum(h)
    r_i, r_n = R0 - (bot - h), R0 - bot
    reg = np.arange(L) < L - 1
    with np.errstate(all="ignore"):
        fltd = np.log(r_i / r_n)
        dif = np.where(reg, (1.0 / r_n - 1.0 / r_i) * R0 / fltd, R0 / r_i)
        qqq = np.where(reg, (r_i ** p - r_n ** p) / (fltd * R0 ** p * p), (r_i / R0) ** p)
        d = np.where(reg, R0 * fltd, 0.0)
    if frozen0 is not None:
        dif[0], qqq[0] = frozen0
    qsq = qs * np.log(1.0 / T) / np.pi
    qpq = qsq * (4.0 / 3.0) * vs * vs / (vp * vp)
    return dict(a=vp * (1.0 + qpq) * dif, b=vs * (1.0 + qsq) * dif, rho=rho * qqq, d=d), (dif[0], qqq[0])


def cut_index(m, T):
    """Number of layers kept: the first layer whose top lies below 36 T km is the half space."""
    ztop = np.cumsum(m[3]) - m[3]
    deep = np.flatnonzero(ztop >= 36.0 * T)
    return int(deep[0]) + 1 if deep.size else m.shape[1]


def cut(lay, mmax):
    return {k: v[:mmax] for k, v in lay.items()}


def secular(lay, c, om, w):
    T = 2.0 * np.pi / om                                   # secular64 forms k = 2 pi / (c T)
    L = lay["a"].size
    if w == "R":
        return S.delta_rayleigh(lay["a"], lay["b"], lay["rho"], lay["d"], L, c, T)[0]
    return S.delta_love(lay["b"], lay["rho"], lay["d"], L, c, T)[0]


def polish(f, lo, hi, flo, fhi):
    """Illinois regula falsi inside a sign-changing bracket, to machine precision."""
    for _ in range(200):
        x = (lo * fhi - hi * flo) / (fhi - flo)
        if not (lo < x < hi):
            x = 0.5 * (lo + hi)
        fx = f(x)
        if fx == 0.0 or hi - lo <= 4e-16 * hi:
            return x
        if (fx > 0) == (flo > 0):
            lo, flo = x, fx
            fhi *= 0.5
        else:
            hi, fhi = x, fx
            flo *= 0.5
    return 0.5 * (lo + hi)


def root_scan(lay, om, w):
    """The fundamental mode: the first sign change of the secular function from below."""
    solid = lay["b"] > 0
    cmin = 0.7 * lay["b"][solid].min()
    if w == "R" and not solid[0]:
        cmin = min(cmin, 0.7 * lay["a"][0])
    cmax = lay["b"][-1]
    f = lambda c: secular(lay, c, om, w)
    c0, f0 = cmin, f(cmin)
    while c0 < cmax:
        c1 = min(c0 + 2.0e-3, cmax * (1 - 1e-12))
        f1 = f(c1)
        if (f1 > 0) != (f0 > 0):
            return polish(f, c0, c1, f0, f1)
        if c1 >= cmax * (1 - 1e-12):
            break
        c0, f0 = c1, f1
    raise RuntimeError("no root")


def root_near(lay, om, w, c0, half=2.0e-3):
    f = lambda c: secular(lay, c, om, w)
    lo, hi = c0 - half, c0 + half
    flo, fhi = f(lo), f(hi)
    assert (flo > 0) != (fhi > 0), "the bracket around the unperturbed root lost its sign change"
    return polish(f, lo, hi, flo, fhi)


def group_velocity(lay, om, w, c0):
    """d omega / dk at frozen layer values."""
    cs = {s: root_near(lay, om * np.exp(s * EU), w, c0, 2.0e-2) for s in (-2, -1, 1, 2)}
    d1 = (cs[1] - cs[-1]) / (2 * EU)
    d2 = (cs[2] - cs[-2]) / (4 * EU)
    dcdlnw = (4.0 * d1 - d2) / 3.0
    return c0 / (1.0 - dcdlnw / c0)


def system(a, b, rho, k, om, w):
    mu = rho * b * b
    if w == "L":
        return np.array([[0.0, 1.0 / mu], [k * k * mu - om * om * rho, 0.0]]), rho * np.diag([1.0, 0.0])
    lam = rho * (a * a - 2.0 * b * b)
    a12 = 1.0 / (lam + 2.0 * mu)
    a13 = k * lam * a12
    a21 = -om * om * rho
    a43 = a21 + 4.0 * k * k * mu * (lam + mu) * a12
    A = np.array([[0.0, -k, 0.0, 1.0 / mu], [a13, 0.0, a12, 0.0], [0.0, a21, 0.0, k], [a43, 0.0, -a13, 0.0]])
    return A, rho * np.diag([1.0, 1.0, 0.0, 0.0])


def energy_down(A, Q, H, v):
    """int_0^H v(s)^T Q v(s) ds, v(s) = exp(A s) v: Van Loan's block exponential."""
    n = A.shape[0]
    M = np.zeros((2 * n, 2 * n))
    M[:n, :n] = -A.T; M[:n, n:] = Q; M[n:, n:] = A
    E = senskernel._expm(M * H)
    return float(v @ (E[n:, n:].T @ E[:n, n:]) @ v)


def eigenfunction(lay, T, c, w):
    """v [comp][L] at the layer tops and I0."""
    L = lay["a"].size
    om = TWOPI32 / T
    k = om / c
    wet = not (lay["b"][0] > 0)
    e = 1 if wet else 0
    hs = L - 1
    A, Q = system(lay["a"][hs], lay["b"][hs], lay["rho"][hs], k, om, w)
    lamv, vec = np.linalg.eig(A)
    dec = np.flatnonzero(lamv.real < 0)
    assert np.abs(lamv.imag).max() == 0 and dec.size == A.shape[0] // 2
    Y = vec[:, dec].real
    lam_d = lamv[dec].real
    # knots: per layer NSUB sublayers, from the half space up; the subspace re-orthonormalised at every knot
    knots = []                                             # (layer, sub index from the top, basis at the knot's top, R)
    Yq, Rq = np.linalg.qr(Y)
    hs_basis, hs_R = Yq, Rq                                # Y = Yq Rq
    cur = Yq
    for i in range(hs - 1, e - 1, -1):
        Pm = senskernel.eigen_layer_matrix(lay, i, T, c, w, 1.0 / NSUB, fp32_inputs=False)
        for s in range(NSUB - 1, -1, -1):
            Yn, Rn = np.linalg.qr(Pm @ cur)
            knots.append((i, s, Yn, Rn))
            cur = Yn
    # surface condition at the top of the first solid layer: tr = 0 (Love: tq = 0 holds at the root), uz = 1 (ut = 1)
    ncomp = A.shape[0]
    if w == "L":
        coef = np.array([1.0 / cur[0, 0]])
    else:
        t = cur[3, :]
        coef = np.array([t[1], -t[0]])
        coef = coef / (cur[1, :] @ coef)
    v = np.zeros((ncomp, L))
    I0 = 0.0
    # walk down: coefficients at the knot below are R^-1 of those above
    for (i, s, Yn, Rn) in reversed(knots):
        vtop = Yn @ coef
        if s == 0:
            v[:, i] = vtop
        Ai, Qi = system(lay["a"][i], lay["b"][i], lay["rho"][i], k, om, w)
        I0 += energy_down(Ai, Qi, lay["d"][i] / NSUB, vtop)
        coef = np.linalg.solve(Rn, coef)
    vh = hs_basis @ coef
    v[:, hs] = vh
    ah = np.linalg.solve(hs_R, coef)                       # in the decaying eigenvectors (Y = hs_basis hs_R): closed-form integral
    for p_ in range(dec.size):
        for q_ in range(dec.size):
            I0 += ah[p_] * ah[q_] * float(Y[:, p_] @ Q @ Y[:, q_]) / (-(lam_d[p_] + lam_d[q_]))
    resid = abs(v[-1, e]) / np.abs(v[-1]).max() if w == "L" else (abs(v[2, e]) / np.abs(v[2]).max() if not wet else 0.0)
    if wet and w == "R":
        # the water column above the sea floor: (uz, tz), uz' = tz / lam - k^2 tz / (rho om^2), tz' = -rho om^2 uz
        rw, aw, Hw = lay["rho"][0], lay["a"][0], lay["d"][0]
        lam = rw * aw * aw
        Aw = np.array([[0.0, 1.0 / lam - k * k / (rw * om * om)], [-rw * om * om, 0.0]])
        Qw = np.diag([rw, k * k / (rw * om ** 4)])
        top = senskernel._expm(-Hw * Aw) @ v[[1, 2], 1]
        resid = abs(top[1]) / max(abs(v[2, 1]), 1e-300)    # the pressure vanishes at the sea surface
        for s in range(NSUB):
            vs_ = senskernel._expm(-(Hw * (NSUB - s) / NSUB) * Aw) @ v[[1, 2], 1]
            I0 += energy_down(Aw, Qw, Hw / NSUB, vs_)
    return v, I0, resid


def one(job):
    """All periods of one (stack, wave type)."""
    name, w, m32 = job
    m0 = np.asarray(m32, np.float32).astype(np.float64)
    L = m0.shape[1]
    wet = not (m0[1, 0] > 0)
    P = len(PERIODS)
    ncomp = 4 if w == "R" else 2
    rec = dict(c=np.zeros(P), u=np.zeros(P), I0=np.zeros(P), v=np.zeros((P, ncomp, L)), fd_h=np.zeros((P, L)),
               fd_vs=np.zeros((P, L)), fd_vp=np.zeros((P, L)), fd_rho=np.zeros((P, L)), lay=np.zeros((P, 4, L)), mmax=np.zeros(P, np.int32))
    for ip, T in enumerate(PERIODS):
        om = TWOPI32 / T
        mmax = cut_index(m0, T)
        lay, f0 = flatten64(m0, T, w)
        lay = cut(lay, mmax)
        frozen = f0 if wet else None
        c0 = root_scan(lay, om, w)
        rec["c"][ip] = c0
        rec["u"][ip] = group_velocity(lay, om, w, c0)
        v, I0, resid = eigenfunction(lay, T, c0, w)
        assert resid < 1e-6, (name, w, T, resid)
        rec["v"][ip, :, :mmax], rec["I0"][ip] = v, I0
        rec["lay"][ip, :, :mmax] = np.stack([lay["a"], lay["b"], lay["rho"], lay["d"]])
        rec["mmax"][ip] = mmax

        def fd(row, i, step):
            cs = []
            for s in (-1.0, 1.0):
                m = m0.copy()
                m[row, i] += s * step
                cs.append(root_near(cut(flatten64(m, T, w, frozen)[0], mmax), om, w, c0))
            return (cs[1] - cs[0]) / (2.0 * step)
        for i in range(mmax):
            if i < mmax - 1:
                rec["fd_h"][ip, i] = fd(3, i, DH)
            if wet and i == 0:
                continue
            rec["fd_vs"][ip, i] = fd(1, i, DREL * m0[1, i])
            rec["fd_rho"][ip, i] = fd(2, i, DREL * m0[2, i])
            if w == "R":
                rec["fd_vp"][ip, i] = fd(0, i, DREL * m0[0, i])
        print(f"{name} {w} T={T:g}: layers {mmax} c {c0:.9f} U {rec['u'][ip]:.9f} I0 {I0:.6g} surface residual {resid:.1e}", flush=True)
    return name, w, rec


def main():
    import multiprocessing
    fix = np.load(os.path.join(HERE, "ref_eigen.npz"))
    out = {"names": np.array(NAMES), "periods": np.array(PERIODS)}
    jobs = []
    for name in NAMES:
        out[f"{name}_model"] = np.asarray(fix[f"{name}_model"], np.float32)
        jobs += [(name, w, out[f"{name}_model"]) for w in ("R", "L")]
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        for name, w, rec in pool.map(one, jobs):
            for k_, a_ in rec.items():
                out[f"{name}_{w}_{k_}"] = a_
    np.savez_compressed(os.path.join(HERE, "thickness_fd.npz"), **out)


if __name__ == "__main__":
    main()
