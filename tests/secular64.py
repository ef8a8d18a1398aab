"""float64 restatement of the production secular functions of pysurfinv_amd/csrc/surfdisp_kernels.hip.

The same factorised recursion as the kernel (comment above ray_step): the Rayleigh state (b1, h2..h5) carried in the
layer's density scale, stepped by the nine coefficient products and closed by the half-space row (ray_close); the liquid
top layer (only cosp and sinpr); the Love 2-vector (ut, tt) from the half space up (delta_love).  Every quantity is
float64, and the layer coefficients are formed from sin(x)/x and sinh(x)/x, which are accurate for small x, so the
functions are continuous where c crosses a layer velocity.  Inputs are the float32 values the kernel sees (a, b, rho, d,
c, T), taken exactly.  tests/test_secular_functions.py compares the kernel with this; tests/test_secular64.py checks this
against a brute-force (matrix-exponential) propagation of the equations of motion."""
import numpy as np

ACCUR = 1.0e-8       # |b| at or below this: a liquid layer (the kernel's ACCUR)


def sinc(x):
    """sin(x)/x, float64; 1 at 0."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(x) / np.where(x == 0.0, 1.0, x))


def sinhc(x):
    """sinh(x)/x, float64; 1 at 0."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(x == 0.0, 1.0, np.sinh(x) / np.where(x == 0.0, 1.0, x))


def coef(arg, wd):
    """layer_coef: arg = 1 - c^2/v^2, wd = k d -> (rsin, sinr, cs, x, ph) as float64 arrays.
    r = sqrt(-arg) continued to r = -sqrt(arg) where arg > 0 (evanescent), x = wd r:
    rsin = r sin x = -arg wd sinc(x) (r sinh side: -arg wd sinhc), sinr = sin(x)/r = wd sinc(x) (wd sinhc(|x|)),
    cs = cos x (cosh |x|), ph = x where oscillatory, else 0."""
    arg = np.asarray(arg, np.float64); wd = np.asarray(wd, np.float64)
    s = np.sqrt(np.abs(arg))
    ev = arg > 0.0
    x = np.where(ev, -wd * s, wd * s)
    xa = wd * s
    shape = np.where(ev, sinhc(xa), sinc(xa))
    with np.errstate(over="ignore"):
        cs = np.where(ev, np.cosh(xa), np.cos(xa))
    return -arg * wd * shape, wd * shape, cs, x, np.where(ev, 0.0, x)


def _trial(c, T):
    c = float(c); T = float(T)
    return 2.0 * np.pi / (c * T), c * c


def ray_step(s, c, T, a, b, d, rho, rho_prev, start, first):
    """one layer of delta_rayleigh: state (b1, h2, h3, h4, h5) at the layer's top in the scale of rho_prev (ignored when
    first) -> the state at its bottom in the scale of rho, and the layer's vertical phase."""
    b1, h2, h3, h4, h5 = (float(v) for v in s)
    wvno, csq = _trial(c, T)
    a, b, d, rho = float(a), float(b), float(d), float(rho)
    if not first:
        rat = float(rho_prev) / rho
        h2 *= rat; h3 *= rat; h4 *= rat; h5 *= rat * rat
    wd = wvno * d
    arga = 1.0 - csq / (a * a)
    if first and not abs(b) > ACCUR:                        # liquid top layer: a11 = cosp, a21 = rhoc sinpr
        if start != 1:
            return (b1, h2, h3, h4, h5), 0.0
        _, sinpr, cosp, _, ph = (float(v) for v in coef(arga, wd))
        return (cosp * b1, sinpr * b1, 0.0, 0.0, cosp * h5 - sinpr * h4), ph
    argb = 1.0 - csq / (b * b)
    rsinp, sinpr, cosp, _, php = (float(v) for v in coef(arga, wd))
    rsinq, sinqr, cosq, _, phq = (float(v) for v in coef(argb, wd))
    g = 2.0 * b * b / csq
    g1 = g - 1.0
    u1 = g * g * b1 + 2.0 * g * h3 - h5
    u2 = g1 * g1 * b1 + 2.0 * g1 * h3 - h5
    D = 1.0 - cosp * cosq
    t1 = rsinq * u1 + cosq * h2
    t2 = sinqr * u2 - cosq * h4
    E1 = rsinp * t1 - cosp * rsinq * h4 + D * u2
    E2 = sinpr * t2 + cosp * sinqr * h2 + D * u1
    n1 = b1 - E1 - E2
    n2 = cosp * t1 + sinpr * (rsinq * h4 + cosq * u2)
    n3 = h3 + g * E1 + g1 * E2
    n4 = rsinp * (sinqr * h2 - cosq * u1) - cosp * t2
    n5 = h5 + g * g * E1 + g1 * g1 * E2
    return (n1, n2, n3, n4, n5), php + phq


def ray_close(s, c, T, a, b, rho_last, rho_prev, start):
    """half-space closure -> (value, mag): value = -bb1 for start 1 (bb1 otherwise), mag = the sum of the magnitudes of
    its five terms."""
    b1, h2, h3, h4, h5 = (float(v) for v in s)
    _, csq = _trial(c, T)
    a, b, rho_last, rho_prev = float(a), float(b), float(rho_last), float(rho_prev)
    ia2 = 1.0 / (a * a)
    arga = 1.0 - csq * ia2
    argb = 1.0 - csq / (b * b)
    ra = -np.sqrt(arga) if arga > 0 else np.sqrt(-arga)
    rb = -np.sqrt(argb) if argb > 0 else np.sqrt(-argb)
    irho = 1.0 / rho_last
    rhoc = rho_prev * csq
    sss = b * b
    g = 2.0 * sss / csq
    g1 = g - 1.0
    gra = g * ra
    it12 = ia2 * irho
    h11 = -2.0 * rb * sss * ia2 + csq * g1 * g1 * ia2 / gra
    h12 = -it12 / g
    h13 = -rb * it12 + g1 * it12 / gra
    h14 = rb * it12 / gra
    h15 = (rb - 1.0 / ra) * irho * irho * ia2 / csq / g
    terms = (h11 * b1, rhoc * h12 * h2, rhoc * 2.0 * h13 * h3, rhoc * h14 * h4, rhoc * rhoc * h15 * h5)
    bb1 = sum(terms)
    mag = sum(abs(t) for t in terms)
    return (-bb1 if start == 1 else bb1), mag


def delta_rayleigh(a, b, rho, d, mmax, c, T):
    """delta_rayleigh (start 1) on layers 0 .. mmax-1 (mmax-1: the half space) -> (value, mag, phi)."""
    s = (1.0, 0.0, 0.0, 0.0, 0.0)
    phi = 0.0
    last = mmax - 1
    for m in range(last):
        s, ph = ray_step(s, c, T, a[m], b[m], d[m], rho[m], rho[m - 1] if m else 0.0, 1, m == 0)
        phi += ph
    v, mag = ray_close(s, c, T, a[last], b[last], rho[last], rho[last - 1] if last >= 1 else 0.0, 1)
    return v, mag, phi


def delta_love(b, rho, d, mmax, c, T):
    """delta_love on layers 0 .. mmax-1 -> (value, mag, phi); liquid layers (b == 0) are passed over."""
    wvno, csq = _trial(c, T)
    mh = mmax - 1
    bh = float(b[mh])
    h = float(rho[mh]) * bh * bh
    ut, tt = 1.0, h * np.sqrt(abs(csq / (bh * bh) - 1.0))
    mag = 0.0
    phi = 0.0
    for m in range(mh - 1, -1, -1):
        bm = float(b[m])
        if bm == 0.0:
            continue
        h = float(rho[m]) * bm * bm
        rsin, sinr, cs, _, ph = (float(v) for v in coef(1.0 - csq / (bm * bm), wvno * float(d[m])))
        yv, z = -sinr, -rsin                                  # at q = -k d rb: sin(q)/rb, rb sin q
        eut = cs * ut - yv * tt / h
        ett = h * z * ut + cs * tt
        mag = abs(h * z * ut) + abs(cs * tt)
        phi += ph
        ut, tt = eut, ett
    return -tt, mag, phi
