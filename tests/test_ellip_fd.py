"""The ellipticity kernels (surfdisp_forward_ellip_kernels_device, include/surfdisp.h section (5d)) against float64 central
differences of chi: tests/golden/ellip_fd.npz, made by tests/golden/make_golden_ellip.py from the project's own float64
checker (tests/secular64.py) alone.  Without a device: the fixture's own consistency, its tie to thickness_fd.npz and to the CPU
oracle's chi, and the census of the cs_of branches its units reach.  On the GPU: c, ratio, dedb / deda / dedr and dcdb / dcda /
dcdr of every unit against the fixture, the fixed-c pieces, and a period list against one-period launches.

The fixture holds every quantity twice: at the float64-flattened layer values of thickness_fd.npz (set "") and at the fp32
layer values of the library's own prep stage (set "32").  The library flattens in fp32, and the flattened thickness of a
layer is off by up to R0 2^-24 = 4e-4 km whatever its own thickness (1.5e-3 of a 0.25 km layer of eus_L68): against set ""
that is what the figures measure, against set "32" it is gone and the kernel's own mathematics at its fp32 root remains.

Measured on one MI355X, worst over the team sizes 0, 4, 16 and 64 (two units apart, below), and the bar, 4 x rounded up:

                       set ""  (float64-flattened layers)            set "32"  (the kernel's fp32 layers)
    c                  5.35e-4  sediment_L10 6 s        3e-3         1.59e-6  sediment_L10 6 s        7e-6
    ratio              1.23e-3  deepwater_L9 6 s        5e-3         1.53e-5  deepwater_L9 10 s       7e-5
    dchi rows  (a)     1.21e-3  eus_L68 16 s            5e-3         5.89e-5  eus_L68 6 s, team 4     3e-4
    dc rows    (a)     2.62e-3  synth_L12_s3 6 s        2e-2         2.82e-3  synth_L12_s3 6 s        2e-2
    pieces     (b)     8.13e-3  synth_L12_s3 6 s        4e-2         8.95e-3  synth_L12_s3 6 s        4e-2
    own bars: synth_L5 6 s  dchi rows 7.77e-3 / 7.66e-3 (4e-2), dc rows 544 (3e3), pieces 1.50e3 (7e3);
              eus_L68 6 s   dchi rows of set "" 4.14e-3 (2e-2); reasons at OWN_BARS
    later periods (c), set "32":  c 2.02e-2 (9e-2), ratio 3.56e-3 (2e-2), dchi rows 0.905 (4), dc rows 0.422 (2), pieces 1.03 (5),
              all at 16 s after 6 s (synth_L5, sediment_L10); at 40 and 100 s the dchi rows are 1.2e-7 .. 5.0e-3

The bar on the dchi rows was to come out at or below 1e-3 of the peak.  Against set "" it does not (5e-3), and the reason is
the fixture's layer values, not the kernel: on eus_L68 at 6 s the rows are 2.2e-3 .. 4.1e-3 of the peak from fd_* and 2e-6 ..
8e-6 from the same float64 differences taken at the fp32 layer values, which is why set "32" exists; there the bar is 3e-4.
The dc rows and with them the pieces are no sharper than 3e-3 in either set: dcdb / dcda / dcdr come from the (5b) rows, whose
quadrature leaves 2.8e-3 on synth_L12_s3 at 6 s (profiles/thickness/parity.txt, A_b), and dedb - dchidc dcdb inherits it.

That the bars bite, tried once on the rows of one MI355X run with the error put into the fixture side: dchidc x 1.01 is
rejected by the pieces of 8 of the 22 units; one part_vs entry off by 1e-3 of the peak is NOT rejected by the pieces (bar
4e-2), the same error in fd32_vs is rejected by the dchi rows of every unit but synth_L5 at 6 s.
"""
import numpy as np
import pytest

import ellip_fd_lib as EL

# bar = 4 x the worst figure measured on one MI355X over the team sizes 0, 4, 16 and 64, rounded up to one digit
# (profiles/ellip_kernels/parity.txt has the figures); quantity -> bar, per set of the fixture
BARS = {"": dict(c=3e-3, ratio=5e-3, de=5e-3, dc=2e-2, piece=4e-2),
        "32": dict(c=7e-6, ratio=7e-5, de=3e-4, dc=2e-2, piece=4e-2)}
# the rows of periods 1..3 of the (6, 16, 40, 100) s list, against set "32": what the stale layers of the replayed working
# stack cost (at 16 s the layers still carry the attenuation correction of 6 s: c itself moves by 2e-2)
LATER_BARS = dict(c=9e-2, ratio=2e-2, de=4.0, dc=2.0, piece=5.0)
# two units with a bar of their own (4 x their own figure) in the quantities named; every other quantity: the common bar
OWN_BARS = {
    # at 6 s the stack is its 40 km top layer over a half space the mode does not feel: chi hardly depends on any density
    # (the dedr column peaks at 1.8e-6 where dedb peaks at 0.12, dcdr at 6.8e-6 where dcdb is 0.81), and absolute errors that are
    # 1e-7 of the Vs column - the fp32 root's residual in layer 0, which the formula evaluated in float64 at the library's root
    # reproduces to five digits, and an error of 1.4e-8 below a layer 15 radians thick - are 8e-3 of that peak; dcdr[0] of the
    # (5b) rows is off by 3.7e-3 absolute, 3.5e-3 of the energy terms it is the difference of (the A_b of
    # profiles/thickness/parity.txt for this unit), which is 544 peaks of its column
    ("synth_L5", 6.0): {"": dict(de=4e-2, dc=3e3, piece=7e3), "32": dict(de=4e-2, dc=3e3, piece=7e3)},
    # 0.25 km layers whose fp32 flattened thickness is off by up to R0 2^-24 / 0.25 km = 1.5e-3: set "" only
    ("eus_L68", 6.0): {"": dict(de=2e-2)},
}


# ---- without a device -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("x", EL.SETS)
def test_fixture_total_is_part_plus_root_motion(x):
    """fd = part + dchidc dc: every entry within 1e-6 of the column's peak."""
    assert len(EL.UNITS) == 22
    worst = 0.0
    for n, T in EL.UNITS:
        f = EL.unit(n, T)
        for k in EL.COLS:
            fd = f[f"fd{x}_{k}"]
            worst = max(worst, np.abs(fd - f[f"part{x}_{k}"] - f["dchidc" + x] * f[f"dc{x}_{k}"]).max() / np.abs(fd).max())
    print(f"total - (part + dchidc dc): worst {worst:.3e} of the column's peak")
    assert worst <= 1e-6


@pytest.mark.parametrize("x", EL.SETS)
def test_fixture_density_scaling_identity(x):
    """chi does not change when every density is scaled by one factor: sum_i rho_i fd_rho_i = 0 on the stacks without water."""
    worst = 0.0
    for n, T in EL.UNITS:
        if EL.wet(n):
            continue
        t = EL.unit(n, T)[f"fd{x}_rho"][:EL.model(n).shape[1]] * EL.model(n)[2].astype(np.float64)
        worst = max(worst, abs(t.sum()) / np.abs(t).sum())
    print(f"density identity: worst {worst:.3e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("x", EL.SETS)
def test_fixture_step_error(x):
    """The differences at the step (1e-5) and at twice the step agree to 1e-6 of the column's peak in every unit and column."""
    err = np.array([EL.unit(n, T)[f"fd{x}_err"] for n, T in EL.UNITS])
    print(f"fd_err: worst {err.max():.3e}")
    assert err.shape == (22, 3) and (err <= 1e-6).all()


def test_fixture_roots_are_the_thickness_fixture_s():
    """The twenty shared units: c equals thickness_fd.npz's to 1e-12, dc_vs / dc_vp / dc_rho its fd_vs / fd_vp / fd_rho to 1e-9."""
    import thickcheck_lib as TL
    n_shared = 0
    for n, T in EL.UNITS:
        if n not in TL.FD_NAMES:
            continue
        f, t = EL.unit(n, T), TL.fd_unit(n, "R", T)
        assert np.array_equal(EL.model(n), t["model"])
        assert abs(f["c"] - t["c"]) <= 1e-12, (n, T)
        assert np.array_equal(f["lay"], t["lay"])
        for k in EL.COLS:
            assert np.abs(f[f"dc_{k}"] - t[f"fd_{k}"]).max() <= 1e-9, (n, T, k)
        n_shared += 1
    assert n_shared == 20


@pytest.mark.parametrize("x", EL.SETS)
def test_fixture_chi_is_the_oracle_s(x):
    """chi within 2e-3 relative of the CPU oracle's P = 1 ratio for every unit.  Measured: 1.2e-3 at worst (deepwater_L9 and
    eus_L68 at 6 s: the fp32 flattening of the layers, for chi32 at the fp32 layer values is within 2e-5)."""
    worst = 0.0
    for n, T in EL.UNITS:
        c, r = EL.oracle_ratio(n, T)
        chi = float(EL.unit(n, T)["chi" + x])
        assert c > 0
        worst = max(worst, abs(r - chi) / abs(chi))
        assert abs(r - chi) <= 2e-3 * abs(chi), (n, T, r, chi)
    print(f"chi{x} against the oracle: worst {worst:.3e}")


def test_fixture_branch_census():
    """The units reach cs_of's branches: z < -1 and |z| < 1 at least ten times each in the P and in the S row, a solid layer
    with zS > 1, a liquid layer with z > 1."""
    z = sum(EL.unit(n, T)["zreg"].astype(np.int64) for n, T in EL.UNITS)
    zliq = np.array([EL.unit(n, T)["zliq"] for n, T in EL.UNITS])
    print(f"census P {z[0].tolist()} S {z[1].tolist()} (z < -1, |z| <= 1, z > 1); zliq {zliq[np.isfinite(zliq)].round(3).tolist()}")
    assert (z[:, :2] >= 10).all()
    assert z[1, 2] >= 1
    assert np.nanmax(zliq) > 1
    assert np.isfinite(zliq).sum() == 6


# ---- on the GPU -------------------------------------------------------------------------------------------------------------

def _bar(q, x, n, T):
    return OWN_BARS.get((n, T), {}).get(x, {}).get(q, BARS[x][q])


def _line(f):
    return (f"c {f['c']:.2e} ratio {f['ratio']:.2e} dchi rows {f['de']:.2e} dc rows {f['dc']:.2e} pieces {f['piece']:.2e}")


@pytest.mark.gpu
def test_fresh_stack_rows_against_float64_differences():
    """(a) One P = 1 launch per period (6, 10, 16, 40, 100 s), each a ragged batch (Lmax = 68) of the stacks that have that
    period, at team sizes 0, 4, 16 and 64: status 0, no non-finite unit, the water rows of dedb / deda / dedr and dcdb exactly
    zero (dcda and dcdr of a water layer are not: its Vp and rho move c); c and ratio relative to the fixture's; every column of
    dedb / deda / dedr and of dcdb / dcda / dcdr over layers 0 .. mmax-1 (the water column left out) as a fraction of the
    fixture column's peak.  (b) dedb - dchidc dcdb (the fixture's dchidc, the library's dcdb) against part_vs, likewise Vp
    and rho, on the yardstick of the dchi rows: a failure in the rows that passes here is in gamma, one here is in the
    matrices, the adjoint or the chain factors - as far as the accuracy of dcdb / dcda / dcdr lets it see."""
    fail = []
    for team in EL.TEAMS:
        for T, res in EL.fresh_launches(team).items():
            assert res["nnf"] == 0 and (res["status"] == 0).all(), (team, T)
            for b, n in enumerate(res["names"]):
                assert res["c"][b, 0] > 0
                if EL.wet(n):
                    assert all(y[b, 0, 0] == 0 for y in res["de"] + res["dc"][:1]), (team, n, T)
                for x in EL.SETS:
                    f = EL.unit_figures(res, b, 0, x)
                    print(f"team {team:2d} set {x or '64':2s} {n:13s} T={T:5g}: {_line(f)}")
                    fail += [(team, x, n, T, q, v) for q, v in f.items() if not v <= _bar(q, x, n, T)]
    assert not fail, fail


@pytest.mark.gpu
def test_period_list_against_one_period_launches():
    """(c) One P = 4 launch at (6, 16, 40, 100) s on the six stacks: period 0's c, ratio and rows equal a P = 1 launch's bit
    for bit at the same team size (no history exists yet); the units of periods 1..3 against set "32" of the fixture, which
    differentiates the fresh stack of each period: what the stale layers of the replayed working stack cost."""
    from pysurfinv_amd import _lib
    team = _lib.lib().surfdisp_get_team2(len(EL.NAMES), EL.LMAX, len(EL.LIST4), 2)
    r4 = EL.launch(EL.NAMES, EL.LIST4, team)
    r1 = EL.launch(EL.NAMES, EL.LIST4[:1], team)
    assert (r1["c"][:, 0] > 0).all() and r1["nnf"] == 0 and r4["nnf"] == 0 and (r4["status"] == 0).all()
    for k in ("c", "ratio"):
        assert np.array_equal(r4[k][:, 0], r1[k][:, 0]), k
    for y4, y1 in zip(r4["de"] + r4["dc"], r1["de"] + r1["dc"]):
        assert np.isfinite(y1[:, 0]).all() and np.array_equal(y4[:, 0], y1[:, 0])
    fail, n_units = [], 0
    for b, n in enumerate(EL.NAMES):
        for ip, T in enumerate(EL.LIST4):
            if ip == 0 or T not in EL.PERIODS_OF[n]:
                continue
            assert r4["c"][b, ip] > 0
            f = EL.unit_figures(r4, b, ip, "32")
            n_units += 1
            print(f"{n:13s} T={T:5g}: {_line(f)}")
            fail += [(n, T, q, v) for q, v in f.items() if not v <= LATER_BARS[q]]
    assert n_units == 15
    assert not fail, fail
