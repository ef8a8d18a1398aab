"""The descriptor zoo (tests/descriptor_zoo.py) on the CPU: the zoo reaches every descriptor branch (so that it cannot lose one later),
the float64 torch statement the device tests compare with equals the modelled project's own output on the zoo's settings
(tests/golden/ref_zoo.npz, written by tests/golden/make_golden_zoo.py), and the dual-number copy of the descriptor walk
(csrc/surfdisp_layers_dual.h, compiled for the host) agrees with that statement on every setting."""
import os

import numpy as np
import pytest
import torch

import descriptor_zoo as Z
from param_lsq_cases import REL_STEP, jac_error
from pysurfinv_amd import paramlsq
from pysurfinv_amd.layers_batch import Model1DBatch
from pysurfinv_amd.mcmc import PriorRules

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_zoo.npz"))


def test_every_setting_is_static_with_the_stated_structure():
    for name in Z.ZOO:
        mb = Z.cpu_model(name)
        assert mb._static_sig == Z.STATIC_SIG[name], name
        desc = mb.native_descriptor()
        assert desc is not None and desc[2] == Z.LAYERS[name], name
        assert not mb._native_thermal


def test_the_zoo_reaches_every_descriptor_branch():
    got, flags = set(), set()
    for name in Z.ZOO:
        mb = Z.cpu_model(name)
        b = Z.branches(mb)
        print(name, sorted(map(str, b)))
        got |= b
        for kw in Z.RULES[name]:
            flags |= Z.flag_branches(mb, PriorRules(mb, **kw))
    assert Z.REQUIRED <= got, Z.REQUIRED - got
    assert Z.REQUIRED_FLAGS <= flags, Z.REQUIRED_FLAGS - flags
    # what each setting is there for
    assert {("pair", "sediment"), ("pair", "crust"), ("pair", "mantle"), ("ncoef", 8), "mixed_slots", "bottom_last", ("has_ref", 1)} \
        <= Z.branches(Z.cpu_model("pairs"))
    assert {"bottom_middle", "topo_slot", "topo_negative", ("kind", 3), ("kind", 7), ("ncoef", 1)} <= Z.branches(Z.cpu_model("moho"))
    assert {("nin", 10), "h_slot", "h_const", "z_const"} | {("kind", k) for k in (0, 1, 2, 3, 4, 5, 7)} <= Z.branches(Z.cpu_model("ten"))
    assert ("bit_with_next", 2) in Z.flag_branches(Z.cpu_model("pairs"), PriorRules(Z.cpu_model("pairs"), **Z.RULES["pairs"][0]))


def test_params_are_v0_then_draws_inside_the_box():
    mb = Z.cpu_model("ten")
    p = Z.zoo_params(mb, 50, seed=1)
    assert np.array_equal(p[0], mb.spec.v0) and (p[1:] > mb.spec.vmin).all() and (p[1:] < mb.spec.vmax).all()
    assert np.array_equal(p, Z.zoo_params(mb, 50, seed=1)) and Z.zoo_rows(mb, 5) is None
    rows = Z.zoo_rows(Z.cpu_model("moho"), 301)
    assert set(rows) == {0, 1, 2, 3} and (np.diff(rows) < 0).any()


def _golden_model(name):
    if name == "ten_ref":                                   # `ten` without the two names the modelled project does not know
        return Model1DBatch({k: v for k, v in Z.ZOO["ten"].items() if not k.startswith("Land")})
    return Z.cpu_model(name)


@pytest.mark.parametrize("name", ["pairs", "moho", "ten_ref"])
def test_torch_statement_matches_the_modelled_project(name):
    """seisPropLayers of 12 parameter vectors and seisPropGrids (with groups) of four of them: <= 1e-9, the bar of
    tests/test_layers_batch.py."""
    mb = _golden_model(name)
    params = torch.from_numpy(G[f"{name}/params"])
    rows = torch.from_numpy(G[f"{name}/rows"]) if mb.n_aux else None
    assert params.shape == (12, mb.spec.n) and np.allclose(mb.spec.v0, G[f"{name}/params"][0])
    (h, vs, vp, rho, qs, qp), nlay = mb.seis_prop_layers(params, rows)
    ref = G[f"{name}/layers"]
    assert np.array_equal(nlay.numpy(), G[f"{name}/nlay"])
    worst = 0.0
    for a, r in zip((h, vs, vp, rho, qs, qp), np.moveaxis(ref, 1, 0)):
        assert a.shape == r.shape
        worst = max(worst, float(np.abs(a.numpy() - r).max()))
    sel = G[f"{name}/grid_of"]
    out, grp, ngrid = mb.seis_prop_grids(params[sel], None if rows is None else rows[sel])
    gref = G[f"{name}/grids"]
    assert np.array_equal(ngrid.numpy(), G[f"{name}/ngrid"]) and list(Model1DBatch.GROUP_NAMES) == list(G["groups"])
    for a, r in zip(out, np.moveaxis(gref[:, :6], 1, 0)):
        assert a.shape == r.shape
        worst = max(worst, float(np.abs(a.numpy() - r).max()))
    assert np.array_equal(grp.numpy(), gref[:, 6].astype(np.int64))
    print(f"{name}: largest difference from the modelled project {worst:.2e}")
    assert worst < 1e-9
    if name == "moho":                                      # the points differ: topo moves the stack's top under a fixed BottomDepth
        assert len(np.unique(G["moho/rows"])) == 4 and np.abs(ref[0, 0] - ref[9, 0]).max() > 1e-3


@pytest.mark.parametrize("name", list(Z.ZOO))
def test_rule_sets_discriminate_on_the_float64_statement(name):
    """Every rule set's accept share on 2000 uniform draws lies in [0.05, 0.95] (the GPU test asserts it on its 5000)."""
    mb = Z.cpu_model(name)
    p = Z.zoo_params(mb, 2000, seed=17)
    rows = Z.zoo_rows(mb, 2000)
    for kw in Z.RULES[name]:
        share = float(PriorRules(mb, **kw)(torch.from_numpy(p), rows=rows).float().mean())
        print(name, kw, f"accept share {share:.3f}")
        assert 0.05 <= share <= 0.95, (name, kw, share)


# ------------------------------------------------------------------------------------- the dual-number walk, host build
@pytest.fixture(scope="module")
def lib():
    from test_param_jacobian_host import load_jaccheck
    return load_jaccheck()


@pytest.mark.parametrize("name", list(Z.ZOO))
def test_dual_numbers_on_the_zoo(lib, name):
    """40 rows per setting: the value part within 1e-12 relative of the torch statement, the Jacobian within JAC_BAR of central
    differences, every unknown with a non-zero column."""
    from test_param_jacobian_host import host_jacobian
    mb = Z.cpu_model(name)
    idesc, fdesc, L = mb.native_descriptor()
    idesc, fdesc = np.ascontiguousarray(idesc.numpy()), np.ascontiguousarray(fdesc.numpy())
    p = Z.zoo_params(mb, 40, seed=23)
    rows = Z.zoo_rows(mb, 40)
    full = mb._full(torch.from_numpy(p), rows).numpy()
    layer, jac = host_jacobian(lib, mb, idesc, fdesc, L, full, mb.spec.n)
    layer_fd, fd = paramlsq.jacobian_reference(mb, p, REL_STEP, rows=rows)
    assert jac.shape == fd.shape == (40, 4, Z.LAYERS[name], mb.spec.n) and np.isfinite(jac).all()
    assert np.abs(layer - layer_fd).max() <= 1e-12 * np.abs(layer_fd).max()
    ratio, worst = jac_error(jac, fd)
    print(f"{name}: largest |jac - fd| {worst:.2e}, worst error / bar {ratio:.2e}")
    assert ratio <= 1.0, (name, ratio, worst)
    assert (np.abs(jac).max(axis=(1, 2)) > 0).all()
