"""Settings that between them reach every branch of the params -> stack descriptor (csrc/surfdisp_layers_grid.h: grid_value,
closed_forms, layer_span), for the tests that run every kernel reading a descriptor on them (tests/test_descriptor_zoo*.py, and the
zoo cases of test_prior_redraw.py / test_posterior_gpu.py).  A plain module, not a conftest.

  pairs  two adjacent input layers in each of the three groups (sediment, crust, mantle: the prior's bit 1, monotone on to the next
         layer's top), a mantle of 8 coefficient slots with constants among them and `deg`, a free BottomDepth on the last layer,
         the reference mantle.
  moho   BottomDepth on a MIDDLE layer (every later top depends on it), a scalar crust Vs, a water top, Info.topo per point (K = 1,
         one negative entry), no reference mantle.
  ten    the cap of ten input layers, every kind but the thermal one, thicknesses from slots and from constants.

The float64 statement every device test compares with is Model1DBatch.seis_prop_layers / seis_prop_grids / prior_good on the CPU,
itself pinned to the modelled project's output by tests/golden/ref_zoo.npz (test_descriptor_zoo.py)."""
import functools

import numpy as np

from pysurfinv_amd.layers_batch import Model1DBatch

ZOO = {
    "pairs": {
        'Sediment': {'H': [1.0, 'abs', 0.5, 0.05], 'Vs': [1.2, 'abs', 0.4, 0.05]},
        'OceanSediment': {'H': [0.8, 'abs', 0.3, 0.05], 'Vs': [1.8, 'abs', 0.4, 0.05]},
        'OceanCrust': {'H': [6.0, 'abs', 0.9, 0.2], 'Vs': [[2.9, 'abs', 0.3, 0.02], [3.3, 'abs', 0.3, 0.02]]},
        'Crust': {'H': [25., 'abs', 4., 1.0],
                  'Vs': [[3.4, 'abs', 0.3, 0.02], [3.6, 'abs', 0.3, 0.02], [3.8, 'abs', 0.3, 0.02], [3.9, 'abs', 0.3, 0.02]]},
        'Mantle': {'H': [50., 'abs', 9., 1.0], 'Vs': [[4.3, 'abs', 0.3, 0.02], 4.35, [4.4, 'abs', 0.3, 0.02]]},
        'OceanMantle': {'BottomDepth': [200., 'abs', 10., 2.0], 'deg': 3,
                        'Vs': [[4.4, 'abs', 0.4, 0.02], [4.35, 'abs', 0.4, 0.02], 4.4, [4.5, 'abs', 0.4, 0.02], [4.6, 'abs', 0.4, 0.02], 4.6,
                               [4.65, 'abs', 0.2, 0.02], 4.7]},
        'Info': {'modelType': 'MCInv', 'refLayer': True}},
    "moho": {
        'OceanWater': {'H': 1.5},
        'OceanSedimentCascadia': {'H': [0.5, 'abs', 0.1, 0.03]},
        'OceanCrust': {'BottomDepth': [7.6, 'abs', 0.3, 0.1], 'Vs': [3.5, 'abs', 0.3, 0.02]},
        'Mantle': {'H': 120., 'Vs': [[4.4, 'abs', 0.4, 0.02], [4.2, 'abs', 0.4, 0.02], [4.3, 'abs', 0.4, 0.02], [4.5, 'abs', 0.4, 0.02]]},
        'Info': {'modelType': 'MCInv', 'refLayer': False, 'topo': 0.0}},
    "ten": {
        'OceanWater': {'H': 2.0},
        'OceanSediment': {'H': [0.4, 'abs', 0.2, 0.05], 'Vs': [1.0, 0.5, 1.6, 0.05]},
        'OceanSedimentCascadia': {'H': [0.5, 'abs', 0.2, 0.03]},
        'Sediment': {'H': 1.0, 'Vs': [[1.5, 'abs', 0.3, 0.05], [2.2, 'abs', 0.3, 0.05]]},
        'LandSediment': {'H': 1.0, 'Vs': 2.4},
        'OceanCrust': {'H': [6.0, 'abs', 0.9, 0.2], 'Vs': [[3.0, 'abs', 0.3, 0.02], [3.4, 'abs', 0.3, 0.02]]},
        'Crust': {'H': [12., 'abs', 1.5, 0.5], 'Vs': [[3.5, 'abs', 0.2, 0.02], [3.7, 'abs', 0.2, 0.02], [3.8, 'abs', 0.2, 0.02]]},
        'LandCrust': {'H': 8., 'Vs': [3.9, [4.0, 'abs', 0.1, 0.02], 4.05]},
        'Mantle': {'H': [40., 'abs', 9., 1.0], 'Vs': [[4.3, 'abs', 0.3, 0.02], [4.4, 'abs', 0.3, 0.02], [4.45, 'abs', 0.3, 0.02]]},
        'OceanMantle': {'BottomDepth': 180.,
                        'Vs': [[4.4, 'abs', 0.4, 0.02], [4.35, 'abs', 0.4, 0.02], [4.4, 'abs', 0.4, 0.02], [4.5, 'abs', 0.4, 0.02]]},
        'Info': {'modelType': 'MCInv', 'refLayer': False}},
}
# per-point local constants of a setting: (local_keys, table [rows, K])
LOCAL = {"moho": (["topo"], np.array([[-1.0], [0.0], [0.3], [0.6]]))}
STATIC_SIG = {"pairs": [1, 1, 3, 15, 15, 30], "moho": [1, 1, 3, 30], "ten": [1, 1, 1, 1, 1, 3, 10, 5, 15, 30]}
LAYERS = {"pairs": 85, "moho": 35, "ten": 68}

# PriorRules keywords, three sets per setting.  (The default rules - sediment and crust monotone - accept nothing where a sediment
# layer has a constant Vs, as the Cascadia sediment and `ten`'s LandSediment do.)
RULES = {
    "pairs": [dict(monotone_groups=("crust",), positive_jumps=False), dict(monotone_groups=(), positive_jumps=True),
              dict(monotone_groups=("crust",), positive_jumps=True)],
    "moho": [dict(monotone_groups=(), positive_jumps=True, vs_max=4.5), dict(monotone_groups=("mantle",), positive_jumps=False),
             dict(monotone_groups=(), positive_jumps=False, vs_max=4.55)],
    "ten": [dict(monotone_groups=(), positive_jumps=True, vs_max=4.6), dict(monotone_groups=("crust",), positive_jumps=True),
            dict(monotone_groups=(), positive_jumps=False, vs_max=4.55)],
}

GROUP_OF_KIND = {0: "sediment", 4: "sediment", 7: "sediment", 1: "crust", 5: "crust", 2: "mantle", 6: "mantle", 3: "water"}

# what the zoo as a whole must reach (test_descriptor_zoo.py asserts it)
REQUIRED = (
    {("kind", k) for k in (0, 1, 2, 3, 4, 5, 7)} | {("ncoef", n) for n in (0, 1, 2, 3, 4, 8)}
    | {"mixed_slots", "h_slot", "h_const", "bottom_last", "bottom_middle", "topo_slot", "topo_negative", "z_const",
       ("has_ref", 0), ("has_ref", 1), ("nin", 10), ("pair", "sediment"), ("pair", "crust"), ("pair", "mantle")})
REQUIRED_FLAGS = {("bit", 1), ("bit", 2), ("bit", 4), ("bit", 8), ("bit_with_next", 2), ("bit_with_next", 4)}


def zoo_model(name, device="cpu"):
    """The Model1DBatch of a zoo setting on `device`, its per-point table set."""
    keys, table = LOCAL.get(name, (None, None))
    mb = Model1DBatch(ZOO[name], device=device, local_keys=keys)
    if table is not None:
        mb.set_local_info(table)
    return mb


@functools.lru_cache(maxsize=None)
def cpu_model(name):
    return zoo_model(name)


def zoo_params(mb, C, seed):
    """float64 [C, Nu]: row 0 is v0, the rest uniform in the prior box."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(mb.spec.vmin, np.float64), np.asarray(mb.spec.vmax, np.float64)
    p = lo + (hi - lo) * rng.random((C, lo.size))
    p[0] = np.asarray(mb.spec.v0, np.float64)
    return np.ascontiguousarray(p)


def zoo_rows(mb, C):
    """The local-info row of each of C parameter vectors, given out of order (None: the model has no per-point constants)."""
    if not mb.n_aux:
        return None
    n = int(mb._aux.shape[0])
    return ((np.arange(C) * 3 + 1) % n).astype(np.int64)


def branches(mb):
    """The set of descriptor branches ``mb.native_descriptor()`` reaches, read off idesc (layout: csrc/surfdisp_layers.hip):
    ("kind", k), ("ncoef", n), "mixed_slots" (constant and parameter slots in one layer), "h_slot" / "h_const", "bottom_last" /
    "bottom_middle" (BottomDepth on the last / on an earlier layer), "topo_slot" (with "topo_negative" where the table has a
    negative entry) / "z_const", ("has_ref", 0 | 1), ("nin", n), ("pair", group) for two adjacent input layers of one group."""
    idesc = mb.native_descriptor()[0].cpu().numpy()
    nin, has_ref = int(idesc[0]), int(idesc[3])
    lay_i = idesc[4:4 + 8 * nin].reshape(nin, 8)
    coef_i = idesc[4 + 8 * nin:4 + 16 * nin].reshape(nin, 8)
    out = {("nin", nin), ("has_ref", has_ref)}
    for l in range(nin):
        kind, hs, bottom, nc = (int(x) for x in lay_i[l, :4])
        out |= {("kind", kind), ("ncoef", nc), "h_slot" if hs >= 0 else "h_const"}
        if bottom:
            out.add("bottom_last" if l == nin - 1 else "bottom_middle")
        sl = coef_i[l, :nc]
        if nc and (sl >= 0).any() and (sl < 0).any():
            out.add("mixed_slots")
        if l + 1 < nin and GROUP_OF_KIND[kind] == GROUP_OF_KIND[int(lay_i[l + 1, 0])]:
            out.add(("pair", GROUP_OF_KIND[kind]))
    topo = int(lay_i[0, 6])
    if topo > 0:
        out.add("topo_slot")
        if float(mb._aux[:, topo - 1 - mb.spec.n].min()) < 0:
            out.add("topo_negative")
    else:
        out.add("z_const")
    return out


def flag_branches(mb, rules):
    """("bit", b) for every bit value b in a flag word of ``mb.prior_flags(rules)``, and ("bit_with_next", b) for b = 2, 4 where the
    word sits on the last output layer of an input layer that has a next one (the kernel then reads the next layer's top)."""
    flags = mb.prior_flags(rules).cpu().numpy()
    idesc = mb.native_descriptor()[0].cpu().numpy()
    nin = int(idesc[0])
    lay_i = idesc[4:4 + 8 * nin].reshape(nin, 8)
    out = {("bit", b) for b in (1, 2, 4, 8) if (flags & b).any()}
    o = 0
    for l in range(nin):
        o += int(lay_i[l, 5] - lay_i[l, 4]) - 1                # N output layers of input layer l
        if l + 1 < nin:
            out |= {("bit_with_next", b) for b in (2, 4) if flags[o - 1] & b}
    return out
