#!/usr/bin/env python3
"""Golden vectors for the settings of tests/descriptor_zoo.py from the imported reference Python (development container only; see
_refimport.py), in the manner of make_golden_grids.py: 12 parameter vectors per setting - the setting's own and the reference's own
``reset()`` draws - with their ``seisPropLayers``, and ``seisPropGrids`` (with the group of each point) of every third of them
(`grid_of`; the layers are the midpoint form of the grids, models.py:93-102, so the rest would say the same twice).

  pairs    as it stands
  moho     one model per row of its per-point table (``Info.topo`` through localInfo, as ``Point(setting, localInfo)`` passes it),
           three vectors each
  ten_ref  `ten` without its two Land* keys, which the reference's layerClassDict does not know (layers.py:553-570)

Data only.  The archive is written with fixed member dates, so a second run gives the same bytes.

    python tests/golden/make_golden_zoo.py        ->  tests/golden/ref_zoo.npz
"""
import io
import os
import random
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refimport  # noqa: E402

_refimport.install()
from pySurfInv.models import buildModel1D            # noqa: E402
from descriptor_zoo import LOCAL, ZOO                # noqa: E402

GROUPS = ["water", "sediment", "crust", "mantle"]


def ten_ref():
    return {k: v for k, v in ZOO["ten"].items() if not k.startswith("Land")}


def capture(setting, infos, ndraw, seed):
    """infos: one localInfo dict (or None) per point; ndraw vectors per point."""
    random.seed(seed)
    ref = setting['Info'].get('refLayer', False)
    P, Ls, Gs, rows, grid_of = [], [], [], [], []
    for i, info in enumerate(infos):
        mod0 = buildModel1D(setting, info) if info is not None else buildModel1D(setting)
        for m in [mod0] + [mod0.reset() for _ in range(ndraw - 1)]:
            P.append(m._brownians())
            Ls.append(np.array(m.seisPropLayers(refLayer=ref)[:6], float))
            rows.append(i)
            if (len(P) - 1) % 3 == 0:
                g = m.seisPropGrids(refLayer=ref)
                Gs.append(np.array(list(g[:6]) + [[GROUPS.index(x) for x in g[6]]], float))
                grid_of.append(len(P) - 1)
    pad = lambda arrs: np.stack([np.pad(a, ((0, 0), (0, max(b.shape[1] for b in arrs) - a.shape[1]))) for a in arrs])
    return dict(params=np.array(P), layers=pad(Ls), nlay=np.array([a.shape[1] for a in Ls]), grids=pad(Gs),
                ngrid=np.array([a.shape[1] for a in Gs]), grid_of=np.array(grid_of), rows=np.array(rows))


def save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    keys, table = LOCAL["moho"]
    cases = (("pairs", ZOO["pairs"], [None], 12), ("moho", ZOO["moho"], [dict(zip(keys, map(float, r))) for r in table], 3),
             ("ten_ref", ten_ref(), [None], 12))
    out = {"groups": np.array(GROUPS)}
    for name, setting, infos, ndraw in cases:
        d = capture(setting, infos, ndraw, seed=41)
        for k, v in d.items():
            out[f"{name}/{k}"] = v
        print(name, d["layers"].shape, np.unique(d["nlay"]), d["grids"].shape, np.unique(d["ngrid"]))
    save(os.path.join(HERE, "ref_zoo.npz"), out)
    print("wrote ref_zoo.npz")


if __name__ == "__main__":
    main()
