#!/usr/bin/env python3
"""Parses the apparent quality factors of the reference's sensitivity-kernel toolkit (data files of its known-answer
test, ``senskernel-1.0/TEST1/test.{R,L}.att``) into tests/golden/test1_eus_att.npz.  Each file holds two blocks of ten
rows ``period  Q_apparent`` (T = 10..100 s) separated by blank lines: mode 0 first, then mode 1.  Both blocks are stored;
the tests use mode 0 (this library solves the fundamental mode).  The model is ``eus_model`` = tests/golden/test1_eus.npz.

    python tests/golden/make_golden_att.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
T1 = "/root/reference/senskernel-1.0/TEST1"


def blocks(path):
    out, cur = [], []
    for ln in open(path):
        f = ln.split()
        if f:
            cur.append([float(x) for x in f])
        elif cur:
            out.append(cur); cur = []
    if cur:
        out.append(cur)
    return [np.array(b) for b in out]


def main():
    out = {}
    for w in ("R", "L"):
        b = blocks(os.path.join(T1, f"test.{w}.att"))
        assert len(b) == 2 and all(x.shape == (10, 2) for x in b), [x.shape for x in b]
        assert np.array_equal(b[0][:, 0], b[1][:, 0])
        out.setdefault("periods", b[0][:, 0])
        assert np.array_equal(out["periods"], b[0][:, 0])
        out[f"Q_{w}"] = np.stack([b[0][:, 1], b[1][:, 1]])        # [mode 0, mode 1][period]
        print(w, "mode 0", out[f"Q_{w}"][0].round(3))
    np.savez_compressed(os.path.join(HERE, "test1_eus_att.npz"), **out)


if __name__ == "__main__":
    main()
