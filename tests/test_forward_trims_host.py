"""CPU checks of the two trims of the group-velocity kernel that move work without changing a value (surfdisp_kernels.hip),
through the stand-alone host program tests/hostcheck/trimscheck.hip:

  * LStash: group_rayleigh with a stash buffer (the fit's per-layer values kept for the later sweeps) against
    group_rayleigh without one - U and the sixteen debug words (surface vectors, fit, energy integrals) byte for byte, on
    bench-like ten-layer stacks at 8, 30 and 100 s (8 s drops layers), a two-layer stack, water-topped stacks and
    high-contrast stacks, some of which redo the fit in the reference's split (own -> false) and some of which take the
    robust path (the step-by-step second fit).  The program also counts the sweeps: with a buffer every MODE 1 / MODE 2
    sweep takes the kept values, without one none does, and both make the same sweeps.
  * the no-drop shortcut (group_no_cut) against the walk (drop_group) on 120 000 random (stack, c, T) of both wave types:
    wherever the shortcut fires the walk returns {n - 1, 0}; at least a quarter of the cases fire it, at least a quarter
    do not, and cases with the total thickness within 2e-4 of 4 c T lie on either side.

No GPU needed; skipped if hipcc is absent."""
import os
import re
import subprocess

import numpy as np
import pytest

import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcheck")
SRC = os.path.join(HC, "trimscheck.hip")
EXE = os.path.join(HC, "trimscheck")


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build(SRC, EXE, shared=False)


def _oracle(model, nlay, per):
    """the oracle's Rayleigh c and ellipticity per stack (each stack its own layer count)"""
    import ctypes
    from oracle import cport
    O = cport.lib()
    B = model.shape[0]; P = len(per)
    c = np.zeros((B, P), np.float32); u = np.zeros((B, P), np.float32); r = np.zeros((B, P), np.float32)
    fpf = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for i in range(B):
        m = np.ascontiguousarray(model[i, :, :nlay[i]])
        O.surfdisp_oracle_forward_dbg(int(nlay[i]), 2, fpf(m[0]), fpf(m[1]), fpf(m[2]), fpf(m[3]), fpf(m[4]),
                                      fpf(per), P, fpf(c[i]), fpf(u[i]), fpf(r[i]))
    return c, r


def _stash_cases():
    from pysurfinv_amd import synth
    rng = np.random.default_rng(31)
    bench = synth.synth_models(4, 10, seed=0)
    two = synth.synth_models(2, 2, seed=1)
    wet = synth.water_models(3, seed=5)
    B, L = 48, 10                                            # high contrast: Vs in random order, thick layers (tests/test_group_split.py)
    vs = rng.uniform(1.5, 4.8, (B, L)); vp = vs * rng.uniform(1.6, 2.2, (B, L)); h = rng.uniform(2.0, 60.0, (B, L))
    hc = np.stack([vp, vs, 0.541 + 0.3601 * vp, h, 1.0 / np.where(vs < 4.0, 600.0, 150.0)], axis=1).astype(np.float32)
    t3 = np.array([8.0, 30.0, 100.0], np.float32)
    return {"bench": (bench, t3), "two_layers": (two, t3), "water": (wet, t3),
            "high_contrast": (hc, np.geomspace(2.0, 100.0, 10).astype(np.float32))}


def _parse(line):
    t = line.split()
    d = {"b": int(t[1]), "k": int(t[2])}
    for key, val in zip(t[3::2], t[4::2]):
        d[key] = int(val, 16) if key == "u" else int(val)
    return d


@pytest.mark.parametrize("case", ["bench", "two_layers", "water", "high_contrast"])
def test_stash_equals_recompute_bit_for_bit(exe, tmp_path, case):
    model, per = _stash_cases()[case]
    model = np.ascontiguousarray(model, np.float32)
    B, _, L = model.shape
    nlay = np.full(B, L, np.int32)
    c, r = _oracle(model, nlay, per)
    path = str(tmp_path / "in.txt")
    with open(path, "w") as fh:
        fh.write(f"{B} {L} {len(per)}\n")
        fh.write(" ".join("%d" % v for v in nlay) + "\n")
        for a in (model, per, c, r):
            fh.write(" ".join("%.9g" % v for v in a.ravel()) + "\n")
    p = subprocess.run([exe, "stash", path], capture_output=True, text=True, timeout=300)
    rows = [_parse(ln) for ln in p.stdout.splitlines() if ln.startswith("unit ")]
    solved = int((c > 0).sum())
    print(f"{case}: {len(rows)} units of {c.size} ({solved} with a root); refit in the reference's split "
          f"{sum(r_['ref_split_fits'] > 0 and r_['mode1'] == 0 for r_ in rows)}, robust path {sum(r_['mode1'] > 0 for r_ in rows)}, "
          f"layers dropped {sum(r_['hs'] < L - 1 for r_ in rows)}")
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert len(rows) == solved and solved >= (0.25 if case == "high_contrast" else 0.99) * c.size
    assert all(r_["same"] == 1 and r_["sweeps"] == 1 for r_ in rows)
    assert all(r_["kept"] == r_["mode1"] + r_["mode2"] and r_["mode2"] == 1 for r_ in rows)
    if case == "bench":                                      # 8 s drops layers, 30 s and 100 s do not
        by_k = {k: [r_["hs"] for r_ in rows if r_["k"] == k] for k in range(3)}
        assert all(h < L - 1 for h in by_k[0]) and all(h == L - 1 for h in by_k[1] + by_k[2])
    if case == "high_contrast":
        # fast path with the fit redone in the reference's split (own -> false): two MODE 0 fits, the second not its own
        assert sum(r_["fits"] == 2 and r_["ref_split_fits"] == 1 and r_["mode1"] == 0 for r_ in rows) >= 1
        # robust path: the step-by-step second fit reads the kept values too
        assert sum(r_["mode1"] >= 1 for r_ in rows) >= 1


def test_no_drop_shortcut_agrees_with_the_walk(exe):
    p = subprocess.run([exe, "drop", "120000", "7"], capture_output=True, text=True, timeout=300)
    print(p.stdout.strip())
    t = p.stdout.split()
    d = dict(zip(t[1::2], map(int, t[2::2])))
    assert p.returncode == 0 and d["violations"] == 0, p.stdout + p.stderr
    assert d["cases"] >= 100000
    assert d["fired"] >= d["cases"] / 4 and d["not_fired"] >= d["cases"] / 4
    assert d["near_below"] >= 1000 and d["near_above"] >= 1000
    assert d["walk_cuts"] >= d["cases"] / 10                 # the walk does cut on a good share of the rest
