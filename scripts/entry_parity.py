#!/usr/bin/env python3
"""GPU box: every forward entry of two builds of the library, compared as raw 32-bit words, and the return code and
surfdisp_last_error() text of one deliberately bad call per entry and kind of refusal (these return before any launch).

    entry_parity.py parent.so [candidate.so]     each library in processes of its own (candidate: the tree's); prints the
                                                 verdict, exit status 1 on a difference
    entry_parity.py --dump part out.npz          what those processes run, on the library SURFDISP_LIB_PATH names
                                                 (part: device | host; the host part reads SURFDISP_HOST_CHUNK / _SLOTS)

Device part: BatchPlan.run (plain, want_ratio, events, timed), run_kernels (both routes), run_group_kernels,
run_ellip_kernels, run_atten, run_eigen, run_thickness_kernels, run_group_thickness_kernels on a ragged 3 x L6 x P4 batch, the
sediment_R family of tests/golden/ref_families.npz, 256 x L10 x P20, 64 x L64 x P19 and the two batches of
tests/kernel_rows_ref.py that cross the 64-unit and 64-layer tile edges of the rows kernels (deep 130 x L70, tall 66 x L129, periods
10 / 30 / 100 s); both wave types; flags none / PHASE_ONLY / INDEPENDENT / PIPELINED / STRICT where the entry accepts them; forced
teams 0, 2, 16, 64.  Host part: surfdisp_forward_batch on one stack
(the arena path) and on 40 000 x L10 x P20 (chunked when SURFDISP_HOST_CHUNK=163840: three chunks)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TEAMS = (0, 2, 16, 64)


def shapes():
    from pysurfinv_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kernel_rows_ref as kr
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_families.npz"))
    tiles = np.array([10.0, 30.0, 100.0], np.float32)
    return {"deep": kr.deep_batch()[:1] + (tiles,) + kr.deep_batch()[1:], "tall": kr.tall_batch()[:1] + (tiles,) + kr.tall_batch()[1:],
            "ragged3": (synth.synth_models(3, 6, seed=5), synth.default_periods(4), np.array([6, 4, 2], np.int32)),
            "sediment": (z["sediment_R/model"], z["sediment_R/periods"].astype(np.float32), z["sediment_R/nlay"].astype(np.int32)),
            "b256": (synth.synth_models(256, 10, seed=11), synth.default_periods(20), None),
            "l64": (synth.synth_models(64, 64, seed=3), synth.default_periods(19), None)}


def dump_device(out):
    import torch
    from pysurfinv_amd import _lib, forward
    L = _lib.lib()
    flags = {"none": 0, "phase": _lib.PHASE_ONLY, "indep": _lib.INDEPENDENT, "pipe": _lib.PIPELINED, "strict": _lib.STRICT}
    res = {}

    def keep(key, tensors):
        for i, t in enumerate(tensors):
            if isinstance(t, torch.Tensor):
                res[f"{key}/{i}"] = t.contiguous().view(torch.int32).cpu().numpy().copy()
            elif t is not None:
                res[f"{key}/{i}"] = np.array([int(t)], np.int32)

    for sname, (m, per, nl) in shapes().items():
        B, _, Lm = m.shape
        dm, dp = torch.from_numpy(np.ascontiguousarray(m, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(per, np.float32)).cuda()
        dn = None if nl is None else torch.from_numpy(nl).cuda()
        plan = forward.BatchPlan(B, Lm, per.size)
        ring = forward.EventRing(1)
        for wave in (2, 1):
            for fname, f in flags.items():
                for team in TEAMS:
                    L.surfdisp_set_team(team)
                    k, key = wave | f, f"{sname}/w{wave}/{fname}/t{team}"
                    keep(key + "/run", plan.run(dm, dp, kind=k, nlay=dn))
                    keep(key + "/run2", plan.run(dm, dp, kind=k, nlay=dn, want_ratio=True))
                    keep(key + "/run_ev", plan.run(dm, dp, kind=k, nlay=dn, events=ring.slot(0)))
                    keep(key + "/run2_ev", plan.run(dm, dp, kind=k, nlay=dn, want_ratio=True, events=ring.slot(0)))
                    keep(key + "/timed", plan.run(dm, dp, kind=k, nlay=dn, _timed=True)[:3])
                    if fname == "phase":
                        continue
                    keep(key + "/kernels", plan.run_kernels(dm, dp, kind=k, nlay=dn))
                    keep(key + "/kernels_small", plan.run_kernels(dm, dp, kind=k, nlay=dn, small_workspace=True))
                    keep(key + "/group", plan.run_group_kernels(dm, dp, kind=k, nlay=dn))
                    keep(key + "/shifted", [plan.shifted_roots()])
                    if wave == 2 and fname != "strict":
                        keep(key + "/ellip", plan.run_ellip_kernels(dm, dp, kind=k, nlay=dn))
                    keep(key + "/atten", plan.run_atten(dm, dp, kind=k, nlay=dn))
                    keep(key + "/eigen", plan.run_eigen(dm, dp, kind=k, nlay=dn))
                    keep(key + "/thickness", plan.run_thickness_kernels(dm, dp, kind=k, nlay=dn))
                    keep(key + "/group_thickness", plan.run_group_thickness_kernels(dm, dp, kind=k, nlay=dn))
        L.surfdisp_set_team(0)
        torch.cuda.synchronize()
    res.update(bad_calls(L, _lib, torch))
    np.savez_compressed(out, **res)
    print("wrote", out, len(res), "arrays")


def bad_calls(L, _lib, torch):
    """name -> (return code, error text): per entry a null required pointer, a refused flag, the entry's own extra refusal, a bad
    shape or kind and a workspace one byte short or NULL.  Every output points at one scratch tensor: none of these calls reaches a launch."""
    B, Lm, P = 3, 6, 4
    scratch = torch.zeros(B * P * Lm * 8, dtype=torch.float32, device="cuda")
    ws = torch.zeros(int(L.surfdisp_ellip_kernels_workspace_bytes(B, Lm, P)) + int(L.surfdisp_group_kernels_workspace_bytes(B, Lm, P)),
                     dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(scratch.data_ptr())
    # entry -> (arguments between kind and workspace, index of a required pointer there, its size function, a refused flag)
    entries = {"surfdisp_forward_batch_device": (3, 0, "surfdisp_workspace_bytes", 0),
               "surfdisp_forward_batch_device2": (4, 0, "surfdisp_workspace_bytes", 0),
               "surfdisp_forward_kernels_device": (6, 3, "surfdisp_workspace_bytes", _lib.PHASE_ONLY),
               "surfdisp_forward_group_kernels_device": (10, 6, "surfdisp_group_kernels_workspace_bytes", _lib.KERN_REFCOORD),
               "surfdisp_forward_ellip_kernels_device": (11, 2, "surfdisp_ellip_kernels_workspace_bytes", _lib.STRICT),
               "surfdisp_forward_atten_device": (9, 6, "surfdisp_atten_workspace_bytes", _lib.PHASE_ONLY),
               "surfdisp_forward_eigen_device": (8, 3, "surfdisp_eigen_workspace_bytes", _lib.PHASE_ONLY),
               "surfdisp_forward_thickness_kernels_device": (9, 6, "surfdisp_thickness_kernels_workspace_bytes", _lib.KERN_REFCOORD)}
    out = {}
    for name, (nmid, req, size_fn, refused) in entries.items():
        need = int(getattr(L, size_fn)(B, Lm, P))

        def call(tag, kind=2, null=None, shape=(B, Lm, P), nbytes=need, dln=0.01, wsnull=False):
            mid = [p] * nmid
            if null is not None:
                mid[null] = None
            if name == "surfdisp_forward_group_kernels_device":
                mid = [ctypes.c_float(dln)] + mid
            rc = getattr(L, name)(None, shape[0], shape[1], None, p, shape[2], p, kind, *mid,
                                  None if wsnull else ctypes.c_void_p(ws.data_ptr()), nbytes)
            out[f"bad/{name}/{tag}"] = np.frombuffer(f"{rc} {L.surfdisp_last_error().decode()}".encode(), np.uint8).copy()

        call("null_pointer", null=req)
        if refused:
            call("refused_flag", kind=2 | refused)
        call("love_workspace_short", kind=1, nbytes=need - 1)                     # (the ellipticity entry: Rayleigh only)
        if name == "surfdisp_forward_group_kernels_device":
            call("dlnT", dln=0.5)
        call("bad_shape", shape=(B, 1, P))
        call("bad_kind", kind=3)
        call("workspace_short", nbytes=need - 1)
        call("workspace_null", wsnull=True)
    return out


def dump_host(out):
    from pysurfinv_amd import forward, synth
    res = {}
    per = synth.default_periods(20)
    for wave in (2, 1):
        one = synth.synth_models(1, 10, seed=2)
        big = synth.synth_models(40000, 10, seed=4)
        nl = (10 - (np.arange(40000) % 3)).astype(np.int32)
        for key, r in ((f"arena/w{wave}", forward.forward_batch(one, per, wave)),
                       (f"big/w{wave}", forward.forward_batch(big, per, wave)),
                       (f"big_nlay_phase/w{wave}", forward.forward_batch(big, per, wave | 0x10, nlay=nl))):
            for i, a in enumerate(r):
                res[f"host/{key}/{i}"] = np.ascontiguousarray(a).view(np.int32).copy()
    np.savez_compressed(out, **res)
    print("wrote", out, len(res), "arrays")


def compare(parent, cand):
    tmp = tempfile.mkdtemp(prefix="entry_parity_")                 # the dumps are large: each is removed once it is read
    parts = [("device", {}), ("host", dict(SURFDISP_HOST_PIPELINE="0")),
             ("host", dict(SURFDISP_HOST_CHUNK="163840", SURFDISP_HOST_SLOTS="2")),
             ("host", dict(SURFDISP_HOST_CHUNK="163840", SURFDISP_HOST_SLOTS="3"))]
    bad = 0
    for n, (part, extra) in enumerate(parts):
        files = []
        for side, lib in (("parent", parent), ("candidate", cand)):
            f = os.path.join(tmp, f"{side}_{n}.npz")
            env = dict(os.environ, **extra)
            if lib:
                env["SURFDISP_LIB_PATH"] = os.path.abspath(lib)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", part, f], env=env, check=True, timeout=420,
                           stdout=subprocess.DEVNULL)
            with np.load(f) as z:
                files.append({k: z[k] for k in z.files})
            os.remove(f)
        a, b = files
        assert sorted(a) == sorted(b), "the two libraries did not run the same calls"
        words = diff = texts = tdiff = 0
        for k in a:
            if k.startswith("bad/"):
                texts += 1
                if a[k].tobytes() != b[k].tobytes():
                    tdiff += 1
                    print("TEXT", k, a[k].tobytes(), b[k].tobytes())
            else:
                words += a[k].size
                d = int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else max(a[k].size, b[k].size)
                if d:
                    print("WORDS", k, d)
                diff += d
        print(f"{part} {extra or ''}: {len(a) - texts} arrays, {words} words, differing words {diff}; "
              f"bad calls {texts}, differing codes / texts {tdiff}")
        if part == "device":
            for k in sorted(a):
                if k.startswith("bad/"):
                    print("   ", k[4:], "->", a[k].tobytes().decode())
        bad += diff + tdiff
    os.rmdir(tmp)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--dump":
        {"device": dump_device, "host": dump_host}[sys.argv[2]](sys.argv[3])
    else:
        sys.exit(compare(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None))
