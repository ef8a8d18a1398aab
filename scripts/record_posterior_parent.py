#!/usr/bin/env python3
"""Record what the PARENT commit computes for the cases of tests/test_posterior_parent_gpu.py (``run_parent_cases``: profiles,
sources and statistics entries of pysurfinv_amd.posterior), or compare two revisions of the numpy statements.

    python scripts/record_posterior_parent.py ROOT                 (GPU box)
        ROOT: a checkout of the parent commit with its own library built by its own Makefile.  ``pysurfinv_amd`` is imported from
        ROOT, the inputs come from this tree's tests/posterior_cases.py, and every tensor of every returned dict goes to
        tests/golden/posterior_parent.npz, which tests/test_posterior_parent_gpu.py compares the tree under test with, byte for byte.
        The fixture is never recorded from the code under test: without ROOT the script refuses.
    python scripts/record_posterior_parent.py --host OUT.npz [ROOT]     (CPU)
        ``posterior_reference`` on the carry track with a histogram under the three selections, and ``predictive_reference`` on
        the host fixture track with the oracle ``forward=`` hook and per-column ranges, of the ``pysurfinv_amd`` of ROOT (default:
        this tree), saved to OUT.npz.
    python scripts/record_posterior_parent.py --compare A.npz B.npz     (CPU)
        two such files word for word (keys, dtypes, shapes, bytes); exit status 1 if anything differs
        (profiles/posterior_refactor/host_parity.txt)."""
import os
import sys

import numpy as np

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def use_tree(root):
    """``pysurfinv_amd`` (and ``oracle``) from ``root``, the cases from this tree's tests/."""
    sys.path[:0] = [os.path.abspath(root), os.path.join(HERE_ROOT, "tests")]
    os.environ.pop("SURFDISP_LIB_PATH", None)            # the tree's own library
    import pysurfinv_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(pysurfinv_amd.__file__))) == os.path.abspath(root), pysurfinv_amd.__file__


def host_cases():
    import torch
    import posterior_cases as pc
    from pysurfinv_amd import posterior
    from pysurfinv_amd.layers_batch import Model1DBatch
    from pysurfinv_amd.mcmc import MetropolisBatch
    mb = Model1DBatch(pc.CONT)
    res = {}
    for s, sel in pc.SELECTIONS.items():
        res[f"posterior_reference_{s}"] = posterior.posterior_reference(mb, torch.from_numpy(pc._carry_track(mb)), pc.DEPTHS,
                                                                        hist=(1.0, 5.0, 40), **sel)
    obs = np.load(pc.POST_NPZ, allow_pickle=True)["obs"][()]
    P = len(obs["T"])
    mc = MetropolisBatch(mb.spec, mb.to_model, obs["T"], obs["c"], obs["uncer"], device="cpu",
                         forward=pc._oracle_forward(np.asarray(obs["T"], np.float32)))
    res["predictive_reference"] = posterior.predictive_reference(mc, torch.from_numpy(pc._track()),
                                                                 hist=(np.linspace(2.0, 3.0, P), np.linspace(4.0, 5.0, P), 50))
    return {f"{case}/{k}": v.numpy() for case, r in res.items() for k, v in r.items()}


def compare(a, b):
    A, B = dict(np.load(a)), dict(np.load(b))
    bad = [f"keys: {sorted(set(A) ^ set(B))}"] if set(A) != set(B) else []
    for k in sorted(set(A) & set(B)):
        x, y = A[k], B[k]
        same = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        print(f"{k:44s} {str(x.dtype):8s} {str(x.shape):14s} {'equal' if same else 'DIFFERS'}")
        if not same:
            bad.append(k)
    print(f"{len(A)} arrays of {a}, {len(B)} of {b}: " + ("FAILED: " + ", ".join(bad) if bad else "all equal word for word"))
    return 1 if bad else 0


def main():
    args = sys.argv[1:]
    if args[:1] == ["--compare"]:
        sys.exit(compare(args[1], args[2]))
    if args[:1] == ["--host"]:
        use_tree(args[2] if len(args) > 2 else HERE_ROOT)
        out, path = host_cases(), args[1]
    else:
        if not args or os.path.abspath(args[0]) == HERE_ROOT:
            sys.exit("give the root of a checkout of the parent commit (library built): the fixture is not recorded from the code under test")
        use_tree(args[0])
        import test_posterior_parent_gpu as cases
        out, path = cases.run_parent_cases(), os.path.join(HERE_ROOT, "tests", "golden", "posterior_parent.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
