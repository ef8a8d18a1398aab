#!/usr/bin/env python3
"""GPU box: run the cases of tests/scan_waits_cases.py with the library this process loads and save c, u and status.

    SURFDISP_LIB_PATH=/path/to/parent/libsurfdisp_hip.so python scripts/record_scan_waits_parent.py

records tests/golden/scan_waits_parent.npz: the outputs of a build of the PARENT commit (the commit before the lean scan
pass's guard took the half-space velocity from the evaluation), every launch with the team forced to two lanes, which
tests/test_scan_waits_gpu.py compares the library under test with, byte for byte.  The fixture is never recorded from the
code under test: without SURFDISP_LIB_PATH the script refuses to write into tests/golden.  With an output path as its
argument it writes there instead."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import scan_waits_cases as swc
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        if not os.environ.get("SURFDISP_LIB_PATH"):
            sys.exit("set SURFDISP_LIB_PATH to a build of the parent commit: the fixture is not recorded from the code under test")
        path = os.path.join(ROOT, "tests", "golden", "scan_waits_parent.npz")
    out = swc.run_all()
    np.savez_compressed(path, **out)
    solved = sum(int((v > 0).sum()) for k, v in out.items() if k.endswith("_c"))
    teams = sorted({int(v[0]) for k, v in out.items() if k.endswith("_team")})
    print(f"{len(out) // 4} cases, lanes per stack {teams}, {solved} solved (stack, period) units -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
