"""The one place where the tests compile a harness that includes the kernel sources (tests/hostcheck/*.hip,
tests/probe/secular_probe.hip) with hipcc.  A plain module: no fixtures, no pytest settings."""
import glob
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pysurfinv_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def sources(src):
    """What a harness is built from: itself, every csrc/*.hip and *.h (surfdisp_kernels.hip includes its first stages
    and the rows walk of its last ones as surfdisp_k_*.h, and the argument blocks live in surfdisp_internal.h) and the public header."""
    return [src, *glob.glob(os.path.join(CSRC, "*.hip")), *glob.glob(os.path.join(CSRC, "*.h")), os.path.join(INCLUDE, "surfdisp.h")]


def build(src, out, extra=(), opt="-O2", shared=True, quiet=True):
    """Compile the harness `src` to `out` (a shared library, or with shared=False an executable) unless `out` is newer than
    every file of sources(src); -> out.  Skips the calling test without hipcc.  A failed compilation raises with the
    compiler's messages in the text; quiet=False also passes on the warnings of a successful one."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in sources(src)):
        cmd = [HIPCC, opt, "-std=c++17", "--offload-arch=gfx950", *(["-fPIC"] if shared else []), *extra,
               "-I" + INCLUDE, "-I" + CSRC, *(["-shared"] if shared else []), "-o", out, src]
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)}\nfailed with exit status {r.returncode}:\n{r.stderr}")
        if not quiet:
            sys.stderr.write(r.stderr)
    return out
