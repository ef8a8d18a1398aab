"""The ``hostlib`` fixture shared by the CPU tests of the device math: tests/hostcheck/hostcheck.hip (the SD_HD functions of
surfdisp_kernels.hip compiled for the host with hipcc) behind tests/hostcheck/run_hostcheck.py.  Skipped if hipcc is absent."""
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcheck")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def hostlib():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    so = os.path.join(HC, "libhostcheck.so")
    if os.environ.get("SURFDISP_HOSTCHECK_LIB"):               # sanitizer build (scripts/sanitize_cpu.sh): use as is
        sys.path.insert(0, HC)
        import run_hostcheck
        return run_hostcheck
    src = [os.path.join(HC, "hostcheck.hip"), os.path.join(HERE, "..", "pysurfinv_amd", "csrc", "surfdisp_kernels.hip")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in src):
        subprocess.check_call([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
                               "-I" + os.path.join(HERE, "..", "include"),
                               "-I" + os.path.join(HERE, "..", "pysurfinv_amd", "csrc"),
                               "-shared", "-o", so, src[0]], stderr=subprocess.DEVNULL)
    sys.path.insert(0, HC)
    import run_hostcheck
    return run_hostcheck
