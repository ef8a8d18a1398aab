"""The ``hostlib`` fixture shared by the CPU tests of the device math: tests/hostcheck/hostcheck.hip (the SD_HD functions of
surfdisp_kernels.hip compiled for the host with hipcc) behind tests/hostcheck/run_hostcheck.py.  Skipped if hipcc is absent."""
import os
import sys

import pytest

import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcheck")


@pytest.fixture(scope="module")
def hostlib():
    if not os.path.exists(hostbuild.HIPCC):
        pytest.skip("hipcc not available")
    so = os.path.join(HC, "libhostcheck.so")
    if os.environ.get("SURFDISP_HOSTCHECK_LIB"):               # sanitizer build (scripts/sanitize_cpu.sh): use as is
        sys.path.insert(0, HC)
        import run_hostcheck
        return run_hostcheck
    hostbuild.build(os.path.join(HC, "hostcheck.hip"), so)
    sys.path.insert(0, HC)
    import run_hostcheck
    return run_hostcheck
