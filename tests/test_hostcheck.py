"""CPU-side check of the group-velocity DEVICE math: tests/hostcheck compiles the very functions
the group kernel runs (layer_derive, drop_group, make_prop/prop_apply, rayleigh_sweep,
group_rayleigh, group_love - marked __host__ __device__ in surfdisp_kernels.hip) for the host with
hipcc, and this test compares them with the oracle on the golden cases, fed with the oracle's own
c and ellipticity.  No GPU needed; skipped if hipcc is absent."""
import numpy as np
import pytest

from hostcheck_lib import hostlib  # noqa: F401  (fixture)


@pytest.mark.parametrize("case", ["synth_L5_R", "synth_L10_R", "synth_L21_R", "synth_L64_R", "water_L9_R",
                                  "two_layer_R", "rough_L10_R", "synth_L10_L", "synth_L64_L", "water_L9_L"])
def test_group_velocity_device_math_on_host(hostlib, ref_cases, case):
    d = ref_cases[case]
    per = np.ascontiguousarray(d["periods"], np.float32)
    c, u, r = hostlib.oracle_dbg(d["model"], per, d["kind"])
    uh = hostlib.host_group(d["model"], per, d["kind"], c, r)
    ok = u != 0
    assert ok.any()
    assert np.abs(uh[ok] / u[ok] - 1).max() < 5e-6
