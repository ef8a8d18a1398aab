#!/usr/bin/env python3
"""GPU box: how many units (lanes) and wavefronts of the Rayleigh group kernel restart their fast fit (xtest >= 1e-5,
group_rayleigh), on the bench batch (65 536 x L10 x P20, seed 0).  Needs the development build
`make -C pysurfinv_amd/csrc variant EXTRA=-DSD_COUNT_RESTARTS`, loaded with SURFDISP_LIB_PATH=<that .so>."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pysurfinv_amd import _lib, forward, synth  # noqa: E402

L = _lib.lib()
if not hasattr(L, "surfdisp_dev_restart_count"):
    raise SystemExit("this library was not built with -DSD_COUNT_RESTARTS")
cnt = (ctypes.c_ulonglong * 2)()
B, NL, P = 65536, 10, 20
model = torch.from_numpy(synth.synth_models(B, NL, seed=0)).to("cuda:0")
per = torch.from_numpy(synth.default_periods(P)).to("cuda:0")
assert L.surfdisp_dev_restart_count(cnt, 1) == 0                # clear
c, u, st = forward.forward_batch_torch(model, per, kind=2)
torch.cuda.synchronize()
assert L.surfdisp_dev_restart_count(cnt, 0) == 0
units = int((c > 0).sum())
print(f"restart count: {cnt[0]} of {units} solved units restart, in {cnt[1]} of {B * P // 64} wavefronts")
