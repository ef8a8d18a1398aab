"""Host side of the forward-call boundary (reference layer L2, models.py:11-33).

* ``_calForward`` mirrors ``pySurfInv.models._calForward`` (same name, arguments,
  return value and failure convention) on top of the HIP library.
* ``forward_batch`` / ``forward_batch_torch`` are the batched entry points the
  reference does not have: B layer stacks -> c[B,P], U[B,P] in one launch.

numpy / torch are plumbing only; the arithmetic is in libsurfdisp_hip.so.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from . import fast_surf as _fast_surf_mod


def _calForward(inProfile, wavetype="Ray", periods=(5, 10, 20, 40, 60, 80), debug=False):
    """models.py:11-33: profile rows (h, Vs, Vp, rho, qs, qp) -> cR[:nper] or None."""
    if wavetype == "Ray":
        ilvry = 2
    elif wavetype == "Love":
        ilvry = 1
    else:
        raise ValueError("Wrong surface wave type: %s!" % wavetype)
    inProfile = np.asarray(inProfile)
    ind = np.where(inProfile[0] > 1e-3)[0]                 # models.py:20
    h, Vs, Vp, rho, qs, qp = inProfile[:, ind]
    qsinv = 1.0 / qs
    nper = len(periods)
    per = np.zeros(200, dtype=np.float64)
    per[:nper] = periods[:]
    nlay = h.size
    (ur0, ul0, cr0, cl0) = _fast_surf_mod.fast_surf(nlay, ilvry, Vp, Vs, rho, h, qsinv, per, nper)
    if np.any(cr0[:nper] < 0.01):                          # models.py:29 (yes: cr0 for Love too)
        if debug:
            print(cr0[:nper])
        return None
    return cr0[:nper]


def forward_batch(model, periods, kind=2, nlay=None, device=0, independent=False, fast_scan=False, strict=False):
    """model float32 [B,5,L] rows (vp, vs, rho, h, qsinv) -> (c[B,P], u[B,P], status[B]).

    Host buffers in, host buffers out (C ABI surfdisp_forward_batch).  ``independent=True`` ORs
    SURFDISP_INDEPENDENT into ``kind`` (one team per (stack, period); see include/surfdisp.h).
    The scan evaluates every 0.01 km/s grid point as the reference does; ``fast_scan=True`` opts into the
    count-guided coarse-to-fine scan (SURFDISP_FASTSCAN); ``strict=True`` solves every stack with the kernel that restates
    the reference's arithmetic statement by statement (SURFDISP_STRICT: a verification mode, several times slower)."""
    if independent:
        kind = int(kind) | _lib.INDEPENDENT
    if strict:
        kind = int(kind) | _lib.STRICT
    if fast_scan:                                  # opt-in count-guided scan (SURFDISP_FASTSCAN); default: every grid point
        kind = int(kind) | _lib.FASTSCAN
    L = _lib.lib()
    model = np.ascontiguousarray(model, dtype=np.float32)
    if model.ndim != 3 or model.shape[1] != 5:
        raise ValueError("model must be [B, 5, L]")
    B, _, Lmax = model.shape
    per = np.ascontiguousarray(periods, dtype=np.float32).ravel()
    P = per.size
    c = np.zeros((B, P), np.float32); u = np.zeros((B, P), np.float32)
    status = np.zeros(B, np.int32)
    fp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ip = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    nl = None
    if nlay is not None:
        nlay = np.ascontiguousarray(nlay, dtype=np.int32)
        if nlay.size != B:
            raise ValueError("nlay must have B entries")
        nl = ip(nlay)
    _lib.check(L.surfdisp_forward_batch(int(device), B, Lmax, nl, fp(model), P, fp(per), int(kind),
                                        fp(c), fp(u), ip(status)))
    return c, u, status


class BatchPlan:
    """Device-resident, stream-ordered batched solve on torch tensors.

    Owns the workspace and output tensors for a fixed (B, L, P); ``run`` launches the
    three kernels on torch's current stream without allocating or synchronising, so it
    can be captured in a HIP graph."""

    def __init__(self, B, L, P, device="cuda:0"):
        import torch
        self.torch = torch
        self.B, self.L, self.P = int(B), int(L), int(P)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SurfdispError("BatchPlan needs a HIP device tensor (no CPU fallback)")
        lib = _lib.lib()
        self.ws_bytes = int(lib.surfdisp_workspace_bytes(self.B, self.L, self.P))
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self.c = torch.zeros(self.B, self.P, dtype=torch.float32, device=self.device)
        self.u = torch.zeros(self.B, self.P, dtype=torch.float32, device=self.device)
        self.status = torch.zeros(self.B, dtype=torch.int32, device=self.device)

    def run_timed(self, model, periods, kind=2, nlay=None, independent=False):
        """As run(), but blocks and also returns the (prep, phase, group) kernel durations in ms,
        measured with HIP events on the launch stream (surfdisp_forward_batch_device_timed)."""
        return self.run(model, periods, kind=kind, nlay=nlay, _timed=True, independent=independent)

    def run(self, model, periods, kind=2, nlay=None, _timed=False, independent=False, events=None,
            pipelined=False, fast_scan=False, strict=False, want_ratio=False):
        """Launch the kernels on torch's current stream (no allocation, no sync).  ``events``: an
        ``EventRing`` slot (4 HIP events recorded on the launch stream around the kernels).
        ``pipelined``: the caller keeps a second batch in flight on another stream
        (``SURFDISP_PIPELINED``: a launch hint, same results)."""
        torch = self.torch
        if independent:
            kind = int(kind) | _lib.INDEPENDENT
        if pipelined:
            kind = int(kind) | _lib.PIPELINED
        if fast_scan:                                  # opt-in count-guided scan (SURFDISP_FASTSCAN)
            kind = int(kind) | _lib.FASTSCAN
        if strict:                                     # verification mode (SURFDISP_STRICT): the exact kernel for every stack
            kind = int(kind) | _lib.STRICT
        for t, shape in ((model, (self.B, 5, self.L)), (periods, (self.P,))):
            if (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape
                    or t.device != self.device):
                raise ValueError(f"expected contiguous float32 {shape} on {self.device}")
        if nlay is not None and (nlay.dtype != torch.int32 or nlay.numel() != self.B
                                 or nlay.device != self.device):
            raise ValueError("nlay must be int32 [B] on the same device")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._last_ws = self.workspace
        args = [ctypes.c_void_p(stream), self.B, self.L,
                ctypes.c_void_p(nlay.data_ptr() if nlay is not None else 0),
                ctypes.c_void_p(model.data_ptr()), self.P, ctypes.c_void_p(periods.data_ptr()),
                int(kind), ctypes.c_void_p(self.c.data_ptr()), ctypes.c_void_p(self.u.data_ptr()),
                ctypes.c_void_p(self.status.data_ptr()), ctypes.c_void_p(self.workspace.data_ptr()),
                self.ws_bytes]
        with torch.cuda.device(self.device):
            if _timed:
                ms = (ctypes.c_float * 3)()
                rc = _lib.lib().surfdisp_forward_batch_device_timed(*args, ms)
                _lib.check(rc)
                return self.c, self.u, self.status, tuple(float(x) for x in ms)
            if want_ratio:
                # ABI 3: also the Rayleigh ellipticity (the reference's COMMON /o/ ratio, calcul.f:195) -> self.ratio [B, P]
                if getattr(self, "ratio", None) is None:
                    self.ratio = torch.zeros(self.B, self.P, dtype=torch.float32, device=self.device)
                a2 = args[:10] + [ctypes.c_void_p(self.ratio.data_ptr())] + args[10:]
                if events is not None:
                    rc = _lib.lib().surfdisp_forward_batch_device2_events(*a2, events)
                else:
                    rc = _lib.lib().surfdisp_forward_batch_device2(*a2)
            elif events is not None:
                rc = _lib.lib().surfdisp_forward_batch_device_events(*args, events)
            else:
                rc = _lib.lib().surfdisp_forward_batch_device(*args)
        _lib.check(rc)
        if want_ratio:
            return self.c, self.u, self.status, self.ratio
        return self.c, self.u, self.status


    def fallback_count(self):
        """Stacks of the last ``run`` that the production root search handed to the exact fallback kernel
        (``surfdisp_workspace_fallback_count``; synchronises the current stream)."""
        n = ctypes.c_int(0)
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        with self.torch.cuda.device(self.device):
            _lib.check(_lib.lib().surfdisp_workspace_fallback_count(ctypes.c_void_p(stream), ctypes.c_void_p(getattr(self, '_last_ws', self.workspace).data_ptr()),
                                                                    self.B, self.L, self.P, ctypes.byref(n)))
        return int(n.value)

    def counters(self):
        """(stacks through the exact fallback kernel, brackets refined with NEVILL by the phase test, ellipticities evaluated
        again with the reference's arithmetic) of the last solve (``surfdisp_workspace_counters``; synchronises the stream)."""
        n = (ctypes.c_int * 3)()
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        with self.torch.cuda.device(self.device):
            _lib.check(_lib.lib().surfdisp_workspace_counters(ctypes.c_void_p(stream), ctypes.c_void_p(getattr(self, '_last_ws', self.workspace).data_ptr()),
                                                              self.B, self.L, self.P, n))
        return tuple(int(x) for x in n)

    def run_kernels(self, model, periods, kind=2, nlay=None, want_vp=True, want_rho=True, small_workspace=False):
        """Forward solve + analytic partial derivatives of the phase velocity
        (``surfdisp_forward_kernels_device``): returns (c, u, status, dcdb, dcda, dcdr) with the
        partials float32 [B, P, L] = d c(period) / d (Vs | Vp | rho) of input layer i (``None`` where
        not requested; Love has no dcda).  Same launch as ``run`` plus per-layer sums in the
        group-velocity kernel - what ``SensKernelPert`` obtains from 2L+1 perturbed solves."""
        torch = self.torch
        for t, shape in ((model, (self.B, 5, self.L)), (periods, (self.P,))):
            if (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape
                    or t.device != self.device):
                raise ValueError(f"expected contiguous float32 {shape} on {self.device}")
        if nlay is not None and (nlay.dtype != torch.int32 or nlay.numel() != self.B
                                 or nlay.device != self.device):
            raise ValueError("nlay must be int32 [B] on the same device")
        mk = lambda: torch.empty((self.B, self.P, self.L), dtype=torch.float32, device=self.device)
        dcdb = mk()
        dcda = mk() if (want_vp and (int(kind) & 3) == _lib.KIND_RAYLEIGH) else None
        dcdr = mk() if want_rho else None
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if small_workspace:                            # the direct route into the rows (tests compare the two)
            ws, ws_bytes = self.workspace, self.ws_bytes
        else:
            if getattr(self, "kworkspace", None) is None:      # + the layer-major scratch of the partials, kept for reuse
                self.kws_bytes = int(_lib.lib().surfdisp_kernels_workspace_bytes(self.B, self.L, self.P))
                self.kworkspace = torch.empty(self.kws_bytes, dtype=torch.uint8, device=self.device)
            ws, ws_bytes = self.kworkspace, self.kws_bytes
        self._last_ws = ws
        with torch.cuda.device(self.device):
            rc = _lib.lib().surfdisp_forward_kernels_device(
                ctypes.c_void_p(stream), self.B, self.L, ptr(nlay), ptr(model), self.P, ptr(periods), int(kind),
                ptr(self.c), ptr(self.u), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr),
                ptr(ws), ws_bytes)
        _lib.check(rc)
        return self.c, self.u, self.status, dcdb, dcda, dcdr

    def run_group_kernels(self, model, periods, kind=2, nlay=None, dlnT_frac=0.01, want_vp=True, want_rho=True, count=True):
        """``run_kernels`` plus the analytic partials of the GROUP velocity (``surfdisp_forward_group_kernels_device``):
        returns (c, u, status, dcdb, dcda, dcdr, dudb, duda, dudr, n_failed).  c .. dcdr equal ``run_kernels``' bit for bit;
        dudb / duda / dudr float32 [B, P, L] = d U(period) / d (Vs | Vp | rho) of input layer i (``None`` where not
        requested; Love has no duda), from the phase partials at T (1 -+ dlnT_frac).  Rows of unsolved periods are zeros,
        rows of units whose shifted root failed are NaN; ``n_failed`` (int, synchronises the stream) counts the latter
        (``count=False``: the device tensor itself, no synchronisation)."""
        torch = self.torch
        for t, shape in ((model, (self.B, 5, self.L)), (periods, (self.P,))):
            if (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape
                    or t.device != self.device):
                raise ValueError(f"expected contiguous float32 {shape} on {self.device}")
        if nlay is not None and (nlay.dtype != torch.int32 or nlay.numel() != self.B
                                 or nlay.device != self.device):
            raise ValueError("nlay must be int32 [B] on the same device")
        mk = lambda: torch.empty((self.B, self.P, self.L), dtype=torch.float32, device=self.device)
        rayleigh = (int(kind) & 3) == _lib.KIND_RAYLEIGH
        dcdb, dudb = mk(), mk()
        dcda, duda = (mk(), mk()) if (want_vp and rayleigh) else (None, None)
        dcdr, dudr = (mk(), mk()) if want_rho else (None, None)
        if getattr(self, "gworkspace", None) is None:          # kept for reuse, as run_kernels' workspace
            self.gws_bytes = int(_lib.lib().surfdisp_group_kernels_workspace_bytes(self.B, self.L, self.P))
            self.gworkspace = torch.empty(self.gws_bytes, dtype=torch.uint8, device=self.device)
            self.nfail = torch.zeros(1, dtype=torch.int32, device=self.device)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._last_ws = self.gworkspace
        with torch.cuda.device(self.device):
            rc = _lib.lib().surfdisp_forward_group_kernels_device(
                ctypes.c_void_p(stream), self.B, self.L, ptr(nlay), ptr(model), self.P, ptr(periods), int(kind),
                float(dlnT_frac), ptr(self.c), ptr(self.u), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr),
                ptr(dudb), ptr(duda), ptr(dudr), ptr(self.nfail), ptr(self.gworkspace), self.gws_bytes)
        _lib.check(rc)
        return self.c, self.u, self.status, dcdb, dcda, dcdr, dudb, duda, dudr, int(self.nfail.item()) if count else self.nfail

    def run_ellip_kernels(self, model, periods, kind=2, nlay=None, want_vp=True, want_rho=True, count=True):
        """``run_kernels`` plus the Rayleigh ellipticity and its analytic partials (``surfdisp_forward_ellip_kernels_device``):
        returns (c, u, status, ratio, dcdb, dcda, dcdr, dedb, deda, dedr, n_nonfinite).  c .. dcdr equal ``run_kernels``' bit
        for bit, ratio [B, P] is ``run(want_ratio=True)``'s; dedb / deda / dedr float32 [B, P, L] = d chi(period) / d (Vs | Vp |
        rho) of input layer i (``None`` where not requested).  Rows of unsolved periods, water layers and layers below the half
        space are zeros, rows of units whose result is not finite are NaN; ``n_nonfinite`` (int, synchronises the stream)
        counts the latter (``count=False``: the device tensor itself, no synchronisation).  Rayleigh only."""
        torch = self.torch
        if (int(kind) & 3) != _lib.KIND_RAYLEIGH:
            raise ValueError("run_ellip_kernels: Rayleigh only (kind=2); Love waves have no ellipticity")
        for t, shape in ((model, (self.B, 5, self.L)), (periods, (self.P,))):
            if (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape
                    or t.device != self.device):
                raise ValueError(f"expected contiguous float32 {shape} on {self.device}")
        if nlay is not None and (nlay.dtype != torch.int32 or nlay.numel() != self.B
                                 or nlay.device != self.device):
            raise ValueError("nlay must be int32 [B] on the same device")
        mk = lambda: torch.empty((self.B, self.P, self.L), dtype=torch.float32, device=self.device)
        dcdb, dedb = mk(), mk()
        dcda, deda = (mk(), mk()) if want_vp else (None, None)
        dcdr, dedr = (mk(), mk()) if want_rho else (None, None)
        ratio = torch.empty((self.B, self.P), dtype=torch.float32, device=self.device)
        if getattr(self, "eworkspace", None) is None:          # kept for reuse, as run_kernels' workspace
            self.ews_bytes = int(_lib.lib().surfdisp_ellip_kernels_workspace_bytes(self.B, self.L, self.P))
            self.eworkspace = torch.empty(self.ews_bytes, dtype=torch.uint8, device=self.device)
            self.nnonfin = torch.zeros(1, dtype=torch.int32, device=self.device)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._last_ws = self.eworkspace
        with torch.cuda.device(self.device):
            rc = _lib.lib().surfdisp_forward_ellip_kernels_device(
                ctypes.c_void_p(stream), self.B, self.L, ptr(nlay), ptr(model), self.P, ptr(periods), int(kind),
                ptr(self.c), ptr(self.u), ptr(ratio), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr),
                ptr(dedb), ptr(deda), ptr(dedr), ptr(self.nnonfin), ptr(self.eworkspace), self.ews_bytes)
        _lib.check(rc)
        return (self.c, self.u, self.status, ratio, dcdb, dcda, dcdr, dedb, deda, dedr, int(self.nnonfin.item()) if count else self.nnonfin)

    def run_atten(self, model, periods, kind=2, nlay=None, want_vp=True, want_rho=True, want_kernel=True, want_gamma=True):
        """``run_kernels`` plus the apparent attenuation of the mode (``surfdisp_forward_atten_device``): returns (c, u, status,
        dcdb, dcda, dcdr, qinv, gamma, dqdq).  c .. dcdr equal ``run_kernels``' bit for bit; qinv [B, P] = 1 / Q_apparent
        (calcul.f:256-265, 341-349: what the reference forms from its partials and the layers' 1/Qs and never returns),
        gamma [B, P] the attenuation coefficient in 1/km, dqdq float32 [B, P, L] = d qinv / d (1/Qs of layer i) at fixed
        eigenfunction (``None`` with ``want_kernel=False``; gamma ``None`` with ``want_gamma=False``).  Unsolved periods and
        bad stacks are zeros, as are water layers and layers below the half space in dqdq.  Rayleigh and Love."""
        torch = self.torch
        for t, shape in ((model, (self.B, 5, self.L)), (periods, (self.P,))):
            if (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape
                    or t.device != self.device):
                raise ValueError(f"expected contiguous float32 {shape} on {self.device}")
        if nlay is not None and (nlay.dtype != torch.int32 or nlay.numel() != self.B
                                 or nlay.device != self.device):
            raise ValueError("nlay must be int32 [B] on the same device")
        mk = lambda: torch.empty((self.B, self.P, self.L), dtype=torch.float32, device=self.device)
        mk2 = lambda: torch.empty((self.B, self.P), dtype=torch.float32, device=self.device)
        dcdb = mk()
        dcda = mk() if (want_vp and (int(kind) & 3) == _lib.KIND_RAYLEIGH) else None
        dcdr = mk() if want_rho else None
        qinv = mk2()
        gamma = mk2() if want_gamma else None
        dqdq = mk() if want_kernel else None
        if getattr(self, "aworkspace", None) is None:          # kept for reuse, as run_kernels' workspace
            self.aws_bytes = int(_lib.lib().surfdisp_atten_workspace_bytes(self.B, self.L, self.P))
            self.aworkspace = torch.empty(self.aws_bytes, dtype=torch.uint8, device=self.device)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._last_ws = self.aworkspace
        with torch.cuda.device(self.device):
            rc = _lib.lib().surfdisp_forward_atten_device(
                ctypes.c_void_p(stream), self.B, self.L, ptr(nlay), ptr(model), self.P, ptr(periods), int(kind),
                ptr(self.c), ptr(self.u), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr),
                ptr(qinv), ptr(gamma), ptr(dqdq), ptr(self.aworkspace), self.aws_bytes)
        _lib.check(rc)
        return self.c, self.u, self.status, dcdb, dcda, dcdr, qinv, gamma, dqdq

    def run_eigen(self, model, periods, kind=2, nlay=None, want_uz=True, want_tz=True, want_tr=True, want_energy=True):
        """``run`` plus the mode's eigenfunction at the top of every input layer and its energy integrals
        (``surfdisp_forward_eigen_device``): returns (c, u, status, ur, uz, tz, tr, energy).  c, u, status equal ``run``'s bit
        for bit (``kind`` may carry the INDEPENDENT / STRICT / scan flags); ur, uz, tz, tr float32 [B, P, L] = horizontal and
        vertical displacement, normal and shear traction at the TOP of layer i of the earth-flattened, attenuation-corrected
        stack at the period (Love: ur the transverse displacement, tr the shear traction, uz and tz zeros), normalised to
        uz = 1 (Love ut = 1) at the top of the first solid layer; energy [B, P, 4] = (I0, I1, I2, 1 / (2 c U I0)).  Zeros below
        the unit's effective half space, beyond nlay, for unsolved periods and bad stacks.  ``None`` where not requested.
        The conventions are those of include/surfdisp.h section (5f)."""
        torch = self.torch
        for t, shape in ((model, (self.B, 5, self.L)), (periods, (self.P,))):
            if (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape
                    or t.device != self.device):
                raise ValueError(f"expected contiguous float32 {shape} on {self.device}")
        if nlay is not None and (nlay.dtype != torch.int32 or nlay.numel() != self.B
                                 or nlay.device != self.device):
            raise ValueError("nlay must be int32 [B] on the same device")
        mk = lambda: torch.empty((self.B, self.P, self.L), dtype=torch.float32, device=self.device)
        ur = mk()
        uz = mk() if want_uz else None
        tz = mk() if want_tz else None
        tr = mk() if want_tr else None
        energy = torch.empty((self.B, self.P, 4), dtype=torch.float32, device=self.device) if want_energy else None
        if getattr(self, "eigworkspace", None) is None:        # kept for reuse, as run_kernels' workspace
            self.eigws_bytes = int(_lib.lib().surfdisp_eigen_workspace_bytes(self.B, self.L, self.P))
            self.eigworkspace = torch.empty(self.eigws_bytes, dtype=torch.uint8, device=self.device)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._last_ws = self.eigworkspace
        with torch.cuda.device(self.device):
            rc = _lib.lib().surfdisp_forward_eigen_device(
                ctypes.c_void_p(stream), self.B, self.L, ptr(nlay), ptr(model), self.P, ptr(periods), int(kind),
                ptr(self.c), ptr(self.u), ptr(self.status), ptr(ur), ptr(uz), ptr(tz), ptr(tr), ptr(energy),
                ptr(self.eigworkspace), self.eigws_bytes)
        _lib.check(rc)
        return self.c, self.u, self.status, ur, uz, tz, tr, energy

    def run_thickness_kernels(self, model, periods, kind=2, nlay=None, want_vp=True, want_rho=True, want_dcdz=True, count=True):
        """``run_kernels`` plus the derivatives of the phase velocity with respect to the layer thicknesses and the interface
        depths (``surfdisp_forward_thickness_kernels_device``): returns (c, u, status, dcdb, dcda, dcdr, dcdh, dcdz,
        n_nonfinite).  c .. dcdr equal ``run_kernels``' bit for bit; dcdh float32 [B, P, L] = d c(period) / d (thickness of input
        layer i), everything below shifted rigidly - what a change of ``model[:, 3, i]`` does; dcdz [B, P, L] = d c(period) /
        d (depth of the top of layer j), the other interfaces fixed (``None`` with ``want_dcdz=False``); dcdh[i] = sum_{j>i}
        dcdz[j].  Zeros below a unit's effective half space, beyond nlay, for unsolved periods and bad stacks, in
        dcdh[nlay - 1] and dcdz[0]; rows of a unit with a value that is not finite are NaN and ``n_nonfinite`` (int,
        synchronises the stream; ``count=False``: the device tensor itself) counts them.  Rayleigh and Love; the
        conventions are those of include/surfdisp.h section (5g)."""
        torch = self.torch
        for t, shape in ((model, (self.B, 5, self.L)), (periods, (self.P,))):
            if (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape
                    or t.device != self.device):
                raise ValueError(f"expected contiguous float32 {shape} on {self.device}")
        if nlay is not None and (nlay.dtype != torch.int32 or nlay.numel() != self.B
                                 or nlay.device != self.device):
            raise ValueError("nlay must be int32 [B] on the same device")
        mk = lambda: torch.empty((self.B, self.P, self.L), dtype=torch.float32, device=self.device)
        dcdb, dcdh = mk(), mk()
        dcda = mk() if (want_vp and (int(kind) & 3) == _lib.KIND_RAYLEIGH) else None
        dcdr = mk() if want_rho else None
        dcdz = mk() if want_dcdz else None
        if getattr(self, "tworkspace", None) is None:          # kept for reuse, as run_kernels' workspace
            self.tws_bytes = int(_lib.lib().surfdisp_thickness_kernels_workspace_bytes(self.B, self.L, self.P))
            self.tworkspace = torch.empty(self.tws_bytes, dtype=torch.uint8, device=self.device)
            self.tnonfin = torch.zeros(1, dtype=torch.int32, device=self.device)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._last_ws = self.tworkspace
        with torch.cuda.device(self.device):
            rc = _lib.lib().surfdisp_forward_thickness_kernels_device(
                ctypes.c_void_p(stream), self.B, self.L, ptr(nlay), ptr(model), self.P, ptr(periods), int(kind),
                ptr(self.c), ptr(self.u), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr),
                ptr(dcdh), ptr(dcdz), ptr(self.tnonfin), ptr(self.tworkspace), self.tws_bytes)
        _lib.check(rc)
        return (self.c, self.u, self.status, dcdb, dcda, dcdr, dcdh, dcdz, int(self.tnonfin.item()) if count else self.tnonfin)

    def shifted_roots(self):
        """[2, B, P] float32: the roots at T (1 - dlnT_frac) and T (1 + dlnT_frac) the last ``run_group_kernels`` used (a unit's
        own c where it is unsolved or its shifted root failed) - a read-out of the workspace for tests."""
        off = int(_lib.lib().surfdisp_group_kernels_shift_offset(self.B, self.L, self.P))
        n = 2 * self.P * self.B * 4
        return self.gworkspace[off:off + n].view(self.torch.float32).view(2, self.P, self.B).transpose(1, 2).clone()


class EventRing:
    """n x 4 HIP events owned by the caller, recorded by ``BatchPlan.run(..., events=ring.slot(i))``
    on the launch stream; ``kernel_ms()`` (after the caller synchronised) returns the
    [n, 3] prep / root-search / group+finish durations in milliseconds."""

    def __init__(self, n):
        self.n = int(n)
        self._ev = (ctypes.c_void_p * (4 * self.n))()
        _lib.check(_lib.lib().surfdisp_events_create(4 * self.n, self._ev))

    def slot(self, i):
        return ctypes.cast(ctypes.byref(self._ev, 4 * (i % self.n) * ctypes.sizeof(ctypes.c_void_p)),
                           ctypes.POINTER(ctypes.c_void_p))

    def kernel_ms(self, used=None):
        out = np.zeros((self.n if used is None else used, 3))
        ms = ctypes.c_float()
        for i in range(out.shape[0]):
            for k in range(3):
                _lib.check(_lib.lib().surfdisp_events_elapsed_ms(self._ev[4 * i + k], self._ev[4 * i + k + 1],
                                                                 ctypes.byref(ms)))
                out[i, k] = ms.value
        return out

    def __del__(self):
        try:
            _lib.lib().surfdisp_events_destroy(4 * self.n, self._ev)
        except Exception:
            pass


def forward_batch_torch(model, periods, kind=2, nlay=None):
    """One-shot torch entry: allocates a BatchPlan and runs it (outputs stay on the device)."""
    B, _, L = model.shape
    plan = BatchPlan(B, L, periods.numel(), device=model.device)
    return plan.run(model, periods, kind=kind, nlay=nlay)


class JointPlan:
    """Rayleigh + Love, phase + group velocity of the same stacks (BASELINE configs[4] shape): two BatchPlans on two HIP
    streams.  ``order``: "concurrent" - both root searches share the chip from the start (each sized for half of it);
    "rayleigh_first" / "love_first" - the second wave type's kernels wait for the END OF THE FIRST ONE'S ROOT SEARCH
    (an event recorded between its kernels), so each root search has the whole chip and the first one's group-velocity
    kernel runs beside the second root search.  Outputs stay on the device: dict(cR, uR, cL, uL, statusR, statusL)."""

    def __init__(self, B, L, P, device="cuda:0", order=None):
        import os
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.order = order or os.environ.get("SURFDISP_JOINT_ORDER", "concurrent")
        if self.order not in ("concurrent", "concurrent_love", "rayleigh_first", "love_first"):
            raise ValueError("order: concurrent | concurrent_love | rayleigh_first | love_first")
        self.ray = BatchPlan(B, L, P, device=device)
        self.love = BatchPlan(B, L, P, device=device)
        self.s_ray = torch.cuda.Stream(device=self.device)
        self.s_love = torch.cuda.Stream(device=self.device)
        self._ring = EventRing(2)                   # own events when the caller brings none (ordering needs one)

    def run(self, model, periods, nlay=None, events=(None, None)):
        """``events``: (Rayleigh, Love) ``EventRing`` slots, recorded on each plan's own stream (measurement)."""
        torch = self.torch
        cur = torch.cuda.current_stream(self.device)
        for s in (self.s_ray, self.s_love):
            s.wait_stream(cur)                       # inputs were produced on the caller's stream
        evR = events[0] if events[0] is not None else self._ring.slot(0)
        evL = events[1] if events[1] is not None else self._ring.slot(1)
        conc = self.order in ("concurrent", "concurrent_love")      # (concurrent_love: the Love kernels are enqueued first)

        def ray():
            with torch.cuda.stream(self.s_ray):
                return self.ray.run(model, periods, kind=_lib.KIND_RAYLEIGH, nlay=nlay, pipelined=conc, events=evR)

        def love():
            with torch.cuda.stream(self.s_love):
                return self.love.run(model, periods, kind=_lib.KIND_LOVE, nlay=nlay, pipelined=conc, events=evL)

        def wait(stream, ev):                        # ev[2]: recorded after the root search of the other solve
            _lib.check(_lib.lib().surfdisp_stream_wait_event(ctypes.c_void_p(stream.cuda_stream), ev[2]))

        if self.order == "concurrent_love":
            cL, uL, sL = love()
            cR, uR, sR = ray()
        elif self.order == "love_first":
            cL, uL, sL = love()
            wait(self.s_ray, evL)
            cR, uR, sR = ray()
        else:
            cR, uR, sR = ray()
            if not conc:
                wait(self.s_love, evR)
            cL, uL, sL = love()
        cur.wait_stream(self.s_ray); cur.wait_stream(self.s_love)
        return dict(cR=cR, uR=uR, cL=cL, uL=uL, statusR=sR, statusL=sL)
