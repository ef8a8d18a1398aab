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

    # entry name -> the library function that sizes its workspace
    _WS_BYTES = {"forward": "surfdisp_workspace_bytes", "kernels": "surfdisp_kernels_workspace_bytes",
                 "group": "surfdisp_group_kernels_workspace_bytes", "ellip": "surfdisp_ellip_kernels_workspace_bytes",
                 "atten": "surfdisp_atten_workspace_bytes", "eigen": "surfdisp_eigen_workspace_bytes",
                 "thickness": "surfdisp_thickness_kernels_workspace_bytes",
                 "group_thickness": "surfdisp_group_thickness_kernels_workspace_size"}

    def __init__(self, B, L, P, device="cuda:0"):
        import torch
        self.torch = torch
        self.B, self.L, self.P = int(B), int(L), int(P)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SurfdispError("BatchPlan needs a HIP device tensor (no CPU fallback)")
        self._ws = {}                                  # entry name -> (uint8 tensor, bytes), kept for reuse
        self._last_ws = self.workspace("forward")[0]   # (run() allocates nothing: made here)
        self.c = torch.zeros(self.B, self.P, dtype=torch.float32, device=self.device)
        self.u = torch.zeros(self.B, self.P, dtype=torch.float32, device=self.device)
        self.status = torch.zeros(self.B, dtype=torch.int32, device=self.device)

    def workspace(self, entry, tensor=None):
        """(uint8 tensor, bytes) of the workspace of ``entry`` (a key of ``_WS_BYTES``), created on first use with the size the
        library asks for; ``tensor``: install the caller's own contiguous uint8 device tensor instead (all of it is handed over)."""
        if tensor is not None:
            self._ws[entry] = (tensor, int(tensor.numel()))
        elif entry not in self._ws:
            n = int(getattr(_lib.lib(), self._WS_BYTES[entry])(self.B, self.L, self.P))
            self._ws[entry] = (self.torch.empty(n, dtype=self.torch.uint8, device=self.device), n)
        return self._ws[entry]

    def _check(self, model, periods, nlay):
        torch = self.torch
        for t, shape in ((model, (self.B, 5, self.L)), (periods, (self.P,))):
            if (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape
                    or t.device != self.device):
                raise ValueError(f"expected contiguous float32 {shape} on {self.device}")
        if nlay is not None and (nlay.dtype != torch.int32 or nlay.numel() != self.B
                                 or nlay.device != self.device):
            raise ValueError("nlay must be int32 [B] on the same device")

    @staticmethod
    def _ptr(t):
        return ctypes.c_void_p(t.data_ptr() if t is not None else 0)

    def _out(self, *tail, want=True):
        """An uninitialised float32 [B, P, *tail] output (``None`` unless ``want``)."""
        return self.torch.empty((self.B, self.P) + tail, dtype=self.torch.float32, device=self.device) if want else None

    def _counter(self, name):
        """The int32 [1] device counter ``self.<name>``, kept for reuse."""
        if getattr(self, name, None) is None:
            setattr(self, name, self.torch.zeros(1, dtype=self.torch.int32, device=self.device))
        return getattr(self, name)

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, fn, entry, model, periods, kind, nlay, mid, tail=()):
        """Check the inputs and call the library's ``fn`` on torch's current stream with the workspace of ``entry``: the common
        head (stream, B, L, nlay, model, P, periods, kind), ``mid``, (workspace, bytes), ``tail``."""
        self._check(model, periods, nlay)
        ws, nbytes = self.workspace(entry)
        self._last_ws = ws
        ptr = self._ptr
        with self.torch.cuda.device(self.device):
            rc = getattr(_lib.lib(), fn)(self._stream(), self.B, self.L, ptr(nlay), ptr(model), self.P, ptr(periods), int(kind),
                                         *mid, ptr(ws), nbytes, *tail)
        _lib.check(rc)

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
        if independent:
            kind = int(kind) | _lib.INDEPENDENT
        if pipelined:
            kind = int(kind) | _lib.PIPELINED
        if fast_scan:                                  # opt-in count-guided scan (SURFDISP_FASTSCAN)
            kind = int(kind) | _lib.FASTSCAN
        if strict:                                     # verification mode (SURFDISP_STRICT): the exact kernel for every stack
            kind = int(kind) | _lib.STRICT
        ptr = self._ptr
        out = (ptr(self.c), ptr(self.u), ptr(self.status))
        if _timed:
            ms = (ctypes.c_float * 3)()
            self._call("surfdisp_forward_batch_device_timed", "forward", model, periods, kind, nlay, out, (ms,))
            return self.c, self.u, self.status, tuple(float(x) for x in ms)
        fn, tail = "surfdisp_forward_batch_device", ()
        if want_ratio:
            # ABI 3: also the Rayleigh ellipticity (the reference's COMMON /o/ ratio, calcul.f:195) -> self.ratio [B, P]
            if getattr(self, "ratio", None) is None:
                self.ratio = self.torch.zeros(self.B, self.P, dtype=self.torch.float32, device=self.device)
            fn, out = fn + "2", (out[0], out[1], ptr(self.ratio), out[2])
        if events is not None:
            fn, tail = fn + "_events", (events,)
        self._call(fn, "forward", model, periods, kind, nlay, out, tail)
        if want_ratio:
            return self.c, self.u, self.status, self.ratio
        return self.c, self.u, self.status

    def _read_counters(self, fn, out):
        with self.torch.cuda.device(self.device):
            _lib.check(getattr(_lib.lib(), fn)(self._stream(), self._ptr(self._last_ws), self.B, self.L, self.P, out))

    def fallback_count(self):
        """Stacks of the last ``run`` that the production root search handed to the exact fallback kernel
        (``surfdisp_workspace_fallback_count``; synchronises the current stream)."""
        n = ctypes.c_int(0)
        self._read_counters("surfdisp_workspace_fallback_count", ctypes.byref(n))
        return int(n.value)

    def counters(self):
        """(stacks through the exact fallback kernel, brackets refined with NEVILL by the phase test, ellipticities evaluated
        again with the reference's arithmetic) of the last solve (``surfdisp_workspace_counters``; synchronises the stream)."""
        n = (ctypes.c_int * 3)()
        self._read_counters("surfdisp_workspace_counters", n)
        return tuple(int(x) for x in n)

    def run_kernels(self, model, periods, kind=2, nlay=None, want_vp=True, want_rho=True, small_workspace=False):
        """Forward solve + analytic partial derivatives of the phase velocity
        (``surfdisp_forward_kernels_device``): returns (c, u, status, dcdb, dcda, dcdr) with the
        partials float32 [B, P, L] = d c(period) / d (Vs | Vp | rho) of input layer i (``None`` where
        not requested; Love has no dcda).  Same launch as ``run`` plus per-layer sums in the
        group-velocity kernel - what ``SensKernelPert`` obtains from 2L+1 perturbed solves."""
        ptr, L = self._ptr, self.L
        dcdb = self._out(L)
        dcda = self._out(L, want=want_vp and (int(kind) & 3) == _lib.KIND_RAYLEIGH)
        dcdr = self._out(L, want=want_rho)
        # small_workspace: the direct route into the rows (tests compare the two); else + the partials' layer-major scratch
        self._call("surfdisp_forward_kernels_device", "forward" if small_workspace else "kernels", model, periods, kind, nlay,
                   (ptr(self.c), ptr(self.u), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr)))
        return self.c, self.u, self.status, dcdb, dcda, dcdr

    def run_group_kernels(self, model, periods, kind=2, nlay=None, dlnT_frac=0.01, want_vp=True, want_rho=True, count=True):
        """``run_kernels`` plus the analytic partials of the GROUP velocity (``surfdisp_forward_group_kernels_device``):
        returns (c, u, status, dcdb, dcda, dcdr, dudb, duda, dudr, n_failed).  c .. dcdr equal ``run_kernels``' bit for bit;
        dudb / duda / dudr float32 [B, P, L] = d U(period) / d (Vs | Vp | rho) of input layer i (``None`` where not
        requested; Love has no duda), from the phase partials at T (1 -+ dlnT_frac).  Rows of unsolved periods are zeros,
        rows of units whose shifted root failed are NaN; ``n_failed`` (int, synchronises the stream) counts the latter
        (``count=False``: the device tensor itself, no synchronisation)."""
        ptr, L = self._ptr, self.L
        rayleigh = (int(kind) & 3) == _lib.KIND_RAYLEIGH
        dcdb, dudb = self._out(L), self._out(L)
        dcda, duda = self._out(L, want=want_vp and rayleigh), self._out(L, want=want_vp and rayleigh)
        dcdr, dudr = self._out(L, want=want_rho), self._out(L, want=want_rho)
        nfail = self._counter("nfail")
        self._call("surfdisp_forward_group_kernels_device", "group", model, periods, kind, nlay,
                   (float(dlnT_frac), ptr(self.c), ptr(self.u), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr),
                    ptr(dudb), ptr(duda), ptr(dudr), ptr(nfail)))
        return self.c, self.u, self.status, dcdb, dcda, dcdr, dudb, duda, dudr, int(nfail.item()) if count else nfail

    def run_ellip_kernels(self, model, periods, kind=2, nlay=None, want_vp=True, want_rho=True, count=True):
        """``run_kernels`` plus the Rayleigh ellipticity and its analytic partials (``surfdisp_forward_ellip_kernels_device``):
        returns (c, u, status, ratio, dcdb, dcda, dcdr, dedb, deda, dedr, n_nonfinite).  c .. dcdr equal ``run_kernels``' bit
        for bit, ratio [B, P] is ``run(want_ratio=True)``'s; dedb / deda / dedr float32 [B, P, L] = d chi(period) / d (Vs | Vp |
        rho) of input layer i (``None`` where not requested).  Rows of unsolved periods, water layers and layers below the half
        space are zeros, rows of units whose result is not finite are NaN; ``n_nonfinite`` (int, synchronises the stream)
        counts the latter (``count=False``: the device tensor itself, no synchronisation).  Rayleigh only."""
        if (int(kind) & 3) != _lib.KIND_RAYLEIGH:
            raise ValueError("run_ellip_kernels: Rayleigh only (kind=2); Love waves have no ellipticity")
        ptr, L = self._ptr, self.L
        dcdb, dedb = self._out(L), self._out(L)
        dcda, deda = self._out(L, want=want_vp), self._out(L, want=want_vp)
        dcdr, dedr = self._out(L, want=want_rho), self._out(L, want=want_rho)
        ratio = self._out()
        nnonfin = self._counter("nnonfin")
        self._call("surfdisp_forward_ellip_kernels_device", "ellip", model, periods, kind, nlay,
                   (ptr(self.c), ptr(self.u), ptr(ratio), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr),
                    ptr(dedb), ptr(deda), ptr(dedr), ptr(nnonfin)))
        return (self.c, self.u, self.status, ratio, dcdb, dcda, dcdr, dedb, deda, dedr, int(nnonfin.item()) if count else nnonfin)

    def run_atten(self, model, periods, kind=2, nlay=None, want_vp=True, want_rho=True, want_kernel=True, want_gamma=True):
        """``run_kernels`` plus the apparent attenuation of the mode (``surfdisp_forward_atten_device``): returns (c, u, status,
        dcdb, dcda, dcdr, qinv, gamma, dqdq).  c .. dcdr equal ``run_kernels``' bit for bit; qinv [B, P] = 1 / Q_apparent
        (calcul.f:256-265, 341-349: what the reference forms from its partials and the layers' 1/Qs and never returns),
        gamma [B, P] the attenuation coefficient in 1/km, dqdq float32 [B, P, L] = d qinv / d (1/Qs of layer i) at fixed
        eigenfunction (``None`` with ``want_kernel=False``; gamma ``None`` with ``want_gamma=False``).  Unsolved periods and
        bad stacks are zeros, as are water layers and layers below the half space in dqdq.  Rayleigh and Love."""
        ptr, L = self._ptr, self.L
        dcdb = self._out(L)
        dcda = self._out(L, want=want_vp and (int(kind) & 3) == _lib.KIND_RAYLEIGH)
        dcdr = self._out(L, want=want_rho)
        qinv = self._out()
        gamma = self._out(want=want_gamma)
        dqdq = self._out(L, want=want_kernel)
        self._call("surfdisp_forward_atten_device", "atten", model, periods, kind, nlay,
                   (ptr(self.c), ptr(self.u), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr), ptr(qinv), ptr(gamma), ptr(dqdq)))
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
        ptr, L = self._ptr, self.L
        ur = self._out(L)
        uz = self._out(L, want=want_uz)
        tz = self._out(L, want=want_tz)
        tr = self._out(L, want=want_tr)
        energy = self._out(4, want=want_energy)
        self._call("surfdisp_forward_eigen_device", "eigen", model, periods, kind, nlay,
                   (ptr(self.c), ptr(self.u), ptr(self.status), ptr(ur), ptr(uz), ptr(tz), ptr(tr), ptr(energy)))
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
        ptr, L = self._ptr, self.L
        dcdb, dcdh = self._out(L), self._out(L)
        dcda = self._out(L, want=want_vp and (int(kind) & 3) == _lib.KIND_RAYLEIGH)
        dcdr = self._out(L, want=want_rho)
        dcdz = self._out(L, want=want_dcdz)
        tnonfin = self._counter("tnonfin")
        self._call("surfdisp_forward_thickness_kernels_device", "thickness", model, periods, kind, nlay,
                   (ptr(self.c), ptr(self.u), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr), ptr(dcdh), ptr(dcdz), ptr(tnonfin)))
        return (self.c, self.u, self.status, dcdb, dcda, dcdr, dcdh, dcdz, int(tnonfin.item()) if count else tnonfin)

    def run_group_thickness_kernels(self, model, periods, kind=2, nlay=None, dlnT_frac=0.01, want_vp=True, want_rho=True,
                                    want_dcdz=True, want_dudz=True, count=True):
        """``run_group_kernels`` and ``run_thickness_kernels`` in one pass plus the derivatives of the GROUP velocity with respect
        to the layer thicknesses and the interface depths (``surfdisp_forward_group_thickness_kernels_device``): returns (c, u,
        status, dcdb, dcda, dcdr, dudb, duda, dudr, dcdh, dcdz, dudh, dudz, n_failed, n_nonfinite).  c .. dudr equal
        ``run_group_kernels``' at the same ``dlnT_frac`` and dcdh, dcdz ``run_thickness_kernels``' bit for bit; dudh float32
        [B, P, L] = d U(period) / d (thickness of input layer i), everything below shifted rigidly - what a change of
        ``model[:, 3, i]`` does; dudz [B, P, L] = d U(period) / d (depth of the top of layer j) alone (``None`` with
        ``want_dudz=False``), from the thickness rows at T (1 -+ dlnT_frac) by the rule of ``senskernel.group_thickness_reference``.
        Zeros where dcdh is zero; rows of units whose shifted root failed are NaN (``n_failed``, the units of dudb's NaN rows), as
        are rows of units whose thickness rows are not finite (``n_nonfinite``); both counts are ints and synchronise the stream
        (``count=False``: the device tensors).  Rayleigh and Love; include/surfdisp.h section (5h)."""
        ptr, L = self._ptr, self.L
        rayleigh = (int(kind) & 3) == _lib.KIND_RAYLEIGH
        dcdb, dudb, dcdh, dudh = self._out(L), self._out(L), self._out(L), self._out(L)
        dcda, duda = self._out(L, want=want_vp and rayleigh), self._out(L, want=want_vp and rayleigh)
        dcdr, dudr = self._out(L, want=want_rho), self._out(L, want=want_rho)
        dcdz, dudz = self._out(L, want=want_dcdz), self._out(L, want=want_dudz)
        nfail, nnonfin = self._counter("nfail"), self._counter("gtnonfin")
        self._call("surfdisp_forward_group_thickness_kernels_device", "group_thickness", model, periods, kind, nlay,
                   (float(dlnT_frac), ptr(self.c), ptr(self.u), ptr(self.status), ptr(dcdb), ptr(dcda), ptr(dcdr),
                    ptr(dudb), ptr(duda), ptr(dudr), ptr(dcdh), ptr(dcdz), ptr(dudh), ptr(dudz), ptr(nfail), ptr(nnonfin)))
        if count:
            nfail, nnonfin = int(nfail.item()), int(nnonfin.item())
        return self.c, self.u, self.status, dcdb, dcda, dcdr, dudb, duda, dudr, dcdh, dcdz, dudh, dudz, nfail, nnonfin

    def shifted_roots(self):
        """[2, B, P] float32: the roots at T (1 - dlnT_frac) and T (1 + dlnT_frac) the last ``run_group_kernels`` used (a unit's
        own c where it is unsolved or its shifted root failed) - a read-out of the workspace for tests."""
        off = int(_lib.lib().surfdisp_group_kernels_shift_offset(self.B, self.L, self.P))
        n = 2 * self.P * self.B * 4
        return self.workspace("group")[0][off:off + n].view(self.torch.float32).view(2, self.P, self.B).transpose(1, 2).clone()


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
