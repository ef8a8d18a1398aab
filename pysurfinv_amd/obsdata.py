"""Observed dispersion data of a joint inversion: Rayleigh and Love, phase (c) and group (U) velocities, and the Rayleigh
ellipticity (E, the H/V ratio).

The reference's ``Point.misfit`` (``point.py:15-31``) fits one curve, Rayleigh phase velocity.  A
``MetropolisBatch(data=[DispersionData, ...])`` fits any set of the five curves at once:

    chi2 = sum_d w_d sum_{unmasked p} ((obs - pred) / uncer)^2,   N = unmasked entries (unweighted),
    misfit = sqrt(chi2 / N), then the reference's clamp (chi2 := sqrt(50 chi2) when >= 50) and L = exp(-chi2/2).

One forward solve per wave type with data.  Its period list (``JointData.solve_periods``):

* every data set of the wave type has the same period array: that array as given (order kept) - a lone Rayleigh-phase
  set is then solved exactly as ``MetropolisBatch(periods, c_obs, uncer)`` solves it;
* otherwise the ascending, de-duplicated union of the data sets' periods (compared in float32).  The reference's root
  search carries its start rule (0.9 c(k-1)) and dropped layers from one period to the next, so a curve solved on the
  union can differ in the last digits from the same curve solved on its own period list.

A solve fails the model - (misfit, chi2, L) = (88888, 88888, 0) - when its status is not 0, when any phase velocity of
that solve (at any of its periods, masked or not) is below 0.01 (``models.py:29-33``, per wave type), or when a group
velocity at a period of a U data set is not finite or below 0.01.  A wave type with U data is solved without
SURFDISP_PHASE_ONLY (the group-velocity kernel runs as well); a wave type with phase data only keeps the phase-only solve.

Ellipticity: an ``"E"`` set of wave ``"R"`` is compared with chi as the Rayleigh solve returns it (``BatchPlan.run(
want_ratio=True)``, the reference's COMMON /o/ ratio, calcul.f:195) - signed, or ``|chi|`` with ``absolute=True`` (a measured
H/V curve is an amplitude ratio and carries no sign).  Its periods join the Rayleigh period-list rule above; the solve's kind
flags do not change (a phase-only solve still runs the ellipticity passes when the ratio is asked for).  On top of the rule
above a model fails (88888, 88888, 0) when an ellipticity value that a column reads is not finite.  There is no lower bound:
chi near 0 and negative chi are legitimate predictions (an unsolved period has chi = 0, but the status / c < 0.01 test of the
Rayleigh solve has caught it already).  Non-finite values arise where D(e2) ~ 0, a node of the vertical motion at the surface
(include/surfdisp.h, surfdisp_forward_ellip_kernels_device).
"""
from __future__ import annotations

import numpy as np

WAVES = ("R", "L")
QUANTITIES = ("c", "U", "E")
# column sources of the joint accept kernels, in this order (include/surfdisp.h, surfdisp_mcmc_accept_joint_device /
# surfdisp_mcmc_accept_joint5_device): the key of the forward dict each one reads; 4 is chi, 5 is |chi| of the same array
SOURCES = ("cR", "uR", "cL", "uL", "eR", "eR")
SRC_ELLIP, SRC_ELLIP_ABS = 4, 5
DICT_KEYS = {"RayPhase": ("R", "c"), "RayGroup": ("R", "U"), "LovePhase": ("L", "c"), "LoveGroup": ("L", "U"),
             "RayEllip": ("R", "E"), "RayHV": ("R", "E", True)}          # (wave, quantity[, absolute])


class DispersionData:
    """One observed curve: ``wave`` "R" | "L", ``quantity`` "c" (phase) | "U" (group) | "E" (ellipticity, Rayleigh only),
    ``periods`` [P_d], ``values`` and ``uncer`` [P_d] or [C, P_d] (one row per chain), ``weight`` of its chi-square.  A
    non-finite value, or an uncertainty that is non-finite or <= 0, masks the entry out.  ``absolute`` (an "E" set only):
    the prediction compared is |chi|, not the signed chi of the solver."""

    def __init__(self, wave, quantity, periods, values, uncer, weight=1.0, absolute=False):
        if wave not in WAVES:
            raise ValueError(f"DispersionData: wave must be one of {WAVES}, not {wave!r}")
        if quantity not in QUANTITIES:
            raise ValueError(f"DispersionData: quantity must be one of {QUANTITIES}, not {quantity!r}")
        if quantity == "E" and wave != "R":
            raise ValueError("DispersionData: Love waves have no ellipticity (quantity 'E' needs wave 'R')")
        if absolute and quantity != "E":
            raise ValueError("DispersionData: absolute=True is for an ellipticity ('E') set only")
        self.wave, self.quantity, self.absolute = wave, quantity, bool(absolute)
        self.periods = np.asarray(periods, np.float64).ravel()
        self.values = np.asarray(values, np.float64)
        self.uncer = np.asarray(uncer, np.float64)
        self.weight = float(weight)
        P = self.periods.size
        if P == 0:
            raise ValueError("DispersionData: no periods")
        if not (np.isfinite(self.periods).all() and (self.periods > 0).all()):
            raise ValueError("DispersionData: periods must be finite and positive")
        if self.values.ndim not in (1, 2) or self.values.shape[-1] != P:
            raise ValueError(f"DispersionData: values of shape {self.values.shape} against {P} periods")
        if self.uncer.shape != self.values.shape:
            raise ValueError(f"DispersionData: uncer of shape {self.uncer.shape} against values of shape {self.values.shape}")
        if not (np.isfinite(self.weight) and self.weight > 0):
            raise ValueError("DispersionData: weight must be finite and positive")

    @property
    def source(self):
        """Index of the prediction array this set is compared with (``SOURCES``)."""
        if self.quantity == "E":
            return SRC_ELLIP_ABS if self.absolute else SRC_ELLIP
        return 2 * WAVES.index(self.wave) + QUANTITIES.index(self.quantity)

    def to_dict(self):
        """Plain arrays and strings (what the ``.npz`` files keep: readable without this package)."""
        return dict(wave=self.wave, quantity=self.quantity, periods=self.periods, values=self.values, uncer=self.uncer,
                    weight=self.weight, absolute=self.absolute)

    @classmethod
    def from_dict(cls, d):
        return cls(str(d["wave"]), str(d["quantity"]), d["periods"], d["values"], d["uncer"], d.get("weight", 1.0),
                   bool(d.get("absolute", False)))

    def __repr__(self):
        ab = ", absolute" if self.absolute else ""
        return f"DispersionData({self.wave!r}, {self.quantity!r}, {self.periods.size} periods, weight={self.weight}{ab})"


def as_datasets(data):
    """A list of ``DispersionData`` from a list of them (or of their ``to_dict`` form), or from ``Point``'s dict form
    {"RayPhase" | "RayGroup" | "LovePhase" | "LoveGroup" | "RayEllip" (signed chi) | "RayHV" (|chi|): (T, values, uncers)}."""
    if isinstance(data, dict):
        out = []
        for key, v in data.items():
            if key not in DICT_KEYS:
                raise ValueError(f"data: unknown key {key!r} (expected {sorted(DICT_KEYS)})")
            T, vals, unc = v
            wq = DICT_KEYS[key]
            out.append(DispersionData(wq[0], wq[1], T, vals, unc, absolute=len(wq) > 2 and wq[2]))
        return out
    return [d if isinstance(d, DispersionData) else DispersionData.from_dict(d) for d in data]


class JointData:
    """The data sets of one sampler, concatenated: observation columns in data-set order, the solve period list of each
    wave type, and the column table (source array, period index in that solve, weight) - the latter on the device."""

    def __init__(self, datasets, device="cpu"):
        self.datasets = as_datasets(datasets)
        if not self.datasets:
            raise ValueError("data: no data sets")
        pairs = [(d.wave, d.quantity) for d in self.datasets]
        dup = sorted({p for p in pairs if pairs.count(p) > 1})
        if dup:
            raise ValueError(f"data: duplicate (wave, quantity) sets {dup}")
        rows = {d.values.shape[0] for d in self.datasets if d.values.ndim == 2}
        if len(rows) > 1:
            raise ValueError(f"data: per-chain data sets with different numbers of rows {sorted(rows)}")
        self.C = rows.pop() if rows else None
        # solve period list per wave type
        self.solve_periods, self.with_group = {}, {}
        for w in WAVES:
            sets = [d for d in self.datasets if d.wave == w]
            if not sets:
                continue
            f32 = [d.periods.astype(np.float32) for d in sets]
            if all(np.array_equal(f, f32[0]) for f in f32[1:]):
                self.solve_periods[w] = f32[0]
            else:
                self.solve_periods[w] = np.unique(np.concatenate(f32))
            self.with_group[w] = any(d.quantity == "U" for d in sets)
        self.waves = tuple(self.solve_periods)
        self.with_ratio = any(d.quantity == "E" for d in self.datasets)      # the Rayleigh solve returns its ellipticity too
        # column table
        src, idx, wgt = [], [], []
        for d in self.datasets:
            sp = self.solve_periods[d.wave]
            f = d.periods.astype(np.float32)
            if np.array_equal(f, sp):
                k = np.arange(f.size)
            else:
                k = np.searchsorted(sp, f)
                assert np.array_equal(sp[k], f)
            src.append(np.full(f.size, d.source)); idx.append(k); wgt.append(np.full(f.size, d.weight))
        self.col_src = np.concatenate(src).astype(np.int32)
        self.col_idx = np.concatenate(idx).astype(np.int32)
        self.col_w = np.concatenate(wgt).astype(np.float64)
        self.Ptot = int(self.col_src.size)
        # concatenated observations ([Ptot], or [C, Ptot] when any set is per chain)
        if self.C is None:
            obs = np.concatenate([d.values for d in self.datasets])
            unc = np.concatenate([d.uncer for d in self.datasets])
        else:
            bc = lambda a: np.broadcast_to(a, (self.C, a.shape[-1]))
            obs = np.concatenate([bc(d.values) for d in self.datasets], axis=1)
            unc = np.concatenate([bc(d.uncer) for d in self.datasets], axis=1)
        self.obs_raw, self.uncer_raw = obs, unc
        self.to(device)

    def to(self, device):
        """Device copies: ``cols`` int32 [Ptot, 2] (source, period index), ``weights`` float64 [Ptot], the solve period lists
        (float32) and the per-column tensors the torch misfit gathers with."""
        import torch
        self.device = torch.device(device)
        dev = self.device
        self.cols = torch.as_tensor(np.stack([self.col_src, self.col_idx], axis=1), device=dev).contiguous()
        self.weights = torch.as_tensor(self.col_w, device=dev)
        self.periods_t = {w: torch.as_tensor(p, device=dev) for w, p in self.solve_periods.items()}
        self.src_t = torch.as_tensor(self.col_src.astype(np.int64), device=dev)
        self.idx_t = torch.as_tensor(self.col_idx.astype(np.int64), device=dev)
        self.group_cols = {w: torch.as_tensor(np.nonzero(self.col_src == 2 * WAVES.index(w) + 1)[0], device=dev)
                           for w in self.waves if self.with_group[w]}
        self.ellip_cols = torch.as_tensor(np.nonzero(self.col_src >= SRC_ELLIP)[0], device=dev)
        return self

    def kind(self, wave):
        """Solver kind flags of a wave type's solve: phase only unless the wave type has U data."""
        from . import _lib
        k = _lib.KIND_RAYLEIGH if wave == "R" else _lib.KIND_LOVE
        return k if self.with_group[wave] else k | _lib.PHASE_ONLY

    def predictions(self, pred):
        """[B, Ptot] float64 predicted values of the columns from the forward dict (cR, uR, cL, uL, statusR, statusL, and eR
        when there is an ellipticity set), and bool [B] failed (the failure rule of the module docstring)."""
        import torch
        failed = None
        for w in self.waves:
            c = pred["c" + w].to(torch.float64)
            f = (pred["status" + w] != 0) | (c < 0.01).any(dim=1)            # models.py:29-33, per wave type
            if self.with_group[w]:
                ug = pred["u" + w].to(torch.float64)[:, self.idx_t[self.group_cols[w]]]
                f = f | (~(ug >= 0.01)).any(dim=1)                  # NaN or below 0.01 where a U data set reads it
            failed = f if failed is None else failed | f
        if self.with_ratio:
            if pred.get("eR") is None:
                raise ValueError("joint data with an ellipticity set: the forward dict has no 'eR'")
            e = pred["eR"].to(torch.float64)[:, self.idx_t[self.ellip_cols]]
            failed = failed | (~torch.isfinite(e)).any(dim=1)       # NaN or inf where an E data set reads it
        cols, o = [], 0                                              # (the columns of a data set are contiguous)
        for d in self.datasets:
            n = d.periods.size
            v = pred[SOURCES[d.source]].to(torch.float64)[:, self.idx_t[o:o + n]]
            cols.append(v.abs() if d.source == SRC_ELLIP_ABS else v)
            o += n
        return torch.cat(cols, dim=1), failed
