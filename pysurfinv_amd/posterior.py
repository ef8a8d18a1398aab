"""Posterior Vs(z) profiles of a Metropolis track: what the reference's ``PostPoint`` reports per point - the final rows'
models as Vs at depth (``_loadValues(zdeps=...)``, point.py:317-335), their mean, spread and histograms
(``plotVsProfileShaded``: ``std(axis=1)``; ``_check_distribution``) and how those settle with the chain length
(``_check_convergency``, point.py:249-271) - for every point of a track ``[points, R, 3 + N]`` at once.

* ``posterior_reference`` is the statement, in numpy float64 over ``Model1DBatch.value``; it runs on CPU tensors.
* ``posterior_profiles`` is one call of ``surfdisp_posterior_profile_device`` (csrc/surfdisp_post.hip, header section (6f)) on a
  device track, read in place; every result is tested against the reference function.  Models with a static layer structure
  (``Model1DBatch.native_descriptor()``) and no thermal layer.
* ``convergence`` runs either for the row prefixes of ``_check_convergency``.

Selection (point.py:152-168, as ``MetropolisBatch.summarise_points`` states it), per point over its R rows
``[misfit, L, accepted, *params]``: a NaN misfit counts as +inf; ``imin`` = the first row of the smallest misfit;
``thres = max(2 min, min + 0.5)``; a row is final when ``misfit < thres``; with ``true_markov_chain`` a row's parameters are
those of the last accepted row at or before it (row 0 of a point counts as accepted).  ``chainL`` / ``prefix``: only rows with
``r % chainL < prefix`` take part in the minimum, the threshold and the final set.

Both return a dict: ``min_misfit, thres`` float64 and ``imin, n_final`` int64 ``[points]``; ``pmean, pstd`` ``[points, N]``;
``count`` (finite values, int32) and ``vs_mean, vs_std`` (population), ``vs_min, vs_max`` ``[points, D]``, NaN where count is 0;
with ``hist=(vlo, vhi, nbins)``: ``hist`` int32 ``[points, D, nbins]`` over the equal bins of ``[vlo, vhi)``, ``below``,
``above`` ``[points, D]`` and ``quantiles`` ``[points, D, Q]`` (``quantiles_from_hist``).
"""
from __future__ import annotations

import ctypes
import warnings

import numpy as np

from . import _lib

SLAB_ROWS = 4096          # SURFDISP_POST_SLAB_ROWS: rows of one point per workgroup of the profile kernel
DEPTHS_MAX = 256          # SURFDISP_POST_DEPTHS_MAX


def quantiles_from_hist(hist, vlo, vhi, quantiles):
    """Quantiles ``[..., Q]`` of histograms ``[..., nbins]`` over the equal bins of ``[vlo, vhi)`` (torch, on the histogram's
    device).  With n the in-range count, cum the running sum and w the bin width, b is the first bin with cum[b] >= q n
    (and cum[b] > 0), and the value is ``vlo + w (b + (q n - cum[b - 1]) / hist[b])`` - linear inside the bin; NaN where n = 0."""
    import torch
    h = hist.to(torch.float64)
    nb = h.shape[-1]
    w = (float(vhi) - float(vlo)) / nb
    cum = h.cumsum(dim=-1)
    n = cum[..., -1:]
    out = []
    for q in quantiles:
        target = float(q) * n
        b = ((cum >= target) & (cum > 0)).to(torch.int8).argmax(dim=-1, keepdim=True)
        hb = h.gather(-1, b)
        before = cum.gather(-1, b) - hb
        v = float(vlo) + w * (b.to(torch.float64) + (target - before) / hb)
        out.append(torch.where(n > 0, v, torch.full_like(v, float("nan"))))
    return torch.cat(out, dim=-1) if out else h.new_zeros(h.shape[:-1] + (0,))


def _hist_args(hist):
    if hist is None:
        return None
    vlo, vhi, nbins = float(hist[0]), float(hist[1]), int(hist[2])
    if not (np.isfinite(vlo) and np.isfinite(vhi) and vhi > vlo and nbins >= 1):
        raise ValueError("hist = (vlo, vhi, nbins) with finite vlo < vhi and nbins >= 1")
    return vlo, vhi, nbins


def _prefix_args(R, chainL, prefix):
    if prefix is None:
        return 0, 0
    if chainL is None:
        raise ValueError("prefix needs chainL")
    chainL, prefix = int(chainL), int(prefix)
    if chainL < 1 or not 1 <= prefix <= chainL or R % chainL:
        raise ValueError("1 <= prefix <= chainL, and the rows of a point a multiple of chainL")
    return chainL, prefix


def select_reference(track, true_markov_chain=True, chainL=None, prefix=None):
    """The selection alone, numpy: (misfit as selected [points, R], imin, thres, final mask, source row of every row)."""
    tr = np.asarray(track, dtype=np.float64)
    npnt, R, _ = tr.shape
    chainL, prefix = _prefix_args(R, chainL, prefix)
    mis = np.where(np.isnan(tr[:, :, 0]), np.inf, tr[:, :, 0])
    idx = np.arange(R)
    if chainL:
        mis = np.where((idx % chainL < prefix)[None, :], mis, np.inf)
    imin = mis.argmin(axis=1)
    mn = mis[np.arange(npnt), imin]
    thres = np.maximum(2.0 * mn, mn + 0.5)
    final = mis < thres[:, None]
    if true_markov_chain:
        src = np.maximum.accumulate(np.where(tr[:, :, 2] > 0.5, idx[None, :], 0), axis=1)
    else:
        src = np.broadcast_to(idx[None, :], (npnt, R))
    return mis, imin, thres, final, src


def posterior_reference(model_batch, track, zdeps, rows=None, true_markov_chain=True, chainL=None, prefix=None, hist=None,
                        quantiles=(0.16, 0.5, 0.84)):
    """The statement (module docstring) in numpy float64: Vs at depth from ``Model1DBatch.value``, then ``np.nanmean``,
    ``np.nanstd``, ``np.histogram`` on the fixed edges ``vlo + i w``.  ``track``: CPU tensor or array ``[points, R, 3 + N]``;
    ``rows``: the local-information row of each point (models with per-point constants)."""
    import torch
    tr = track.detach().cpu().numpy() if isinstance(track, torch.Tensor) else np.asarray(track)
    tr = np.asarray(tr, dtype=np.float64)
    npnt, R, W = tr.shape
    N = W - 3
    zd = np.asarray(zdeps, dtype=np.float64).ravel()
    D = zd.size
    hist = _hist_args(hist)
    mis, imin, thres, final, src = select_reference(tr, true_markov_chain, chainL, prefix)
    out = dict(min_misfit=mis[np.arange(npnt), imin], thres=thres, imin=imin.astype(np.int64),
               n_final=final.sum(axis=1).astype(np.int64),
               pmean=np.full((npnt, N), np.nan), pstd=np.full((npnt, N), np.nan), count=np.zeros((npnt, D), np.int32),
               vs_mean=np.full((npnt, D), np.nan), vs_std=np.full((npnt, D), np.nan),
               vs_min=np.full((npnt, D), np.nan), vs_max=np.full((npnt, D), np.nan))
    if hist is not None:
        vlo, vhi, nbins = hist
        edges = np.arange(nbins + 1) * ((vhi - vlo) / nbins) + vlo
        out.update(hist=np.zeros((npnt, D, nbins), np.int32), below=np.zeros((npnt, D), np.int32),
                   above=np.zeros((npnt, D), np.int32))
    rows = None if rows is None else np.asarray(torch.as_tensor(rows).cpu().numpy(), dtype=np.int64)
    if rows is None and model_batch.n_aux:                                # point p reads row p of the local-information table
        if model_batch._aux is None or model_batch._aux.shape[0] != npnt:
            raise ValueError(f"{npnt} points against the rows of the model's local info: pass rows=")
        rows = np.arange(npnt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # all-NaN columns: NaN is the answer
        for p in range(npnt):
            par = tr[p, src[p][final[p]], 3:]
            if par.shape[0] == 0:
                continue
            fin_p = np.where(np.isfinite(par), par, np.nan)
            out["pmean"][p], out["pstd"][p] = np.nanmean(fin_p, axis=0), np.nanstd(fin_p, axis=0)
            vals = model_batch.value(torch.as_tensor(par, dtype=torch.float64, device=model_batch.device), zd,
                                     rows=None if rows is None else np.full(par.shape[0], rows[p]))
            vals = np.where(np.isfinite(vals), vals, np.nan)               # [n_final, D]
            out["count"][p] = np.isfinite(vals).sum(axis=0)
            out["vs_mean"][p], out["vs_std"][p] = np.nanmean(vals, axis=0), np.nanstd(vals, axis=0)
            out["vs_min"][p], out["vs_max"][p] = np.nanmin(vals, axis=0), np.nanmax(vals, axis=0)
            if hist is not None:
                for d in range(D):
                    v = vals[:, d][np.isfinite(vals[:, d])]
                    out["below"][p, d], out["above"][p, d] = (v < vlo).sum(), (v >= vhi).sum()
                    v = v[(v >= vlo) & (v < vhi)]
                    out["hist"][p, d] = np.histogram(v, edges)[0] if v.size else 0
    out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}
    if hist is not None:
        out["quantiles"] = quantiles_from_hist(out["hist"], vlo, vhi, quantiles)
    return out


def _host_descriptor(model_batch):
    """(idesc host int32 array, fdesc device tensor) of a model the device route supports; ValueError otherwise."""
    desc = model_batch.native_descriptor()
    if desc is None:
        raise ValueError("posterior_profiles needs a model with a static layer structure (native_descriptor() is None): "
                         "use posterior_reference")
    if model_batch._native_thermal:
        raise ValueError("posterior_profiles does not support the thermal mantle layer: use posterior_reference")
    cached = getattr(model_batch, "_post_idesc", None)
    if cached is None or cached[0] is not desc[0]:
        cached = (desc[0], np.ascontiguousarray(desc[0].cpu().numpy(), dtype=np.int32))
        model_batch._post_idesc = cached
    return cached[1], desc[1]


def posterior_profiles(model_batch, track, zdeps, rows=None, true_markov_chain=True, chainL=None, prefix=None, hist=None,
                       quantiles=(0.16, 0.5, 0.84)):
    """``posterior_reference`` on the device: ``track`` a float64 device tensor ``[points, R, 3 + N]`` (read in place, never
    gathered), one call of ``surfdisp_posterior_profile_device`` on the current stream, a dict of device tensors.  Raises
    ``ValueError`` for a model without a native descriptor or with a thermal layer (checked first, so also without a device),
    ``SurfdispError`` for a track that is not on a HIP device, and ``ValueError`` for a model that lives on another device than
    the track."""
    import torch
    idesc, fdesc = _host_descriptor(model_batch)
    if not isinstance(track, torch.Tensor) or track.device.type != "cuda":
        raise _lib.SurfdispError("posterior_profiles needs a track on a HIP device (no CPU fallback: posterior_reference is the host statement)")
    if fdesc.device != track.device:                                       # the kernel reads the descriptor's float part where the track is
        raise ValueError(f"the model is on {fdesc.device}, the track on {track.device}: build the Model1DBatch on the track's device")
    if track.ndim != 3 or track.dtype != torch.float64:
        raise ValueError("track must be float64 [points, R, 3 + N]")
    N = model_batch.spec.n
    if track.shape[2] != 3 + N:
        raise ValueError(f"track rows have {track.shape[2]} columns, the model has {N} parameters")
    track = track.contiguous()
    npnt, R, W = track.shape
    dev = track.device
    zd = np.ascontiguousarray(np.asarray(zdeps, dtype=np.float64).ravel())
    D = zd.size
    hist = _hist_args(hist)
    chainL, prefix = _prefix_args(R, chainL, prefix)
    aux, K, rows_t = None, model_batch.n_aux, None
    if K:
        aux = model_batch._aux
        if aux is None:
            raise ValueError(f"this model has per-point constants {model_batch.aux_names}: call set_local_info(table) first")
        aux = aux.to(dev)
        if rows is not None:
            rows_t = torch.as_tensor(rows, device=dev).to(torch.int32).contiguous()
            if rows_t.shape != (npnt,):
                raise ValueError("rows must be [points]")
        elif aux.shape[0] != npnt:
            raise ValueError(f"{npnt} points against {aux.shape[0]} rows of local info: pass rows=")
    L = _lib.lib()
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    o = dict(min_misfit=torch.empty(npnt, **f64), thres=torch.empty(npnt, **f64), imin=torch.empty(npnt, **i32),
             n_final=torch.empty(npnt, **i32), pmean=torch.empty((npnt, N), **f64), pstd=torch.empty((npnt, N), **f64),
             count=torch.empty((npnt, D), **i32), vs_mean=torch.empty((npnt, D), **f64), vs_std=torch.empty((npnt, D), **f64),
             vs_min=torch.empty((npnt, D), **f64), vs_max=torch.empty((npnt, D), **f64))
    vlo, vhi, nbins = hist if hist is not None else (0.0, 0.0, 0)
    if hist is not None:
        o.update(hist=torch.empty((npnt, D, nbins), **i32), below=torch.empty((npnt, D), **i32), above=torch.empty((npnt, D), **i32))
    ws = torch.empty(max(int(L.surfdisp_posterior_workspace_bytes(npnt, R, N, max(D, 1))), 8), dtype=torch.uint8, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = L.surfdisp_posterior_profile_device(
            ctypes.c_void_p(stream), npnt, R, N, ptr(track), W,
            idesc.ctypes.data_as(ctypes.c_void_p), int(idesc.size), ptr(fdesc), ptr(aux), K, ptr(rows_t),
            D, zd.ctypes.data_as(ctypes.c_void_p), 1 if true_markov_chain else 0, chainL, prefix, nbins, vlo, vhi,
            ptr(o["min_misfit"]), ptr(o["thres"]), ptr(o["imin"]), ptr(o["n_final"]), ptr(o["pmean"]), ptr(o["pstd"]),
            ptr(o["count"]), ptr(o["vs_mean"]), ptr(o["vs_std"]), ptr(o["vs_min"]), ptr(o["vs_max"]),
            ptr(o.get("hist")), ptr(o.get("below")), ptr(o.get("above")), ptr(ws), ws.numel())
    _lib.check(rc)
    o["imin"], o["n_final"] = o["imin"].to(torch.int64), o["n_final"].to(torch.int64)
    if hist is not None:
        o["quantiles"] = quantiles_from_hist(o["hist"], vlo, vhi, quantiles)
    return o


def convergence(model_batch, track, zdeps, chainL, rows=None, true_markov_chain=True, n_tests=20):
    """``_check_convergency`` (point.py:249-271): mean and std of Vs at depth over the final rows of the first
    ``int(l)`` rows of every chain, ``l`` in ``linspace(chainL / 10, chainL, n_tests)`` (at least 1) - one entry call per prefix on a
    device track, ``posterior_reference`` on a CPU one.  dict(prefixes [n_tests], mean, std [n_tests, points, D])."""
    import torch
    fn = posterior_profiles if (isinstance(track, torch.Tensor) and track.device.type == "cuda") else posterior_reference
    prefixes = [max(int(l), 1) for l in np.linspace(chainL / 10, chainL, int(n_tests))]
    res = [fn(model_batch, track, zdeps, rows=rows, true_markov_chain=true_markov_chain, chainL=chainL, prefix=p) for p in prefixes]
    return dict(prefixes=prefixes, mean=torch.stack([r["vs_mean"] for r in res]), std=torch.stack([r["vs_std"] for r in res]))
