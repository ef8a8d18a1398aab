"""Posterior Vs(z) profiles of a Metropolis track: what the reference's ``PostPoint`` reports per point - the final rows'
models as Vs at depth (``_loadValues(zdeps=...)``, point.py:317-335), their mean, spread and histograms
(``plotVsProfileShaded``: ``std(axis=1)``; ``_check_distribution``) and how those settle with the chain length
(``_check_convergency``, point.py:249-271) - for every point of a track ``[points, R, 3 + N]`` at once.

* ``posterior_reference`` is the statement, in numpy float64 over ``Model1DBatch.value``; it runs on CPU tensors.
* ``posterior_profiles`` is one call of ``surfdisp_posterior_profile_device`` (csrc/surfdisp_post.hip, header section (6f)) on a
  device track, read in place; every result is tested against the reference function.  Models with a static layer structure
  (``Model1DBatch.native_descriptor()``) and no thermal layer.
* ``convergence`` runs either for the row prefixes of ``_check_convergency``.
* ``posterior_predictive`` / ``predictive_reference`` are the data-space half (``PostPoint.plotDisp(ensemble=True)``,
  ``Model3D.checkPhaseVelocity``): the predicted curves of the final rows' models, their mean, spread and histograms per data
  column, held against the observations - for any parameterisation, since the models come from the sampler's own ``to_model``.

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
    device); ``vlo``, ``vhi`` scalars, or ``[P]`` arrays with ``hist`` ``[..., P, nbins]``: one range per column.  With n the
    in-range count, cum the running sum and w the bin width, b is the first bin with cum[b] >= q n (and cum[b] > 0), and the
    value is ``vlo + w (b + (q n - cum[b - 1]) / hist[b])`` - linear inside the bin; NaN where n = 0."""
    import torch
    h = hist.to(torch.float64)
    nb = h.shape[-1]
    # a scalar range stays a Python float: no host-to-device copy, so no wait for the stream the histogram was just launched on
    lo, hi = (float(a) if np.ndim(a) == 0 else torch.as_tensor(np.asarray(a, np.float64), device=h.device)[:, None] for a in (vlo, vhi))
    w = (hi - lo) / nb
    cum = h.cumsum(dim=-1)
    n = cum[..., -1:]
    out = []
    for q in quantiles:
        target = float(q) * n
        b = ((cum >= target) & (cum > 0)).to(torch.int8).argmax(dim=-1, keepdim=True)
        hb = h.gather(-1, b)
        before = cum.gather(-1, b) - hb
        v = lo + w * (b.to(torch.float64) + (target - before) / hb)
        out.append(torch.where(n > 0, v, torch.full_like(v, float("nan"))))
    return torch.cat(out, dim=-1) if out else h.new_zeros(h.shape[:-1] + (0,))


quantiles_from_hist_cols = quantiles_from_hist            # the name the per-column form had


def _hist_args(hist, P=None):
    """None, or ``(vlo, vhi, nbins)`` of ``hist = (vlo, vhi, nbins)``, checked: floats (``P`` None: one range), or float64 arrays
    ``[P]`` from scalars or ``[P]`` arrays (one range per column)."""
    if hist is None:
        return None
    if P is None:
        vlo, vhi, each = float(hist[0]), float(hist[1]), ""
    else:
        try:
            vlo = np.array(np.broadcast_to(np.asarray(hist[0], np.float64), (P,)))
            vhi = np.array(np.broadcast_to(np.asarray(hist[1], np.float64), (P,)))
        except ValueError:
            raise ValueError(f"hist = (vlo, vhi, nbins): vlo and vhi scalars or arrays of the {P} data columns") from None
        each = " in every column"
    nbins = int(hist[2])
    if not (np.all(np.isfinite(vlo)) and np.all(np.isfinite(vhi)) and np.all(vhi > vlo) and nbins >= 1):
        raise ValueError(f"hist = (vlo, vhi, nbins) with finite vlo < vhi{each} and nbins >= 1")
    return vlo, vhi, nbins


_pred_hist_args = _hist_args                              # the name the per-column form had: callers pass (hist, P)


def _column_statistics(vals, name, hist=None):
    """THE per-column statement of both reference functions, numpy float64: ``vals`` ``[n, C]``, a value counts when it is
    finite.  dict ``count`` ``[C]`` and, with n > 0, ``<name>mean, <name>std`` (population), ``<name>min, <name>max`` (NaN where
    count is 0); with ``hist = (vlo, vhi, nbins)`` (scalars or ``[C]``) also ``below`` (v < vlo), ``above`` (v >= vhi) and
    ``hist`` ``[C, nbins]``: ``np.histogram`` on the fixed edges ``vlo + i w``.  All-NaN columns warn: the caller silences
    RuntimeWarning."""
    vals = np.where(np.isfinite(vals), vals, np.nan)
    n, C = vals.shape
    st = dict(count=np.isfinite(vals).sum(axis=0))
    if n == 0:
        return st
    st.update({name + "mean": np.nanmean(vals, axis=0), name + "std": np.nanstd(vals, axis=0),
               name + "min": np.nanmin(vals, axis=0), name + "max": np.nanmax(vals, axis=0)})
    if hist is not None:
        vlo, vhi, nbins = np.broadcast_to(hist[0], (C,)), np.broadcast_to(hist[1], (C,)), hist[2]
        st.update(hist=np.zeros((C, nbins), np.int32), below=np.zeros(C, np.int32), above=np.zeros(C, np.int32))
        for c in range(C):
            edges = np.arange(nbins + 1) * ((vhi[c] - vlo[c]) / nbins) + vlo[c]
            v = vals[:, c][np.isfinite(vals[:, c])]
            st["below"][c], st["above"][c] = (v < vlo[c]).sum(), (v >= vhi[c]).sum()
            v = v[(v >= vlo[c]) & (v < vhi[c])]
            st["hist"][c] = np.histogram(v, edges)[0] if v.size else 0
    return st


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
            st = _column_statistics(par, "p")
            out["pmean"][p], out["pstd"][p] = st["pmean"], st["pstd"]
            vals = model_batch.value(torch.as_tensor(par, dtype=torch.float64, device=model_batch.device), zd,
                                     rows=None if rows is None else np.full(par.shape[0], rows[p]))     # [n_final, D]
            for k, v in _column_statistics(vals, "vs_", hist).items():
                out[k][p] = v
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


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _hist_outputs(hist, npnt, C):
    """The three histogram outputs of an entry over ``[npnt, C]`` columns, as ``_entry_call`` takes them: None without ``hist``."""
    import torch
    shapes = dict(hist=(npnt, C, hist[2] if hist else 0), below=(npnt, C), above=(npnt, C))
    return {k: (v, torch.int32) if hist is not None else None for k, v in shapes.items()}


def _entry_call(entry, dev, ws_bytes, args, outputs):
    """One call of the C entry ``entry`` on the current stream of ``dev``.  ``outputs``: name -> (shape, dtype), in the order of
    the entry's output arguments, or None for an output that is not asked for (passed as NULL, absent from the result); they
    and the workspace of ``ws_bytes`` (the entry's ``*_workspace_bytes`` and its arguments) are allocated on ``dev``, the entry is
    called as ``entry(stream, *args, *outputs, workspace, its bytes)`` and its return code checked.  Returns the dict of device
    tensors."""
    import torch
    L = _lib.lib()
    o = {k: torch.empty(v[0], dtype=v[1], device=dev) for k, v in outputs.items() if v is not None}
    ws = torch.empty(max(int(getattr(L, ws_bytes[0])(*ws_bytes[1:])), 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(getattr(L, entry)(ctypes.c_void_p(stream), *args, *[_ptr(o.get(k)) for k in outputs], _ptr(ws), ws.numel()))
    return o


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
    f64, i32 = torch.float64, torch.int32
    vlo, vhi, nbins = hist if hist is not None else (0.0, 0.0, 0)
    o = _entry_call(
        "surfdisp_posterior_profile_device", dev, ("surfdisp_posterior_workspace_bytes", npnt, R, N, max(D, 1)),
        (npnt, R, N, _ptr(track), W, idesc.ctypes.data_as(ctypes.c_void_p), int(idesc.size), _ptr(fdesc), _ptr(aux), K, _ptr(rows_t),
         D, zd.ctypes.data_as(ctypes.c_void_p), 1 if true_markov_chain else 0, chainL, prefix, nbins, vlo, vhi),
        dict(min_misfit=(npnt, f64), thres=(npnt, f64), imin=(npnt, i32), n_final=(npnt, i32), pmean=((npnt, N), f64),
             pstd=((npnt, N), f64), count=((npnt, D), i32), vs_mean=((npnt, D), f64), vs_std=((npnt, D), f64),
             vs_min=((npnt, D), f64), vs_max=((npnt, D), f64), **_hist_outputs(hist, npnt, D)))
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


# ------------------------------------------------------------------ posterior predictive curves (header section (6g))
PRED_SLAB_ROWS = 4096     # SURFDISP_PRED_SLAB_ROWS: list rows a workgroup of the statistics kernel walks at a time
PRED_SLABS_MAX = 16       # SURFDISP_PRED_SLABS_MAX
PRED_COLS_MAX = 1024      # SURFDISP_PRED_COLS_MAX


def _predictive_args(sampler, shape, obs_rows, chainL, prefix, hist, max_batch):
    """The checks both predictive functions share: (P, obs_rows as an int64 array or None, chainL, prefix, hist)."""
    if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("track must be [points, R, 3 + N]")
    npnt, R, W = shape
    if W != 3 + sampler.spec.n:
        raise ValueError(f"track rows have {W} columns, the sampler's model has {sampler.spec.n} parameters")
    if int(max_batch) < 1:
        raise ValueError("max_batch >= 1")
    P = int(sampler.c_obs.shape[-1])
    if P > PRED_COLS_MAX:
        raise ValueError(f"{P} data columns: at most {PRED_COLS_MAX}")
    # rows of the sampler's per-chain observations / local information (None: the same data for every model)
    nrows = (int(sampler.c_obs.shape[0]) if sampler.c_obs.ndim == 2 else
             int(sampler.local_rows.shape[0]) if sampler.local_rows is not None else None)
    if obs_rows is not None:
        obs_rows = np.asarray(obs_rows.cpu().numpy() if hasattr(obs_rows, "cpu") else obs_rows, dtype=np.int64)
        if obs_rows.shape != (npnt,):
            raise ValueError("obs_rows must be [points]")
        if nrows is not None and (obs_rows.min() < 0 or obs_rows.max() >= nrows):
            raise ValueError(f"obs_rows outside the sampler's {nrows} rows of observations")
    elif nrows is not None:
        if nrows != npnt:
            raise ValueError(f"{npnt} points against {nrows} rows of observations: pass obs_rows=")
        obs_rows = np.arange(npnt, dtype=np.int64)
    chainL, prefix = _prefix_args(R, chainL, prefix)
    return P, obs_rows, chainL, prefix, _hist_args(hist, P)


def _predict(sampler, params, rows, max_batch):
    """The sampler's own prediction of every row of ``params`` (a tensor on its device), ``max_batch`` rows per solve:
    (pred float64 [n, P], misfit [n], failed bool [n]).  ``MetropolisBatch.misfit`` marks a failed solve with 88888."""
    import torch
    from .mcmc import FAIL
    n, P = params.shape[0], int(sampler.c_obs.shape[-1])
    pred = torch.empty((n, P), dtype=torch.float64, device=params.device)
    mis = torch.empty(n, dtype=torch.float64, device=params.device)
    for a in range(0, n, int(max_batch)):
        b = min(n, a + int(max_batch))
        m, _, _, cP = sampler.misfit(params[a:b].contiguous(), rows=None if rows is None else rows[a:b], return_c=True)
        pred[a:b], mis[a:b] = cP, m
    return pred, mis, mis == FAIL


def _fit(torch, sampler, mean, obs_rows_t):
    """(pred_mean - obs) / uncer where the observation is used, NaN elsewhere."""
    c_obs, uncer, mask = sampler.c_obs, sampler.uncer, sampler.mask
    if c_obs.ndim == 2:
        i = obs_rows_t.to(c_obs.device)
        c_obs, uncer, mask = c_obs[i], uncer[i], mask[i]
    c_obs, uncer, mask = (t.to(mean.device) for t in (c_obs, uncer, mask))
    return torch.where(mask.expand_as(mean), (mean - c_obs) / uncer, torch.full_like(mean, float("nan")))


def predictive_reference(sampler, track, obs_rows=None, true_markov_chain=True, chainL=None, prefix=None, hist=None,
                         quantiles=(0.16, 0.5, 0.84), max_batch=65536):
    """The statement of ``posterior_predictive`` in numpy float64, without deduplication: ``select_reference`` expands every final
    row to its source parameters, all of them are predicted by ``sampler.misfit`` (a sampler on any device, or one with the
    ``forward=`` hook), and ``np.mean / np.std / np.min / np.max / np.histogram`` run over the rows that are not failed (per
    column: over their finite values).  ``min_pred`` is the prediction of the source of ``imin``; ``misfit_dev`` the largest
    ``|recomputed - recorded|`` misfit over the source rows (a recorded NaN counts as inf).  ``track``: CPU tensor or array.
    Returns the dict of ``posterior_predictive``, CPU tensors."""
    import torch
    tr = track.detach().cpu().numpy() if isinstance(track, torch.Tensor) else np.asarray(track)
    tr = np.asarray(tr, dtype=np.float64)
    P, obs_rows, _, _, hist = _predictive_args(sampler, tr.shape, obs_rows, chainL, prefix, hist, max_batch)
    npnt, R, W = tr.shape
    mis, imin, thres, final, src = select_reference(tr, true_markov_chain, chainL, prefix)
    pts, fin_rows = np.nonzero(final)                                     # (point, row) order
    src_rows = src[pts, fin_rows]
    dev = sampler.device
    params = torch.as_tensor(tr[pts, src_rows, 3:], dtype=torch.float64, device=dev)
    rows_t = None if obs_rows is None else torch.as_tensor(obs_rows[pts], device=dev)
    pred, rmis, failed = _predict(sampler, params, rows_t, max_batch)
    pred, rmis, failed = pred.cpu().numpy(), rmis.cpu().numpy(), failed.cpu().numpy()
    out = dict(min_misfit=mis[np.arange(npnt), imin], thres=thres, imin=imin.astype(np.int64),
               n_final=final.sum(axis=1).astype(np.int64), n_sources=np.zeros(npnt, np.int64), n_failed=np.zeros(npnt, np.int64),
               count=np.zeros((npnt, P), np.int32), min_pred=np.full((npnt, P), np.nan), misfit_dev=np.full(npnt, np.nan))
    for k in ("pred_mean", "pred_std", "pred_min", "pred_max"):
        out[k] = np.full((npnt, P), np.nan)
    if hist is not None:
        vlo, vhi, nbins = hist
        out.update(hist=np.zeros((npnt, P, nbins), np.int32), below=np.zeros((npnt, P), np.int32),
                   above=np.zeros((npnt, P), np.int32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # all-NaN columns: NaN is the answer
        for p in range(npnt):
            sel = pts == p
            if not sel.any():
                continue
            out["n_sources"][p] = np.unique(src_rows[sel]).size
            out["n_failed"][p] = failed[sel].sum()
            d = np.abs(rmis[sel] - tr[p, src_rows[sel], 0])
            out["misfit_dev"][p] = np.where(np.isnan(d), np.inf, d).max()
            at = np.nonzero(fin_rows[sel] == imin[p])[0]
            if at.size:
                out["min_pred"][p] = pred[sel][at[0]]
            for k, v in _column_statistics(pred[sel][~failed[sel]], "pred_", hist).items():
                out[k][p] = v
    out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}
    out["fit"] = _fit(torch, sampler, out["pred_mean"], None if obs_rows is None else torch.as_tensor(obs_rows))
    if hist is not None:
        out["quantiles"] = quantiles_from_hist(out["hist"], vlo, vhi, quantiles)
    return out


def posterior_sources(track, true_markov_chain=True, chainL=None, prefix=None):
    """One call of ``surfdisp_posterior_sources_device`` on a float64 device track ``[points, R, >= 3]`` (read in place): dict of
    device tensors ``min_misfit, thres`` float64, ``imin, n_final, n_sources, imin_source`` int32 ``[points]`` and ``weight`` int32
    ``[points, R]`` - how many final rows carry the parameters of row r."""
    import torch
    npnt, R, W = track.shape
    chainL, prefix = _prefix_args(R, chainL, prefix)
    f64, i32 = torch.float64, torch.int32
    return _entry_call("surfdisp_posterior_sources_device", track.device, ("surfdisp_posterior_sources_workspace_bytes", npnt, R),
                       (npnt, R, _ptr(track), W, 1 if true_markov_chain else 0, chainL, prefix),
                       dict(min_misfit=(npnt, f64), thres=(npnt, f64), imin=(npnt, i32), n_final=(npnt, i32), weight=((npnt, R), i32),
                            n_sources=(npnt, i32), imin_source=(npnt, i32)))


def predictive_statistics(pred, failed, w, offsets, hist=None):
    """One call of ``surfdisp_posterior_predictive_device``: ``pred`` float32 ``[total, P]`` (rows ``pred.stride(0)`` apart),
    ``failed`` uint8 ``[total]`` or None, ``w`` int32 ``[total]``, ``offsets`` int32 ``[points + 1]``, all on one device;
    ``hist`` None or ``(vlo [P], vhi [P], nbins)`` as ``_hist_args(hist, P)`` returns it.  Dict of device tensors ``count`` int32 and
    ``pred_mean, pred_std, pred_min, pred_max`` float64 ``[points, P]``, ``n_failed`` int32 ``[points]``, and with ``hist``
    ``hist [points, P, nbins]``, ``below``, ``above``."""
    import torch
    total, P = pred.shape
    npnt = offsets.numel() - 1
    f64, i32 = torch.float64, torch.int32
    vlo, vhi, nbins = hist if hist is not None else (None, None, 0)
    if hist is not None:
        vlo, vhi = np.ascontiguousarray(vlo, np.float64), np.ascontiguousarray(vhi, np.float64)
    host = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    return _entry_call(
        "surfdisp_posterior_predictive_device", pred.device, ("surfdisp_posterior_predictive_workspace_bytes", npnt, total, P),
        (npnt, total, P, _ptr(pred), pred.stride(0) if total else P, _ptr(failed), _ptr(w), _ptr(offsets), nbins, host(vlo), host(vhi)),
        dict(count=((npnt, P), i32), pred_mean=((npnt, P), f64), pred_std=((npnt, P), f64), pred_min=((npnt, P), f64),
             pred_max=((npnt, P), f64), n_failed=(npnt, i32), **_hist_outputs(hist, npnt, P)))


def posterior_predictive(sampler, track, obs_rows=None, true_markov_chain=True, chainL=None, prefix=None, hist=None,
                         quantiles=(0.16, 0.5, 0.84), max_batch=65536):
    """Posterior predictive curves of every point of a device track ``[points, R, 3 + N]`` (float64, read in place) under the
    data of ``sampler``, a ``MetropolisBatch`` on the track's device (``(periods, c_obs, uncer)`` or ``data=``; P = its data
    columns).  ``obs_rows`` ``[points]``: the row of the sampler's per-chain observations / local information each point
    belongs to (default: point p reads row p).

    1. ``surfdisp_posterior_sources_device``: the selection (module docstring) and ``weight [points, R]`` - with
       ``true_markov_chain`` a rejected row carries the parameters of the last accepted row before it, so the distinct models
       among the final rows are about (accept rate) of them;
    2. ``torch.nonzero(weight)`` - the ONE host synchronisation of the call (the host must know the batch size) - lists the
       source rows in (point, row) order; their parameters are gathered from the track;
    3. every source row is solved once by ``sampler.misfit(..., return_c=True)`` - ``to_model`` and the batched solver, exactly as
       the sampler fitted it - in slices of ``max_batch`` rows;
    4. ``surfdisp_posterior_predictive_device``: weighted statistics per point and data column.  A row is FAILED when the
       sampler's misfit rule fails it (88888); an entry counts when its row is not failed and its value is finite; the result
       equals the unweighted statistics of the list with every row repeated ``weight`` times (std: population).

    ``hist``: None or ``(vlo, vhi, nbins)`` with scalars or ``[P]`` arrays - one range per data column.
    Returns a dict of device tensors: ``min_misfit, thres`` float64, ``imin, n_final, n_sources, n_failed`` int64 ``[points]``;
    ``count`` int32, ``pred_mean, pred_std, pred_min, pred_max`` float64 ``[points, P]`` (NaN where count is 0); ``min_pred``
    ``[points, P]``: the curve of ``minMod``, taken from the list; ``fit`` ``[points, P]``: ``(pred_mean - obs) / uncer`` where the
    observation is used, NaN elsewhere; ``misfit_dev`` ``[points]``: the largest ``|recomputed - recorded|`` misfit over the
    solved source rows (each is an accepted row, or row 0, so its recorded misfit is that of its own parameters: the staleness
    check of a loaded track; a recorded NaN counts as inf); with ``hist``: ``hist [points, P, nbins]``, ``below``, ``above``,
    ``quantiles [points, P, Q]``.  Raises ``ValueError`` for shapes that do not fit (checked first, so also without a device)
    and for a sampler with the ``forward=`` hook or on another device, ``SurfdispError`` for a track that is not on a HIP device."""
    import torch
    if not isinstance(track, torch.Tensor):
        raise ValueError("track must be a float64 tensor [points, R, 3 + N]")
    P, obs_rows, _, _, hist = _predictive_args(sampler, tuple(track.shape), obs_rows, chainL, prefix, hist, max_batch)
    if track.dtype != torch.float64:
        raise ValueError("track must be float64 [points, R, 3 + N]")
    if getattr(sampler, "_forward", None) is not None:
        raise ValueError("posterior_predictive solves on the device: a sampler with the forward= hook goes through predictive_reference")
    if track.device.type != "cuda":
        raise _lib.SurfdispError("posterior_predictive needs a track on a HIP device (no CPU fallback: predictive_reference is the host statement)")
    if sampler.device != track.device:
        raise ValueError(f"the sampler is on {sampler.device}, the track on {track.device}")
    track = track.contiguous()
    npnt, R, W = track.shape
    dev = track.device
    src = posterior_sources(track, true_markov_chain, chainL, prefix)
    weight = src["weight"]
    nz = torch.nonzero(weight)                                            # (point, row) order; the one host synchronisation
    pt, row = nz[:, 0], nz[:, 1]
    total = int(nz.shape[0])
    w = weight[pt, row].contiguous()
    offsets = torch.zeros(npnt + 1, dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(src["n_sources"], dim=0)
    rows_all = None if obs_rows is None else torch.as_tensor(obs_rows, device=dev)
    pred64, mis, failed = _predict(sampler, track[pt, row, 3:], None if rows_all is None else rows_all[pt], max_batch)
    pred = pred64.to(torch.float32).contiguous()                          # (the solver's own fp32 values: exact)
    o = predictive_statistics(pred, failed.to(torch.uint8).contiguous(), w, offsets, hist)
    d = torch.nan_to_num((mis - track[pt, row, 0]).abs(), nan=float("inf"))
    o["misfit_dev"] = torch.full((npnt,), float("nan"), dtype=torch.float64, device=dev).scatter_reduce(0, pt, d, "amax", include_self=False)
    key = pt * R + row                                                    # ascending: the list position of (point, imin_source)
    want = torch.arange(npnt, device=dev) * R + src["imin_source"].to(torch.int64)
    at = torch.searchsorted(key, want).clamp(max=max(total - 1, 0))
    o["min_pred"] = torch.full((npnt, P), float("nan"), dtype=torch.float64, device=dev)
    if total:
        found = key[at] == want
        o["min_pred"] = torch.where(found[:, None], pred[at].to(torch.float64), o["min_pred"])
    o["fit"] = _fit(torch, sampler, o["pred_mean"], rows_all)
    for k in ("min_misfit", "thres"):
        o[k] = src[k]
    for k in ("imin", "n_final", "n_sources"):
        o[k] = src[k].to(torch.int64)
    o["n_failed"] = o["n_failed"].to(torch.int64)
    if hist is not None:
        o["quantiles"] = quantiles_from_hist(o["hist"], hist[0], hist[1], quantiles)
    return o
