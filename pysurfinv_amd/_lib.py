"""ctypes binding of libsurfdisp_hip.so (C ABI: include/surfdisp.h).

There is no CPU fallback in this package: if the HIP library is missing, or no
gfx950 device is present, every compute entry point raises.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SURFDISP_LIB_PATH: developer override to load an experimental build of the same library (A/B measurements)
LIB_PATH = os.environ.get("SURFDISP_LIB_PATH") or os.path.join(_HERE, "lib", "libsurfdisp_hip.so")

SUCCESS, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_WORKSPACE = 0, -1, -2, -3, -4
OK, PARTIAL, NOROOT, BADMODEL, NUMERIC = 0, 1, 2, 4, 8
KIND_LOVE, KIND_RAYLEIGH = 1, 2
PHASE_ONLY = 0x10
INDEPENDENT = 0x20
PIPELINED = 0x40
EXACTSCAN = 0x80        # every grid point of the scan (Rayleigh: the default anyway; Love: switches the certified coarse scan off)
FASTSCAN = 0x100        # opt-in count-guided scan (include/surfdisp.h)
STRICT = 0x200          # verification mode: every stack through the statement-by-statement kernel
KERN_REFCOORD = 0x400   # surfdisp_forward_kernels_device: partials in the reference's coordinates (flattened, attenuated layer values)
NPER_MAX, NLAY_MAX = 200, 200

# every symbol include/surfdisp.h declares
EXPORTS = (
    "fast_surf_", "surfdisp_forward_batch", "surfdisp_thread_release", "surfdisp_workspace_bytes",
    "surfdisp_forward_batch_device", "surfdisp_forward_batch_device2", "surfdisp_forward_batch_device_timed",
    "surfdisp_forward_batch_device_events", "surfdisp_events_create", "surfdisp_events_destroy",
    "surfdisp_events_elapsed_ms", "surfdisp_stream_wait_event", "surfdisp_params_to_model_device",
    "surfdisp_params_to_model_thermal_device", "surfdisp_thermal_scratch_bytes",
    "surfdisp_mcmc_propose_device", "surfdisp_mcmc_accept_device", "surfdisp_prior_device", "surfdisp_mcmc_propose_masked_device", "surfdisp_mcmc_propose_tree_device", "surfdisp_mcmc_accept_tree_device",
    "surfdisp_mcmc_propose_prior_device", "surfdisp_mcmc_propose_cov_device", "surfdisp_mcmc_cov_factor_device", "surfdisp_mcmc_adapt_device", "surfdisp_mcmc_accept_joint_device", "surfdisp_mcmc_accept_tree_joint_device",
    "surfdisp_mcmc_accept_joint5_device", "surfdisp_mcmc_accept_tree_joint5_device", "surfdisp_forward_batch_device2_events",
    "surfdisp_forward_kernels_device", "surfdisp_kernels_workspace_bytes",
    "surfdisp_forward_group_kernels_device", "surfdisp_group_kernels_workspace_bytes",
    "surfdisp_forward_ellip_kernels_device", "surfdisp_ellip_kernels_workspace_bytes",
    "surfdisp_forward_atten_device", "surfdisp_atten_workspace_bytes", "surfdisp_forward_eigen_device", "surfdisp_eigen_workspace_bytes",
    "surfdisp_forward_thickness_kernels_device", "surfdisp_thickness_kernels_workspace_bytes",
    "surfdisp_forward_group_thickness_kernels_device", "surfdisp_group_thickness_kernels_workspace_size",
    "surfdisp_lsq_step_device", "surfdisp_lsq_resolution_device",
    "surfdisp_lsq_step_modes_device", "surfdisp_lsq_resolution_modes_device",
    "surfdisp_params_jacobian_device", "surfdisp_lsq_step_params_device",
    "surfdisp_posterior_profile_device", "surfdisp_posterior_workspace_bytes",
    "surfdisp_posterior_sources_device", "surfdisp_posterior_sources_workspace_bytes",
    "surfdisp_posterior_predictive_device", "surfdisp_posterior_predictive_workspace_bytes", "surfdisp_workspace_fallback_count", "surfdisp_workspace_counters", "surfdisp_set_team", "surfdisp_get_team", "surfdisp_get_team2",
    "surfdisp_device_count", "surfdisp_abi_version", "surfdisp_last_error",
    "surfdisp_kernel_name",
)


class SurfdispError(RuntimeError):
    pass


_lib = None


def lib() -> ctypes.CDLL:
    """Load the HIP library; raises SurfdispError (never falls back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SurfdispError(
            f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). pysurfinv_amd has no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.  If this library
    # pulled in /opt/rocm's copy first, a later ``import torch`` would bring up a second runtime that
    # sees no GPU.  So when torch is installed let it load its runtime first; the dynamic linker then
    # binds libsurfdisp_hip.so's libamdhip64.so.N dependency to that same copy.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    fp = ctypes.POINTER(ctypes.c_float)
    ip = ctypes.POINTER(ctypes.c_int)
    vp = ctypes.c_void_p
    L.fast_surf_.restype = None
    L.fast_surf_.argtypes = [ip, ip, fp, fp, fp, fp, fp, fp, ip, fp, fp, fp, fp]
    L.surfdisp_forward_batch.restype = ctypes.c_int
    L.surfdisp_forward_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, fp,
                                         ctypes.c_int, fp, ctypes.c_int, fp, fp, ip]
    L.surfdisp_workspace_bytes.restype = ctypes.c_size_t
    L.surfdisp_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.surfdisp_kernels_workspace_bytes.restype = ctypes.c_size_t
    L.surfdisp_kernels_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.surfdisp_forward_batch_device.restype = ctypes.c_int
    L.surfdisp_forward_batch_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                                ctypes.c_int, vp, ctypes.c_int, vp, vp, vp,
                                                vp, ctypes.c_size_t]
    L.surfdisp_forward_batch_device2.restype = ctypes.c_int
    L.surfdisp_forward_batch_device2.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                                 ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, vp,
                                                 vp, ctypes.c_size_t]
    L.surfdisp_forward_batch_device_timed.restype = ctypes.c_int
    L.surfdisp_forward_batch_device_timed.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                                      ctypes.c_int, vp, ctypes.c_int, vp, vp, vp,
                                                      vp, ctypes.c_size_t, fp]
    L.surfdisp_forward_batch_device_events.restype = ctypes.c_int
    L.surfdisp_forward_batch_device_events.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                                       ctypes.c_int, vp, ctypes.c_int, vp, vp, vp,
                                                       vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    if hasattr(L, "surfdisp_forward_batch_device2_events"):   # (absent from an older build loaded through SURFDISP_LIB_PATH)
        L.surfdisp_forward_batch_device2_events.restype = ctypes.c_int
        L.surfdisp_forward_batch_device2_events.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                                            ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, vp,
                                                            vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    L.surfdisp_events_create.restype = ctypes.c_int
    L.surfdisp_events_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.surfdisp_events_destroy.restype = ctypes.c_int
    L.surfdisp_events_destroy.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.surfdisp_stream_wait_event.restype = ctypes.c_int
    L.surfdisp_stream_wait_event.argtypes = [vp, vp]
    L.surfdisp_events_elapsed_ms.restype = ctypes.c_int
    L.surfdisp_events_elapsed_ms.argtypes = [vp, vp, fp]
    L.surfdisp_params_to_model_device.restype = ctypes.c_int
    L.surfdisp_params_to_model_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    L.surfdisp_forward_kernels_device.restype = ctypes.c_int
    L.surfdisp_forward_kernels_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int,
                                                  vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
    L.surfdisp_group_kernels_workspace_bytes.restype = ctypes.c_size_t
    L.surfdisp_group_kernels_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.surfdisp_forward_group_kernels_device.restype = ctypes.c_int
    L.surfdisp_forward_group_kernels_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int,
                                                        ctypes.c_float, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
    L.surfdisp_ellip_kernels_workspace_bytes.restype = ctypes.c_size_t
    L.surfdisp_ellip_kernels_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.surfdisp_forward_ellip_kernels_device.restype = ctypes.c_int
    L.surfdisp_forward_ellip_kernels_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int,
                                                        vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
    L.surfdisp_atten_workspace_bytes.restype = ctypes.c_size_t
    L.surfdisp_atten_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.surfdisp_forward_atten_device.restype = ctypes.c_int
    L.surfdisp_forward_atten_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int,
                                                vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
    if hasattr(L, "surfdisp_forward_eigen_device"):           # (absent from an older build loaded through SURFDISP_LIB_PATH)
        L.surfdisp_eigen_workspace_bytes.restype = ctypes.c_size_t
        L.surfdisp_eigen_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        # (stream, B, Lmax, nlay, model, P, per, kind, c, u, status, ur, uz, tz, tr, energy, workspace, workspace_bytes)
        L.surfdisp_forward_eigen_device.restype = ctypes.c_int
        L.surfdisp_forward_eigen_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int,
                                                    vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
    if hasattr(L, "surfdisp_forward_thickness_kernels_device"):   # (absent from an older build loaded through SURFDISP_LIB_PATH)
        L.surfdisp_thickness_kernels_workspace_bytes.restype = ctypes.c_size_t
        L.surfdisp_thickness_kernels_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        # (stream, B, Lmax, nlay, model, P, per, kind, c, u, status, dcdb, dcda, dcdr, dcdh, dcdz, n_nonfinite, workspace, workspace_bytes)
        L.surfdisp_forward_thickness_kernels_device.restype = ctypes.c_int
        L.surfdisp_forward_thickness_kernels_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int,
                                                                vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
    if hasattr(L, "surfdisp_forward_group_thickness_kernels_device"):   # (absent from an older build loaded through SURFDISP_LIB_PATH)
        L.surfdisp_group_thickness_kernels_workspace_size.restype = ctypes.c_size_t
        L.surfdisp_group_thickness_kernels_workspace_size.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        # (stream, B, Lmax, nlay, model, P, per, kind, dlnT_frac, c, u, status, dcdb, dcda, dcdr, dudb, duda, dudr, dcdh, dcdz, dudh, dudz,
        #  n_shift_failed, n_nonfinite, workspace, workspace_bytes)
        L.surfdisp_forward_group_thickness_kernels_device.restype = ctypes.c_int
        L.surfdisp_forward_group_thickness_kernels_device.argtypes = ([vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int,
                                                                       ctypes.c_float] + [vp] * 16 + [ctypes.c_size_t])
    L.surfdisp_group_kernels_shift_offset.restype = ctypes.c_size_t     # test read-out (not in include/surfdisp.h)
    L.surfdisp_group_kernels_shift_offset.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.surfdisp_workspace_prep_offsets.restype = ctypes.c_int           # test read-out (not in include/surfdisp.h)
    L.surfdisp_workspace_prep_offsets.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    L.surfdisp_thermal_scratch_bytes.restype = ctypes.c_size_t
    L.surfdisp_thermal_scratch_bytes.argtypes = [ctypes.c_int]
    L.surfdisp_params_to_model_thermal_device.restype = ctypes.c_int
    L.surfdisp_params_to_model_thermal_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp,
                                                          vp, ctypes.c_size_t, vp]
    u64 = ctypes.c_ulonglong
    L.surfdisp_mcmc_propose_device.restype = ctypes.c_int
    L.surfdisp_mcmc_propose_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, u64, u64, ctypes.c_int, vp, ctypes.c_long]
    if hasattr(L, "surfdisp_prior_device"):                    # (absent from an r03 build loaded through SURFDISP_LIB_PATH for A/B runs)
        L.surfdisp_mcmc_propose_masked_device.restype = ctypes.c_int
        L.surfdisp_mcmc_propose_masked_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, u64, u64, ctypes.c_int, ctypes.c_int,
                                                          vp, ctypes.c_int, vp, ctypes.c_long]
        L.surfdisp_prior_device.restype = ctypes.c_int
        L.surfdisp_prior_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_double, ctypes.c_int,
                                            ctypes.c_int, vp]
    L.surfdisp_mcmc_propose_tree_device.restype = ctypes.c_int
    L.surfdisp_mcmc_propose_tree_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, u64, u64, vp, ctypes.c_long]
    if hasattr(L, "surfdisp_mcmc_propose_prior_device"):       # (absent from an older build loaded through SURFDISP_LIB_PATH)
        # (stream, C, N, K, L, depth, p, aux, vmin, vmax, step, idesc, fdesc, flags, vs_max, gauss_tries, uniform_tries, seed, counter,
        #  chain0, out, tries, exhausted)
        L.surfdisp_mcmc_propose_prior_device.restype = ctypes.c_int
        L.surfdisp_mcmc_propose_prior_device.argtypes = ([vp] + [ctypes.c_int] * 5 + [vp] * 8 + [ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                                         u64, u64, ctypes.c_long, vp, vp, vp])
    if hasattr(L, "surfdisp_mcmc_propose_cov_device"):         # (absent from an older build loaded through SURFDISP_LIB_PATH)
        # (stream, C, N, K, L, depth, p, aux, vmin, vmax, factor_t, chains_per_factor, F, idesc, fdesc, flags, vs_max, gauss_tries,
        #  uniform_tries, seed, counter, chain0, out, tries, exhausted)
        L.surfdisp_mcmc_propose_cov_device.restype = ctypes.c_int
        L.surfdisp_mcmc_propose_cov_device.argtypes = ([vp] + [ctypes.c_int] * 5 + [vp] * 5 + [ctypes.c_long, ctypes.c_int] + [vp] * 3
                                                       + [ctypes.c_double, ctypes.c_int, ctypes.c_int, u64, u64, ctypes.c_long, vp, vp, vp])
        # (stream, P, N, cov, scale, fallback_step, factor_t, flag)
        L.surfdisp_mcmc_cov_factor_device.restype = ctypes.c_int
        L.surfdisp_mcmc_cov_factor_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_double, vp, vp, vp]
    if hasattr(L, "surfdisp_mcmc_adapt_device"):               # (absent from an older build loaded through SURFDISP_LIB_PATH)
        # (stream, F, cpp, N, p, track, chain_stride, row_stride, row_lo, row_hi, step, forget, target_accept, gain, decay, ls_min,
        #  ls_max, min_weight, ridge, state, cov_out)
        L.surfdisp_mcmc_adapt_device.restype = ctypes.c_int
        L.surfdisp_mcmc_adapt_device.argtypes = ([vp] + [ctypes.c_int] * 3 + [vp, vp, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                                 vp] + [ctypes.c_double] * 8 + [vp, vp])
    # the accept entries: (stream, C, N, [P,] [depth, nsteps,] predictions, c_obs, uncer, mask, obs_per_chain, p1, p0, chi0, row,
    # row_stride, [step_stride,] seed, counter, [first,] chain0) - P and the predictions differ between the Rayleigh-phase entries
    # and the joint ones, the tree entries take depth, nsteps and step_stride in place of first
    vpp, lp, ipp = ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_int)
    pred_c, pred_joint = [vp, vp], [vpp, lp, ipp, vpp, ctypes.c_int, vp, vp]
    for name, tree, head, pred in (("surfdisp_mcmc_accept_device", False, [ctypes.c_int], pred_c),
                                   ("surfdisp_mcmc_accept_tree_device", True, [ctypes.c_int], pred_c),
                                   ("surfdisp_mcmc_accept_joint_device", False, [], pred_joint),
                                   ("surfdisp_mcmc_accept_tree_joint_device", True, [], pred_joint),
                                   ("surfdisp_mcmc_accept_joint5_device", False, [], pred_joint),
                                   ("surfdisp_mcmc_accept_tree_joint5_device", True, [], pred_joint)):
        if pred is pred_c or hasattr(L, name):                 # (the joint entries: absent from an older build loaded through SURFDISP_LIB_PATH)
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = ([vp, ctypes.c_int, ctypes.c_int] + head + ([ctypes.c_int, ctypes.c_int] if tree else []) + pred
                                         + [vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_long] + ([ctypes.c_long] if tree else [])
                                         + [u64, u64] + ([] if tree else [ctypes.c_int]) + [ctypes.c_long])
    # (stream, B, Lmax, nlay, model, free_mask, free_per_stack, nfree_max, part[15], pred[5], pred_stride[5], nper[2], N, cols, weights,
    #  obs, uncer, mask, obs_per_stack, vp_slope, rho_slope, slope_per_stack, alpha, Q, q_per_stack, lam, delta, stats, info)
    L.surfdisp_lsq_step_device.restype = ctypes.c_int
    L.surfdisp_lsq_step_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_int, vpp, vpp, lp, ipp,
                                           ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_int, vp, vp, ctypes.c_int,
                                           ctypes.c_double, vp, ctypes.c_int, vp, vp, vp, vp]
    # the same up to lam, then (cov, res, sigma_post, sigma_data, rdiag, stats, info)
    if hasattr(L, "surfdisp_lsq_resolution_device"):          # (absent from an older build loaded through SURFDISP_LIB_PATH)
        L.surfdisp_lsq_resolution_device.restype = ctypes.c_int
        L.surfdisp_lsq_resolution_device.argtypes = L.surfdisp_lsq_step_device.argtypes[:-3] + [vp] * 7
    # the same up to lam, then (K, modes, modes_per_stack, part_h[5], mode_scale, mode_prior, mode_y) and the outputs
    # (delta, delta_y, stats, info) / (cov, res, sigma_post, sigma_data, rdiag, sigma_post_y, sigma_data_y, rdiag_y, stats, info)
    if hasattr(L, "surfdisp_lsq_step_modes_device"):          # (absent from an older build loaded through SURFDISP_LIB_PATH)
        mode_in = [ctypes.c_int, vp, ctypes.c_int, vpp, vp, vp, vp]
        L.surfdisp_lsq_step_modes_device.restype = ctypes.c_int
        L.surfdisp_lsq_step_modes_device.argtypes = L.surfdisp_lsq_step_device.argtypes[:-3] + mode_in + [vp] * 4
        L.surfdisp_lsq_resolution_modes_device.restype = ctypes.c_int
        L.surfdisp_lsq_resolution_modes_device.argtypes = L.surfdisp_lsq_step_device.argtypes[:-3] + mode_in + [vp] * 10
    if hasattr(L, "surfdisp_params_jacobian_device"):         # (absent from an older build loaded through SURFDISP_LIB_PATH)
        # (stream, C, N, Nu, L, params, idesc, fdesc, layer, jac)
        L.surfdisp_params_jacobian_device.restype = ctypes.c_int
        L.surfdisp_params_jacobian_device.argtypes = [vp] + [ctypes.c_int] * 4 + [vp] * 5
        # (stream, B, Lmax, nlay, Nu, jac, part[15], part_h[5], pred[5], pred_stride[5], nper[2], N, cols, weights, obs, uncer, mask,
        #  obs_per_stack, free, free_per_stack, scale, prior_w, prior_ref, params, Np, lam, delta, stats, info, cov, sigma, logdet)
        L.surfdisp_lsq_step_params_device.restype = ctypes.c_int
        L.surfdisp_lsq_step_params_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, vpp, vpp, vpp, lp, ipp,
                                                      ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_int, vp, ctypes.c_int,
                                                      vp, vp, vp, vp, ctypes.c_int, vp] + [vp] * 6
    # (stream, npoints, R, N, track, row_stride, idesc (host), idesc_len, fdesc, aux, K, rows, D, zdeps (host), true_markov_chain, chainL,
    #  prefix, nbins, vlo, vhi, min_misfit, thres, imin, n_final, pmean, pstd, count, vs_mean, vs_std, vs_min, vs_max, hist, below, above,
    #  workspace, workspace_bytes)
    if hasattr(L, "surfdisp_posterior_profile_device"):       # (absent from an older build loaded through SURFDISP_LIB_PATH)
        L.surfdisp_posterior_workspace_bytes.restype = ctypes.c_size_t
        L.surfdisp_posterior_workspace_bytes.argtypes = [ctypes.c_int] * 4
        L.surfdisp_posterior_profile_device.restype = ctypes.c_int
        L.surfdisp_posterior_profile_device.argtypes = ([vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_long, vp, ctypes.c_int, vp,
                                                         vp, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_int, ctypes.c_double, ctypes.c_double] + [vp] * 14 + [vp, ctypes.c_size_t])
    if hasattr(L, "surfdisp_posterior_sources_device"):       # (absent from an older build loaded through SURFDISP_LIB_PATH)
        # (stream, npoints, R, track, row_stride, true_markov_chain, chainL, prefix, min_misfit, thres, imin, n_final, weight, n_sources,
        #  imin_source, workspace, workspace_bytes)
        L.surfdisp_posterior_sources_workspace_bytes.restype = ctypes.c_size_t
        L.surfdisp_posterior_sources_workspace_bytes.argtypes = [ctypes.c_int] * 2
        L.surfdisp_posterior_sources_device.restype = ctypes.c_int
        L.surfdisp_posterior_sources_device.argtypes = ([vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_int] + [vp] * 7 + [vp, ctypes.c_size_t])
        # (stream, npoints, total, P, pred, ld, failed, w, offsets, nbins, vlo (host), vhi (host), count, mean, std, min, max, n_failed,
        #  hist, below, above, workspace, workspace_bytes)
        L.surfdisp_posterior_predictive_workspace_bytes.restype = ctypes.c_size_t
        L.surfdisp_posterior_predictive_workspace_bytes.argtypes = [ctypes.c_int] * 3
        L.surfdisp_posterior_predictive_device.restype = ctypes.c_int
        L.surfdisp_posterior_predictive_device.argtypes = ([vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_long, vp, vp, vp,
                                                            ctypes.c_int, vp, vp] + [vp] * 9 + [vp, ctypes.c_size_t])
    L.surfdisp_thread_release.restype = None
    L.surfdisp_thread_release.argtypes = []
    L.surfdisp_workspace_fallback_count.restype = ctypes.c_int
    L.surfdisp_workspace_fallback_count.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ip]
    if hasattr(L, "surfdisp_workspace_counters"):              # (absent from an r03 build loaded through SURFDISP_LIB_PATH for A/B runs)
        L.surfdisp_workspace_counters.restype = ctypes.c_int
        L.surfdisp_workspace_counters.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ip]
    L.surfdisp_set_team.restype = ctypes.c_int
    L.surfdisp_set_team.argtypes = [ctypes.c_int]
    L.surfdisp_get_team.restype = ctypes.c_int
    L.surfdisp_get_team.argtypes = [ctypes.c_int, ctypes.c_int]
    L.surfdisp_get_team2.restype = ctypes.c_int
    L.surfdisp_get_team2.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.surfdisp_device_count.restype = ctypes.c_int
    L.surfdisp_abi_version.restype = ctypes.c_int
    L.surfdisp_last_error.restype = ctypes.c_char_p
    L.surfdisp_kernel_name.restype = ctypes.c_char_p
    L.surfdisp_kernel_name.argtypes = [ctypes.c_int]
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != SUCCESS:
        msg = lib().surfdisp_last_error().decode(errors="replace")
        raise SurfdispError(f"libsurfdisp_hip error {rc}: {msg}")


def source_hash():
    """sha256 (16 hex digits) over the library's sources (csrc/*.hip, *.h, Makefile, include/surfdisp.h): what a counter
    profile under profiles/ is tagged with beside the binary's own hash - hipcc's output is not bit-reproducible, so a
    rebuilt library keeps the source tag while its binary hash changes."""
    import glob
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "csrc", "*.hip")) + glob.glob(os.path.join(here, "csrc", "*.h"))
                   + [os.path.join(here, "csrc", "Makefile"), os.path.join(os.path.dirname(here), "include", "surfdisp.h")])
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]
