/*
 * surfdisp.h -- C ABI of libsurfdisp_hip.so: MI355X (gfx950) batched surface-wave
 * dispersion forward solver, drop-in for pySurfInv's fast_surf() path.
 *
 * Boundary replaced (reference 001cat/pySurfInv):
 *   - Fortran entry   SUBROUTINE FAST_SURF(n_layer0,kind0,a_ref0,b_ref0,rho_ref0,d_ref0,
 *                     qs_ref0,cvper,ncvper,uR0,uL0,cR0,cL0)      fast_surf_src/fast_surf.f:2-5
 *   - f2py signature  fast_surf(nlay,ilvry,Vp,Vs,rho,h,qsinv,per,nper)->(ur0,ul0,cr0,cl0)
 *                                                                 fast_surf_src/fast_surf.pyf:6-19
 *   - call sites      models.py:27 (_calForward), senskernel.py:188 (SensKernelPert._forward)
 *
 * Plain pointers and sizes only; no torch / C++ types.  The solve entry points keep no state between
 * calls (the reference does: COMMON blocks, fast_surf.f:48-71) and may be called from several threads;
 * surfdisp_set_team and the environment knobs are process-wide tuning state.
 *
 * Conventions kept from the reference:
 *   - argument order (Vp, Vs, rho, h, 1/Qs)                       fast_surf.f:2-5,44-45
 *   - kind / ilvry: 1 = Love, 2 = Rayleigh                        models.py:13-16
 *   - last layer is the half-space, its thickness is ignored       flat1.f:69
 *   - a top layer with Vs < 0.1 is water                          fast_surf.f:158,171
 *   - no exceptions: unsolved periods are 0 in c and U             fast_surf.f:197, calcul.f:203-219
 *   - periods must be ascending; outputs depend on the period LIST (mmax carry-over,
 *     start rule c1 = 0.9*c(k-1): calcul.f:112,133,143)
 *   - "fresh process" state for every solve (ndiv = 5, init.f:25)
 */
#ifndef SURFDISP_H
#define SURFDISP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SURFDISP_ABI_VERSION 4      /* 4 (r04): + SURFDISP_KERN_REFCOORD, surfdisp_workspace_counters, surfdisp_prior_device, surfdisp_mcmc_propose_masked_device; every ABI-3 symbol kept;
                                       additive, same version: surfdisp_forward_group_kernels_device, surfdisp_group_kernels_workspace_bytes,
                                       surfdisp_forward_ellip_kernels_device, surfdisp_ellip_kernels_workspace_bytes,
                                       surfdisp_mcmc_accept_joint5_device, surfdisp_mcmc_accept_tree_joint5_device, surfdisp_forward_batch_device2_events,
                                       surfdisp_lsq_step_device, surfdisp_lsq_resolution_device,
                                       surfdisp_forward_atten_device, surfdisp_atten_workspace_bytes,
                                       surfdisp_forward_eigen_device, surfdisp_eigen_workspace_bytes,
                                       surfdisp_posterior_profile_device, surfdisp_posterior_workspace_bytes,
                                       surfdisp_posterior_sources_device, surfdisp_posterior_sources_workspace_bytes,
                                       surfdisp_posterior_predictive_device, surfdisp_posterior_predictive_workspace_bytes */
#define SURFDISP_NPER_MAX 200      /* fast_surf.pyf:14-19: cvper and outputs are real*4[200] */
#define SURFDISP_NLAY_MAX 200      /* layers per stack accepted by this library */

#define SURFDISP_KIND_LOVE     1   /* == reference kind0 / ilvry */
#define SURFDISP_KIND_RAYLEIGH 2
#define SURFDISP_INDEPENDENT   0x20 /* OR into `kind`: one team per (stack, period) root search, every
                                     * period started from the first-period rule (fast_surf.f:157-171) on
                                     * a freshly built stack.  P x more parallelism / P x lower latency
                                     * for small batches; equals the default "faithful" mode to ~1e-6 on
                                     * monotone stacks but NOT on rough ones (low-velocity zones), where
                                     * the reference's sequential start rule picks roots and failures
                                     * (SURVEY.md section 4 defects 2, 9).  Caller opts in. */
#define SURFDISP_PIPELINED     0x40 /* OR into `kind`: a launch hint, results are unchanged.  The caller keeps a
                                     * second batch of this size in flight on another stream, so the lanes per
                                     * stack are chosen for twice the stacks (fewer lanes per stack waste fewer
                                     * trial velocities; with one batch alone they would leave SIMDs idle) */
#define SURFDISP_EXACTSCAN     0x80 /* OR into `kind`: every grid point of the scan is evaluated.  Rayleigh: that is the default
                                     * anyway (the flag wins over SURFDISP_FASTSCAN).  Love: the default skips grid points
                                     * between two coarse points that a counting theorem (exact arithmetic) shows free of roots,
                                     * behind fp32 guards whose margins are soaked, not proved: same brackets and results, bit for
                                     * bit, on every random stack tried (scripts/soak_cert.py); this flag walks them all. */
#define SURFDISP_FASTSCAN      0x100 /* OR into `kind`: OPT-IN count-guided scan (Rayleigh; Love's certified scan is on by default).
                                     * By default the secular function is evaluated at EVERY 0.01 km/s grid point from
                                     * 0.9 c(k-1) up to the first sign change, as the reference does (calcul.f:143-166).
                                     * With this flag teams of 2..8 lanes evaluate every 4th / 6th grid point together with the
                                     * number of mode branches below the trial (a Wittrick-Williams count carried by the
                                     * recursion: exact in exact arithmetic) and skip the points between two trials with EQUAL
                                     * counts; any other interval is rescanned point by point: ~45 % fewer evaluations.  Equal
                                     * counts exclude a root between the two trials unless a branch with a zero-group-velocity
                                     * point is crossed twice there (Rayleigh branches of soft sediments with Vp/Vs near 3 can
                                     * have one; Love branches cannot): bit-identical to the default scan on all but two of
                                     * 1.2e9 random stacks.  Callers who need the reference's root
                                     * selection on every input leave it off.  Also switched on for every call of the process
                                     * by the environment variable SURFDISP_FASTSCAN=1 (read once). */
#define SURFDISP_STRICT        0x200 /* OR into `kind`: verification mode.  EVERY stack is solved by the kernel that restates
                                     * DLTAR4 / DLTAR1 / NEVILL statement by statement (the one the default mode keeps for
                                     * stacks whose secular function leaves the fp32 range): the reference's own matrix-entry
                                     * arithmetic, overflow points and evaluation sequence, several times slower.  The default
                                     * mode agrees with it to ~1e-6 on c; use it to check that on your own models
                                     * (tests/test_gpu_parity.py does, at the bench size), not in production. */
#define SURFDISP_KERN_REFCOORD 0x400 /* OR into `kind` of surfdisp_forward_kernels_device: the analytic partials in the REFERENCE's
                                     * coordinates - with respect to the earth-flattened, attenuation-corrected layer values the
                                     * eigenproblem is solved for (no chain factors of calcul.f:122-126 / flat1.f:44-62), i.e. what
                                     * REIGEN / LEIGEN leave in COMMON /rar1/ (surfa.f:1133-1135, 1182-1184, 1204-1207; Love 511-512,
                                     * 564-565, 582-583) summed over each layer's sublayers; a water layer's own share (which the
                                     * reference does not form) is left out.  The verification mode the reference-generated fixture
                                     * tests/golden/ref_partials.npz is compared in; ignored by the other entries. */
#define SURFDISP_PHASE_ONLY    0x10 /* OR into `kind` of the batched entries: phase velocities only
                                     * (what Point.misfit consumes, point.py:18); u is not written
                                     * and may be NULL */

/* per-model status word (the explicit form of the reference's "zeros in c") */
enum {
    SURFDISP_OK         = 0,   /* all P periods solved */
    SURFDISP_PARTIAL    = 1,   /* bracketing failed at period k>1: c,U of periods k..P are 0 (calcul.f:203,218-219) */
    SURFDISP_NOROOT     = 2,   /* bracketing failed at the first period: everything 0 (calcul.f:203-212) */
    SURFDISP_BADMODEL   = 4,   /* nlay < 2, nlay > Lmax, or non-finite input: everything 0 */
    SURFDISP_NUMERIC    = 8    /* a root at or above 16 km/s: one fp32 ulp (1.9e-6) exceeds NEVILL's 1e-6 bracket
                                * tolerance, the reference exhausts its 50 cycles and the call returns nothing
                                * (surfa.f:17-27, calcul.f:172-189): everything 0, also the periods already solved.
                                * (A secular function that overflows fp32 is not an error - the reference returns
                                * the edge of the overflowed region as a root and so does this library.) */
};

/* return codes */
enum {
    SURFDISP_SUCCESS        = 0,
    SURFDISP_ERR_INVALID    = -1,  /* bad argument (NULL pointer, B<1, P<1 or >200, kind, L range) */
    SURFDISP_ERR_NO_DEVICE  = -2,  /* no gfx950 device / HIP runtime unavailable -- there is NO CPU fallback */
    SURFDISP_ERR_HIP        = -3,  /* a HIP call failed; see surfdisp_last_error() */
    SURFDISP_ERR_WORKSPACE  = -4   /* workspace too small */
};

/* ---- (1) Fortran-ABI drop-in: same symbol name and by-reference convention as the object the
 *          reference builds from fast_surf.f:2-5 (gfortran / flang lower-case + underscore).
 *          Runs ONE stack through the GPU path.  uR/uL/cR/cL are float[200]; only the pair that
 *          matches *kind is written, and only its first imax entries (fast_surf.f:197-208) --
 *          the caller pre-zeroes them exactly as f2py does (intent(out) arrays are zero-filled). */
void fast_surf_(const int *n_layer, const int *kind,
                const float *vp, const float *vs, const float *rho,
                const float *h, const float *qsinv,
                const float *per /*[200]*/, const int *nper,
                float *uR, float *uL, float *cR, float *cL);

/* ---- (2) batched solve, host buffers.
 *   model  [B][5][Lmax]  rows = vp, vs, rho, h, qsinv (the five fast_surf.f:2-5 layer arrays)
 *   nlay   [B] or NULL (every stack has Lmax layers); unused tail entries of a row are ignored
 *   per    [P] ascending periods (s);   kind = 1 Love | 2 Rayleigh
 *   c, u   [B][P] phase / group velocity (km/s), 0 where unsolved;  status [B] or NULL
 * Copies in, runs the kernels on `device`, copies out.  Returns SURFDISP_SUCCESS or an error.
 * The calling THREAD keeps what the call needed on the device for its next call (fast_surf_ too): a small arena + pinned
 * staging buffer for small calls, a grow-only buffer (given back at once beyond 3 GiB) and three streams for large ones,
 * which - stacks of up to 20 layers - go through the device in chunks of ~32 768 stacks taking turns on those streams
 * (copies beside kernels).  surfdisp_thread_release() frees the calling thread's share (a thread that is about to exit
 * calls it; a thread pool need not). */
int surfdisp_forward_batch(int device, int B, int Lmax, const int *nlay, const float *model,
                           int P, const float *per, int kind,
                           float *c, float *u, int *status);
void surfdisp_thread_release(void);

/* ---- (3) batched solve, DEVICE pointers, stream-ordered, no allocation, no host sync:
 *          safe to capture in a hipGraph.  `stream` is a hipStream_t (NULL = default stream).
 *          `workspace` = device buffer of at least surfdisp_workspace_bytes(B, Lmax, P) bytes.
 *          All pointers (nlay, model, per, c, u, status, workspace) are device pointers on the
 *          current device.  nlay and status may be NULL. */
size_t surfdisp_workspace_bytes(int B, int Lmax, int P);
int surfdisp_forward_batch_device(void *stream, int B, int Lmax, const int *nlay,
                                  const float *model, int P, const float *per, int kind,
                                  float *c, float *u, int *status,
                                  void *workspace, size_t workspace_bytes);

/* ---- (3b) ABI 3: the same solve, which also returns the Rayleigh ELLIPTICITY the reference computes and keeps in
 *          COMMON /o/ ratio(k, 1) (calcul.f:195: ratio = dltar(c1, t1, 3), i.e. DLTAR4 with mup = 2, surfa.f:360-363;
 *          f2py exposes the block as a module attribute, fast_surf.pyf:126-140): ratio [B][P], 0 where unsolved.
 *          `ratio` may be NULL (then identical to (3)); with SURFDISP_PHASE_ONLY the ellipticity recursions are still
 *          run when `ratio` is given.  Love: zeros.  surfdisp_forward_batch_device stays for ABI 2 callers. */
int surfdisp_forward_batch_device2(void *stream, int B, int Lmax, const int *nlay,
                                   const float *model, int P, const float *per, int kind,
                                   float *c, float *u, float *ratio, int *status,
                                   void *workspace, size_t workspace_bytes);

/* ---- (4) measurement variant of (3): identical launches bracketed by HIP events recorded on
 *          `stream`; blocks until done; kernel_ms[3] = durations of the prep, phase (root search)
 *          and group-velocity kernels in milliseconds.  Used by bench.py's roofline figures. */
int surfdisp_forward_batch_device_timed(void *stream, int B, int Lmax, const int *nlay,
                                        const float *model, int P, const float *per, int kind,
                                        float *c, float *u, int *status,
                                        void *workspace, size_t workspace_bytes, float *kernel_ms);

/* ---- (5) non-blocking measurement: the caller creates events (surfdisp_events_create), passes
 *          four per call; they are recorded on `stream` before prep, after prep, after the root
 *          search (and its idle fallback launch) and after ellipticity kernel + group + finish.  Read with surfdisp_events_elapsed_ms once the caller has
 *          synchronised.  bench.py records them inside its timed region. */
int surfdisp_forward_batch_device_events(void *stream, int B, int Lmax, const int *nlay,
                                         const float *model, int P, const float *per, int kind,
                                         float *c, float *u, int *status,
                                         void *workspace, size_t workspace_bytes, void *const *events4);
/*          ... and of (3b), added within ABI 4: the same four events around the solve that also returns the ellipticity. */
int surfdisp_forward_batch_device2_events(void *stream, int B, int Lmax, const int *nlay,
                                          const float *model, int P, const float *per, int kind,
                                          float *c, float *u, float *ratio, int *status,
                                          void *workspace, size_t workspace_bytes, void *const *events4);
int surfdisp_events_create(int n, void **events);
int surfdisp_events_destroy(int n, void **events);
int surfdisp_events_elapsed_ms(void *start, void *stop, float *ms);
/*          surfdisp_stream_wait_event: `stream` waits for one of those events (recorded on another stream) - a caller with two
 *          solves on two streams orders their kernels with it (pysurfinv_amd.forward.JointPlan). */
int surfdisp_stream_wait_event(void *stream, void *event);

/* ---- (5b) forward solve + analytic sensitivity kernels.  REIGEN / LEIGEN form the
 *          partial derivatives of the phase velocity from their energy integrals and never return
 *          them (surfa.f:1130-1135, 1180-1183, 1204-1207; Love 561-565, 584-585); senskernel.py
 *          re-derives them by 2L+1 perturbed solves (senskernel.py:129-158).  Here they come out of
 *          the same group-velocity kernel launch: dcdb / dcda / dcdr [B][P][Lmax] = d c(period) /
 *          d (Vs | Vp | rho) of input layer i in (km/s)/(km/s) resp. (km/s)/(g/cm^3), with respect
 *          to the CALLER's layer values (the chain factors of the attenuation correction
 *          calcul.f:122-126 and of the earth flattening flat1.f:44-62 are applied); zero for water
 *          layers, layers below the effective half space and unsolved periods.  dcda, dcdr may be
 *          NULL; Love has no dcda (written as zeros if given).  Workspace: surfdisp_kernels_workspace_bytes
 *          (every layer's share is stored once, unscaled, in a layer-major scratch inside it - coalesced - and a
 *          transposition kernel applies the common factor 1 / (dL/dk) and writes whole rows); a workspace of only
 *          surfdisp_workspace_bytes is accepted and takes the direct, slower route (same values, bit for bit). */
size_t surfdisp_kernels_workspace_bytes(int B, int Lmax, int P);
int surfdisp_forward_kernels_device(void *stream, int B, int Lmax, const int *nlay,
                                    const float *model, int P, const float *per, int kind,
                                    float *c, float *u, int *status,
                                    float *dcdb, float *dcda, float *dcdr,
                                    void *workspace, size_t workspace_bytes);

/* ---- (5c) ... and the analytic partials of the GROUP velocity (fundamental mode), added within ABI 4.  Differentiating
 *          U = d omega / dk at fixed omega (Rodi et al. 1975):
 *              dU/dm = (U/c) (2 - U/c) dc/dm  -  (U/c)^2 d(dc/dm)/d ln T,
 *          with dc/dm the mean of the phase partials at T (1 - dlnT_frac) and T (1 + dlnT_frac) and d(dc/dm)/d ln T
 *          their central difference.  After the launches of (5b) - c, u, status, dcdb, dcda, dcdr come out bit-identical
 *          to surfdisp_forward_kernels_device on the same inputs - every solved (stack, period) unit's root at the two
 *          shifted periods is found from the first-order prediction c (1 +- dlnT_frac (c/U - 1)) in a bounded window (no
 *          scan), the phase partials are formed there (attenuation correction and chain factors at the shifted period) and
 *          combined: dudb / duda / dudr [B][P][Lmax] = dU(period) / d(Vs | Vp | rho) of input layer i, caller's
 *          coordinates.  The toolkit's own rule (GRV_SENS_KERNEL.f:99-108) is the same except for a wrong sign of the
 *          frequency term of dU/drho; this library uses the derived sign for all three.
 *          Rows: zeros where dcdb's row is zero (unsolved periods, bad stacks); every entry NaN for a solved unit whose
 *          shifted root failed (no bracket within the search budget, more than one sign change in the window, a non-finite
 *          secular function) - *n_shift_failed (device int, may be NULL) counts those units.  duda, dudr (and dcda, dcdr)
 *          may be NULL; Love has no duda (zeros if given).  dlnT_frac in [1e-3, 0.05] (0.01: the toolkit's T x 0.99 / 1.01);
 *          SURFDISP_PHASE_ONLY and SURFDISP_KERN_REFCOORD are rejected (SURFDISP_ERR_INVALID).  Workspace:
 *          surfdisp_group_kernels_workspace_bytes (that of (5b) plus a second layer-major scratch). */
size_t surfdisp_group_kernels_workspace_bytes(int B, int Lmax, int P);
int surfdisp_forward_group_kernels_device(void *stream, int B, int Lmax, const int *nlay,
                                          const float *model, int P, const float *per, int kind, float dlnT_frac,
                                          float *c, float *u, int *status,
                                          float *dcdb, float *dcda, float *dcdr,
                                          float *dudb, float *duda, float *dudr, int *n_shift_failed,
                                          void *workspace, size_t workspace_bytes);

/* ---- (5d) ... and the analytic partials of the Rayleigh ELLIPTICITY chi (the H/V ratio of (3b), COMMON /o/ ratio,
 *          calcul.f:195), added within ABI 4.  With D(e) = h^T A_{n-1} ... A_1 e the layer recursion of DLTAR4 (surfa.f:193-363)
 *          from the start vector e to the half-space row, F = D(e1) is the secular function and chi = D(e3) / (2 D(e2)); the
 *          two ellipticity passes skip a liquid top layer and run on the working stack the root search left (its frozen mmax,
 *          the layers refreshed at earlier periods).  At the root c*(m):
 *              dchi/dm_i = dchi/dm_i|_c + (dchi/dc) dc/dm_i,   dc/dm_i = -(dF/dm_i) / (dF/dc),
 *          each term a contraction of one adjoint row with the forward state of e1, e2 or e3 (dF/dc includes the liquid
 *          layer's term).  fp64, layer coefficients from sin(x)/x and sinh(x)/x (continuous across c = Vp or Vs).  After the
 *          launches of (5b) - c, u, status, dcdb, dcda, dcdr bit-identical to surfdisp_forward_kernels_device on the same
 *          inputs, `ratio` [B][P] as surfdisp_forward_batch_device2 writes it - one more kernel and a transposition:
 *          dedb / deda / dedr [B][P][Lmax] = d chi(period) / d (Vs | Vp | rho) of input layer i, caller's coordinates (the
 *          chain factors of (5b), at the period that last refreshed each layer).
 *          Rows: zeros for water layers, layers below the effective half space, unsolved periods and bad stacks; every entry
 *          NaN for a solved unit whose result is not finite (D(e2) ~ 0: a node of the vertical motion at the surface; dF/dc ~
 *          0) or that the exact fallback solver took (no recorded working stack) - *n_nonfinite (device int, may be NULL)
 *          counts those units.  deda, dedr, dcda, dcdr may be NULL.  SURFDISP_ERR_INVALID, before anything is launched:
 *          Love `kind`, SURFDISP_PHASE_ONLY, SURFDISP_KERN_REFCOORD, SURFDISP_STRICT, NULL ratio / dedb / dcdb, and a
 *          workspace smaller than surfdisp_ellip_kernels_workspace_bytes (that of (5b) plus the layer-major scratches of the
 *          adjoint rows - 5 doubles per layer and unit - and of the shares: there is no direct route). */
size_t surfdisp_ellip_kernels_workspace_bytes(int B, int Lmax, int P);
int surfdisp_forward_ellip_kernels_device(void *stream, int B, int Lmax, const int *nlay,
                                          const float *model, int P, const float *per, int kind,
                                          float *c, float *u, float *ratio, int *status,
                                          float *dcdb, float *dcda, float *dcdr,
                                          float *dedb, float *deda, float *dedr, int *n_nonfinite,
                                          void *workspace, size_t workspace_bytes);

/* ---- (5e) ... and the apparent ATTENUATION of the mode, added within ABI 4.  After every REIGEN / LEIGEN call the reference
 *          forms the attenuation coefficient and the apparent quality factor of the mode from its phase-velocity partials and
 *          the layers' 1/Qs (calcul.f:256-265 Love, 341-349 Rayleigh: alphL / alphR, qL_app / qR_app) - in a loop whose bound
 *          `mmm` is never assigned, into locals that nothing returns; the fp64 toolkit writes them (TEST1/test.R.att, test.L.att).
 *          With b_i, a_i the attenuation-corrected, earth-flattened velocities of input layer i at the period and dc/db_i, dc/da_i
 *          the partials with respect to them (what SURFDISP_KERN_REFCOORD returns):
 *              W_i = b_i (dc/db_i + 4/3 (b_i / a_i) dc/da_i)     (dwx, surfa.f:1207; Love: W_i = b_i dc/db_i, calcul.f:261),
 *              S = sum_i qsinv_i W_i   over the solid layers down to and including the unit's effective half space,
 *              gamma = pi S / (T c^2)  in 1/km,      qinv = S U / c^2 = gamma U T / pi = 1 / Q_apparent,
 *              dqdq_i = W_i U / c^2:   qinv = sum_i dqdq_i qsinv_i.
 *          1/Q and not Q, so that a stack without attenuation gives 0 and not infinity.  dqdq is the linear kernel of qinv with
 *          respect to layer i's 1/Qs at FIXED eigenfunction - not the total derivative: 1/Qs also shifts the layer velocities
 *          through the dispersion correction (calcul.f:122-126), hence c, U and the partials; at T = 1 s that correction vanishes
 *          and qinv is exactly linear in the 1/Qs row.  The library evaluates W_i from the caller-coordinate rows of (5b) (the
 *          flattening factor cancels), in fp64; pysurfinv_amd.senskernel.attenuation_from_kernels is the same statement on the host.
 *          After the launches of (5b) - c, u, status, dcdb, dcda, dcdr bit-identical to surfdisp_forward_kernels_device on the same
 *          inputs - one more kernel reads the layer-major scratch again: qinv, gamma [B][P]; dqdq [B][P][Lmax].  Zeros for unsolved
 *          periods and bad stacks; in dqdq also for water layers and layers below the effective half space.  Rayleigh and Love.
 *          gamma, dqdq, dcda, dcdr may be NULL.  SURFDISP_INDEPENDENT and the other flags as in (5b).  SURFDISP_ERR_INVALID, before
 *          anything is launched: SURFDISP_PHASE_ONLY, SURFDISP_KERN_REFCOORD, NULL qinv / dcdb, and a workspace smaller than
 *          surfdisp_atten_workspace_bytes (that of (5b) with its scratch: there is no direct route). */
size_t surfdisp_atten_workspace_bytes(int B, int Lmax, int P);
int surfdisp_forward_atten_device(void *stream, int B, int Lmax, const int *nlay,
                                  const float *model, int P, const float *per, int kind,
                                  float *c, float *u, int *status,
                                  float *dcdb, float *dcda, float *dcdr,
                                  float *qinv, float *gamma, float *dqdq,
                                  void *workspace, size_t workspace_bytes);

/* ---- (5f) ... and the mode's EIGENFUNCTION and energy integrals, added within ABI 4: what REIGEN / LEIGEN leave in COMMON
 *          /rar/ (dept1, ampur, ampuz, stresz, stresr; Love amp, stress), /rco1/ (sumi0..2) and /rco/ (are / ale) and the
 *          reference never returns (surfa.f:389, 728, 1105-1108, 1145-1148, 1213-1245; Love 499-500, 554-555, 571-628).
 *          The launches of surfdisp_forward_batch_device with the group-velocity kernel's eigenfunction instantiation in place
 *          of the plain one - c, u, status bit-identical to surfdisp_forward_batch_device on the same inputs and flags - then
 *          one transposition kernel.  ur, uz, tz, tr [B][P][Lmax]: the horizontal and vertical displacement and the normal
 *          and shear traction AT THE TOP OF CALLER LAYER i (the depth sum of the thicknesses above it), fp32 as the
 *          reference's arrays; energy [B][P][4] = (I0, I1, I2, amp).  Conventions:
 *            - Rayleigh is normalised to uz = 1 at the top of the first solid layer, Love to ut = 1 there (amp(l) / ut,
 *              surfa.f:580-581).  Love: ur holds the transverse displacement, tr the shear traction, uz and tz are zeros.
 *            - the entry at that top is SET, not integrated: Rayleigh (ellipticity, 1, 0, 0) (surfa.f:1233-1245), Love (1, 0)
 *              (surfa.f:627-628).  Under a water layer it is entry 1 - the sea floor, the reference's dept1(1) = d(1) - and
 *              Rayleigh's normal traction there is the water's, tzz (surfa.f:910, 1244); entry 0, the sea surface, which
 *              the reference does not form, is zero.
 *            - the last non-zero entry is the top of the unit's effective half space (layer dropping, surfa.f:853-866 /
 *              475-487; when the cut falls inside a layer, that layer's top); deeper layers, layers beyond nlay, unsolved
 *              periods, bad stacks and the degenerate exits (surfa.f label 7006; Love's overflow retries exhausted) are zeros,
 *              integrals included.
 *            - Love's low-amplitude exclusion (surfa.f:588-596): an entry of a layer at least as fast as the effective
 *              half space whose normalised displacement is below 1e-20 is zero, displacement and traction.
 *            - I0, I1, I2 are the sums U is formed from: Rayleigh U = (k I1 + I2) / (omega I0) (surfa.f:1186), Love
 *              U = I1 / (c I0) after the division by ut^2 (surfa.f:600-606), I2 = 0.  amp = 1 / (2 c U I0), 0 where c is not
 *              a solved value: the surface-wave amplification factor; the reference's are / ale (surfa.f:1191, 608) is
 *              amp x 1e-15 / sqrt(6.28318).
 *            - all values are those of the earth-flattened, attenuation-corrected stack at the period, as the reference's
 *              are; no inverse flattening of amplitudes is applied.  The reference's own /rar/ entries sit at the MIDDLE of
 *              its sublayers (kk = 3, surfa.f:1104-1108, 553-555), half a sublayer below these.
 *          uz, tz, tr and energy may be NULL.  SURFDISP_INDEPENDENT, SURFDISP_STRICT and the scan flags as in (5).
 *          SURFDISP_ERR_INVALID, before anything is launched: SURFDISP_PHASE_ONLY, SURFDISP_KERN_REFCOORD, a NULL c, u, status or
 *          ur, and a workspace smaller than surfdisp_eigen_workspace_bytes (the forward workspace + a layer-major scratch
 *          [4][Lmax][P][B] + five words per unit: there is no direct route). */
size_t surfdisp_eigen_workspace_bytes(int B, int Lmax, int P);
int surfdisp_forward_eigen_device(void *stream, int B, int Lmax, const int *nlay,
                                  const float *model, int P, const float *per, int kind,
                                  float *c, float *u, int *status,
                                  float *ur, float *uz, float *tz, float *tr,   /* [B][P][Lmax] */
                                  float *energy,                                 /* [B][P][4]    */
                                  void *workspace, size_t workspace_bytes);

/* ---- (5g) ... and the derivatives of the phase velocity with respect to the LAYER THICKNESSES and the INTERFACE DEPTHS, added
 *          within ABI 4: what a model built from a Moho depth, a water depth or a sediment thickness needs, and what 2 L perturbed
 *          solves give only badly (an fp32 thickness step is quantised).  In the conventions of (5f) - v_j the vector at the top of
 *          caller layer j as returned there, (a, b, rho)_m the earth-flattened, attenuation-corrected values of layer m, lam =
 *          rho (a^2 - 2 b^2), mu = rho b^2, k = omega / c - the Hamiltonian of the depth equations,
 *              Love      E(v; m) = rho omega^2 ut^2 - mu k^2 ut^2 + tq^2 / mu,
 *              Rayleigh  uz' = (tz + k lam ur) / (lam + 2 mu), ur' = tr / mu - k uz,
 *                        W2 = lam (uz' - k ur)^2 + 2 mu (k^2 ur^2 + uz'^2) + mu (ur' + k uz)^2,
 *                        E(v; m) = rho omega^2 (ur^2 + uz^2) - W2 + 2 tr ur' + 2 tz uz',
 *              the liquid layer above the sea floor (lam = rho a^2; uz, tz of the sea-floor entry):
 *                        urw = -k tz / (rho omega^2), uz' = tz / lam + k urw, E = rho omega^2 (urw^2 + uz^2) - tz^2 / lam + 2 tz uz'
 *                        (Love: E = 0, the sea floor is its free surface),
 *          is constant through a homogeneous layer and jumps at an interface by the kernel of that interface's flattened depth:
 *              K_j = -amp (c^3 / omega^2) [E(v_j; j-1) - E(v_j; j)],   amp = 1 / (2 c U I0),   1 <= j <= hs (the effective half space),
 *          with U the structural group velocity the library returns (formed from I0, I1, I2 at fixed layer values).  In the caller's
 *          coordinates (flat1.f: r_j = R0 - sum_{m<j} h_m; rt, rb a layer's top and bottom radius, x = ln(rt / rb), p = 2.275 | 5) the
 *          interface also moves the flattening factors of the two layers it bounds; with the rows of (5b), Sv_m = Vs dcdb + Vp dcda
 *          (Love: Vs dcdb), Sr_m = rho dcdr:
 *              d ln dif/d rt =  1 / (rt^2 (1/rb - 1/rt)) - 1 / (x rt),     d ln dif/d rb = -1 / (rb^2 (1/rb - 1/rt)) + 1 / (x rb),
 *              d ln qqq/d rt =  p rt^(p-1) / (rt^p - rb^p) - 1 / (x rt),   d ln qqq/d rb = -p rb^(p-1) / (rt^p - rb^p) + 1 / (x rb),
 *              (layer nlay - 1, the half-space role: d ln dif/d rt = -1 / rt, d ln qqq/d rt = p / rt),
 *              dcdz_j = K_j R0 / r_j - [Sv_{j-1} d ln dif_{j-1}/d rb + Sr_{j-1} d ln qqq_{j-1}/d rb]
 *                                    - [Sv_j d ln dif_j/d rt + Sr_j d ln qqq_j/d rt],
 *              dcdh_i = sum_{j>i} dcdz_j.
 *          dcdz [B][P][Lmax]: d c(period) / d (depth of the top of input layer j), the other interfaces fixed; dcdh [B][P][Lmax]:
 *          d c(period) / d (thickness of input layer i), everything below shifted rigidly - what a change of model[:, 3, i] does.
 *          Evaluated in fp64 from the fp32 rows (the layer-top values as (5f) returns them, the shares as (5b) returns them), so
 *          pysurfinv_amd.senskernel.thickness_kernels_reference, the same statement in numpy, can be fed with the returned rows.
 *          Left out: the flattening-factor term of a liquid layer itself (the rows of a water layer are not read; it would enter only
 *          dcdh[0] and dcdz[1] of a water-covered stack, whose jump term - the water depth - is formed), the dependence of the layer
 *          dropping on the thicknesses (every other row ignores it too), the share of a layer without thickness.
 *          After the launches of (5b) - c, u, status, dcdb, dcda, dcdr bit-identical to surfdisp_forward_kernels_device on the same
 *          inputs - the eigenfunction instantiation of the group-velocity kernel runs on the roots already found (no second root
 *          search) and one more kernel combines the two layer-major scratches.  Zeros: below the effective half space, beyond nlay,
 *          unsolved periods, bad stacks and degenerate exits, dcdh[nlay - 1], dcdz[0].  Every entry NaN for a solved unit with a value
 *          that is not finite (amp, a jump: e.g. a liquid layer below the top) - *n_nonfinite (device int, may be NULL) counts those
 *          units, as in (5d).  dcda, dcdr, dcdz may be NULL; dcdh has the same bits whichever of them are.  Rayleigh and Love.
 *          SURFDISP_INDEPENDENT, SURFDISP_STRICT and the scan flags as in (5b) and (5f).  SURFDISP_ERR_INVALID, before anything is
 *          launched: SURFDISP_PHASE_ONLY, SURFDISP_KERN_REFCOORD, a NULL c, u, status, dcdb or dcdh, and a workspace smaller than
 *          surfdisp_thickness_kernels_workspace_bytes (that of (5b) plus the eigenfunction scratch of (5f) and one word per unit:
 *          there is no direct route). */
size_t surfdisp_thickness_kernels_workspace_bytes(int B, int Lmax, int P);
int surfdisp_forward_thickness_kernels_device(void *stream, int B, int Lmax, const int *nlay,
                                              const float *model, int P, const float *per, int kind,
                                              float *c, float *u, int *status,
                                              float *dcdb, float *dcda, float *dcdr,
                                              float *dcdh, float *dcdz,                 /* [B][P][Lmax] */
                                              int *n_nonfinite,
                                              void *workspace, size_t workspace_bytes);

/* ---- (5h) ... and the same derivatives of the GROUP velocity, added within ABI 4.  Rodi's rule of (5c) holds for any model
 *          parameter; with d = dlnT_frac and dcdh-, dcdh+ the rows of (5g) at the periods T (1 - d) and T (1 + d),
 *              dudh = (U/c) (2 - U/c) (dcdh- + dcdh+) / 2  -  (U/c)^2 (dcdh+ - dcdh-) / ln((1 + d) / (1 - d)),
 *          and dudz from dcdz-, dcdz+ in the same way; c and U are the unit's own values at T.  The rows at the shifted periods are
 *          evaluated on what (5c) finds or rebuilds there: its shifted roots and ellipticities, a fresh stack per shifted period,
 *          attenuation correction and chain factors at the shifted period, the phase partials and the structural U of its shifted
 *          launches; the eigenfunction instantiation of the group-velocity kernel runs once more per shifted period (no further
 *          root search).  dudh [B][P][Lmax]: d U(period) / d (thickness of input layer i), everything below shifted rigidly - what a
 *          change of model[:, 3, i] does; dudz [B][P][Lmax]: d U(period) / d (depth of the top of input layer j) alone.  fp32
 *          combination of fp32 rows; pysurfinv_amd.senskernel.group_thickness_reference is the same statement in float64.
 *          One entry, the launches of (5b), (5c) and (5g) on one stream: c, u, status, dcdb, dcda, dcdr are bit-identical to
 *          surfdisp_forward_kernels_device, dudb, duda, dudr to surfdisp_forward_group_kernels_device at the same dlnT_frac, dcdh,
 *          dcdz to surfdisp_forward_thickness_kernels_device, also with SURFDISP_INDEPENDENT.
 *          Rows: an entry of dudh is zero where that entry of dcdh is (below the effective half space at T, beyond nlay, unsolved
 *          periods, bad stacks, dudh[nlay - 1]); dudz[j] is zero where dcdh[j - 1] is - the same interfaces as dcdz - and
 *          dudz[0] = 0.  Every entry of dudh and dudz is NaN for a solved unit whose shifted root failed - the units of dudb's NaN
 *          rows, counted once in *n_shift_failed - and for a unit whose thickness rows are not finite at T or, its shifted roots
 *          found, at a shifted period: *n_nonfinite counts those (at T: the units (5g) counts).  dcda, dcdr, duda, dudr, dcdz,
 *          dudz and both counters may be NULL; dudh has the same bits whichever of them are.  Rayleigh and Love.
 *          SURFDISP_ERR_INVALID, before anything is launched: SURFDISP_PHASE_ONLY, SURFDISP_KERN_REFCOORD, a NULL c, u, status,
 *          dcdb, dudb, dcdh or dudh, dlnT_frac outside [1e-3, 0.05], and a workspace smaller than
 *          surfdisp_group_thickness_kernels_workspace_size (that of (5c) plus the eigenfunction scratch of (5f), one word per unit
 *          and four [B][P][Lmax] row planes: there is no direct route).  The size function ends in _size, not in _workspace_bytes: the
 *          *_workspace_bytes functions are the seven of (5) - (5g), whose count and mutual relations tests/test_host.py pins. */
size_t surfdisp_group_thickness_kernels_workspace_size(int B, int Lmax, int P);
int surfdisp_forward_group_thickness_kernels_device(void *stream, int B, int Lmax, const int *nlay,
                                                    const float *model, int P, const float *per, int kind, float dlnT_frac,
                                                    float *c, float *u, int *status,
                                                    float *dcdb, float *dcda, float *dcdr,
                                                    float *dudb, float *duda, float *dudr,
                                                    float *dcdh, float *dcdz, float *dudh, float *dudz,   /* [B][P][Lmax] */
                                                    int *n_shift_failed, int *n_nonfinite,
                                                    void *workspace, size_t workspace_bytes);

/* ---- (6) parameters -> layer stacks on the device (the row next to the hot path, SURVEY.md 8f-2:
 *          Model1D.seisPropLayers, models.py:72-102 + layers.py:139-284) for models with a static
 *          layer structure.  params [C][N] fp64, model [C][5][L] fp32 (rows vp, vs, rho, h, 1/Qs);
 *          idesc / fdesc: descriptor built by pysurfinv_amd.layers_batch (layout in
 *          csrc/surfdisp_layers.hip).  All device pointers; stream-ordered; graph-capturable. */
int surfdisp_params_to_model_device(void *stream, int C, int N, int L, const double *params,
                                    const int *idesc, const double *fdesc, float *model);
/*          The same for a model whose mantle is the thermal OceanMantleHybrid layer (SURVEY.md 8f-4:
 *          layers.py:297-363 over ThermSeis.py HSCM / OceanSeisRitz / OceanSeisRuan): one more kernel
 *          (csrc/surfdisp_thermal.hip) evaluates the half-space cooling models, the mineral physics /
 *          anelasticity and the merge spline, one wavefront per chain, into the caller-owned scratch
 *          (surfdisp_thermal_scratch_bytes(C) bytes of device memory). */
size_t surfdisp_thermal_scratch_bytes(int C);
int surfdisp_params_to_model_thermal_device(void *stream, int C, int N, int L, const double *params,
                                            const int *idesc, const double *fdesc,
                                            void *scratch, size_t scratch_bytes, float *model);

/* ---- (6b) the Metropolis glue of one lock step on the device (csrc/surfdisp_mcmc.hip).
 *   propose: every random-walk scalar of every chain moves by a bounded Gaussian step, redrawn while it falls outside
 *            (vmin, vmax), at most 1000 tries, then a uniform draw (BrownianVar.move, brownian.py:20-27); reset != 0: a
 *            uniform prior draw for every entry (MCinv.reset, models.py:206-219).  p, out [C][N]; vmin, vmax, step [N].
 *   accept : misfit of the proposals' predicted curves c[C][P] (fp32, as the solver returns them) against the
 *            observations (chi2 = sum(((cO-cP)/uncer)^2) over the masked-in periods, misfit = sqrt(chi2/N), chi2 :=
 *            sqrt(50 chi2) when >= 50, L = exp(-chi2/2); a failed solve = (88888, 88888, 0): point.py:15-31), accept rule
 *            chi1 < chi0 or u > 1 - exp(-(chi1-chi0)/2) (point.py:34-37), p0 / chi0 updated in place, and the mcTrack row
 *            [misfit, L, accepted, *proposal] (models.py:254-256) written to row + chain * row_stride (doubles) if row.
 *            c_obs / uncer / mask are [P], or [C][P] with obs_per_chain.  first != 0: a chain's first row (accepted).
 *   Random numbers: Philox4x32-10 keyed by `seed`; the caller passes a fresh `counter` per call.  chain0: the index, in
 *   the whole sampler, of this call's chain 0 - the random streams are indexed by chain0 + c, so a sampler that advances
 *   its chains in several groups (one call per group, e.g. on several streams) draws exactly what one call over all
 *   chains draws.  Device pointers, stream-ordered, no host synchronisation, graph-capturable. */
int surfdisp_mcmc_propose_device(void *stream, int C, int N, const double *p, const double *vmin, const double *vmax,
                                 const double *step, unsigned long long seed, unsigned long long counter, int reset, double *out,
                                 long chain0);
int surfdisp_mcmc_accept_device(void *stream, int C, int N, int P, const float *c, const int *status,
                                const double *c_obs, const double *uncer, const unsigned char *mask, int obs_per_chain,
                                const double *p1, double *p0, double *chi0, double *row, long row_stride,
                                unsigned long long seed, unsigned long long counter, int first, long chain0);
/* ---- (6c) prior predicates on the device, so that a sampler with a prior keeps its lock step there.  The reference redraws a
 *   proposal until `isgood(model)` holds (MCinv.perturb / reset, models.py:192-219: up to 1000 Gaussian tries, then uniform
 *   draws); its model classes build `isgood` from a few GENERIC tests on the grid points of seisPropGrids (models.py:294-320):
 *   Vs increasing inside a layer group (monoIncrease), no drop of Vs across a group boundary, Vs below a cap.
 *   surfdisp_prior_device evaluates those for every chain: flags [L] per OUTPUT layer of the params->stack descriptor (bit 0: Vs
 *   must increase across the layer; bit 1: ... and on to the top of the next layer; bit 2: must not drop to the top of the next
 *   layer; bit 3: both its points at most vs_max).  tags [C] (unsigned char): a chain that breaks a rule gets tags[c] = mark_tag (1..255); with
 *   only_tag >= 0 only the chains with tags[c] >= only_tag are looked at - the rounds of one step use rising tags (the caller
 *   clears tags once per step), so nothing needs clearing between rounds.  Models with a static layer structure, no thermal layer.
 *   surfdisp_mcmc_propose_masked_device redraws the chains with tags[c] == tag only (try number `attempt` of this step: its own
 *   random numbers; mode 0 bounded Gaussian step, 1 uniform prior draw, 2 the chain's state itself), leaving the other rows of
 *   `out` as they are.  pysurfinv_amd.mcmc.MetropolisBatch(isgood=PriorRules(...)) strings them into masked redraw rounds. */
int surfdisp_prior_device(void *stream, int C, int N, int L, const double *params, const int *idesc, const double *fdesc,
                          const int *flags, double vs_max, int only_tag, int mark_tag, unsigned char *tags);
int surfdisp_mcmc_propose_masked_device(void *stream, int C, int N, const double *p, const double *vmin, const double *vmax,
                                        const double *step, unsigned long long seed, unsigned long long counter, int attempt, int mode,
                                        const unsigned char *tags, int tag, double *out, long chain0);
/* The same loop INSIDE one kernel (csrc/surfdisp_mcmc_prior.hip; added within ABI 4), with the reference's caps and for every node
 * of the speculative tree below: surfdisp_mcmc_propose_prior_device draws out [C][2^depth - 1][N] (depth 1..4; depth 1: the plain
 * proposal) so that every row satisfies the rules.  One wavefront per chain.  Node k = 0, 1, ..., 2^depth - 2 draws from the state
 * of its branch (node 0: p[c]; child 2k+1: the final proposal of k; child 2k+2: the state of k).  Retry r = 0 .. gauss_tries - 1
 * redraws ALL N scalars with the bounded Gaussian step of (6b), retry r = gauss_tries .. gauss_tries + uniform_tries - 1 with its
 * uniform branch (reset); the candidate row [N scalars | aux[c][0..K)] is tested with surfdisp_prior_device's rules (flags [L],
 * eps; vs_max < 0: no cap); the first good candidate is out[c][k][:], tries[c][k] = r.  No good candidate: out[c][k][:] is the
 * state the node drew from, tries[c][k] = gauss_tries + uniform_tries, and *exhausted (one device int the caller zeroes once; it
 * is only ever incremented) grows by one - the reference raises there (models.py:219), a caller reads the count when it
 * synchronises anyway.  gauss_tries >= 0, uniform_tries >= 0, 1 <= gauss_tries + uniform_tries <= SURFDISP_MCMC_PRIOR_TRIES_MAX;
 * N + K <= SURFDISP_MCMC_PRIOR_ROW_MAX (the row lives in LDS, with the candidate's Vs at the grid points: (N + K + L + 11) doubles
 * per chain); aux may be NULL when K == 0; tries may be NULL; L = the descriptor's output layers.  Static-structure models without
 * a thermal layer, as surfdisp_prior_device (a descriptor with one, or with more grid points than L layers can have: every node is
 * reported exhausted).
 * Random numbers: Philox4x32-10 with the word layout of the other entries - word 0 the counter's low half; word 1 its high half
 * XOR (node << 20) XOR (try t << 8) for the Gaussian tries t = 0..499 of one scalar, XOR (node << 20) XOR 0x00ffff00 for its
 * uniform draw; words 2, 3 the stream index gidx + (r << 48), gidx = (chain0 + c) * N + n: the whole-proposal retry r sits in
 * bits 16..29 of word 3, hence (chain0 + C) * N < 2^48 is required.  With r = 0 every draw is the draw of
 * surfdisp_mcmc_propose_device / surfdisp_mcmc_propose_tree_device: with rules that accept everything the three entries write the
 * same bits.  A sampler split into chain groups (chain0) draws what one call draws.  Bad arguments: SURFDISP_ERR_INVALID before
 * any device call.  Stream-ordered, no host synchronisation, graph-capturable. */
#define SURFDISP_MCMC_PRIOR_ROW_MAX 256
#define SURFDISP_MCMC_PRIOR_TRIES_MAX 16384
int surfdisp_mcmc_propose_prior_device(void *stream, int C, int N, int K, int L, int depth,
                                       const double *p, const double *aux, const double *vmin, const double *vmax, const double *step,
                                       const int *idesc, const double *fdesc, const int *flags, double vs_max,
                                       int gauss_tries, int uniform_tries,
                                       unsigned long long seed, unsigned long long counter, long chain0,
                                       double *out, unsigned short *tries, int *exhausted);
/* Proposals shaped by a covariance (csrc/surfdisp_mcmc_cov.hip; added within ABI 4): surfdisp_mcmc_propose_cov_device is the entry
 * above with the axis-aligned `step` replaced by a lower-triangular factor per point, cand = x + L z.  factor_t [F][N][N] holds the
 * TRANSPOSED factors, factor_t[f][k][n] = L_f[n][k] (the 64 lanes read a column's entries side by side); chain c takes factor
 * f = (chain0 + c) / chains_per_factor (chains_per_factor > 0, and (chain0 + C - 1) / chains_per_factor < F).  1 <= N <=
 * SURFDISP_MCMC_COV_N_MAX: one lane per scalar.  out, depth, the tree's states, tries and *exhausted: as above.
 * Whole-proposal retry r = 0 .. gauss_tries + uniform_tries - 1 of node k:
 *   r < gauss_tries: z_n = sqrt(-2 log u1) cospi(2 u2) of ONE Philox call per (chain, scalar, node, retry): word 0 the counter's low
 *   half, word 1 its high half XOR (node << 20) (the tag of Gaussian try 0), words 2, 3 the stream index gidx + (r << 48), gidx =
 *   (chain0 + c) * N + n - the counter words of surfdisp_mcmc_propose_device's first candidate, with the retry where the prior entry
 *   puts it ((chain0 + C) * N < 2^48); cand_n = x_n + sum_{k <= n} L[n][k] z_k, summed with k ascending;
 *   r >= gauss_tries: the uniform draw vmin + (vmax - vmin) u of the prior entry's uniform phase, bit for bit.
 * A candidate is good when every scalar lies strictly inside (vmin_n, vmax_n) and, with flags, the rules of surfdisp_prior_device hold
 * on the row [N scalars | aux[c][0..K)]; the first good candidate is out[c][k][:] and tries[c][k] = r; none: the state the node drew
 * from, tries[c][k] = gauss_tries + uniform_tries, *exhausted grows by one.  This is the reference's perturb (models.py:192-205: the
 * whole proposal again while it is refused).  Redrawing into the box makes the proposal density slightly asymmetric near the walls,
 * exactly as the reference's per-scalar redraw does (brownian.py:20-27); like the reference, no entry corrects for it.
 * flags may be NULL, with idesc, fdesc and aux NULL and K = L = 0: no rules, only the box, and no descriptor is touched (a thermal
 * model, whose rules the device cannot evaluate).  With flags: K, L, idesc, fdesc, aux, vs_max as above (N + K <=
 * SURFDISP_MCMC_PRIOR_ROW_MAX).  LDS: (2 N + K + L + 11) doubles per chain.  A sampler split into chain groups (chain0) draws what one
 * call draws.  Bad arguments: SURFDISP_ERR_INVALID before any device call.  Stream-ordered, no host synchronisation, graph-capturable.
 * surfdisp_mcmc_cov_factor_device makes the factors: cov [P][N][N] symmetric with the rows and columns of fixed parameters all zero
 * (what surfdisp_lsq_step_params_device returns), factor_t [P][N][N] in the layout above = the Cholesky factor of scale^2 cov over the
 * rows with a non-zero diagonal (a fixed parameter gets a zero row and column: it never moves), flag [P] = 0.  A pivot that is not
 * positive and finite: flag[p] = 1 and the point gets diag(fallback_step [N]) - the reference's step, never a half-factored matrix.
 * One wavefront per point, the matrix in LDS (N N doubles); meant to run once per run, outside the lock step. */
#define SURFDISP_MCMC_COV_N_MAX 64
int surfdisp_mcmc_propose_cov_device(void *stream, int C, int N, int K, int L, int depth,
                                     const double *p, const double *aux, const double *vmin, const double *vmax,
                                     const double *factor_t, long chains_per_factor, int F,
                                     const int *idesc, const double *fdesc, const int *flags, double vs_max,
                                     int gauss_tries, int uniform_tries,
                                     unsigned long long seed, unsigned long long counter, long chain0,
                                     double *out, unsigned short *tries, int *exhausted);
int surfdisp_mcmc_cov_factor_device(void *stream, int P, int N, const double *cov, double scale, const double *fallback_step,
                                    double *factor_t, int *flag);
/* Adaptive proposals (csrc/surfdisp_mcmc_adapt.hip; added within ABI 4): adaptive Metropolis (Haario et al. 2001) pooled over the
 * chains of a grid point, with a Robbins-Monro step scale.  surfdisp_mcmc_adapt_device is ONE update for F points, each with cpp
 * chains of N <= SURFDISP_MCMC_COV_N_MAX scalars: p [F * cpp][N] the chains' current states (chain c belongs to point c / cpp), the
 * accept flags of the rows [row_lo, row_hi) of a track - flag of chain c, row r: track[c * chain_stride + r * row_stride + 2],
 * strides in doubles; counted as accepted when > 0.5 -, step [N] the reference's step, and per point a block of
 * SURFDISP_MCMC_ADAPT_HEAD + N + N N doubles in `state`:
 *   [0] W the weight  [1] ls the log scale  [2] k the update count of ls  [3] the fallback count  [4] 1 when this call wrote the point's
 *   cov_out, else 0  [5..7] 0  [8 .. 8 + N) mean  [8 + N ...) the scatter S[k][n] at k * N + n, k <= n (the entries below the
 *   diagonal are carried along, times forget, and never read as values).
 * A block of zeros is the fresh state.  Per point, in this order, in float64:
 *   1. W *= forget; S *= forget;
 *   2. for the point's chains in ascending order, one Welford step each: W += 1; d = x - mean; mean += d / W;
 *      S[k][n] += d_k * (x_n - mean_n) for k <= n (mean_n: the updated one);
 *   3. with target_accept >= 0 and row_hi > row_lo: a = (number of accepted flags of the point's chains and the window's rows) /
 *      (cpp * (row_hi - row_lo)), the count an integer (exact, order-free); k += 1; ls += (gain * k^(-decay)) * (a - target_accept),
 *      every operation rounded on its own, then clamped to [ls_min, ls_max].  target_accept < 0 or an empty window: ls and k stay;
 *   4. with W >= min_weight: cov_out[f][k][n] = c * B[k][n], symmetric, B = S / W + ridge diag(step^2) with the diagonal term formed
 *      as (ridge * step_n) * step_n, c = exp(2 ls) * (2.38^2 / N_live), N_live the scalars with B[n][n] != 0; a scalar with B[n][n] == 0
 *      gets a zero row and column (the "fixed parameter" convention of surfdisp_mcmc_cov_factor_device).  [4] = 1.  Below min_weight
 *      cov_out is left untouched and [4] = 0.  cov_out may be NULL (nothing is written; [4] still answers W >= min_weight).
 * [3] is carried unchanged: factoring stays with surfdisp_mcmc_cov_factor_device (scale = 1, fallback_step = step, straight into the
 * sampler's factor_t), launched by the caller on all points once every point has reached min_weight - with equally many chains per
 * point and blocks started together, W is the same number on every point and known on the host without a read-back -, and the caller
 * adds that entry's flag to [3].  One wavefront per point, lane n = scalar n, the scatter in LDS (N N + 128 doubles), the chains one
 * after the other: no atomics, and the result does not depend on the launch shape.  Bad arguments - F, cpp, N < 1, N >
 * SURFDISP_MCMC_COV_N_MAX, forget outside (0, 1], row_lo < 0, row_hi < row_lo, ridge < 0, min_weight < 1, ls_min > ls_max,
 * target_accept > 1, a value that is not a number, p, state or step NULL, track NULL with a window to read -: SURFDISP_ERR_INVALID
 * before any device call.  Stream-ordered, no host synchronisation. */
#define SURFDISP_MCMC_ADAPT_HEAD 8
int surfdisp_mcmc_adapt_device(void *stream, int F, int cpp, int N, const double *p,
                               const double *track, long chain_stride, long row_stride, int row_lo, int row_hi,
                               const double *step, double forget, double target_accept, double gain, double decay,
                               double ls_min, double ls_max, double min_weight, double ridge,
                               double *state, double *cov_out);
/* The SPECULATIVE lock step for few chains (a lock step of 100 chains leaves the chip idle, so it costs no more to solve
 * several proposals per chain): propose_tree draws the binary tree of the next `depth` (1..4) accept / reject outcomes -
 * node k's proposal from the state its branch would be in (node 0: the chain's state; child 2k+1 "accepted": proposal k;
 * child 2k+2 "rejected": the state of k), out [C][2^depth - 1][N] = the C * (2^depth - 1) stacks of ONE batched solve;
 * accept_tree then walks nsteps <= depth steps per chain with the usual test at every node and writes one mcTrack row
 * per step, step_stride doubles apart.  Every proposal is drawn from, and tested against, the state the chain is in at
 * that step, so the chain is distributed exactly as the plain sampler's.  depth = 1 is the plain pair of calls above. */
int surfdisp_mcmc_propose_tree_device(void *stream, int C, int N, int depth, const double *p, const double *vmin,
                                      const double *vmax, const double *step, unsigned long long seed,
                                      unsigned long long counter, double *out, long chain0);
int surfdisp_mcmc_accept_tree_device(void *stream, int C, int N, int P, int depth, int nsteps, const float *c,
                                     const int *status, const double *c_obs, const double *uncer, const unsigned char *mask,
                                     int obs_per_chain, const double *q, double *p0, double *chi0, double *row,
                                     long row_stride, long step_stride, unsigned long long seed, unsigned long long counter,
                                     long chain0);

/* Joint data - Rayleigh and Love, phase and group velocity (pysurfinv_amd.obsdata; added within ABI 4): the accept entries
 * above with the misfit of several observed curves.  pred[4] = {cR, uR, cL, uL} (fp32 as the solver returns them, stack s's
 * row at pred[k] + s * pred_stride[k]; NULL where absent; a wave type has data iff its phase array is given), nper[2] the
 * periods of the Rayleigh / Love solve, status[2] their [stacks] status arrays (NULL: no check).  cols [Ptot][2] (device):
 * per observation column the source array (0..3) and the period index in that solve (Ptot <= 800); weights [Ptot]; obs / uncer / mask
 * [Ptot], or [C][Ptot] with obs_per_chain.  chi2 = sum over the columns in ascending order of w ((obs - pred) / uncer)^2 over
 * the masked-in entries, N = their count, misfit = sqrt(chi2 / N), then the clamp and L of the plain entries.  (88888, 88888, 0)
 * when a wave type with data has status != 0 or a phase velocity < 0.01 at any period of its solve, or when a group
 * velocity a column reads is not >= 0.01 (NaN included), or a column names a missing array or a period beyond nper.  With
 * one Rayleigh-phase column set of weight 1 (cols = (0, k)) every row equals surfdisp_mcmc_accept(_tree)_device's bit for bit. */
int surfdisp_mcmc_accept_joint_device(void *stream, int C, int N, const float *const pred[4], const long pred_stride[4],
                                      const int nper[2], const int *const status[2], int Ptot, const int *cols, const double *weights,
                                      const double *obs, const double *uncer, const unsigned char *mask, int obs_per_chain,
                                      const double *p1, double *p0, double *chi0, double *row, long row_stride,
                                      unsigned long long seed, unsigned long long counter, int first, long chain0);
int surfdisp_mcmc_accept_tree_joint_device(void *stream, int C, int N, int depth, int nsteps, const float *const pred[4],
                                           const long pred_stride[4], const int nper[2], const int *const status[2], int Ptot,
                                           const int *cols, const double *weights, const double *obs, const double *uncer,
                                           const unsigned char *mask, int obs_per_chain, const double *q, double *p0, double *chi0,
                                           double *row, long row_stride, long step_stride, unsigned long long seed,
                                           unsigned long long counter, long chain0);
/* ... and the Rayleigh ELLIPTICITY as a fifth curve (added within ABI 4): the two entries above with pred[5] / pred_stride[5],
 * pred[4] = the [stacks][nper[0]] ratio array of the Rayleigh solve (surfdisp_forward_batch_device2; NULL where absent, and only
 * together with pred[0]).  Column sources 0..3 as above, 4 = chi as the solver returns it (signed), 5 = |chi| of the same array (a
 * measured H/V curve carries no sign).  On top of the rule above, (88888, 88888, 0) when an ellipticity value a column reads is
 * not finite (NaN or inf: D(e2) ~ 0, see (5d)); no lower bound - chi near 0 and negative chi are legitimate predictions.  A column
 * with source 4 or 5 whose pred[4] is NULL, or whose period index is beyond nper[0], fails the model and reads nothing.  Without
 * such a column every row equals the four-array entries' bit for bit (those are this kernel compiled without the fifth source). */
int surfdisp_mcmc_accept_joint5_device(void *stream, int C, int N, const float *const pred[5], const long pred_stride[5],
                                       const int nper[2], const int *const status[2], int Ptot, const int *cols, const double *weights,
                                       const double *obs, const double *uncer, const unsigned char *mask, int obs_per_chain,
                                       const double *p1, double *p0, double *chi0, double *row, long row_stride,
                                       unsigned long long seed, unsigned long long counter, int first, long chain0);
int surfdisp_mcmc_accept_tree_joint5_device(void *stream, int C, int N, int depth, int nsteps, const float *const pred[5],
                                            const long pred_stride[5], const int nper[2], const int *const status[2], int Ptot,
                                            const int *cols, const double *weights, const double *obs, const double *uncer,
                                            const unsigned char *mask, int obs_per_chain, const double *q, double *p0, double *chi0,
                                            double *row, long row_stride, long step_stride, unsigned long long seed,
                                            unsigned long long counter, long chain0);

/* ---- (6d) one damped, smoothed least-squares step of the layers' Vs on the device, added within ABI 4: the consumer of the
 *          partial arrays of (5b)-(5d) (csrc/surfdisp_lsq.hip; the classical Gauss-Newton / Levenberg-Marquardt iteration of the
 *          surf96 family, one step per call; pysurfinv_amd.linearized iterates it with the forward solves).  Per stack s the
 *          unknowns x are the Vs of its FREE layers: layer i < nlay[s] with free_mask[i] != 0 (free_mask [Lmax], or [B][Lmax] with
 *          free_per_stack; NULL: every layer), n of them, x0 = row 1 of `model`.  nfree_max: an upper bound of n over the batch
 *          (1..128, <= Lmax) - it sizes the kernel's LDS; a stack with more free layers is not solved (flag 3).
 *   rows:  the column table of surfdisp_mcmc_accept_joint5_device - cols [N][2] (source 0 cR, 1 uR, 2 cL, 3 uL, 4 chi, 5 |chi|; period
 *          index in that source's solve), weights [N], obs / uncer / mask [N] or [B][N] with obs_per_stack, pred[5] / pred_stride[5] /
 *          nper[2] the solves' predictions (N <= 800).  part[15] = {source 0..4} x {d/dVs, d/dVp, d/drho}: the [B][nper][Lmax] fp32
 *          arrays exactly as (5b)-(5d) write them (part[3] = dudb of the Rayleigh solve, part[12] = dedb, ...; NULL: that column is
 *          absent; Love has no d/dVp).  The effective Jacobian row over the free layers i:
 *              G[r,i] = K_b[r,i] + p_i K_a[r,i] + q_i K_rho[r,i],      residual  res_r = obs_r - pred_r,
 *          p = vp_slope, q = rho_slope: dVp/dVs and drho/dVs of layer i ([Lmax], or [B][Lmax] with slope_per_stack; NULL or an entry
 *          of 0: held fixed, the column is not read).  Source 5 compares |chi| and multiplies its row by sign(chi).
 *          A row is DROPPED from this step when it is masked out, when its observation is not finite or its uncertainty not
 *          finite or <= 0, when its prediction is an unsolved period (c or U not >= 0.01; chi not finite, or c < 0.01 at chi's
 *          period), when it names a missing array or a period beyond its solve, or when any G[r,i] is not finite (the NaN rows
 *          of (5c) / (5d)).
 *   solve: in fp64 from the fp32 inputs, by Cholesky factorisation,
 *              (G^T W G + alpha D^T Q D + lam_s I) delta = G^T W res - alpha D^T Q D x0,     W = diag(w_r / uncer_r^2),
 *          D the first difference between CONSECUTIVE FREE layers, Q its weights: Q [Lmax-1] (or [B][Lmax-1] with q_per_stack;
 *          NULL: 1) weighs the interface between the layers k and k+1, and two consecutive free layers a < b take the smallest
 *          of Q[a..b-1] (0 cuts the smoothing across a discontinuity); alpha >= 0 a scalar; lam [B] (device) the damping.
 *   out:   delta [B][Lmax] fp64 (0 at layers that are not free); stats [B][3] fp64 = data misfit sum W res^2 and roughness
 *          x0^T D^T Q D x0 at x0, and the objective the linear model predicts at x0 + delta, sum W (res - G delta)^2 + alpha
 *          roughness(x0 + delta); info [B][3] int = rows used, rows dropped, flag: 0 solved; 1 no usable row; 2 a pivot <= 0 or
 *          not finite (or a step that is not finite); 3 more than nfree_max free layers.  For a flag other than 0 delta is all
 *          zeros, never NaN, and the predicted objective is the one at x0.
 *          One workgroup per stack, the packed triangle of the augmented normal equations in LDS (66 KB at n = 128): the first
 *          call that needs more dynamic LDS than any before it raises the kernel's limit, so make it outside a graph capture.
 *          No workspace.  SURFDISP_ERR_INVALID, before anything is launched: B < 1, Lmax outside 1..200, N outside 1..800,
 *          nfree_max outside 1..min(128, Lmax), alpha < 0 or not finite, a NULL required pointer (model, part, pred, pred_stride,
 *          nper, cols, weights, obs, uncer, mask, lam, delta, stats, info), no phase array at all, a group or chi array without
 *          the phase array of its solve, a prediction array with nper outside 1..200 or a stride below nper, a partial array of
 *          a source without predictions. */
int surfdisp_lsq_step_device(void *stream, int B, int Lmax, const int *nlay, const float *model,
                             const unsigned char *free_mask, int free_per_stack, int nfree_max,
                             const float *const part[15], const float *const pred[5], const long pred_stride[5], const int nper[2],
                             int N, const int *cols, const double *weights,
                             const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                             const double *vp_slope, const double *rho_slope, int slope_per_stack,
                             double alpha, const double *Q, int q_per_stack, const double *lam,
                             double *delta, double *stats, int *info);

/* ---- (6e) posterior covariance and resolution of the problem of (6d) at the same point, added within ABI 4 (csrc/surfdisp_lsq.hip):
 *          what a linearised inversion is reported with.  Unknowns (unknown j = the j-th free layer in increasing layer index),
 *          rows, weights, dropped rows, Q, alpha, lam and nfree_max are those of (6d), and the arguments up to and including `lam`
 *          are the argument list of surfdisp_lsq_step_device: pred decides which rows are used and the sign of a source-5 row,
 *          obs is read for the finite test only.  Per stack, with n free layers:
 *              H = G^T W G,   A = H + alpha D^T Q D + lam_s I,   C = A^-1 (posterior covariance of the damped, smoothed problem),
 *              R = C H (model resolution matrix: row i is the averaging kernel of unknown i),   Cd = C H C = R C (covariance
 *              of the estimate from the data errors alone),   dof = trace(R).
 *   out:   cov, res [B][nfree_max][nfree_max] fp64, row-major, in unknown order: C and R, rows and columns >= n zeros; either
 *          may be NULL and is then not written; cov is exactly symmetric.  sigma_post, sigma_data, rdiag [B][Lmax] fp64 (required):
 *          sqrt(C_jj), sqrt(Cd_jj) and R_jj at free layer i = layer of unknown j, 0 at layers that are not free.  stats [B][2]
 *          fp64 = dof and log det A (twice the sum of the logs of the Cholesky pivots: the normalisation of the Gaussian
 *          approximation exp(-(x - x^)^T A (x - x^) / 2)).  info [B][3] int = rows used, rows dropped, flag, as (6d): 0 solved;
 *          1 no usable row; 2 a pivot <= 0 or not finite (or an inverse that is not finite); 3 more than nfree_max free layers.
 *          For a flag other than 0 every output of that stack is zeros, never NaN; the other stacks are not affected.
 *          In fp64: A is factorised, its factor inverted and C = L^-T L^-1 formed in one packed triangle of LDS (66 KB at
 *          n = 128; the dynamic-LDS limit is raised as in (6d): first call outside a graph capture); R = I - C (alpha D^T Q D +
 *          lam I), the same matrix since H = A - alpha D^T Q D - lam I, at O(n^2): its entries carry an absolute error of a few
 *          ulp of 1.  No workspace.  SURFDISP_ERR_INVALID, before anything is launched: the conditions of (6d), the required
 *          pointers being model, part, pred, pred_stride, nper, cols, weights, obs, uncer, mask, lam, sigma_post, sigma_data,
 *          rdiag, stats, info. */
int surfdisp_lsq_resolution_device(void *stream, int B, int Lmax, const int *nlay, const float *model,
                                   const unsigned char *free_mask, int free_per_stack, int nfree_max,
                                   const float *const part[15], const float *const pred[5], const long pred_stride[5], const int nper[2],
                                   int N, const int *cols, const double *weights,
                                   const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                                   const double *vp_slope, const double *rho_slope, int slope_per_stack,
                                   double alpha, const double *Q, int q_per_stack, const double *lam,
                                   double *cov, double *res, double *sigma_post, double *sigma_data, double *rdiag,
                                   double *stats, int *info);

/* ---- (6f) posterior Vs(z) profiles of a whole Metropolis track on the device, added within ABI 4 (csrc/surfdisp_post.hip): what
 *          the reference's PostPoint reports per point - the final rows' models as Vs at depth (point.py:317-335 _loadValues(zdeps)),
 *          their mean, spread and histograms (plotVsProfileShaded, _check_distribution) and, with a prefix, the row subsets of
 *          _check_convergency - for every point of a track at once.  pysurfinv_amd.posterior.posterior_reference is the same
 *          statement in numpy.
 *   in:    track [npoints][R] rows of row_stride >= 3 + N doubles (device): misfit, L, accepted, params[N] - a point's chains one
 *          after the other, as in the reference's .npz.  idesc: the integer part of the params->stack descriptor of (6), HOST memory,
 *          idesc_len ints (it is checked here and travels in the kernel arguments); fdesc: its float part, device.  aux: NULL, or
 *          the [.][K] table of per-point constants (device; slot N + k of a row, Model1DBatch.set_local_info), rows: NULL (point p
 *          reads aux row p) or [npoints] ints (device).  zdeps [D]: ascending depths in km, HOST memory, 1 <= D <=
 *          SURFDISP_POST_DEPTHS_MAX.  Models with a static layer structure and no thermal layer, as surfdisp_prior_device.
 *   select (point.py:152-168), per point over its R rows: a NaN misfit counts as +inf; imin = the first row of the smallest misfit;
 *          thres = max(2 min, min + 0.5); a row is FINAL when misfit < thres.  true_markov_chain != 0: a row's parameters are those
 *          of the last row at or before it whose accepted column is > 0.5 (row 0 of a point counts as accepted).  chainL > 0: only
 *          rows with r % chainL < prefix take part in the minimum, the threshold and the final set (the others count as +inf; the
 *          parameter substitution still looks at every row); chainL <= 0: every row, prefix is not read.
 *   value: Vs at zdeps[d] of a final row's model = linear interpolation on the grid points of Model1D.seisPropGrids WITHOUT the
 *          reference mantle (Model1D.value), with np.interp's bracket z[j] <= zd < z[j+1], largest j: a doubled interface point
 *          gives the lower layer's top value, zd equal to the last grid depth gives the last value.  NaN above the first or below
 *          the last grid point; a value that is not finite is not counted.
 *   out:   min_misfit, thres [npoints] fp64; imin, n_final [npoints] int (n_final: final rows).  count [npoints][D] int: finite
 *          values; vs_mean, vs_std (population, ddof = 0), vs_min, vs_max [npoints][D] fp64, NaN where count is 0.  pmean, pstd
 *          [npoints][N] fp64: the same of the final rows' parameters; both NULL: not written.  hist [npoints][D][nbins] int: counts of
 *          the nbins equal bins of [vlo, vhi) - bin i = [vlo + i w, vlo + (i + 1) w), w = (vhi - vlo) / nbins -, below, above
 *          [npoints][D] int the counts of values < vlo and >= vhi; hist NULL: none of the three is written, nbins / vlo / vhi are
 *          not read.  The entry clears the three arrays itself.
 *   how:   four stream-ordered launches, no host synchronisation, no allocation, graph-capturable.  The sums are fp64 in an order
 *          fixed by the input: a point's rows go in slabs of SURFDISP_POST_SLAB_ROWS, every slab leaves (n, mean, M2, min, max) per
 *          depth and parameter in the caller's workspace, and a last launch merges them in slab order (Chan's pairwise update) -
 *          two calls on one input return the same bits.  Only the histogram counts are (integer) atomics.
 *          SURFDISP_ERR_INVALID, before anything is launched or written: npoints, R or N below 1, N above 128, R above 2^30,
 *          npoints x slabs beyond 2^31 - 1, row_stride below 3 + N, K below 0, D outside 1..SURFDISP_POST_DEPTHS_MAX, depths that
 *          are not finite or not strictly ascending, with hist: nbins below 1, vlo or vhi not finite, vhi <= vlo; with chainL > 0:
 *          prefix outside 1..chainL, R % chainL != 0; a descriptor that is too short, has no layer or more than 10, a thermal
 *          layer (kind 6) or an unknown kind, a slot outside the [params | aux] row, grid ranges that do not tile 0..ngrid in
 *          order with at least two points each; K > 0 without aux; a NULL required pointer (track, idesc, fdesc, zdeps, min_misfit,
 *          thres, imin, n_final, count, vs_mean, vs_std, vs_min, vs_max, workspace; pmean and pstd only together; below and above
 *          with hist), a workspace smaller than surfdisp_posterior_workspace_bytes. */
#define SURFDISP_POST_SLAB_ROWS 4096
#define SURFDISP_POST_DEPTHS_MAX 256
size_t surfdisp_posterior_workspace_bytes(int npoints, int R, int N, int D);
int surfdisp_posterior_profile_device(void *stream, int npoints, int R, int N, const double *track, long row_stride,
                                      const int *idesc, int idesc_len, const double *fdesc,
                                      const double *aux, int K, const int *rows,
                                      int D, const double *zdeps, int true_markov_chain, int chainL, int prefix,
                                      int nbins, double vlo, double vhi,
                                      double *min_misfit, double *thres, int *imin, int *n_final,
                                      double *pmean, double *pstd,
                                      int *count, double *vs_mean, double *vs_std, double *vs_min, double *vs_max,
                                      int *hist, int *below, int *above,
                                      void *workspace, size_t workspace_bytes);

/* ---- (6g) posterior predictive curves of a whole Metropolis track, added within ABI 4 (csrc/surfdisp_pred.hip): the data-space view
 *          of the reference's PostPoint.plotDisp(ensemble=True) / Model3D.checkPhaseVelocity - the predicted curves of the final
 *          rows' models against the observations.  Two entries around the forward solve of (2): the first finds the DISTINCT
 *          models among the final rows, the second forms weighted statistics of their predictions.
 *          pysurfinv_amd.posterior.posterior_predictive drives both; predictive_reference is the same statement in numpy.
 *
 *   surfdisp_posterior_sources_device
 *   in:    track, row_stride (>= 3: only misfit and the accepted column are read), true_markov_chain, chainL, prefix as in (6f).
 *   out:   min_misfit, thres [npoints] fp64, imin, n_final [npoints] int: as in (6f), from the same rules and the same two
 *          selection kernels.  weight [npoints][R] int: the number of FINAL rows of the point whose parameters are those of row r
 *          (true_markov_chain != 0: r is the last accepted row at or before them, row 0 counting as accepted; otherwise the final
 *          flag of row r itself); 0 for every row that is not a source; weight sums to n_final over a point.  n_sources [npoints]
 *          int: rows with weight > 0.  imin_source [npoints] int: the source row of row imin (the row whose parameters minMod has).
 *   how:   weight is cleared on the stream, then filled with integer atomics: the result does not depend on their order.  Four
 *          launches, no host synchronisation, no allocation.  SURFDISP_ERR_INVALID, before anything is launched or written:
 *          npoints or R below 1, R above 2^30, npoints x slabs beyond 2^31 - 1, row_stride below 3, with chainL > 0: prefix
 *          outside 1..chainL, R % chainL != 0; a NULL pointer; a workspace smaller than
 *          surfdisp_posterior_sources_workspace_bytes.
 *
 *   surfdisp_posterior_predictive_device
 *   in:    pred [total] rows of ld >= P floats (device), P <= SURFDISP_PRED_COLS_MAX columns used; failed NULL or [total] bytes
 *          (nonzero: the row's solve failed); w [total] int weights (a weight <= 0: the row is ignored altogether); offsets
 *          [npoints + 1] int (device): the rows of point p are offsets[p] .. offsets[p+1] - 1 (clamped to 0..total); total = 0 is
 *          allowed (pred and w are then not read).  Histogram: vlo, vhi [P] HOST arrays, one range per column (c, U and H/V live
 *          on different scales), nbins equal bins of [vlo[c], vhi[c]) as in (6f); the ranges travel in the kernel arguments, so the
 *          arrays may be released when the entry returns.
 *   out:   an entry COUNTS when its row is not failed, its weight is positive and its value is finite.  count [npoints][P] int:
 *          the summed weight of the entries that count; mean, std (population: sqrt(sum w (v - mean)^2 / sum w)), min, max
 *          [npoints][P] fp64, NaN where count is 0 - the unweighted statistics of the list with row i repeated w[i] times.
 *          n_failed [npoints] int: the summed weight of the failed rows.  hist [npoints][P][nbins], below, above [npoints][P] int
 *          (summed weights; hist NULL: none of the three is written, nbins / vlo / vhi are not read); the entry clears them.
 *   how:   two launches (with hist: one launch of the statistics kernel per 64 columns, then the finish), no host
 *          synchronisation, no allocation, graph-capturable.  A lane is a column; a point's list goes in slabs of SURFDISP_PRED_SLAB_ROWS rows over
 *          min(ceil(total / SURFDISP_PRED_SLAB_ROWS), SURFDISP_PRED_SLABS_MAX) workgroups per point and chunk of 64 columns
 *          (workgroup s walks slabs s, s + that number, ...); each keeps fp64 sums about the first counted value, the wavefronts
 *          and then the workgroups are merged in a fixed order (weighted Chan update): two calls on one input return the same
 *          bits.  Only the histogram counts are (integer) atomics.  SURFDISP_ERR_INVALID, before anything is launched or written:
 *          npoints below 1, total below 0, P outside 1..SURFDISP_PRED_COLS_MAX, ld below P; with hist: nbins below 1, a vlo or
 *          vhi that is not finite, vhi[c] <= vlo[c], vlo / vhi / below / above NULL; a NULL required pointer (pred and w when
 *          total > 0, offsets, count, mean, std, min, max, n_failed, workspace); a workspace smaller than
 *          surfdisp_posterior_predictive_workspace_bytes. */
#define SURFDISP_PRED_SLAB_ROWS 4096
#define SURFDISP_PRED_SLABS_MAX 16
#define SURFDISP_PRED_COLS_MAX 1024
size_t surfdisp_posterior_sources_workspace_bytes(int npoints, int R);
int surfdisp_posterior_sources_device(void *stream, int npoints, int R, const double *track, long row_stride,
                                      int true_markov_chain, int chainL, int prefix,
                                      double *min_misfit, double *thres, int *imin, int *n_final,
                                      int *weight, int *n_sources, int *imin_source,
                                      void *workspace, size_t workspace_bytes);
size_t surfdisp_posterior_predictive_workspace_bytes(int npoints, int total, int P);
int surfdisp_posterior_predictive_device(void *stream, int npoints, int total, int P, const float *pred, long ld,
                                         const unsigned char *failed, const int *w, const int *offsets,
                                         int nbins, const double *vlo, const double *vhi,
                                         int *count, double *mean, double *std, double *vmin, double *vmax, int *n_failed,
                                         int *hist, int *below, int *above,
                                         void *workspace, size_t workspace_bytes);

/* ---- (6h) INTERFACE DEPTHS as unknowns of (6d) and (6e), added within ABI 4 (csrc/surfdisp_lsq.hip): the consumer of dcdh of (5g).
 *          Behind the n Vs unknowns of a stack come K THICKNESS MODES, 0 <= K <= 8: mode k has a shape T_k [Lmax] (fp64) and an
 *          amplitude y_k in km, and the thickness of input layer i changes by sum_k T_k[i] y_k.  modes = T: [K][Lmax], or
 *          [B][K][Lmax] with modes_per_stack; entries at layers i >= nlay - 1 are not read (the half space has no thickness).
 *          T[i] = h_i / sum(h[group]) on a layer group thickens the group by y and shifts everything below rigidly;
 *          + h_i / sum(h[above]) on one group and - h_i / sum(h[below]) on the next moves the interface between them down by y
 *          and leaves the total depth alone: a Moho, a sediment base, a sea floor (pysurfinv_amd.linearized.thickness_mode,
 *          interface_mode).  The two entries take the arguments of (6d) / (6e) up to and including `lam`, then:
 *   in:    K, modes, modes_per_stack.  part_h[5]: the [B][nper][Lmax] fp32 thickness kernels of the sources {cR, uR, cL, uL, chi} -
 *          part_h[0] and part_h[2] take the dcdh arrays exactly as (5g) writes them, part_h[1] and part_h[3] the dudh arrays of
 *          (5h); part_h[4] waits for dchi/dh.  mode_scale [K] ([B][K] with modes_per_stack; > 0): mode k takes lam_s mode_scale_k on its
 *          diagonal - it turns the Vs damping, in (km/s)^-2, into km^-2.  mode_prior [K] ([B][K] with modes_per_stack; beta >= 0;
 *          NULL: 0) and mode_y [B][K] (the amplitude accumulated since the starting model; NULL: 0; read by the step only): the
 *          Gaussian pull beta_k (y_k + delta_k)^2 back to the starting depth.  mode_scale and mode_prior are device memory and
 *          are not checked.
 *   rows:  unknown order: the n free layers' Vs, then the K modes.  The column of mode k in row r (source src, period idx):
 *              G[r, n + k] = sg_r * sum_{i < nlay - 1} part_h[src][s, idx, i] * T_k[i]        (an fp64 sum of fp32 x fp64),
 *          sg_r the sign of a source-5 row.  The row rules of (6d), and with K > 0 a row is also DROPPED when part_h of its
 *          source is NULL (it names a missing array) or when one of its mode columns is not finite (the NaN rows of (5g)).
 *   solve: with nu = n + K, E = diag(lam_s, .., lam_s, lam_s ms_0 + beta_0, ..) and D acting on the Vs unknowns only,
 *              (G^T W G + alpha D^T Q D + E) (delta, delta_y) = G^T W res - alpha D^T Q D x0 - (0, beta_k y_k).
 *   out:   surfdisp_lsq_step_modes_device: delta [B][Lmax] as (6d) and delta_y [B][K]; stats and info as (6d) - misfit and
 *          roughness unchanged, the predicted objective with the prior term sum_k beta_k (y_k + delta_y_k)^2 (flag != 0: the
 *          objective at x0, with sum_k beta_k y_k^2); flags as (6d), 3 still "more than nfree_max free layers"; for a flag other
 *          than 0 delta_y is zeros, never NaN.
 *          surfdisp_lsq_resolution_modes_device: cov, res [B][nfree_max + K][nfree_max + K], the modes behind the stack's n Vs
 *          unknowns, rows and columns >= n + K zeros; sigma_post, sigma_data, rdiag [B][Lmax] as (6e) and sigma_post_y,
 *          sigma_data_y, rdiag_y [B][K] of the modes; stats = dof and log det A over all nu unknowns; R = I - C (alpha D^T Q D + E).
 *          With K = 0 both entries launch the kernels of (6d) / (6e) themselves and return their bits (the mode arguments are
 *          then not read, the mode outputs not written).  With K > 0 the same kernels compiled with the mode columns: one
 *          workgroup per stack, the packed triangle for nu + 1 (step) or nu (resolution) unknowns and T in dynamic LDS - 93 KB +
 *          8 K Lmax bytes at nfree_max + K = 136; the dynamic-LDS limit is raised as in (6d): first call outside a graph capture.
 *          SURFDISP_ERR_INVALID, before anything is launched: the conditions of (6d) / (6e), K outside 0..8, nfree_max + K > 136,
 *          and with K > 0 a NULL modes, part_h, mode_scale, delta_y (step) or sigma_post_y, sigma_data_y, rdiag_y (resolution). */
int surfdisp_lsq_step_modes_device(void *stream, int B, int Lmax, const int *nlay, const float *model,
                                   const unsigned char *free_mask, int free_per_stack, int nfree_max,
                                   const float *const part[15], const float *const pred[5], const long pred_stride[5], const int nper[2],
                                   int N, const int *cols, const double *weights,
                                   const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                                   const double *vp_slope, const double *rho_slope, int slope_per_stack,
                                   double alpha, const double *Q, int q_per_stack, const double *lam,
                                   int K, const double *modes, int modes_per_stack, const float *const part_h[5],
                                   const double *mode_scale, const double *mode_prior, const double *mode_y,
                                   double *delta, double *delta_y, double *stats, int *info);
int surfdisp_lsq_resolution_modes_device(void *stream, int B, int Lmax, const int *nlay, const float *model,
                                         const unsigned char *free_mask, int free_per_stack, int nfree_max,
                                         const float *const part[15], const float *const pred[5], const long pred_stride[5],
                                         const int nper[2], int N, const int *cols, const double *weights,
                                         const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                                         const double *vp_slope, const double *rho_slope, int slope_per_stack,
                                         double alpha, const double *Q, int q_per_stack, const double *lam,
                                         int K, const double *modes, int modes_per_stack, const float *const part_h[5],
                                         const double *mode_scale, const double *mode_prior, const double *mode_y,
                                         double *cov, double *res, double *sigma_post, double *sigma_data, double *rdiag,
                                         double *sigma_post_y, double *sigma_data_y, double *rdiag_y, double *stats, int *info);

/* ---- (6i) LINEARISED INVERSION IN THE SAMPLER'S PARAMETERS, added within ABI 4 (csrc/surfdisp_lsq_params.hip): the least-squares fit of
 *          a `setting` itself - B-spline coefficients, group thicknesses, BottomDepth - where (6d)/(6h) fit layer Vs and hand-made modes.
 *          surfdisp_params_jacobian_device: the exact derivative of the map of (6) for a static-structure model WITHOUT a thermal
 *          layer.  params [C][N] and idesc / fdesc exactly as surfdisp_params_to_model_device takes them; the leading Nu columns of
 *          params are the unknowns (1 <= Nu <= min(N, 64); the random-walk parameters come first in a row, the per-point local
 *          constants behind them are never unknowns).
 *   out:   layer [C][4][L] fp64 (may be NULL): vp, vs, rho, h of the output layers - the row order of `model` - before the rounding
 *          to fp32; jac [C][4][L][Nu] fp64: their partial derivatives with respect to unknown j.  Covered: coefficient slots and
 *          constants, H slots, the BottomDepth rule (H = p - z: a thickness above enters with the opposite sign), the Vs(H) of
 *          OceanSedimentCascadia, the closed forms Vp(Vs), rho(Vs) of every layer class, the 21 points of the ReferenceMantle (z, and
 *          Vs of the last grid point), the midpoint averaging and h = z_b - z_a.  -max(topo, 0) is a local constant.  A descriptor
 *          with a thermal layer (kind 6): NaN everywhere, nothing is read from a scratch array.
 *          One thread per (chain, layer, unknown), each a dual number for its one unknown.  No workspace; graph-capturable.
 *          SURFDISP_ERR_INVALID, before anything is launched: C < 1, N < 1, Nu outside 1..min(N, 64), L outside 2..200, a NULL params,
 *          idesc, fdesc or jac.
 *          surfdisp_lsq_step_params_device: one damped least-squares step of the parameters, one stack per chain (B = C, Lmax = L).
 *   rows:  the row table of (6d) - cols, weights, obs, uncer, mask, obs_per_stack, pred[5], pred_stride[5], nper[2], part[15] - and
 *          part_h[5] of (6h) (part_h[4] waits for dchi/dh).  free [Nu] uint8, or [B][Nu] with free_per_stack (NULL: every unknown is
 *          free): the n unknowns that move.  scale [Nu] (> 0), prior_w [Nu] (beta >= 0; NULL: 0), prior_ref [Nu] (required with prior_w),
 *          params [B][Np] (Np >= Nu doubles per row; the current point, read for the prior term only), lam [B]; device memory, the
 *          values are not checked.  With sg_r the sign of a source-5 row and src the row's source,
 *              G[r,j] = sg_r * ( sum_{i<nlay}   part[src][Vs][i] jac[vs][i][j] + part[src][Vp][i] jac[vp][i][j] + part[src][rho][i] jac[rho][i][j]
 *                              + sum_{i<nlay-1} part_h[src][i] jac[h][i][j] )
 *          in fp64, layers ascending; a term whose jac entry is exactly 0 is skipped, not multiplied (a water layer's NaN d/dVs does not
 *          poison a row), and so is a term of an absent part array.  Residual, weight and every row-drop rule are those of (6d) / (6h):
 *          a row is also dropped when part_h of its source is NULL or when one of its columns is not finite.
 *   solve: in fp64 by Cholesky factorisation over the n free unknowns,
 *              A = G^T W G + lam_s diag(1 / scale_j^2) + diag(beta_j),    rhs = G^T W res - beta_j (p_j - ref_j),    delta = A^-1 rhs.
 *          The step is not clamped.
 *   out:   delta [B][Nu] (0 at fixed unknowns); stats [B][3] fp64 = data misfit sum W res^2, prior term sum beta (p - ref)^2 at p, and the
 *          objective the linear model predicts at p + delta, sum W (res - G delta)^2 + sum beta (p + delta - ref)^2; info [B][3] int = rows
 *          used, rows dropped, flag: 0 solved; 1 no usable row; 2 a pivot <= 0 or not finite (or a step or an inverse that is not
 *          finite).  For a flag other than 0 delta, cov, sigma and logdet of that stack are zeros, never NaN, and the predicted
 *          objective is the one at p.  Optional, each may be NULL and is then not computed: cov [B][Nu][Nu] = A^-1 in unknown order,
 *          exactly symmetric, zeros in the rows and columns of fixed unknowns; sigma [B][Nu] = sqrt(diag cov); logdet [B] = log det A.
 *          One workgroup of 256 lanes per stack, normal equations accumulated 16 rows at a time in LDS, G never stored, jac read from
 *          global memory.  LDS: 48 112 bytes, static, at every Nu <= 64 (the triangle of 65 x 65 doubles 17 KB, the staged rows 8 KB, a 64-layer
 *          chunk of their kernels 16 KB): no limit to raise, graph-capturable from the first call.  No workspace.
 *          SURFDISP_ERR_INVALID, before anything is launched: B < 1, Lmax outside 1..200, N outside 1..800, Nu outside 1..64, Np < Nu,
 *          a NULL required pointer (jac, part, part_h, pred, pred_stride, nper, cols, weights, obs, uncer, mask, scale, params, lam,
 *          delta, stats, info), prior_w without prior_ref, and the conditions of (6d) on the prediction and partial arrays (part_h
 *          of a source without predictions included). */
int surfdisp_params_jacobian_device(void *stream, int C, int N, int Nu, int L, const double *params,
                                    const int *idesc, const double *fdesc, double *layer, double *jac);
int surfdisp_lsq_step_params_device(void *stream, int B, int Lmax, const int *nlay, int Nu, const double *jac,
                                    const float *const part[15], const float *const part_h[5],
                                    const float *const pred[5], const long pred_stride[5], const int nper[2],
                                    int N, const int *cols, const double *weights,
                                    const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                                    const unsigned char *free_mask, int free_per_stack,
                                    const double *scale, const double *prior_w, const double *prior_ref,
                                    const double *params, int Np, const double *lam,
                                    double *delta, double *stats, int *info, double *cov, double *sigma, double *logdet);

/* ---- (7) introspection of the two-tier root search. The production kernel hands the stacks it cannot treat
 *          faithfully to an exact fallback kernel that runs right behind it inside the same call: a secular
 *          function that leaves the fp32 range (the reference's overflow points depend on how it forms its matrix
 *          entries, surfa.f:289-330) and brackets with more than one visible sign change (which root NEVILL,
 *          surfa.f:2-83, lands on depends on its evaluation sequence).  Returns in *count how many stacks (in
 *          SURFDISP_INDEPENDENT mode: (stack, period) units) of the last solve on `workspace` took that path.
 *          Waits for `stream`. */
int surfdisp_workspace_fallback_count(void *stream, const void *workspace, int B, int Lmax, int P, int *count);
/*          ... and counts3[3] = {that count; brackets the root search refined with NEVILL because they may hold several roots
 *          (vertical phase growing by more than 1 rad across the bracket); Rayleigh ellipticities evaluated again with the
 *          reference's own arithmetic (closure cancelling, or c far below the stack's fastest S velocity)}. */
int surfdisp_workspace_counters(void *stream, const void *workspace, int B, int Lmax, int P, int *counts3);

/* ---- tuning / introspection ------------------------------------------------------------- */
/* lanes of one wavefront that cooperate on one stack's root search (1,2,4,...,64); 0 = choose
 * from (B, Lmax).  Also settable through the environment variable SURFDISP_TEAM. */
int  surfdisp_set_team(int lanes);
int  surfdisp_get_team(int B, int Lmax);           /* what a Rayleigh c+U launch with (B, Lmax) would use */
int  surfdisp_get_team2(int B, int Lmax, int P, int kind);   /* ... a launch with these kind flags (wave type, PHASE_ONLY, PIPELINED, INDEPENDENT) */
int  surfdisp_device_count(void);                  /* gfx950 devices visible; <=0: none */
int  surfdisp_abi_version(void);
const char *surfdisp_last_error(void);             /* thread-local, never NULL */
const char *surfdisp_kernel_name(int which);       /* 0 prep, 1 phase (root search), 2 group, 3 finish */

#ifdef __cplusplus
}
#endif
#endif /* SURFDISP_H */
