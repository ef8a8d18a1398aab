// surfdisp_internal.h -- kernel argument blocks and launch prototypes shared by
// surfdisp_kernels.hip and surfdisp_capi.hip.  Not part of the public ABI (include/surfdisp.h).
// surfdisp_kernels.hip is one translation unit; its first stages are headers it includes: surfdisp_k_common.h,
// surfdisp_k_prep.h (K0), surfdisp_k_secular.h, and so is surfdisp_k_rows.h: the scratch-to-rows tile walk of K2b, K2d, K4c and
// K5d and the unit part of Rodi's rule, which surfdisp_group_thick.hip (K4d) includes too.  The root search (K1) and what
// follows it stand in the .hip itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "surfdisp.h"

namespace sd {

struct PrepArgs {
    int B, Lmax;
    const int *nlay;      // [B] or nullptr
    const float *model;   // [B][5][Lmax] (vp, vs, rho, h, qsinv) as handed over by the caller
    float *mdl;           // [9][Lmax][B] SoA: vp, vs, rho, 1/Qs + five flattening factors
    int *nl;              // [B] validated layer count, 0 = bad model
    int P;
    int *nsolved_init;    // nullptr, or [B]: set to P (independent mode reduces it with atomicMin)
    float *fsafe;         // [B]: thickest layer (km) of a stack whose Vs and Vp never decrease with depth,
                          // 1e30 otherwise (the scan then skips nothing on that stack)
    float *ovf;           // [3][B]: thickest flattened layer, 2 ln(max rho), 4 ln(2 max Vs^2): entry_overflow_risk
    int *fb_count;        // [1]: zeroed here; stacks the production root search hands to the exact fallback
    float *rows;          // nullptr, or [B][9][Lmax]: the same nine fields one ROW per stack and field - what the root
                          // search's per-period rebuild reads when a stack has >= 8 lanes (consecutive lanes = consecutive
                          // layers: coalesced; the SoA copy costs a cache line per value there)
    int write_soa;        // 0: only the rows are needed (phase-only call with wide teams: no group-velocity kernel)
};

struct PhaseArgs {
    int B, Lmax, P;
    const float *mdl;
    const int *nl;
    const float *per;     // [P]
    float *c;             // [P][B] period-major (internal; transposed by the finish kernel)
    float *ratio;         // [P][B] ellipticity (Rayleigh), input of the group-velocity kernel
    int *nsolved;         // [B]
    int *status;          // [B] or nullptr
    float wtol;           // bracket width below which the root may be read off by interpolation
    float atol;           // ... provided secant and 3-point estimates agree to this (km/s)
    int fast;             // count-guided coarse-to-fine scan (Love's default, Rayleigh's opt-in SURFDISP_FASTSCAN); 0 = every grid point
    const float *fsafe;   // [B], see PrepArgs
    // (always 0 since the r02 second LDS slot and the r01 phase rule went; the two words keep the argument block's layout:
    // taking them out regroups the kernels' argument loads and changes their instruction counts, which the committed
    // counter profiles are tagged with - see profiles/variants_removed/README.md)
    int overlap;
    float phimax;
    const float *ovf;     // [3][B], see PrepArgs
    int *fb_count;        // [1] number of entries of fb_list
    int *fb_list;         // [teams]: team indices (stack, or period * B + stack in independent mode) for the exact kernel
    int balance;          // wavefront priority by progress (one batch in flight), see the kernel's main loop
    int strict;           // SURFDISP_STRICT: every team hands its stack to the exact kernel
    // where the root search reads the staged fields: value (field f, layer i) of stack b at
    // msrc[b * ms_b + f * ms_f + i * ms_i] - the SoA copy (1, Lmax * B, B) or the rows (9 * Lmax, Lmax, 1)
    const float *msrc;
    long ms_b, ms_f, ms_i;
    // nullptr, or [P][B]: per solved period the state the ellipticity kernel replays the working stack from - (number of
    // layers the period's rebuild refreshed) | (frozen effective half space << 16); sign bit set: this period's ellipticity
    // was computed in the kernel itself (exact fallback; the two fields are still recorded for the ellipticity kernels)
    int *hist;
    int lockstep;         // the teams of a wavefront refine and end their periods together (see the root search's main loop)
    float ambig;          // (always 0, unread: kept for the layout like overlap / phimax)
    float phimulti;       // a bracket across which the vertical phase grows by more than this (rad) goes to NEVILL
    int *amb_count;       // nullptr, or [2]: brackets sent to NEVILL by the phase rule / ellipticities evaluated again (statistics)
    float ell_ambig;      // in-kernel ellipticity passes: a closure below this fraction of its terms marks the pair for the ellipticity kernel
    float ell_gmax;       // ... and so does g = 2 b^2 / c^2 of the stack's fastest layer beyond this
    int scan_general;     // 1: pure scan passes also run the general pass body (SURFDISP_LEANSCAN=0, for A/B and the tests)
#ifdef SD_WAVECLOCK
    unsigned long long *wclk;   // developer build: [waves][24], s_memrealtime at wavefront start / end and the counters of scripts/waveclock.py
#endif
};

struct GroupArgs {
    int B, Lmax, P;
    const float *mdl;
    const int *nl;
    const float *per;
    const float *c;       // [P][B]
    const float *ratio;
    const int *nsolved;
    float *u;             // [P][B]
    double *dbg;          // nullptr, or [B][P][16] intermediate values (developer builds)
    float *kb, *ka, *kr;  // nullptr, or [B][P][Lmax] analytic partials dc/dVs, dc/dVp, dc/drho
    float *kscr;          // nullptr, or the layer-major scratch [3][Lmax][P][B] the unscaled shares are stored in (coalesced)
    float *kscale;        // with kscr: [P][B] the unit's factor 1 / (dL/dk), 0 = no partials (unsolved / invalid unit)
    int *khs;             // with kscr: [P][B] deepest layer the unit wrote (-1: none)
    int kraw;             // SURFDISP_KERN_REFCOORD: partials in the reference's coordinates (unit chain factors)
    int xcd_order;        // set by launch_group: workgroup -> (stack block, period) order that keeps a stack block's periods on one XCD
    int krev;             // (developer knob, SURFDISP_GROUP_ORDER + 100: periods in descending order)
    int group_order;      // SURFDISP_GROUP_ORDER: < 0 the library's rule (launch_group), 0 plain period-major order, g > 0: an XCD takes g stack blocks at a time
    // eigenfunctions (surfdisp_forward_eigen_device; the EIG instantiations only, which write no partials)
    float *escr;          // nullptr, or the layer-major scratch [4][Lmax][P][B] (Love: 2 planes) of the layer-top values
    float *ediv;          // with escr: [P][B] the unit's divisor (Rayleigh 1, Love ut at the top)
    int *ehs;             // with escr: [P][B] deepest layer the unit wrote (-1: none - unsolved, bad stack, degenerate exit)
    float *esum;          // with escr: [3][P][B] the energy integrals I0, I1, I2 the group velocity is formed from
    int stash;            // in: < 0 never keep the fit's layer values in LDS (SURFDISP_GROUP_STASH=0), 0 the library's rule; set by launch_group: 1 = this launch keeps them
};
// eigenfunctions from the layer-major scratch to the caller's rows, see K2d
struct EigenTransposeArgs {
    int B, P, Lmax, kind;
    const float *mdl;     // SoA staged fields (Love: the layers' Vs of the low-amplitude exclusion)
    const int *nl;        // [B]
    const float *per;     // [P]
    const float *escr;    // [4][Lmax][P][B] (Love: planes 0, 1)
    const float *ediv;    // [P][B]
    const int *ehs;       // [P][B]
    const float *esum;    // [3][P][B]
    const float *c, *u;   // [P][B] period-major
    float *ur, *uz, *tz, *tr;   // the caller's [B][P][Lmax] rows (all but ur may be nullptr)
    float *energy;        // nullptr, or the caller's [B][P][4]: I0, I1, I2, 1 / (2 c U I0)
};
hipError_t launch_eigen_transpose(hipStream_t s, const EigenTransposeArgs &a);
struct KernTransposeArgs {
    int B, P, Lmax, kind;
    const float *kscr;    // [3][Lmax][P][B]
    const float *kscale;  // [P][B]
    const int *khs;       // [P][B]
    float *kb, *ka, *kr;  // the caller's [B][P][Lmax] rows (ka, kr may be nullptr)
};
// apparent attenuation of the mode (surfdisp_forward_atten_device) from the same scratch, see K2c
struct AttenArgs {
    int B, P, Lmax, kind;
    const float *mdl;     // SoA staged fields (Vs, Vp, 1/Qs of every layer)
    const float *per;     // [P]
    const float *kscr;    // [3][Lmax][P][B] unscaled shares; planes 0 (dc/dVs) and, Rayleigh, 1 (dc/dVp) are read
    const float *kscale;  // [P][B]
    const int *khs;       // [P][B]
    const float *c, *u;   // [P][B] period-major
    float *qinv, *gamma;  // the caller's [B][P] arrays: 1 / Q_apparent, attenuation coefficient (1/km; may be nullptr)
    float *dqdq;          // nullptr, or the caller's [B][P][Lmax] rows: d (1 / Q_apparent) / d (1/Qs of layer i)
};
hipError_t launch_atten(hipStream_t s, const AttenArgs &a);
// thickness and interface-depth kernels of c (surfdisp_forward_thickness_kernels_device) from both scratches, see K2e
struct ThickArgs {
    int B, P, Lmax, kind;
    const float *model;   // the caller's [B][5][Lmax]: row 3, the thicknesses (the staged fields hold only the flattened ones)
    const float *mdl;     // SoA staged fields
    const int *nl;        // [B]
    const float *per;     // [P]
    const float *escr;    // [4][Lmax][P][B] layer-top values (Love: planes 0, 1)
    const float *ediv;    // [P][B]
    const int *ehs;       // [P][B]
    const float *esum;    // [3][P][B]: plane 0, I0, is read
    const float *kscr;    // [3][Lmax][P][B] unscaled shares (Love: planes 0, 2)
    const float *kscale;  // [P][B]
    const int *khs;       // [P][B]
    const float *c, *u;   // [P][B] period-major
    float *dcdh, *dcdz;   // the caller's [B][P][Lmax] rows (dcdz may be nullptr)
    int *n_nonfinite;     // nullptr, or [1]: solved units with NaN rows
};
hipError_t launch_thickness(hipStream_t s, const ThickArgs &a);

// group-velocity kernels (surfdisp_forward_group_kernels_device): the fundamental-mode roots at the shifted periods
// T (1 -+ dfrac) of every solved (stack, period) unit, found from the first-order prediction without a scan
struct ShiftArgs {
    int B, Lmax, P, kind;
    const float *mdl;     // SoA staged fields
    const int *nl;
    const float *per;     // [P] the solve's periods
    const float *c, *u;   // [P][B] the solve's roots and group velocities (period-major)
    const int *nsolved;   // [B]
    float dfrac;          // relative period shift
    float *pers;          // [2][P] out: the shifted periods T (1 - dfrac), T (1 + dfrac)
    float *cs;            // [2][P][B] out: the roots there; the unit's own c where the unit is unsolved or failed
    float *ratio;         // [2][P][B] out (Rayleigh): the ellipticity at the shifted root, formed as surfdisp_ellip_kernel does
    unsigned char *fail;  // [2][P][B] out: 1 = no unique root inside the search budget (or a non-finite value)
    float ell_ambig, ell_gmax;   // see EllipArgs
    const float *ovf;     // [3][B] prep statistics
};
hipError_t launch_shift(hipStream_t s, const ShiftArgs &a);
// dU/d(Vs, Vp, rho) from the partials at the two shifted periods (layer-major scratches, as KernTransposeArgs) and c, U
struct GroupCombineArgs {
    int B, P, Lmax, kind;
    const float *kscr_m, *kscr_p;       // [3][Lmax][P][B] unscaled shares at T (1 - dfrac) and T (1 + dfrac)
    const float *ksc_m, *ksc_p;         // [P][B] their factors 1 / (dL/dk)
    const int *khs_m, *khs_p;           // [P][B] their deepest layers
    const float *ksc0;                  // [P][B] the factor of the unshifted unit: 0 = no partials (unsolved), rows of zeros
    const unsigned char *fail;          // [2][P][B] see ShiftArgs
    const float *c, *u;                 // [P][B] c and U at T
    float inv_dlnT;                     // 1 / ln((1 + dfrac) / (1 - dfrac))
    float *ub, *ua, *ur;                // the caller's [B][P][Lmax] rows (ua, ur may be nullptr)
    int *n_failed;                      // nullptr, or [1]: solved units whose shifted pass failed (NaN rows)
};
hipError_t launch_group_combine(hipStream_t s, const GroupCombineArgs &a);
// dU/d(layer thickness, interface depth) (surfdisp_forward_group_thickness_kernels_device) from the rows of K2e at the two shifted
// periods, see K4d in surfdisp_group_thick.hip
struct GroupThickCombineArgs {
    int B, P, Lmax;
    const float *hm, *hp;               // [B][P][Lmax] dcdh at T (1 - dfrac) and T (1 + dfrac), as K2e writes them
    const float *zm, *zp;               // ... and dcdz there (read with dudz only)
    const float *h0;                    // [B][P][Lmax] dcdh at T (the caller's rows): where it is zero the results are
    const float *ksc_m, *ksc_p, *ksc0;  // [P][B] as GroupCombineArgs: the units the shifted pass failed for are the same
    const unsigned char *fail;          // [2][P][B] see ShiftArgs
    const float *c, *u;                 // [P][B] c and U at T
    float inv_dlnT;                     // 1 / ln((1 + dfrac) / (1 - dfrac))
    float *dudh, *dudz;                 // the caller's [B][P][Lmax] rows (dudz may be nullptr)
    int *n_nonfinite;                   // nullptr, or [1]: units with a NaN thickness row at T or at a shifted period
};
hipError_t launch_group_thick_combine(hipStream_t s, const GroupThickCombineArgs &a);

struct EllipArgs {
    int B, Lmax, P;
    const float *mdl;     // SoA staged fields
    const int *nl;
    const float *per;
    const float *c;       // [P][B] roots
    const int *hist;      // [P][B], see PhaseArgs
    const int *nsolved;   // [B]
    float *ratio;         // [P][B]
    float ell_ambig;      // a closure below this fraction of its terms: both passes again with the reference's arithmetic (0: never; < 0: always)
    int only_flagged;     // 1: the root search wrote the ellipticities itself; redo only the pairs it marked (bit 30 of hist)
    int *amb_count;       // nullptr, or [2] statistics, see PhaseArgs
    float ell_gmax;       // ... and where g = 2 b^2 / c^2 of the stack's fastest layer exceeds this
    const float *ovf;     // [3][B] prep statistics (entry 2: 4 ln(2 bmax^2))
};
hipError_t launch_ellip(hipStream_t s, const EllipArgs &a);

// ellipticity kernels (surfdisp_forward_ellip_kernels_device): dchi/d(Vs, Vp, rho) of the Rayleigh ellipticity, see K5
struct EllipKernArgs {
    int B, Lmax, P;
    const float *mdl;     // SoA staged fields
    const int *nl;
    const float *per;
    const float *c;       // [P][B] roots
    const int *hist;      // [P][B], see PhaseArgs
    const int *nsolved;   // [B]
    int *kpk;             // [Lmax][P][B] scratch: per layer the period whose rebuild it comes from | 0x10000 (half-space form)
    double *wscr;         // [5][Lmax][P][B] scratch: the adjoint rows
    float *xscr, *fscr;   // [3][Lmax][P][B] scratch: per layer dchi/d(Vs, Vp, rho) at fixed c, and dF/d(Vs, Vp, rho)
    float *gam;           // [P][B] out: -(dchi/dc) / (dF/dc)
    int *khs;             // [P][B] out: deepest layer with partials; -1 none (zeros), -2 non-finite (NaN rows)
    int *n_nonfinite;     // nullptr, or [1]: units with NaN rows
};
struct EllipTransposeArgs {
    int B, P, Lmax;
    const float *xscr, *fscr, *gam;
    const int *khs;
    float *eb, *ea, *er;  // the caller's [B][P][Lmax] rows (ea, er may be nullptr)
};
hipError_t launch_ellip_kern(hipStream_t s, const EllipKernArgs &a, const EllipTransposeArgs &t);

struct FinishArgs {
    int B, P;
    const float *ct, *ut; // [P][B]
    float *c, *u;         // [B][P] caller's arrays
    const int *nsolved;   // nullptr (faithful) or [B] first failing period (independent mode)
    const int *nl;
    int *status;
    const float *rt;      // nullptr, or [P][B] ellipticity (period-major, Rayleigh) ...
    float *ratio;         // ... and the caller's [B][P] array it goes to (ABI 3)
    const int *nsolved_all; // [B] periods solved (either mode): unsolved periods of `ratio` are written as 0
};

struct LayersArgs {
    int C, N;
    const double *params;  // [C][N]
    const int *idesc;      // see surfdisp_layers.hip
    const double *fdesc;
    float *model;          // [C][5][L]
    double *scratch;       // [C][64][2] (vs, qs) of the thermal layer's grid points, or nullptr
};
constexpr int SD_MCMC_MAX_DEPTH = 4, SD_MCMC_MAX_NODES = (1 << SD_MCMC_MAX_DEPTH) - 1;
constexpr int SD_MCMC_JOINT_MAX_COLS = 800;   // observation columns of the joint accept kernel: four curves of <= 200 periods
struct McmcProposeArgs {
    int C, N;
    const double *p;        // [C][N] current parameters
    const double *vmin, *vmax, *step;   // [N]
    unsigned long long seed, counter;
    int reset;              // 1: uniform prior draw for every entry (MCinv.reset), 0: bounded Gaussian step
    double *out;            // [C][N]
    long chain0;            // global index of chain 0 of this launch (keys the random streams: a sampler split into chain groups draws what the unsplit one draws)
    int depth;              // <= 1: one proposal per chain; d > 1: the speculative tree of 2^d - 1 proposals (out [C][2^d-1][N])
    const unsigned char *redo;   // nullptr, or [C]: only chains with redo[c] == redo_tag draw (masked redraw, depth 1)
    int attempt;            // ... try number of this step: its own random numbers
    int redo_tag;
};
struct McmcAcceptArgs {
    int C, N, P;
    const float *c;         // [C][P] predicted phase velocities of the proposals
    const int *status;      // [C] or nullptr
    const double *c_obs, *uncer;   // [P], or [C][P] when obs_per_chain
    const unsigned char *mask;     // same shape: 1 = the period counts
    int obs_per_chain;
    const double *p1;       // [C][N] proposals
    double *p0;             // [C][N] chain states, updated in place
    double *chi0;           // [C] chi-square of the states, updated in place
    double *row;            // nullptr, or row c at row + c * row_stride: [misfit, L, accepted, params of the proposal]
    long row_stride;        // in doubles
    unsigned long long seed, counter;
    int first;              // 1: first row of a chain (always accepted: the start model)
    long chain0;            // global index of chain 0 of this launch
    int depth, nsteps;      // speculative tree: walk nsteps <= depth steps (depth <= 1: the plain single test)
    long step_stride;       // doubles between the mcTrack rows of consecutive steps of one chain
};
// the proposal tree of a sampler with a prior, redrawn inside the kernel until the rules hold (csrc/surfdisp_mcmc_prior.hip;
// include/surfdisp.h section (6c))
constexpr int SD_MCMC_PRIOR_ROW = SURFDISP_MCMC_PRIOR_ROW_MAX;   // doubles of the candidate row in LDS: N + K
constexpr int SD_MCMC_PRIOR_TRIES = SURFDISP_MCMC_PRIOR_TRIES_MAX;
constexpr int SD_MCMC_PRIOR_GRID_EXTRA = 11;   // grid points whose Vs it keeps in LDS, beyond L: L output layers of <= 10 input layers have <= L + 10 (with the ReferenceMantle's 21 points: <= L + 11)
struct McmcPriorArgs {
    int C, N, K, L, depth;
    const double *p;        // [C][N] chain states
    const double *aux;      // [C][K] per-chain local constants (slots N .. N + K - 1 of a row), nullptr when K == 0
    const double *vmin, *vmax, *step;   // [N]
    const int *idesc;       // the params -> stack descriptor, see surfdisp_layers.hip
    const double *fdesc;
    const int *flags;       // [L] the rules per output layer, see surfdisp_prior_kernel
    double vs_max;          // < 0: no cap
    int gauss_tries, uniform_tries;
    unsigned long long seed, counter;
    long chain0;
    double *out;            // [C][2^depth - 1][N]
    unsigned short *tries;  // [C][2^depth - 1] or nullptr
    int *exhausted;         // [1], incremented per node without a good candidate
};
hipError_t launch_mcmc_propose_prior(hipStream_t s, const McmcPriorArgs &a);
// the same tree with proposals x + F z, F the lower-triangular factor of the chain's point, and that factor from a covariance
// (csrc/surfdisp_mcmc_cov.hip; include/surfdisp.h section (6c))
constexpr int SD_MCMC_COV_MAX_N = SURFDISP_MCMC_COV_N_MAX;        // one lane per scalar
struct McmcCovArgs {
    int C, N, K, L, depth;
    const double *p;        // [C][N] chain states
    const double *aux;      // [C][K] per-chain local constants, nullptr when K == 0
    const double *vmin, *vmax;   // [N]
    const double *factor_t; // [F][N][N]: factor_t[f][k][n] = L_f[n][k]
    long chains_per_factor; // chain chain0 + c takes factor (chain0 + c) / chains_per_factor
    const int *idesc;       // the params -> stack descriptor, see surfdisp_layers.hip; nullptr without flags
    const double *fdesc;
    const int *flags;       // [L] the rules per output layer, see surfdisp_prior_kernel; nullptr: the box alone (K = L = 0)
    double vs_max;          // < 0: no cap
    int gauss_tries, uniform_tries;
    unsigned long long seed, counter;
    long chain0;
    double *out;            // [C][2^depth - 1][N]
    unsigned short *tries;  // [C][2^depth - 1] or nullptr
    int *exhausted;         // [1], incremented per node without a good candidate
};
hipError_t launch_mcmc_propose_cov(hipStream_t s, const McmcCovArgs &a);
struct McmcCovFactorArgs {
    int P, N;
    const double *cov;      // [P][N][N] symmetric; zero rows and columns at fixed parameters
    double scale;
    const double *fallback_step;   // [N]
    double *factor_t;       // [P][N][N]
    int *flag;              // [P]: 0 factored, 1 diag(fallback_step)
};
hipError_t launch_mcmc_cov_factor(hipStream_t s, const McmcCovFactorArgs &a);
// adaptive proposals: one pooled update of every point's mean, scatter and log scale, and the covariance the factor kernel takes
// (csrc/surfdisp_mcmc_adapt.hip; include/surfdisp.h section (6c))
constexpr int SD_MCMC_ADAPT_HEAD = SURFDISP_MCMC_ADAPT_HEAD;
struct McmcAdaptArgs {
    int F, cpp, N;
    const double *p;        // [F * cpp][N] the chains' current states
    const double *track;    // the accept flags: track[chain * chain_stride + row * row_stride + 2]; nullptr without a window
    long chain_stride, row_stride;
    int row_lo, row_hi;     // the window's rows [row_lo, row_hi)
    const double *step;     // [N]
    double forget, target_accept, gain, decay, ls_min, ls_max, min_weight, ridge;
    double *state;          // [F][SD_MCMC_ADAPT_HEAD + N + N N]
    double *cov_out;        // [F][N][N] or nullptr
};
hipError_t launch_mcmc_adapt(hipStream_t s, const McmcAdaptArgs &a);
// joint data (Rayleigh / Love, phase / group, Rayleigh ellipticity): the accept kernel's arguments plus the solves' predictions and
// the column table.  In `a`, c and P are unused; c_obs / uncer / mask have Ptot columns (P of `a` = Ptot).
struct McmcJointArgs {
    McmcAcceptArgs a;
    const float *pred[5];   // cR, uR, cL, uL, chi of the Rayleigh solve: [stacks][pstride[s]] or nullptr; a wave type has data iff its c array is given
    long pstride[5];        // floats between the stacks' rows of each array
    int nper[2];            // periods of the Rayleigh / Love solve
    const int *status[2];   // [stacks] or nullptr
    const int *cols;        // [Ptot][2]: source (0..3 the arrays; 4 chi, 5 |chi|: pred[4], the joint5 entries only), period index in that solve
    const double *weights;  // [Ptot]
};
// damped least-squares step of the free layers' Vs (csrc/surfdisp_lsq.hip; include/surfdisp.h section (6d))
constexpr int SD_LSQ_MAX_FREE = 128;    // unknowns per stack: the packed triangle of 129 x 129 doubles is 66 KB of LDS
constexpr int SD_LSQ_MAX_MODES = 8;     // thickness modes per stack behind the Vs unknowns (section (6h)): 137 x 137 doubles, 93 KB
constexpr int SD_LSQ_TILE_ROWS = 16;    // data rows staged in LDS at a time
struct LsqArgs {
    int B, Lmax, N, nmax;   // stacks, layers per row, data rows, upper bound of the free layers of any stack (sizes the LDS)
    const int *nlay;        // [B] or nullptr
    const float *model;     // [B][5][Lmax]: row 1 (Vs) is the linearisation point
    const unsigned char *free_mask;   // [Lmax] or [B][Lmax] (free_per_stack), nullptr: every layer below nlay
    int free_per_stack;
    const float *part[15];  // [source 0..4: cR, uR, cL, uL, chi][d/dVs, d/dVp, d/drho]: [B][nper of the source's solve][Lmax] or nullptr
    const float *pred[5];   // the same solves' predictions (McmcJointArgs)
    long pstride[5];
    int nper[2];
    const int *cols;        // [N][2] (McmcJointArgs)
    const double *weights;  // [N]
    const double *obs, *uncer;        // [N], or [B][N] when obs_per_stack
    const unsigned char *mask;        // same shape
    int obs_per_stack;
    const double *vp_slope, *rho_slope;   // dVp/dVs, drho/dVs: [Lmax] or [B][Lmax] (slope_per_stack), nullptr: 0
    int slope_per_stack;
    double alpha;
    const double *Q;        // interface weights [Lmax-1] or [B][Lmax-1] (q_per_stack), nullptr: 1
    int q_per_stack;
    const double *lam;      // [B]
    double *delta;          // [B][Lmax]
    double *stats;          // [B][3]: data misfit, roughness, predicted objective
    int *info;              // [B][3]: rows used, rows dropped, flag
    // the resolution kernel only (section (6e)); there stats is [B][2]: dof, log det A, and delta is not used
    double *cov, *res;      // [B][nmax][nmax] or nullptr
    double *sigma_post, *sigma_data, *rdiag;   // [B][Lmax]
    // thickness modes (section (6h)); K = 0: none of these is read, the kernels are those of (6d) / (6e).  With K > 0 cov and res
    // are [B][nmax + K][nmax + K]
    int K;                  // 0..SD_LSQ_MAX_MODES
    const double *modes;    // [K][Lmax], or [B][K][Lmax] when modes_per_stack
    int modes_per_stack;
    const float *part_h[5]; // dcdh of the five sources: [B][nper of the source's solve][Lmax] or nullptr
    const double *mode_scale, *mode_prior;     // [K] or [B][K] (modes_per_stack); mode_prior nullptr: 0
    const double *mode_y;   // [B][K] or nullptr: 0 (the step kernel only)
    double *delta_y;        // [B][K] (the step kernel)
    double *sigma_post_y, *sigma_data_y, *rdiag_y;   // [B][K] (the resolution kernel)
};
// Jacobian of the params -> stack map and the least-squares step in parameter space (csrc/surfdisp_lsq_params.hip; include/surfdisp.h
// section (6i))
constexpr int SD_PLSQ_MAX_UNKNOWNS = 64;   // unknowns per stack: the packed triangle of 65 x 65 doubles is 17 KB of LDS
constexpr int SD_PLSQ_CHUNK = 64;          // layers of the staged rows' partial arrays held in LDS at a time
struct ParamsJacArgs {
    int C, N, Nu, L;
    const double *params;   // [C][N]
    const int *idesc;       // see surfdisp_layers.hip
    const double *fdesc;
    double *layer;          // [C][4][L] or nullptr
    double *jac;            // [C][4][L][Nu]
};
struct ParamLsqArgs {
    int B, Lmax, N, Nu, Np; // stacks, layers per row, data rows, unknowns, doubles between the rows of params
    const int *nlay;        // [B] or nullptr
    const double *jac;      // [B][4][Lmax][Nu]: d(vp, vs, rho, h of layer i) / d(unknown j)
    const float *part[15];  // as LsqArgs
    const float *part_h[5];
    const float *pred[5];
    long pstride[5];
    int nper[2];
    const int *cols;        // [N][2]
    const double *weights;  // [N]
    const double *obs, *uncer;        // [N], or [B][N] when obs_per_stack
    const unsigned char *mask;
    int obs_per_stack;
    const unsigned char *free_mask;   // [Nu] or [B][Nu] (free_per_stack), nullptr: every unknown
    int free_per_stack;
    const double *scale, *prior_w, *prior_ref;   // [Nu]; prior_w nullptr: 0 (prior_ref is then not read)
    const double *params;   // [B][Np]: the current point, read for the prior term
    const double *lam;      // [B]
    double *delta;          // [B][Nu]
    double *stats;          // [B][3]: data misfit, prior term at p, predicted objective at p + delta
    int *info;              // [B][3]: rows used, rows dropped, flag
    double *cov, *sigma, *logdet;     // [B][Nu][Nu], [B][Nu], [B], each or nullptr
};
hipError_t launch_params_jacobian(hipStream_t s, const ParamsJacArgs &a);
hipError_t launch_lsq_step_params(hipStream_t s, const ParamLsqArgs &a);
// posterior Vs(z) profiles of a Metropolis track (csrc/surfdisp_post.hip; include/surfdisp.h section (6f)).  The descriptor's
// integer part and the depths travel in the kernel arguments: the entry has checked them on the host.
constexpr int SD_POST_SLAB = SURFDISP_POST_SLAB_ROWS;   // rows of one point a workgroup walks: the unit of the per-slab partials
constexpr int SD_POST_MAX_LAYERS = 10;                  // input layers of the descriptor (Model1DBatch.native_descriptor's own cap)
constexpr int SD_POST_MAX_PARAMS = 128;                 // two parameters per lane of the profile kernel
struct PostArgs {
    int npoints, R, N, K, D, nslab;
    int tmc, chainL, prefix;   // true_markov_chain; chainL > 0: only rows with r % chainL < prefix are selected
    int nbins;
    long row_stride;           // doubles between the rows of the track; a point's rows are R * row_stride apart
    const double *track;       // [npoints][R][row_stride]: misfit, L, accepted, params[N]
    const double *fdesc;       // the descriptor's float part (device)
    const double *aux;         // nullptr, or [.][K] per-point constants: slot N + k of a row
    const int *rows;           // nullptr (point p reads aux row p), or [npoints] the aux row of each point
    double vlo, vhi, bin_w, inv_w;
    double *min_misfit, *thres;   // [npoints]
    int *imin, *n_final;          // [npoints]
    double *pmean, *pstd;         // nullptr, or [npoints][N]
    int *count;                   // [npoints][D]
    double *vs_mean, *vs_std, *vs_min, *vs_max;   // [npoints][D]
    int *hist, *below, *above;    // nullptr, or [npoints][D][nbins], [npoints][D], [npoints][D]
    double *ws_part;           // workspace: [npoints][nslab][D + N][5] (n, mean, M2, min, max)
    double *ws_mis;            // [npoints][nslab] smallest misfit of the slab
    int *ws_row, *ws_last, *ws_carry, *ws_nfin;   // [npoints][nslab] its row, the slab's last accepted row, the one it starts from, final rows
    int idesc[4 + 16 * SD_POST_MAX_LAYERS];
    double zdeps[SURFDISP_POST_DEPTHS_MAX];
};
hipError_t launch_posterior(hipStream_t s, const PostArgs &a);
hipError_t launch_post_selection(hipStream_t s, const PostArgs &a);   // K1 and K2 of launch_posterior alone
// source rows of a track and weighted statistics of a list of predictions (csrc/surfdisp_pred.hip; include/surfdisp.h section (6g))
constexpr int SD_PRED_SLAB = SURFDISP_PRED_SLAB_ROWS;   // list rows a workgroup of the statistics kernel walks at a time
struct PostSourcesArgs {
    PostArgs sel;              // what launch_post_selection reads and writes; its ws_nfin holds the slabs' final rows
    int *weight;               // [npoints][R]
    int *n_sources, *imin_source;   // [npoints]
};
struct PredArgs {
    int npoints, total, P, nslab, nbins;
    long ld;                   // floats between the rows of pred
    const float *pred;         // [total][ld]
    const unsigned char *failed;   // nullptr, or [total]
    const int *w;              // [total]
    const int *offsets;        // [npoints + 1]
    int chunk0;                // the chunk of 64 columns of blockIdx.y = 0 (with a histogram: one launch per chunk)
    double vlo[64], vhi[64];   // with hist: the histogram ranges of this launch's 64 columns, by value
    int *count;                // [npoints][P]
    double *mean, *std, *mn, *mx;   // [npoints][P]
    int *n_failed;             // [npoints]
    int *hist, *below, *above; // nullptr, or [npoints][P][nbins], [npoints][P], [npoints][P]
    double *ws_part;           // [npoints][nslab][P][5] (n, mean, M2, min, max)
    int *ws_nfail;             // [npoints][nslab]
};
hipError_t launch_post_sources(hipStream_t s, const PostSourcesArgs &a);
hipError_t launch_pred_stats(hipStream_t s, PredArgs a, const double *vlo, const double *vhi);   // vlo, vhi: host [P], read with a.hist
size_t lsq_lds_bytes(int nmax);
size_t lsq_resolution_lds_bytes(int nmax);
hipError_t launch_lsq_step(hipStream_t s, const LsqArgs &a);
hipError_t launch_lsq_resolution(hipStream_t s, const LsqArgs &a);
hipError_t launch_mcmc_propose(hipStream_t s, const McmcProposeArgs &a);
hipError_t launch_mcmc_accept(hipStream_t s, const McmcAcceptArgs &a);
hipError_t launch_mcmc_accept_joint(hipStream_t s, const McmcJointArgs &a, bool ellip);   // ellip: the kernel that knows the sources 4 and 5
hipError_t launch_layers(hipStream_t s, const LayersArgs &a, int L);
hipError_t launch_prior(hipStream_t s, const LayersArgs &a, int L, const int *flags, double vs_max, int only_tag, int mark_tag, unsigned char *tags);
hipError_t launch_thermal(hipStream_t s, const LayersArgs &a);

// lanes per workgroup of the root search.  Nothing in it synchronises across wavefronts, so any multiple of 64
// works; measured with two batches in flight (M solves/s): 64 lanes 28.0, 128 30.8, 256 32.3, 512 32.7 - smaller
// workgroups do NOT help the second batch in, they slow the pair down
#ifndef SD_PHASE_BLOCK
#define SD_PHASE_BLOCK 256
#endif
size_t phase_lds_bytes(int Lmax, int G, int kind);   // per workgroup of SD_PHASE_BLOCK lanes (kind: 1 Love, 2 Rayleigh); the exact fallback's too
int phase_exact_team(int Lmax, int kind);                // lanes per stack of the exact fallback kernel
hipError_t launch_phase_exact(hipStream_t s, int kind, bool independent, const PhaseArgs &a);
hipError_t launch_finish(hipStream_t s, const FinishArgs &a);
hipError_t launch_kern_transpose(hipStream_t s, const KernTransposeArgs &a);
hipError_t launch_prep(hipStream_t s, int kind, const PrepArgs &a);
hipError_t launch_phase(hipStream_t s, int kind, int G, bool independent, const PhaseArgs &a);
hipError_t launch_group(hipStream_t s, int kind, const GroupArgs &a);

}  // namespace sd
